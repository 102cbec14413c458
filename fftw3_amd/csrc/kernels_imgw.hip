/*
 * kernels_imgw.hip -- instantiations and launcher of the one-trip image kernel for an extent of 128 (pass2dw.hpp):
 * batches of contiguous 2-D transforms 128 x 128, 64 x 128 and 128 x 64, a tile of 16384 elements per workgroup of 512
 * work-items.  The sizes are those of img2dw_menu.inc.  A translation unit of its own.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass2d.hpp"
#include "pass2dl.hpp"
#include "pass2dw.hpp"
#include "launch.hpp"

template <int R0, int R1>
static void launch_img2dw(const Img2DLArgs &ia, dim3 grid, hipStream_t st, bool bwd, bool nt_out) {
    const size_t lds = Img2DWGeom<R0, R1>::lds_doubles * sizeof(double);
    const dim3 block(FA_IMG2DW_ITEMS);
    if (bwd && nt_out) fa_launch_lds<img2dw_kernel<R0, R1, true, true>>(grid, block, lds, lds, st, ia);
    else if (bwd) fa_launch_lds<img2dw_kernel<R0, R1, true, false>>(grid, block, lds, lds, st, ia);
    else if (nt_out) fa_launch_lds<img2dw_kernel<R0, R1, false, true>>(grid, block, lds, lds, st, ia);
    else fa_launch_lds<img2dw_kernel<R0, R1, false, false>>(grid, block, lds, lds, st, ia);
}

#define FA_IMG2DW_KEY(n0, n1) ((n0) * 256 + (n1))

/* images per tile of the image kernel for n0 rows x n1 columns with an extent of 128 (0: none) */
extern "C" int fa_hip_img2dw_tile(int n0, int n1) {
    if (n0 < 1 || n0 > 128 || n1 < 1 || n1 > 128) return 0;
    switch (FA_IMG2DW_KEY(n0, n1)) {
#define X(R0_, R1_) case FA_IMG2DW_KEY(R0_, R1_): return Img2DWGeom<R0_, R1_>::T;
#include "img2dw_menu.inc"
#undef X
    }
    return 0;
}

/* FFTW_AMD_K_IMG2DW: dense interleaved images, one loop of whole images; table / table2 = stage tables of the row /
   the column axis.  1 = not that step (the step has no other executor: the planner emits it only for aligned arrays
   in exactly this layout) */
int fa_launch_img2dw(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                     i64 cs, i64 cn, hipStream_t st) {
    Img2DLArgs ia;
    const int n0 = d->tile_lo_n, n1 = d->L;
    const int T = fa_hip_img2dw_tile(n0, n1);
    const i64 img = 2 * (i64)n0 * n1;
    const int swap = d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT);
    if (T <= 0 || d->tile != T || !(d->flags & FFTW_AMD_F_LO_DFT) || d->src_im != 1 || d->dst_im != 1 || d->tw_n ||
        d->is_l != 2 || d->os_l != 2 || d->tile_lo_is != 2 * (i64)n1 || d->tile_lo_os != 2 * (i64)n1 || d->ndims != 1 ||
        d->dim_is[0] != img || d->dim_os[0] != img || (swap != 0 && swap != (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT)) ||
        (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_TW_IN)) ||
        d->table < 0 || d->table2 < 0)
        return 1;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned()) return 1;
    ia.src = g.src;
    ia.dst = g.dst;
    ia.tw1 = (const cplx *)tables[d->table];
    ia.tw0 = (const cplx *)tables[d->table2];
    ia.nimg = g.dn[0];
    /* Nontemporal accesses only where every lane run is made of whole, aligned 128-byte lines (the rule of
       rr_dispatch.hpp).  A load run is 64 elements of an image row, the stores are 1 KiB pieces of the tile's run:
       whole lines when the array starts on one. */
    ia.flags = d->flags & FFTW_AMD_F_NT_IN;
    if ((uintptr_t)g.src % 128 != 0) ia.flags = 0;
    const bool nt_out = (d->flags & FFTW_AMD_F_NT_OUT) && (uintptr_t)g.dst % 128 == 0;
    const i64 ntiles = (ia.nimg + T - 1) / T;
    if (ntiles <= 0) return 0;
    if (ntiles > 0x7fffffffLL) return 1;
    const dim3 grid((unsigned)ntiles, 1, 1);
    switch (FA_IMG2DW_KEY(n0, n1)) {
#define X(R0_, R1_) case FA_IMG2DW_KEY(R0_, R1_): launch_img2dw<R0_, R1_>(ia, grid, st, swap != 0, nt_out); return 0;
#include "img2dw_menu.inc"
#undef X
    }
    return 1;
}
