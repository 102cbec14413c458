/*
 * kernels_imgl.hip -- instantiations and launcher of the one-trip image kernel for extents above 32 (pass2dl.hpp):
 * batches of contiguous 2-D transforms n0 x n1 with both extents in {16, 32, 40, 48, 64} and at least one above 32,
 * T whole images per workgroup.  The sizes are those of img2dl_menu.inc.  A translation unit of its own.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass2d.hpp"
#include "pass2dl.hpp"
#include "launch.hpp"

template <int R0, int R1>
static void launch_img2dl(const Img2DLArgs &ia, dim3 grid, hipStream_t st, bool bwd) {
    const size_t lds = Img2DLGeom<R0, R1>::lds_doubles * sizeof(double);
    if (bwd) fa_launch_lds<img2dl_kernel<R0, R1, true>>(grid, dim3(256), lds, lds, st, ia);
    else fa_launch_lds<img2dl_kernel<R0, R1, false>>(grid, dim3(256), lds, lds, st, ia);
}

#define FA_IMG2DL_KEY(n0, n1) ((n0) * 128 + (n1))

/* images per tile of the image kernel for n0 rows x n1 columns with an extent above 32 (0: none) */
extern "C" int fa_hip_img2dl_tile(int n0, int n1) {
    if (n0 < 1 || n0 > 64 || n1 < 1 || n1 > 64) return 0;
    switch (FA_IMG2DL_KEY(n0, n1)) {
#define X(R0_, R1_) case FA_IMG2DL_KEY(R0_, R1_): return Img2DLGeom<R0_, R1_>::T;
#include "img2dl_menu.inc"
#undef X
    }
    return 0;
}

/* FFTW_AMD_K_IMG2DL: dense interleaved images, one loop of whole images; table / table2 = stage tables of the row /
   the column axis where that axis has two stages.  1 = not that step (the step has no other executor: the planner
   emits it only for aligned arrays in exactly this layout) */
int fa_launch_img2dl(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                     i64 cs, i64 cn, hipStream_t st) {
    Img2DLArgs ia;
    const int n0 = d->tile_lo_n, n1 = d->L;
    const int T = fa_hip_img2dl_tile(n0, n1);
    const i64 img = 2 * (i64)n0 * n1;
    const int swap = d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT);
    if (T <= 0 || d->tile != T || !(d->flags & FFTW_AMD_F_LO_DFT) || d->src_im != 1 || d->dst_im != 1 || d->tw_n ||
        d->is_l != 2 || d->os_l != 2 || d->tile_lo_is != 2 * (i64)n1 || d->tile_lo_os != 2 * (i64)n1 || d->ndims != 1 ||
        d->dim_is[0] != img || d->dim_os[0] != img || (swap != 0 && swap != (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT)) ||
        (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_TW_IN)) ||
        (fa_img2dl_b(n1) > 1) != (d->table >= 0) || (fa_img2dl_b(n0) > 1) != (d->table2 >= 0))
        return 1;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned()) return 1;
    ia.src = g.src;
    ia.dst = g.dst;
    ia.tw1 = (d->table >= 0) ? (const cplx *)tables[d->table] : NULL;
    ia.tw0 = (d->table2 >= 0) ? (const cplx *)tables[d->table2] : NULL;
    ia.nimg = g.dn[0];
    /* Nontemporal accesses only where every lane run is made of whole, aligned 128-byte lines (the rule of
       rr_dispatch.hpp).  A load run is one image row of n1 elements; the stores are 1 KiB pieces of the tile's run,
       whole lines when the tile starts on one. */
    ia.flags = d->flags & (FFTW_AMD_F_NT_IN | FFTW_AMD_F_NT_OUT);
    if (n1 % 8 != 0 || (uintptr_t)g.src % 128 != 0) ia.flags &= ~FFTW_AMD_F_NT_IN;
    if (((i64)T * n0 * n1) % 8 != 0 || (uintptr_t)g.dst % 128 != 0) ia.flags &= ~FFTW_AMD_F_NT_OUT;
    const i64 ntiles = (ia.nimg + T - 1) / T;
    if (ntiles <= 0) return 0;
    if (ntiles > 0x7fffffffLL) return 1;
    const dim3 grid((unsigned)ntiles, 1, 1);
    switch (FA_IMG2DL_KEY(n0, n1)) {
#define X(R0_, R1_) case FA_IMG2DL_KEY(R0_, R1_): launch_img2dl<R0_, R1_>(ia, grid, st, swap != 0); return 0;
#include "img2dl_menu.inc"
#undef X
    }
    return 1;
}
