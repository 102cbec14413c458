/*
 * kernels_imglr.hip -- instantiations and launcher of the one-trip real-image kernels for extents above 32
 * (pass2dlr.hpp): batches of 2-D r2c / c2r transforms n0 x n1 with both extents in {16, 32, 40, 48, 64} and at least
 * one above 32, T whole images per workgroup.  The sizes are those of img2dlr_menu.inc.  A translation unit of its own.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass2d.hpp"
#include "pass2dl.hpp"
#include "pass2dlr.hpp"
#include "launch.hpp"

template <int R0, int R1>
static void launch_img2dlr(const Img2DLRArgs &ia, dim3 grid, hipStream_t st) {
    const size_t lds = Img2DLRGeom<R0, R1, true>::lds_doubles * sizeof(double);
    fa_launch_lds<img2dlr_kernel<R0, R1>>(grid, dim3(256), lds, lds, st, ia);
}

template <int R0, int R1>
static void launch_img2dlc(const Img2DLRArgs &ia, dim3 grid, hipStream_t st) {
    const size_t lds = Img2DLRGeom<R0, R1, false>::lds_doubles * sizeof(double);
    fa_launch_lds<img2dlc_kernel<R0, R1>>(grid, dim3(256), lds, lds, st, ia);
}

#define FA_IMG2DLR_KEY(n0, n1) ((n0) * 128 + (n1))

/* images per tile of the real-image kernels for n0 rows x n1 real columns with an extent above 32, r2c (fwd) or c2r
   (0: none) */
extern "C" int fa_hip_img2dlr_tile(int n0, int n1, int fwd) {
    if (n0 < 1 || n0 > 64 || n1 < 1 || n1 > 64) return 0;
    switch (FA_IMG2DLR_KEY(n0, n1)) {
#define X(R0_, R1_) case FA_IMG2DLR_KEY(R0_, R1_): return fwd ? Img2DLRGeom<R0_, R1_, true>::T : Img2DLRGeom<R0_, R1_, false>::T;
#include "img2dlr_menu.inc"
#undef X
    }
    return 0;
}

/* FFTW_AMD_K_IMG2DLR: real images with rows of n1 or n1 + 2 doubles on one side, dense half spectra (rows of n1 + 2
   doubles) on the other, one loop of whole images; table = stage table of the row axis (always), table2 = that of the
   column axis where it has two stages.  1 = not that step (the step has no other executor: the planner emits it only
   for aligned arrays in exactly this layout) */
int fa_launch_img2dlr(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                      i64 cs, i64 cn, hipStream_t st) {
    Img2DLRArgs ia;
    const int n0 = d->tile_lo_n, n1 = d->L;
    const int real = d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT);
    const bool fwd = real == FFTW_AMD_F_REAL_IN;
    const int T = fa_hip_img2dlr_tile(n0, n1, fwd);
    const i64 cpitch = (i64)n1 + 2;
    const i64 rpitch = fwd ? d->tile_lo_is : d->tile_lo_os;
    const i64 cimg = (i64)n0 * cpitch, rimg = (i64)n0 * rpitch;
    if (T <= 0 || d->tile != T || !(d->flags & FFTW_AMD_F_REAL_IMG) || (real != FFTW_AMD_F_REAL_IN && real != FFTW_AMD_F_REAL_OUT) ||
        d->tw_n || d->table < 0 || (fa_img2dl_b(n0) > 1) != (d->table2 >= 0) || d->ndims != 1 || (rpitch != n1 && rpitch != cpitch) ||
        (d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_TW_IN | FFTW_AMD_F_LO_DFT |
                     FFTW_AMD_F_REAL_VOL | FFTW_AMD_F_VOL3D)))
        return 1;
    if (fwd) {
        if (d->src_im != 0 || d->is_l != 1 || d->dst_im != 1 || d->os_l != 2 || d->tile_lo_os != cpitch ||
            d->dim_is[0] != rimg || d->dim_os[0] != cimg) return 1;
    } else {
        if (d->src_im != 1 || d->is_l != 2 || d->dst_im != 0 || d->os_l != 1 || d->tile_lo_is != cpitch ||
            d->dim_is[0] != cimg || d->dim_os[0] != rimg) return 1;
    }
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned()) return 1;
    ia.src = g.src;
    ia.dst = g.dst;
    ia.tw1 = (const cplx *)tables[d->table];
    ia.tw0 = (d->table2 >= 0) ? (const cplx *)tables[d->table2] : NULL;
    ia.nimg = g.dn[0];
    ia.pitch = (int)rpitch;
    /* Nontemporal accesses only where every lane run is made of whole, aligned 128-byte lines (the rule of
       fa_launch_img2dr).  The load runs are image rows: n1 doubles at the real pitch, n1 / 2 + 1 entries of a half
       spectrum (never whole lines).  The stores are 1 KiB pieces of the tile's run, whole lines when the tile starts on
       one and, on the real side, the rows are dense. */
    ia.flags = d->flags & (FFTW_AMD_F_NT_IN | FFTW_AMD_F_NT_OUT);
    if (fwd) {
        if (n1 % 16 != 0 || rpitch % 16 != 0 || (uintptr_t)g.src % 128 != 0) ia.flags &= ~FFTW_AMD_F_NT_IN;
        if (((i64)T * cimg) % 16 != 0 || (uintptr_t)g.dst % 128 != 0) ia.flags &= ~FFTW_AMD_F_NT_OUT;
    } else {
        ia.flags &= ~FFTW_AMD_F_NT_IN;
        if (rpitch != n1 || ((i64)T * rimg) % 16 != 0 || (uintptr_t)g.dst % 128 != 0) ia.flags &= ~FFTW_AMD_F_NT_OUT;
    }
    const i64 ntiles = (ia.nimg + T - 1) / T;
    if (ntiles <= 0) return 0;
    if (ntiles > 0x7fffffffLL) return 1;
    const dim3 grid((unsigned)ntiles, 1, 1);
    switch (FA_IMG2DLR_KEY(n0, n1)) {
#define X(R0_, R1_) case FA_IMG2DLR_KEY(R0_, R1_): if (fwd) launch_img2dlr<R0_, R1_>(ia, grid, st); else launch_img2dlc<R0_, R1_>(ia, grid, st); return 0;
#include "img2dlr_menu.inc"
#undef X
    }
    return 1;
}
