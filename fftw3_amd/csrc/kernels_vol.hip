/*
 * kernels_vol.hip -- instantiations and launcher of the one-trip small-volume kernel (pass3d.hpp): batches of
 * contiguous 3-D transforms n0 x n1 x n2 with every extent at most 32 and at most 8192 points, T whole volumes per
 * workgroup.  The sizes are those of vol3d_menu.inc.  A translation unit of its own.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass2d.hpp"
#include "pass3d.hpp"
#include "launch.hpp"

template <int R0, int R1, int R2>
static void launch_vol3d(const Vol3DArgs &va, dim3 grid, hipStream_t st, bool bwd) {
    const size_t lds = Vol3DGeom<R0, R1, R2>::lds_doubles * sizeof(double);
    if (bwd) fa_launch_lds<vol3d_kernel<R0, R1, R2, true>>(grid, dim3(256), lds, lds, st, va);
    else fa_launch_lds<vol3d_kernel<R0, R1, R2, false>>(grid, dim3(256), lds, lds, st, va);
}

#define FA_VOL3D_KEY(n0, n1, n2) (((n0) * 64 + (n1)) * 64 + (n2))

/* volumes per tile of the small-volume kernel for n0 x n1 x n2 (0: none) */
extern "C" int fa_hip_vol3d_tile(int n0, int n1, int n2) {
    if (n0 < 1 || n0 > 32 || n1 < 1 || n1 > 32 || n2 < 1 || n2 > 32) return 0;
    switch (FA_VOL3D_KEY(n0, n1, n2)) {
#define X(R0_, R1_, R2_) case FA_VOL3D_KEY(R0_, R1_, R2_): return Vol3DGeom<R0_, R1_, R2_>::T;
#include "vol3d_menu.inc"
#undef X
    }
    return 0;
}

/* doubles of the LDS layout of that kernel: *s = row stride, *sp = plane stride (element (t, a0, a1, a2) at
   (t n0 + a0) sp + a1 s + a2); returns the dynamic LDS bytes of a workgroup, 0: no such kernel */
extern "C" int fa_hip_vol3d_lds(int n0, int n1, int n2, int *s, int *sp) {
    if (fa_hip_vol3d_tile(n0, n1, n2) <= 0) return 0;
    switch (FA_VOL3D_KEY(n0, n1, n2)) {
#define X(R0_, R1_, R2_) case FA_VOL3D_KEY(R0_, R1_, R2_): \
        if (s) *s = Vol3DGeom<R0_, R1_, R2_>::S; \
        if (sp) *sp = Vol3DGeom<R0_, R1_, R2_>::SP; \
        return (int)(Vol3DGeom<R0_, R1_, R2_>::lds_doubles * sizeof(double));
#include "vol3d_menu.inc"
#undef X
    }
    return 0;
}

/* FFTW_AMD_K_VOL3D: dense interleaved volumes, one loop of whole volumes; 1 = not that step (the step has no other
   executor: the planner emits it only for aligned arrays in exactly this layout) */
int fa_launch_vol3d(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                    i64 cs, i64 cn, hipStream_t st) {
    Vol3DArgs va;
    if (d->aux_n < 1 || d->aux_n > 32) return 1;
    const int n0 = (int)d->aux_n, n1 = d->tile_lo_n, n2 = d->L;
    const int T = fa_hip_vol3d_tile(n0, n1, n2);
    const i64 row = 2 * (i64)n2, pln = row * n1, vol = pln * n0;
    const int swap = d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT);
    (void)tables;
    if (T <= 0 || d->tile != T || !(d->flags & FFTW_AMD_F_LO_DFT) || !(d->flags & FFTW_AMD_F_VOL3D) || d->src_im != 1 ||
        d->dst_im != 1 || d->tw_n || d->table >= 0 || d->table2 >= 0 || d->is_l != 2 || d->os_l != 2 ||
        d->tile_lo_is != row || d->tile_lo_os != row || d->ndims != 1 || d->dim_is[0] != vol || d->dim_os[0] != vol ||
        (swap != 0 && swap != (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT)) ||
        (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_TW_IN | FFTW_AMD_F_REAL_IMG)))
        return 1;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned()) return 1;
    va.src = g.src;
    va.dst = g.dst;
    va.nvol = g.dn[0];
    /* Nontemporal accesses only where every lane run is made of whole, aligned 128-byte lines (the rule of
       rr_dispatch.hpp).  A load run is a piece of a plane of n1 n2 elements, and the planes of a tile follow each
       other; the stores are 1 KiB pieces of the tile's run, whole lines when the tile starts on one. */
    va.flags = d->flags & (FFTW_AMD_F_NT_IN | FFTW_AMD_F_NT_OUT);
    if (((i64)n1 * n2) % 8 != 0 || (uintptr_t)g.src % 128 != 0) va.flags &= ~FFTW_AMD_F_NT_IN;
    if (((i64)T * n0 * n1 * n2) % 8 != 0 || (uintptr_t)g.dst % 128 != 0) va.flags &= ~FFTW_AMD_F_NT_OUT;
    const i64 ntiles = (va.nvol + T - 1) / T;
    if (ntiles <= 0) return 0;
    if (ntiles > 0x7fffffffLL) return 1;
    const dim3 grid((unsigned)ntiles, 1, 1);
    switch (FA_VOL3D_KEY(n0, n1, n2)) {
#define X(R0_, R1_, R2_) case FA_VOL3D_KEY(R0_, R1_, R2_): launch_vol3d<R0_, R1_, R2_>(va, grid, st, swap != 0); return 0;
#include "vol3d_menu.inc"
#undef X
    }
    return 1;
}
