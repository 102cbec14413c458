/*
 * kernels_volr.hip -- instantiations and launcher of the one-trip small real-volume kernels (pass3dr.hpp): batches of
 * 3-D r2c / c2r transforms n0 x n1 x n2 with every extent at most 32 and n2 even, T whole volumes per workgroup.  The
 * sizes are those of vol3dr_menu.inc.  A translation unit of its own.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass2d.hpp"
#include "pass2dr.hpp"
#include "pass3dr.hpp"
#include "launch.hpp"

template <int R0, int R1, int R2>
static void launch_vol3dr(const Vol3DRArgs &va, dim3 grid, hipStream_t st) {
    const size_t lds = Vol3DRGeom<R0, R1, R2>::lds_doubles * sizeof(double);
    fa_launch_lds<vol3dr_kernel<R0, R1, R2>>(grid, dim3(256), lds, lds, st, va);
}

template <int R0, int R1, int R2>
static void launch_vol3dc(const Vol3DRArgs &va, dim3 grid, hipStream_t st) {
    const size_t lds = Vol3DCGeom<R0, R1, R2>::lds_doubles * sizeof(double);
    fa_launch_lds<vol3dc_kernel<R0, R1, R2>>(grid, dim3(256), lds, lds, st, va);
}

#define FA_VOL3DR_KEY(n0, n1, n2) (((n0) * 64 + (n1)) * 64 + (n2))

/* volumes per tile of the small real-volume kernels for n0 x n1 x n2 reals, r2c (fwd) or c2r (0: none) */
extern "C" int fa_hip_vol3dr_tile(int n0, int n1, int n2, int fwd) {
    if (n0 < 1 || n0 > 32 || n1 < 1 || n1 > 32 || n2 < 1 || n2 > 32) return 0;
    switch (FA_VOL3DR_KEY(n0, n1, n2)) {
#define X(R0_, R1_, R2_) case FA_VOL3DR_KEY(R0_, R1_, R2_): return fwd ? Vol3DRGeom<R0_, R1_, R2_>::T : Vol3DCGeom<R0_, R1_, R2_>::T;
#include "vol3dr_menu.inc"
#undef X
    }
    return 0;
}

/* the LDS layouts of those kernels in doubles: st[0], st[1] = row and plane stride of the first layout (X of the r2c
   kernel, C of the c2r kernel), st[2], st[3] = of the second (O, R); element (t, a0, a1, a2) at
   (t n0 + a0) plane stride + a1 row stride + a2.  Returns the dynamic LDS bytes of a workgroup, 0: no such kernel */
extern "C" int fa_hip_vol3dr_lds(int n0, int n1, int n2, int fwd, int *st) {
    if (fa_hip_vol3dr_tile(n0, n1, n2, fwd) <= 0) return 0;
    switch (FA_VOL3DR_KEY(n0, n1, n2)) {
#define X(R0_, R1_, R2_) case FA_VOL3DR_KEY(R0_, R1_, R2_): \
        if (st && fwd) { st[0] = Vol3DRGeom<R0_, R1_, R2_>::Sx; st[1] = Vol3DRGeom<R0_, R1_, R2_>::SPx; \
                         st[2] = Vol3DRGeom<R0_, R1_, R2_>::So; st[3] = Vol3DRGeom<R0_, R1_, R2_>::SPo; } \
        if (st && !fwd) { st[0] = Vol3DCGeom<R0_, R1_, R2_>::Sc; st[1] = Vol3DCGeom<R0_, R1_, R2_>::SPc; \
                          st[2] = Vol3DCGeom<R0_, R1_, R2_>::Sr; st[3] = Vol3DCGeom<R0_, R1_, R2_>::SPr; } \
        return (int)((fwd ? Vol3DRGeom<R0_, R1_, R2_>::lds_doubles : Vol3DCGeom<R0_, R1_, R2_>::lds_doubles) * sizeof(double));
#include "vol3dr_menu.inc"
#undef X
    }
    return 0;
}

/* FFTW_AMD_K_VOL3DR: real volumes with rows of n2 or n2 + 2 doubles on one side, dense half spectra (rows of n2 + 2
   doubles) on the other, planes and volumes dense at those pitches, one loop of whole volumes; 1 = not that step (the
   step has no other executor: the planner emits it only for aligned arrays in exactly this layout) */
int fa_launch_vol3dr(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                     i64 cs, i64 cn, hipStream_t st) {
    Vol3DRArgs va;
    if (d->aux_n < 1 || d->aux_n > 32) return 1;
    const int n0 = (int)d->aux_n, n1 = d->tile_lo_n, n2 = d->L;
    const int real = d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT);
    const bool fwd = real == FFTW_AMD_F_REAL_IN;
    const int T = fa_hip_vol3dr_tile(n0, n1, n2, fwd);
    const i64 cpitch = (i64)n2 + 2;
    const i64 rpitch = fwd ? d->tile_lo_is : d->tile_lo_os;
    const i64 cvol = (i64)n0 * n1 * cpitch, rvol = (i64)n0 * n1 * rpitch;
    (void)tables;
    if (T <= 0 || d->tile != T || !(d->flags & FFTW_AMD_F_REAL_VOL) || (real != FFTW_AMD_F_REAL_IN && real != FFTW_AMD_F_REAL_OUT) ||
        d->tw_n || d->table >= 0 || d->table2 >= 0 || d->ndims != 1 || (rpitch != n2 && rpitch != cpitch) ||
        (d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_TW_IN | FFTW_AMD_F_LO_DFT |
                     FFTW_AMD_F_REAL_IMG | FFTW_AMD_F_VOL3D)))
        return 1;
    if (fwd) {
        if (d->src_im != 0 || d->is_l != 1 || d->dst_im != 1 || d->os_l != 2 || d->tile_lo_os != cpitch ||
            d->dim_is[0] != rvol || d->dim_os[0] != cvol) return 1;
    } else {
        if (d->src_im != 1 || d->is_l != 2 || d->dst_im != 0 || d->os_l != 1 || d->tile_lo_is != cpitch ||
            d->dim_is[0] != cvol || d->dim_os[0] != rvol) return 1;
    }
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned()) return 1;
    va.src = g.src;
    va.dst = g.dst;
    va.nvol = g.dn[0];
    va.pitch = (int)rpitch;
    /* Nontemporal accesses only where every lane run is made of whole, aligned 128-byte lines (the rule of
       fa_launch_vol3d / fa_launch_img2dr).  The r2c load runs are pieces of a plane of n1 rows, contiguous when the rows
       are dense and whole lines when n2 is a multiple of 16; the c2r load runs are rows of n2 / 2 + 1 entries, never
       whole lines.  The stores are 1 KiB pieces of the tile's run, whole lines when the tile starts on one and, on the
       real side, the rows are dense. */
    va.flags = d->flags & (FFTW_AMD_F_NT_IN | FFTW_AMD_F_NT_OUT);
    if (fwd) {
        if (n2 % 16 != 0 || rpitch != n2 || (uintptr_t)g.src % 128 != 0) va.flags &= ~FFTW_AMD_F_NT_IN;
        if (((i64)T * cvol) % 16 != 0 || (uintptr_t)g.dst % 128 != 0) va.flags &= ~FFTW_AMD_F_NT_OUT;
    } else {
        va.flags &= ~FFTW_AMD_F_NT_IN;
        if (rpitch != n2 || ((i64)T * rvol) % 16 != 0 || (uintptr_t)g.dst % 128 != 0) va.flags &= ~FFTW_AMD_F_NT_OUT;
    }
    const i64 ntiles = (va.nvol + T - 1) / T;
    if (ntiles <= 0) return 0;
    if (ntiles > 0x7fffffffLL) return 1;
    const dim3 grid((unsigned)ntiles, 1, 1);
    switch (FA_VOL3DR_KEY(n0, n1, n2)) {
#define X(R0_, R1_, R2_) case FA_VOL3DR_KEY(R0_, R1_, R2_): if (fwd) launch_vol3dr<R0_, R1_, R2_>(va, grid, st); else launch_vol3dc<R0_, R1_, R2_>(va, grid, st); return 0;
#include "vol3dr_menu.inc"
#undef X
    }
    return 1;
}
