/*
 * kernels_r3w.hip -- instantiations and launcher of the WIDE three-stage rows kernels: contiguous rows of the
 * 7-smooth lengths 8193 ... 16383 of r3w_menu.inc (X(L, R1, R2, R3) entries chosen by tools/gen_r3w_menu.py), one row
 * per workgroup of 512 work-items (pass3g_kernel<R1, R2, R3, 0, 512>, one workgroup per CU like pass3w.hpp's 16384).
 * One trip over HBM where the two-pass plan made two (10 000 = 40 x 250: 38 % of the roofline).  Like the other rows
 * longer than 4096 points these steps have no LDS-kernel fallback (planner: long_rows_ok).
 * Reference counterpart: nested Cooley-Tukey nodes inside one plan (fftw/fftw_api.c:2078-2202).
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass3s.hpp"
#include "pass3g.hpp"
#include "launch.hpp"

template <int R1, int R2, int R3>
static void launch_3gw(const P3SArgs &pa, dim3 grid, hipStream_t st) {
    typedef P3GGeom<R1, R2, R3, 512> G;
    static_assert(G::fits && G::T == 1, "wide menu entry: one row per workgroup, at most 32 elements per item and stage");
    const size_t lds = G::lds_doubles * sizeof(double);
    static_assert(G::lds_doubles * sizeof(double) <= 160 * 1024, "wide menu entry exceeds the LDS");
    fa_launch_lds<pass3g_kernel<R1, R2, R3, 0, 512>>(grid, dim3(512), lds, lds, st, pa);
}

/* 1 when L is a wide menu length */
extern "C" int fa_hip_r3w_has(int L) {
    switch (L) {
#define X(L_, R1_, R2_, R3_) case L_: return 1;
#include "r3w_menu.inc"
#undef X
    }
    return 0;
}

/* contiguous rows of a wide menu length in one pass; 1 = not applicable */
int fa_launch_pass3gw(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                      i64 cs, i64 cn, hipStream_t st) {
    P3SArgs pa = P3SArgs();
    if (!fa_hip_r3w_has(d->L) || d->tile != 1 || d->src_im != 1 || d->dst_im != 1 || d->tw_n || d->is_l != 2 || d->os_l != 2 ||
        d->tile_lo_n > 1 || (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_LO_DFT)))
        return 1;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned() || !g.even_dims()) return 1;
    fa_copy_dims(pa, g);
    pa.wL = (const cplx *)tables[d->table];
    pa.flags = d->flags;
    pa.ntiles = pa.dn[0];
    const StepBlocks nb = fa_step_blocks(pa);
    if (nb.empty()) return 0;
    if (nb.too_large()) return 1;
    switch (d->L) {
#define X(L_, R1_, R2_, R3_) case L_: launch_3gw<R1_, R2_, R3_>(pa, nb.grid(), st); return 0;
#include "r3w_menu.inc"
#undef X
    }
    return 1;
}

/* ---- fused real rows of n = 2L <-> half spectra for the wide half lengths of r3rw_menu.inc (MODE 1 / 2 of
   pass3g_kernel at 512 work-items): real rows of 18 000 ... 30 720 points in ONE trip where round 2 ran a complex
   pass plus an untangle / tangle step */
template <int R1, int R2, int R3>
static void launch_3gw_real(const P3SArgs &pa, dim3 grid, hipStream_t st, bool inverse) {
    typedef P3GGeom<R1, R2, R3, 512> G;
    static_assert(G::fits && G::T == 1, "wide real menu entry: one row per workgroup");
    static_assert(G::lds_doubles * sizeof(double) <= 160 * 1024, "wide real menu entry exceeds the LDS");
    const size_t lds = G::lds_doubles * sizeof(double);
    if (inverse) fa_launch_lds<pass3g_kernel<R1, R2, R3, 2, 512>>(grid, dim3(512), lds, lds, st, pa);
    else fa_launch_lds<pass3g_kernel<R1, R2, R3, 1, 512>>(grid, dim3(512), lds, lds, st, pa);
}

extern "C" int fa_hip_r2c_rows3gw_has(int L) {
    switch (L) {
#define X(L_, R1_, R2_, R3_) case L_: return 1;
#include "r3rw_menu.inc"
#undef X
    }
    return 0;
}

/* pa, grid: filled by fa_launch_r2crows3 (kernels_rr.hip); 1 = no kernel for this length */
int fa_launch_r2crows3gw(int L, const P3SArgs &pa, dim3 grid, hipStream_t st, bool inverse) {
    switch (L) {
#define X(L_, R1_, R2_, R3_) case L_: launch_3gw_real<R1_, R2_, R3_>(pa, grid, st, inverse); return 0;
#include "r3rw_menu.inc"
#undef X
    }
    return 1;
}
