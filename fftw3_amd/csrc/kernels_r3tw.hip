/*
 * kernels_r3tw.hip -- the strided / transposed three-stage kernels (pass3t_kernel, pass3g.hpp) with 512 work-items
 * per workgroup for the lengths of r3tw_menu.inc (1080 ... 2048): tiles of 16384 elements hold 8 ... 15 sequences,
 * i.e. 128 ... 240-byte segments on the strided side, where the 256-item tiles of kernels_r3.hip hold 4 ... 7
 * (64 ... 112 bytes, about 3.2 TB/s).  Serves a strided axis of such a length in one trip (2-D / 3-D transforms)
 * and the 2048-point first pass of the two-trip 2^21 plan; the 2048-point rows trips of the two-trip real plans (r2c: RD = 1,
 * c2r: RD = 2).  One workgroup per CU.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass3s.hpp"
#include "pass3g.hpp"
#include "launch.hpp"

template <int R1, int R2, int R3, bool IN_T, int TW, int RD = 0>
static void launch_3tw_variant(const P1024Args &pa, dim3 grid, hipStream_t st) {
    typedef P3TGeom<R1, R2, R3, 512> G;
    static_assert(G::T >= 8 && G::QA * R1 <= 40 && G::QB * R2 <= 40 && G::QC * R3 <= 40, "wide strided menu entry");
    static_assert(G::lds_doubles * sizeof(double) <= 160 * 1024, "wide strided menu entry exceeds the LDS");
    const size_t lds = G::lds_doubles * sizeof(double);
    fa_launch_lds<pass3t_kernel<R1, R2, R3, IN_T, TW, 512, RD>>(grid, dim3(512), lds, lds, st, pa);
}

template <int R1, int R2, int R3>
static int dispatch_3tw(const P1024Args &pa, dim3 grid, hipStream_t st, bool in_t, bool out_t, int tw) {
    if (in_t && out_t) {
        if (tw == 0) { launch_3tw_variant<R1, R2, R3, true, 0>(pa, grid, st); return 0; }
        if (tw == 1) { launch_3tw_variant<R1, R2, R3, true, 1>(pa, grid, st); return 0; }
        return 1;
    }
    if (!in_t && out_t) {
        if (tw == 0) { launch_3tw_variant<R1, R2, R3, false, 0>(pa, grid, st); return 0; }
        if (tw == 2) { launch_3tw_variant<R1, R2, R3, false, 2>(pa, grid, st); return 0; }
    }
    return 1;
}

/* 1 = the length has the real-decimated rows form (FFTW_AMD_F_REAL_DEC: last trip of a two-trip r2c) */
extern "C" int fa_hip_r3tw_rdec(int L) { return L == 2048; }
/* 1 = the length has the c2r-decimated rows form (FFTW_AMD_F_REAL_DEC_C2R: first trip of a two-trip c2r) */
extern "C" int fa_hip_r3tw_cdec(int L) { return L == 2048; }

/* sequences per tile of the 512-item strided kernel for length L (0: none) */
extern "C" int fa_hip_r3tw_tile(int L) {
    switch (L) {
#define X(L_, R1_, R2_, R3_) case L_: return P3TGeom<R1_, R2_, R3_, 512>::T;
#include "r3tw_menu.inc"
#undef X
    }
    return 0;
}

int fa_launch_pass3tw(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                      i64 cs, i64 cn, hipStream_t st) {
    P1024Args pa;
    const int T = fa_hip_r3tw_tile(d->L);
    const bool rdec = (d->flags & FFTW_AMD_F_REAL_DEC) != 0;
    const bool cdec = (d->flags & FFTW_AMD_F_REAL_DEC_C2R) != 0;
    const int swaps = FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT;
    if (T <= 0 || d->tile != T || d->src_im != 1 || d->dst_im != 1 || d->tile_lo_n > 1 ||
        (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_LO_DFT)))
        return 1;
    if (rdec && (!fa_hip_r3tw_rdec(d->L) || (d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT)) || !(d->flags & FFTW_AMD_F_TW_IN) ||
                 d->tw_n == 0 || d->dim_tw[0] != 1 || d->dim_n[0] < 2 || d->batch_dim == 0))
        return 1;
    /* the c2r twin is a backward step: it carries BOTH swap flags (the kernel form exchanges re and im itself, while
       loading and in its pair exchange), the twiddle on the output, and never the forward form's flag */
    if (cdec && (rdec || !fa_hip_r3tw_cdec(d->L) || (d->flags & swaps) != swaps || (d->flags & FFTW_AMD_F_TW_IN) ||
                 d->tw_n == 0 || d->dim_tw[0] != 1 || d->dim_n[0] < 2 || d->batch_dim == 0 || d->is_l != (d->dim_n[0] - 1) * 2 * d->dim_is[0]))
        return 1;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned() || !g.even_l() || !g.even_dims()) return 1;
    fa_copy_dims(pa, g);
    pa.is_l = d->is_l;
    pa.os_l = d->os_l;
    pa.w1024 = (const cplx *)tables[d->table];
    pa.tw_shift = d->tw_shift;
    pa.tw_lo = d->tw_n ? (const cplx *)tables[d->tw_lo] : NULL;
    pa.tw_hi = d->tw_n ? (const cplx *)tables[d->tw_hi] : NULL;
    pa.flags = d->flags;
    pa.lo_sh = 0; pa.lo_is = 0; pa.lo_os = 0;
    pa.dbg = NULL;
    pa.ntiles = (pa.dn[0] + T - 1) / T;
    const StepBlocks nb = fa_step_blocks(pa);
    if (nb.empty()) return 0;
    if (nb.too_large()) return 1;
    if (pa.dn[0] * 4 < T) return 1;              /* a mostly empty tile: the LDS kernel */
    const dim3 grid = nb.grid();
    const bool in_t = pa.dn[0] > 1 && iabs64(pa.dis[0]) <= iabs64(pa.is_l);
    const bool out_t = pa.dn[0] > 1 && iabs64(pa.dos[0]) <= iabs64(pa.os_l);
    if (rdec) {
        if (in_t || !out_t || d->L != 2048) return 1;
        launch_3tw_variant<8, 16, 16, false, 2, 1>(pa, grid, st);
        return 0;
    }
    if (cdec) {
        if (!in_t || out_t || d->L != 2048) return 1;
        pa.flags &= ~swaps;                       /* applied by the form itself */
        launch_3tw_variant<8, 16, 16, true, 1, 2>(pa, grid, st);
        return 0;
    }
    int tw = d->tw_n == 0 ? 0 : ((d->flags & FFTW_AMD_F_TW_IN) ? 2 : 1);
    switch (d->L) {
#define X(L_, R1_, R2_, R3_) case L_: return dispatch_3tw<R1_, R2_, R3_>(pa, grid, st, in_t, out_t, tw);
#include "r3tw_menu.inc"
#undef X
    }
    return 1;
}
