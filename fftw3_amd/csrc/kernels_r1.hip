/*
 * kernels_r1.hip -- instantiations and launcher of the one-stage rows kernel (pass1r.hpp):
 * dense rows of R = 2 ... 32 points, one butterfly per row.  A translation unit of its own.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass3s.hpp"
#include "pass1r.hpp"
#include "launch.hpp"

#define FA_R1_LENGTHS(X) \
    X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) \
    X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

template <int R>
static void launch_1r(const P3SArgs &pa, dim3 grid, hipStream_t st) {
    const size_t lds = P1RGeom<R>::lds_doubles * sizeof(double);
    fa_launch_lds<pass1r_kernel<R>>(grid, dim3(256), lds, lds, st, pa);
}

/* rows per tile of the one-stage rows kernel for length L (0: none) */
extern "C" int fa_hip_r1_tile(int L) {
    switch (L) {
#define X(R_) case R_: return P1RGeom<R_>::T;
        FA_R1_LENGTHS(X)
#undef X
    }
    return 0;
}

/* dense interleaved rows of a short length in one butterfly per row; 1 = not applicable (the
   caller falls back to the two-stage or the LDS kernel) */
int fa_launch_pass1r(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                     i64 cs, i64 cn, hipStream_t st) {
    P3SArgs pa;
    const int T = fa_hip_r1_tile(d->L);
    (void)tables;
    if (T <= 0 || d->tile != T || d->src_im != 1 || d->dst_im != 1 || d->tw_n ||
        d->is_l != 2 || d->os_l != 2 || d->tile_lo_n > 1 || d->ndims < 1 ||
        d->dim_is[0] != 2 * (i64)d->L || d->dim_os[0] != 2 * (i64)d->L ||
        (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT)))
        return 1;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    if (!g.aligned() || !g.even_dims()) return 1;
    fa_copy_dims(pa, g);
    pa.wL = NULL;
    pa.flags = d->flags;
    pa.ntiles = (pa.dn[0] + T - 1) / T;
    const StepBlocks nb = fa_step_blocks(pa);
    if (nb.empty()) return 0;
    if (nb.too_large()) return 1;
    switch (d->L) {
#define X(R_) case R_: launch_1r<R_>(pa, nb.grid(), st); return 0;
        FA_R1_LENGTHS(X)
#undef X
    }
    return 1;
}

/* ---- dense real rows of n = 2L = 4 ... 64 points <-> half spectra (pass1r_real_kernel) ------------------------ */

template <int R>
static void launch_1r_real(const P3SArgs &pa, dim3 grid, hipStream_t st, bool inverse, bool pad) {
    const size_t lds = P1RRealGeom<R>::lds_doubles * sizeof(double);
    const dim3 blk(256);
    if (inverse && pad) fa_launch_lds<pass1r_real_kernel<R, false, true>>(grid, blk, lds, lds, st, pa);
    else if (inverse) fa_launch_lds<pass1r_real_kernel<R, false, false>>(grid, blk, lds, lds, st, pa);
    else if (pad) fa_launch_lds<pass1r_real_kernel<R, true, true>>(grid, blk, lds, lds, st, pa);
    else fa_launch_lds<pass1r_real_kernel<R, true, false>>(grid, blk, lds, lds, st, pa);
}

extern "C" int fa_hip_r2c_rows1_tile(int L) { return fa_hip_r1_tile(L); }

/* The step (FFTW_AMD_F_R2C_ROWS / _C2R_ROWS with L <= 32) has no other executor; the planner emits it only when a
   loop of at least 256 rows has exactly the dense strides, so anything else is a caller error and fails loudly. */
int fa_launch_r2crows1(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                       i64 cs, i64 cn, hipStream_t st) {
    P3SArgs pa;
    const int T = fa_hip_r2c_rows1_tile(d->L);
    const bool inverse = (d->flags & FFTW_AMD_F_C2R_ROWS) != 0;
    const i64 rs = 2 * (i64)d->L, cst = 2 * ((i64)d->L + 1);          /* row pitch on the real / complex side */
    const i64 want_is = inverse ? cst : rs, want_os = inverse ? rs : cst;
    int dense = -1;
    bool pad = false;
    if (T <= 0 || d->tile != T || d->src_im != 1 || d->dst_im != 1 || d->is_l != 2 || d->os_l != 2 ||
        d->aux_valid || d->aux_buf > 0 || d->tile_lo_n > 1) {
        fprintf(stderr, "fftw3_amd: internal error: short real rows step with an unsupported layout\n");
        abort();
    }
    StepGeom g = fa_step_geom(d, bufs, cs, cn);
    /* the dense loop becomes the tile dim (the planner's tile dim is whichever loop has the smallest stride) */
    for (int i = 0; i < d->ndims; ++i)
        if (g.dis[i] == want_is && g.dos[i] == want_os && (dense < 0 || g.dn[i] > g.dn[dense])) dense = i;
    if (dense < 0) {
        /* FFTW's padded layout: both sides advance by 2 (L + 1) doubles per row */
        for (int i = 0; i < d->ndims; ++i)
            if (g.dis[i] == cst && g.dos[i] == cst && (dense < 0 || g.dn[i] > g.dn[dense])) dense = i;
        pad = dense >= 0;
    }
    if (dense < 0 || !g.aligned() || !g.even_dims()) {
        fprintf(stderr, "fftw3_amd: fftw_execute_dft_r2c / _c2r needs arrays laid out and aligned like the ones the plan "
                        "was created with\n");
        abort();
    }
    if (dense != 0) {
        i64 t;
        t = g.dn[0]; g.dn[0] = g.dn[dense]; g.dn[dense] = t;
        t = g.dis[0]; g.dis[0] = g.dis[dense]; g.dis[dense] = t;
        t = g.dos[0]; g.dos[0] = g.dos[dense]; g.dos[dense] = t;
    }
    fa_copy_dims(pa, g);
    pa.wL = NULL;
    pa.tw_lo = (const cplx *)tables[d->tw_lo];
    pa.tw_hi = (const cplx *)tables[d->tw_hi];
    pa.tw_shift = d->tw_shift;
    pa.flags = 0;
    pa.ntiles = (pa.dn[0] + T - 1) / T;
    const StepBlocks nb = fa_step_blocks(pa);
    if (nb.empty()) return 0;
    if (nb.too_large()) {
        fprintf(stderr, "fftw3_amd: short real rows step with more than 2^31 tiles\n");
        abort();
    }
    switch (d->L) {
#define X(R_) case R_: launch_1r_real<R_>(pa, nb.grid(), st, inverse, pad); return 0;
        FA_R1_LENGTHS(X)
#undef X
    }
    fprintf(stderr, "fftw3_amd: internal error: no short real rows kernel for half length %d\n", d->L);
    abort();
}
