/*
 * kernels_elem.hip -- the element-wise steps (everything that is not a pass) and their launchers, one per step
 * kind.  Which kernel form a step takes is a pure function of the descriptor, the alignment of the two addresses
 * and the chunk length (elem_form, exposed as fa_hip_elem_form and pinned by tests/test_elem_forms.py).
 *
 * What each kernel replaces in the reference (fftw/fftw_api.c, "A.c"):
 *   copy_kernel          <- cpy2d_pair copies A.c:16412-16452, Bluestein
 *       chirp products A.c:1642-1688, Rader gather/scatter A.c:4187-4261.
 *   r2c_post / c2r_pre   <- ct_hc2c_direct_apply A.c:5831-5845 with the
 *       hc2cfdft / hc2cbdft codelets, plus the DC/Nyquist zeroing A.c:7155.
 */
#include "common.hpp"
#include "launch.hpp"

/* ------------------------------------------------------------------------ */
/* index space of the element-wise kernels                                   */
/* ------------------------------------------------------------------------ */
/* Work items run over dims[0..kpos) (the loops that are more contiguous than the
   transform index on the user side), then the transform / pair index k in [0, K), then
   dims[kpos..ndims).  The part up to and including k is the "inner" index: one virtual
   block covers 256 consecutive inner indices of one combination of the outer dims, so
   the outer dims are peeled once per block and the inner ones with 32-bit arithmetic
   instead of a chain of 64-bit divisions per element.  (These kernels run at the
   device-to-device copy rate, 4.0-4.5 TB/s, either way: they are bound by their eight
   interleaved forward / mirrored streams, not by the index arithmetic.) */
struct ElemIdx {
    i64 dn[FFTW_AMD_MAX_DIMS], dis[FFTW_AMD_MAX_DIMS], dos[FFTW_AMD_MAX_DIMS];
    i64 nvb;                 /* virtual blocks = nblk * prod(dn[kpos..ndims)) */
    unsigned K, inner, nblk; /* inner = K * prod(dn[0..kpos)), nblk = ceil(inner / 256) */
    int ndims, kpos;
};

FA_DEV bool elem_index(const ElemIdx &e, i64 vb, i64 *k, i64 *soff, i64 *doff) {
    i64 ob = vb / e.nblk;
    unsigned i = (unsigned)(vb - ob * e.nblk) * 256u + threadIdx.x;
    i64 so = 0, dof = 0;
    for (int d = e.kpos; d < e.ndims; ++d) {       /* uniform over the block */
        i64 q = ob / e.dn[d], r = ob - q * e.dn[d];
        so += r * e.dis[d];
        dof += r * e.dos[d];
        ob = q;
    }
    if (i >= e.inner) return false;
    for (int d = 0; d < e.kpos; ++d) {
        unsigned n = (unsigned)e.dn[d], q = i / n, r = i - q * n;
        so += (i64)r * e.dis[d];
        dof += (i64)r * e.dos[d];
        i = q;
    }
    *k = i;
    *soff = so;
    *doff = dof;
    return true;
}

/* ------------------------------------------------------------------------ */
/* strided copy / pad / multiply / permute                                   */
/* ------------------------------------------------------------------------ */

struct CopyArgs {
    const double *src;
    double *dst;
    i64 src_im, dst_im;
    i64 is_k, os_k;
    i64 K, Kvalid;
    ElemIdx e;
    const cplx *tab;
    const i64 *perm;
    int flags;
};

/* U virtual blocks (U x 256 consecutive inner indices) per trip of a workgroup: the U index chains (table entry ->
   element -> store) of a work-item are independent, so their loads overlap.  U = 4 for plain / padded / table
   copies (Bluestein's chirp products: 3.8 -> 3.0 ms per 2 GiB batch of n = 10007); the PERMUTED copies of Rader's
   gather / scatter stay at U = 1 -- they are bound by their 16-byte accesses to 128-byte lines (3.5 ms per 2 GiB
   where a pass takes 1.5) and four in flight per item change nothing (profiles/r03_prime_plan_steps.txt) */
template <int U>
__global__ void __launch_bounds__(256) copy_kernel(const CopyArgs a) {
    const i64 ngroups = (a.e.nvb + U - 1) / U;
    /* a permuted copy touches every 128-byte line of a row eight times, 16 bytes at a time: with the virtual blocks
       dealt round-robin all eight XCDs (workgroup b runs on XCD b % 8) fill / write back every line of every row.
       Keeping each ROW on one XCD leaves that to one L2: rows of 12288 points 3.5 -> 2.8 ms per 2 GiB, rows of 2^16
       points (1 MiB of the 4 MiB L2) unchanged */
    const i64 nrows = a.e.nvb / a.e.nblk;
    const bool by_rows = U == 1 && (gridDim.x & 7) == 0 && nrows >= 8;
    const i64 xcd = blockIdx.x & 7, per = by_rows ? (gridDim.x >> 3) : gridDim.x;
    for (i64 j = by_rows ? (blockIdx.x >> 3) : blockIdx.x; ; j += per) {
        i64 g = j;
        if (by_rows) {
            const i64 rr = j / a.e.nblk, row = xcd + 8 * rr;
            if (row >= nrows) break;
            g = row * a.e.nblk + (j - rr * a.e.nblk);
        } else if (g >= ngroups) break;
        i64 k[U], soff[U], doff[U], ks[U];
        bool ok[U];
        cplx v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i64 vb = g * U + u;
            ok[u] = vb < a.e.nvb && elem_index(a.e, vb, &k[u], &soff[u], &doff[u]);
            if (!ok[u]) { k[u] = 0; soff[u] = 0; doff[u] = 0; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            ks[u] = (ok[u] && (a.flags & FFTW_AMD_F_PERM_SRC)) ? a.perm[k[u]] : k[u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = c_make(0.0, 0.0);
            if (ok[u] && k[u] < a.Kvalid) v[u] = load_elem<false>(a.src, soff[u] + ks[u] * a.is_k, a.src_im, a.flags);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            if (a.flags & FFTW_AMD_F_MUL_TABLE) v[u] = c_mul(v[u], a.tab[k[u]]);
            if (a.flags & FFTW_AMD_F_MUL_CONJ) v[u] = c_mulc(v[u], a.tab[k[u]]);
            const i64 kd = (a.flags & FFTW_AMD_F_PERM_DST) ? a.perm[k[u]] : k[u];
            store_elem<false>(a.dst, doff[u] + kd * a.os_k, a.dst_im, a.flags, v[u]);
        }
    }
}

/* ------------------------------------------------------------------------ */
/* r2c untangle / c2r tangle                                                 */
/* ------------------------------------------------------------------------ */

struct RealArgs {
    const double *src;
    double *dst;
    i64 src_im, dst_im;
    i64 is_k, os_k;
    i64 h;       /* n / 2 */
    i64 npair;   /* h / 2 + 1 */
    ElemIdx e;
    const cplx *tw_lo;
    const cplx *tw_hi;
    int tw_shift;
    int flags;
    int r2r;     /* fused r2r epilogue (r2c) / prologue (c2r): FFTW_AMD_R2R_* or 0 */
    int twmul;   /* untangle twiddle w_n^k = table entry k * twmul */
    i64 rn;      /* r2r length */
};

#include "r2r_epi.hpp"

/* Y[k] = E + w^k O, Y[h-k] = conj(E - w^k O), E = (Z[k] + conj Z[h-k]) / 2,
   O = -i (Z[k] - conj Z[h-k]) / 2   (the 1/2 is the
   KP500000000 of reference rdft_scalar/r2cf/hc2cfdft_4.c:137) */
__global__ void __launch_bounds__(256) r2c_post_kernel(const RealArgs a) {
    for (i64 vb = blockIdx.x; vb < a.e.nvb; vb += gridDim.x) {
        i64 k, soff, doff;
        if (!elem_index(a.e, vb, &k, &soff, &doff)) continue;
        i64 km = a.h - k;
        cplx zk = load_elem<false>(a.src, soff + k * a.is_k, a.src_im, 0);
        cplx zm = load_elem<false>(a.src, soff + (km == a.h ? 0 : km) * a.is_k, a.src_im, 0);
        cplx E = c_make(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
        cplx D = c_make(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));
        cplx O = c_mni(D);
        cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, k * a.twmul);
        cplx P = c_mulc(O, w);
        cplx yk = c_add(E, P);
        cplx ym = c_sub(E, P);
        ym.y = -ym.y;
        if (k == 0) { yk.y = 0.0; ym.y = 0.0; }
        epi_store(a, doff, k, yk);
        if (km != k) epi_store(a, doff, km, ym);
    }
}

/* Z'[k] = E' + i O', Z'[h-k] = conj(E' - i O'), E' = Y[k] + conj Y[h-k],
   O' = (Y[k] - conj Y[h-k]) w^-k  (transpose of the above; reference
   hc2cbdft codelets, no 1/2) */
__global__ void __launch_bounds__(256) c2r_pre_kernel(const RealArgs a) {
    for (i64 vb = blockIdx.x; vb < a.e.nvb; vb += gridDim.x) {
        i64 k, soff, doff;
        if (!elem_index(a.e, vb, &k, &soff, &doff)) continue;
        i64 km = a.h - k;
        cplx yk = pro_load(a, soff, k);
        cplx ym = pro_load(a, soff, km);
        if (k == 0) { yk.y = 0.0; ym.y = 0.0; }   /* Im Y[0], Im Y[n/2] are ignored */
        cplx E = c_make(yk.x + ym.x, yk.y - ym.y);
        cplx D = c_make(yk.x - ym.x, yk.y + ym.y);
        cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, k * a.twmul);
        cplx O = c_mul(D, w);
        cplx iO = c_mpi(O);
        cplx zk = c_add(E, iO);
        cplx zm = c_sub(E, iO);
        zm.y = -zm.y;
        store_elem<false>(a.dst, doff + k * a.os_k, a.dst_im, a.flags, zk);
        if (km != k && km != a.h)
            store_elem<false>(a.dst, doff + km * a.os_k, a.dst_im, a.flags, zm);
    }
}

/* The same two butterflies for the layout the large 1-D plans produce (interleaved complex on both sides,
   contiguous in k, the batch as the only loop, no r2r hook): 16-byte accesses, 32-bit index arithmetic, one
   work-item per pair (k, h-k); nontemporal on the caller's side.  Pure streaming. */
struct Real2Fast {
    const double *src;
    double *dst;
    i64 sbatch, dbatch;
    unsigned h, npair;
    const cplx *tw_lo;
    const cplx *tw_hi;
    int tw_shift;
};
template <bool NT>
__global__ void __launch_bounds__(256) r2c_post_fast_kernel(const Real2Fast a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.npair) return;
    const unsigned h = a.h, km = h - k;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, (i64)k);
    cplx zk = ld_cplx<false>(s + 2 * (i64)k);
    cplx zm = ld_cplx<false>(s + 2 * (i64)(km == h ? 0 : km));
    cplx E = c_make(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
    cplx D = c_make(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));
    cplx P = c_mulc(c_mni(D), w);
    cplx yk = c_add(E, P);
    cplx ym = c_sub(E, P);
    ym.y = -ym.y;
    if (k == 0) { yk.y = 0.0; ym.y = 0.0; }
    st_cplx<NT>(d + 2 * (i64)k, yk);
    if (km != k) st_cplx<NT>(d + 2 * (i64)km, ym);
}
template <bool NT>
__global__ void __launch_bounds__(256) c2r_pre_fast_kernel(const Real2Fast a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.npair) return;
    const unsigned h = a.h, km = h - k;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, (i64)k);
    cplx yk = ld_cplx<NT>(s + 2 * (i64)k), ym = ld_cplx<NT>(s + 2 * (i64)km);
    if (k == 0) { yk.y = 0.0; ym.y = 0.0; }
    cplx E = c_make(yk.x + ym.x, yk.y - ym.y);
    cplx D = c_make(yk.x - ym.x, yk.y + ym.y);
    cplx iO = c_mpi(c_mul(D, w));
    cplx zk = c_add(E, iO);
    cplx zm = c_sub(E, iO);
    zm.y = -zm.y;
    st_cplx<false>(d + 2 * (i64)k, zk);
    if (km != k && km != h) st_cplx<false>(d + 2 * (i64)km, zm);
}

/* DCT-II / DST-II (REDFT10 / RODFT10) of long contiguous rows, streaming forms of the two element-wise steps
   (reference loops: reodft010e-r2hc, fftw/fftw_api.c:12465-12660):
   shuffle   v[j] = x[2j], v[n-1-j] = +-x[2j+1]: one work-item per input quad, 2 x 16 B in, 2 x 16 B out;
   untangle + epilogue: one work-item per pair (k, h-k) of the half-length spectrum Z (h = n / 2): Y[k], Y[h-k]
   as in r2c_post_fast_kernel, then y[k] = 2 Re(w^k Y[k]), y[n-k] = -2 Im(w^k Y[k]) with w = w_4n (the table's
   modulus; the untangle twiddle is its entry 4k, and w^(h-k) = e^(i pi/4) conj(w^k) saves a table lookup). */
struct DctFast {
    const double *src;
    double *dst;
    i64 sbatch, dbatch;
    unsigned n, nitems;
    const cplx *tw_lo;
    const cplx *tw_hi;
    int tw_shift;
    int odd;            /* RODFT10: negate the odd samples / reverse the output */
};
template <bool NT>
__global__ void __launch_bounds__(256) dct2_shuffle_fast_kernel(const DctFast a) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.nitems) return;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch + 4 * (i64)q;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx u = ld_cplx<NT>(s), v = ld_cplx<NT>(s + 2);
    const double sg = a.odd ? -1.0 : 1.0;
    st_cplx<false>(d + 2 * (i64)q, c_make(u.x, v.x));
    st_cplx<false>(d + ((i64)a.n - 2 - 2 * (i64)q), c_make(sg * v.y, sg * u.y));
}
FA_DEV void dct2_epilogue(const DctFast &a, double *d, unsigned idx, cplx Y, cplx w) {
    const unsigned n = a.n;
    const bool mid = idx > 0 && 2 * idx < n;
    const double vi = mid ? Y.y : 0.0;
    const double dr = Y.x * w.x + vi * w.y, di = vi * w.x - Y.x * w.y;
    d[a.odd ? n - 1 - idx : idx] = 2.0 * dr;
    if (mid) d[a.odd ? idx - 1 : n - idx] = -2.0 * di;
}
__global__ void __launch_bounds__(256) dct2_untangle_fast_kernel(const DctFast a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.nitems) return;
    const unsigned h = a.n / 2, km = h - k;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx wu = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 4 * (i64)k);      /* w_n^k */
    cplx wk = tw2(a.tw_lo, a.tw_hi, a.tw_shift, (i64)k);          /* w_4n^k */
    cplx zk = ld_cplx<false>(s + 2 * (i64)k);
    cplx zm = ld_cplx<false>(s + 2 * (i64)(km == h ? 0 : km));
    cplx E = c_make(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
    cplx D = c_make(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));
    cplx P = c_mulc(c_mni(D), wu);
    cplx yk = c_add(E, P);
    cplx ym = c_sub(E, P);
    ym.y = -ym.y;
    if (k == 0) { yk.y = 0.0; ym.y = 0.0; }
    dct2_epilogue(a, d, k, yk, wk);
    if (km != k) {
        /* w_4n^(h-k) = w_4n^(n/2) conj(w_4n^k), w_4n^(n/2) = (cos, sin)(pi/4) */
        const cplx wm = c_make(FA_SQRT1_2 * (wk.x + wk.y), FA_SQRT1_2 * (wk.x - wk.y));
        dct2_epilogue(a, d, km, ym, wm);
    }
}

/* DCT-III / DST-III (REDFT01 / RODFT01) of long contiguous rows, the transposes of the two kernels above:
   prologue + tangle: Y[idx] = conj-twiddled (x[idx], x[n-idx]) (pro_load, r2r_epi.hpp), then the c2r tangle of
   the pair (k, h-k); unshuffle: y[2j] = v[j], y[2j+1] = +-v[n-1-j], one work-item per output quad. */
FA_DEV cplx dct3_prologue(const DctFast &a, const double *s, unsigned idx, cplx w) {
    const unsigned n = a.n;
    double x, y;
    if (!a.odd) { x = s[idx]; y = idx > 0 ? s[n - idx] : 0.0; }
    else { x = s[n - 1 - idx]; y = idx > 0 ? s[idx - 1] : 0.0; }
    return c_make(x * w.x + y * w.y, x * w.y - y * w.x);
}
__global__ void __launch_bounds__(256) dct3_tangle_fast_kernel(const DctFast a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.nitems) return;
    const unsigned h = a.n / 2, km = h - k;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx wu = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 4 * (i64)k);      /* w_n^k */
    cplx wk = tw2(a.tw_lo, a.tw_hi, a.tw_shift, (i64)k);          /* w_4n^k */
    const cplx wm = c_make(FA_SQRT1_2 * (wk.x + wk.y), FA_SQRT1_2 * (wk.x - wk.y));   /* w_4n^(h-k) */
    cplx yk = dct3_prologue(a, s, k, wk);
    cplx ym = dct3_prologue(a, s, km, wm);
    if (k == 0) { yk.y = 0.0; ym.y = 0.0; }
    cplx E = c_make(yk.x + ym.x, yk.y - ym.y);
    cplx D = c_make(yk.x - ym.x, yk.y + ym.y);
    cplx iO = c_mpi(c_mul(D, wu));
    cplx zk = c_add(E, iO);
    cplx zm = c_sub(E, iO);
    zm.y = -zm.y;
    st_cplx<false>(d + 2 * (i64)k, zk);
    if (km != k && km != h) st_cplx<false>(d + 2 * (i64)km, zm);
}
template <bool NT>
__global__ void __launch_bounds__(256) dct3_unshuffle_fast_kernel(const DctFast a) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.nitems) return;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch + 4 * (i64)q;
    cplx lo = ld_cplx<false>(s + 2 * (i64)q);                          /* v[2q], v[2q+1] */
    cplx hi = ld_cplx<false>(s + ((i64)a.n - 2 - 2 * (i64)q));         /* v[n-2-2q], v[n-1-2q] */
    const double sg = a.odd ? -1.0 : 1.0;
    st_cplx<NT>(d, c_make(lo.x, sg * hi.y));
    st_cplx<NT>(d + 2, c_make(lo.y, sg * hi.x));
}

/* ------------------------------------------------------------------------ */
/* r2r pre / post processing                                                 */
/* ------------------------------------------------------------------------ */
/* One work item per index k of one transform; the flattened index runs over
   the loops in order of the user-side stride with k inserted at position kpos,
   so neighbouring work items touch neighbouring user elements whichever axis is
   transformed.  tw(m) = exp(+2 pi i m / M), M = 4n (kinds 01/10) or 8n (11).
   Index maps and their derivations: DESIGN.md section 9; the reference's loops
   with the same roles are cited at emit_r2r_axis in planner.c. */
struct R2RArgs {
    const double *src;
    double *dst;
    i64 src_im, dst_im;
    i64 is_k, os_k;
    i64 n, K;
    ElemIdx e;
    const cplx *tw_lo;
    const cplx *tw_hi;
    int tw_shift;
    int mode;
};

__global__ void __launch_bounds__(256) r2r_kernel(const R2RArgs a) {
    const i64 n = a.n;
    for (i64 vb = blockIdx.x; vb < a.e.nvb; vb += gridDim.x) {
        i64 k, soff, doff;
        if (!elem_index(a.e, vb, &k, &soff, &doff)) continue;
        const double *S = a.src + soff;
        double *D = a.dst + doff;
#define SR(j) S[(j) * a.is_k]
#define SI(j) S[(j) * a.is_k + a.src_im]
#define DR(j) D[(j) * a.os_k]
#define DI(j) D[(j) * a.os_k + a.dst_im]
/* real sequences on the scratch side are addressed as pairs: element j at
   (j >> 1) * stride + (j & 1) * im  (planner.c emit_r2r_axis) */
#define DP(j) D[((j) >> 1) * a.os_k + ((j) & 1) * a.dst_im]
#define SP(j) S[((j) >> 1) * a.is_k + ((j) & 1) * a.src_im]
        switch (a.mode) {
        case FFTW_AMD_R2R_PRE_HC2R: {
            DR(k) = SR(k);
            DI(k) = (k > 0 && 2 * k < n) ? SR(n - k) : 0.0;
            break;
        }
        case FFTW_AMD_R2R_PRE_E10:
        case FFTW_AMD_R2R_PRE_O10: {
            /* v[j] = x[2j], v[n-1-j] = x[2j+1]: one work item per input pair */
            DP(k) = SR(2 * k);
            if (2 * k + 1 < n) {
                double b = SR(2 * k + 1);
                DP(n - 1 - k) = (a.mode == FFTW_AMD_R2R_PRE_O10) ? -b : b;
            }
            break;
        }
        case FFTW_AMD_R2R_PRE_E01:
        case FFTW_AMD_R2R_PRE_O01: {
            double x, y;
            if (a.mode == FFTW_AMD_R2R_PRE_E01) { x = SR(k); y = (k > 0) ? SR(n - k) : 0.0; }
            else { x = SR(n - 1 - k); y = (k > 0) ? SR(k - 1) : 0.0; }
            cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, k);
            DR(k) = x * w.x + y * w.y;
            DI(k) = x * w.y - y * w.x;
            break;
        }
        case FFTW_AMD_R2R_PRE_E00: {
            i64 N = 2 * (n - 1);
            DP(k) = SR(k < n ? k : N - k);
            break;
        }
        case FFTW_AMD_R2R_PRE_O00: {
            i64 N = 2 * (n + 1);
            double v = 0.0;
            if (k >= 1 && k <= n) v = SR(k - 1);
            else if (k > n + 1) v = -SR(N - k - 1);
            DP(k) = v;
            break;
        }
        case FFTW_AMD_R2R_PRE_E11:
        case FFTW_AMD_R2R_PRE_O11: {
            double xr = SR(2 * k), xi = SR(n - 1 - 2 * k);
            if (a.mode == FFTW_AMD_R2R_PRE_O11) { double t = xr; xr = xi; xi = t; }
            cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 4 * k);
            DR(k) = xr * w.x + xi * w.y;
            DI(k) = xi * w.x - xr * w.y;
            break;
        }
        case FFTW_AMD_R2R_PRE_E11ODD:
        case FFTW_AMD_R2R_PRE_O11ODD: {
            double re = 0.0, im = 0.0;
            if (k < n) {
                double x = (a.mode == FFTW_AMD_R2R_PRE_E11ODD) ? SR(k) : SR(n - 1 - k);
                cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 2 * k);
                re = x * w.x;
                im = -x * w.y;
            }
            DR(k) = re;
            DI(k) = im;
            break;
        }
        case FFTW_AMD_R2R_POST_R2HC: {
            DR(k) = SR(k);
            if (k > 0 && 2 * k < n) DR(n - k) = SI(k);
            break;
        }
        case FFTW_AMD_R2R_POST_DHT: {
            double re = SR(k);
            if (k > 0 && 2 * k < n) {
                double im = SI(k);
                DR(k) = re - im;
                DR(n - k) = re + im;
            } else {
                DR(k) = re;
            }
            break;
        }
        case FFTW_AMD_R2R_POST_E10:
        case FFTW_AMD_R2R_POST_O10: {
            const bool rev = (a.mode == FFTW_AMD_R2R_POST_O10);
            double vr = SR(k), vi = (k > 0 && 2 * k < n) ? SI(k) : 0.0;
            cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, k);
            double dr = vr * w.x + vi * w.y, di = vi * w.x - vr * w.y;
            DR(rev ? n - 1 - k : k) = 2.0 * dr;
            if (k > 0 && 2 * k < n) DR(rev ? k - 1 : n - k) = -2.0 * di;
            break;
        }
        case FFTW_AMD_R2R_POST_E01:
        case FFTW_AMD_R2R_POST_O01: {
            /* y[2j] = v[j], y[2j+1] = v[n-1-j]: one work item per output pair */
            DR(2 * k) = SP(k);
            if (2 * k + 1 < n) {
                double b = SP(n - 1 - k);
                DR(2 * k + 1) = (a.mode == FFTW_AMD_R2R_POST_O01) ? -b : b;
            }
            break;
        }
        case FFTW_AMD_R2R_POST_E00:
            DR(k) = SR(k);
            break;
        case FFTW_AMD_R2R_POST_O00:
            DR(k) = -SI(k + 1);
            break;
        case FFTW_AMD_R2R_POST_E11:
        case FFTW_AMD_R2R_POST_O11: {
            double zr = SR(k), zi = SI(k);
            cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 4 * k + 1);
            double dr = zr * w.x + zi * w.y, di = zi * w.x - zr * w.y;
            DR(2 * k) = 2.0 * dr;
            DR(n - 1 - 2 * k) = (a.mode == FFTW_AMD_R2R_POST_O11) ? 2.0 * di : -2.0 * di;
            break;
        }
        case FFTW_AMD_R2R_POST_E11ODD:
        case FFTW_AMD_R2R_POST_O11ODD: {
            double zr = SR(k), zi = SI(k);
            cplx w = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 2 * k + 1);
            double y = 2.0 * (zr * w.x + zi * w.y);
            if (a.mode == FFTW_AMD_R2R_POST_O11ODD && (k & 1)) y = -y;
            DR(k) = y;
            break;
        }
        default:
            break;
        }
#undef SR
#undef SI
#undef DR
#undef DI
#undef DP
#undef SP
    }
}

/* ------------------------------------------------------------------------ */
/* radix-4 r2c untangle / c2r tangle                                         */
/* ------------------------------------------------------------------------ */
/* n = 4m.  z_v[j] = x[4j+2v] + i x[4j+2v+1] (v = 0,1), Z_v = DFT_m(z_v) stored
   as [v][m].  With X_s = DFT_m(x[4j+s]):  X_{2v} = (Z_v[k] + conj Z_v[m-k]) / 2,
   X_{2v+1} = -i (Z_v[k] - conj Z_v[m-k]) / 2, T_s = w_n^(sk) X_s, and
       Y[k]    = T0 + T1 + T2 + T3        Y[k+m]  = T0 - iT1 - T2 + iT3
       Y[2m-k] = conj(T0 - T1 + T2 - T3)  Y[m-k]  = conj(T0 + iT1 - T2 - iT3)
   This is the reference's rdft2-ct-dit/4 step with the hc2cfdft_4 codelet
   (fftw/fftw_api.c:5579-5590, fftw/rdft_scalar/r2cf/hc2cfdft_4.c:135-212), the
   plan it picks for n = 2^22. */
struct Real4Args {
    const double *src;   /* Z: element k of vector v at src + v*vs + k*is_k */
    double *dst;
    i64 src_im, dst_im;
    i64 is_k, vs, os_k;
    i64 m, npair;
    ElemIdx e;
    const cplx *tw_lo;
    const cplx *tw_hi;
    int tw_shift;
    int flags;
    int r2r, twmul;      /* as in RealArgs */
    i64 rn;
};

__global__ void __launch_bounds__(256) r2c_post4_kernel(const Real4Args a) {
    for (i64 vb = blockIdx.x; vb < a.e.nvb; vb += gridDim.x) {
        i64 k, soff, doff;
        if (!elem_index(a.e, vb, &k, &soff, &doff)) continue;
        const i64 m = a.m, km = (k == 0) ? 0 : m - k;
        cplx T[4];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            cplx zk = load_elem<false>(a.src, soff + v * a.vs + k * a.is_k, a.src_im, 0);
            cplx zm = load_elem<false>(a.src, soff + v * a.vs + km * a.is_k, a.src_im, 0);
            cplx E = c_make(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
            cplx D = c_make(0.5 * (zk.x - zm.x), 0.5 * (zk.y + zm.y));
            T[2 * v] = E;
            T[2 * v + 1] = c_mni(D);
        }
        T[1] = c_mulc(T[1], tw2(a.tw_lo, a.tw_hi, a.tw_shift, k * a.twmul));
        T[2] = c_mulc(T[2], tw2(a.tw_lo, a.tw_hi, a.tw_shift, 2 * k * a.twmul));
        T[3] = c_mulc(T[3], tw2(a.tw_lo, a.tw_hi, a.tw_shift, 3 * k * a.twmul));
        cplx s02 = c_add(T[0], T[2]), d02 = c_sub(T[0], T[2]);
        cplx s13 = c_add(T[1], T[3]), d13 = c_sub(T[1], T[3]);
        cplx y0 = c_add(s02, s13);                 /* Y[k]       */
        cplx y1 = c_add(d02, c_mni(d13));          /* Y[k+m]     */
        cplx y2 = c_sub(s02, s13);  y2.y = -y2.y;  /* Y[2m-k]    */
        cplx y3 = c_add(d02, c_mpi(d13)); y3.y = -y3.y;   /* Y[m-k] */
        if (k == 0) { y0.y = 0.0; y2.y = 0.0; }
        epi_store(a, doff, k, y0);
        epi_store(a, doff, k + m, y1);
        epi_store(a, doff, 2 * m - k, y2);
        if (k != 0 && 2 * k != m) epi_store(a, doff, m - k, y3);
    }
}

/* The same butterfly for the layout the large 1-D plans produce -- Z_0[k], Z_1[k] side by side
   (32 contiguous bytes per k), interleaved complex output, no r2r epilogue, one loop dim (the
   batch): 16-byte accesses, 32-bit index arithmetic, one work-item per pair (k, m-k), w^2k and
   w^3k from w^k instead of four more table loads.  Pure streaming: 4 x 16 B in, 4 x 16 B out. */
struct Real4Fast {
    const double *src;
    double *dst;
    i64 sbatch, dbatch;   /* distance between transforms, in doubles */
    unsigned m, npair;
    const cplx *tw_lo;
    const cplx *tw_hi;
    int tw_shift;
};

template <bool NT>
__global__ void __launch_bounds__(256) r2c_post4_fast_kernel(const Real4Fast a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.npair) return;
    const unsigned m = a.m, km = k ? m - k : 0;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx w1 = tw2(a.tw_lo, a.tw_hi, a.tw_shift, (i64)k);
    cplx zk0 = ld_cplx<false>(s + 4 * (i64)k), zk1 = ld_cplx<false>(s + 4 * (i64)k + 2);
    cplx zm0 = ld_cplx<false>(s + 4 * (i64)km), zm1 = ld_cplx<false>(s + 4 * (i64)km + 2);
    cplx T0 = c_make(0.5 * (zk0.x + zm0.x), 0.5 * (zk0.y - zm0.y));
    cplx T1 = c_mni(c_make(0.5 * (zk0.x - zm0.x), 0.5 * (zk0.y + zm0.y)));
    cplx T2 = c_make(0.5 * (zk1.x + zm1.x), 0.5 * (zk1.y - zm1.y));
    cplx T3 = c_mni(c_make(0.5 * (zk1.x - zm1.x), 0.5 * (zk1.y + zm1.y)));
    cplx w2 = c_mul(w1, w1), w3 = c_mul(w2, w1);
    T1 = c_mulc(T1, w1);
    T2 = c_mulc(T2, w2);
    T3 = c_mulc(T3, w3);
    cplx s02 = c_add(T0, T2), d02 = c_sub(T0, T2);
    cplx s13 = c_add(T1, T3), d13 = c_sub(T1, T3);
    cplx y0 = c_add(s02, s13);                 /* Y[k]       */
    cplx y1 = c_add(d02, c_mni(d13));          /* Y[k+m]     */
    cplx y2 = c_sub(s02, s13);  y2.y = -y2.y;  /* Y[2m-k]    */
    cplx y3 = c_add(d02, c_mpi(d13)); y3.y = -y3.y;   /* Y[m-k] */
    if (k == 0) { y0.y = 0.0; y2.y = 0.0; }
    st_cplx<NT>(d + 2 * (i64)k, y0);
    st_cplx<NT>(d + 2 * ((i64)k + m), y1);
    st_cplx<NT>(d + 2 * (2 * (i64)m - k), y2);
    if (k != 0 && 2 * k != m) st_cplx<NT>(d + 2 * ((i64)m - k), y3);
}

/* c2r: with A = Y[k], B = Y[k+m], C = conj Y[2m-k], D = conj Y[m-k]:
       S0 = A+B+C+D, S1 = A+iB-C-iD, S2 = A-B+C-D, S3 = A-iB-C+iD,
       X'_s = w_n^(-sk) S_s,  Z'_0[k] = X'_0 + i X'_1,  Z'_1[k] = X'_2 + i X'_3;
   the mirror index m-k uses the same four loads with conjugated roles. */
FA_DEV void c2r4_combine(cplx A, cplx B, cplx C, cplx D, cplx w1, cplx w2, cplx w3, cplx *z0, cplx *z1) {
    cplx sAC = c_add(A, C), dAC = c_sub(A, C), sBD = c_add(B, D), dBD = c_sub(B, D);
    cplx S0 = c_add(sAC, sBD);
    cplx S1 = c_add(dAC, c_mpi(dBD));
    cplx S2 = c_sub(sAC, sBD);
    cplx S3 = c_add(dAC, c_mni(dBD));
    cplx X1 = c_mul(S1, w1), X2 = c_mul(S2, w2), X3 = c_mul(S3, w3);
    *z0 = c_add(S0, c_mpi(X1));
    *z1 = c_add(X2, c_mpi(X3));
}

__global__ void __launch_bounds__(256) c2r_pre4_kernel(const Real4Args a) {
    for (i64 vb = blockIdx.x; vb < a.e.nvb; vb += gridDim.x) {
        i64 k, soff, doff;
        if (!elem_index(a.e, vb, &k, &soff, &doff)) continue;
        const i64 m = a.m;
        /* the four half-spectrum entries this pair needs (src here is Y, is_k its stride) */
        cplx Yk = pro_load(a, soff, k);
        cplx Ykm = pro_load(a, soff, k + m);
        cplx Y2 = pro_load(a, soff, 2 * m - k);
        cplx Y1 = pro_load(a, soff, m - k);
        if (k == 0) { Yk.y = 0.0; Y2.y = 0.0; }      /* Im Y[0], Im Y[n/2] are ignored */
        cplx w1 = tw2(a.tw_lo, a.tw_hi, a.tw_shift, k * a.twmul);
        cplx w2 = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 2 * k * a.twmul);
        cplx w3 = tw2(a.tw_lo, a.tw_hi, a.tw_shift, 3 * k * a.twmul);
        cplx z0, z1;
        c2r4_combine(Yk, Ykm, c_make(Y2.x, -Y2.y), c_make(Y1.x, -Y1.y), w1, w2, w3, &z0, &z1);
        store_elem<false>(a.dst, doff + k * a.os_k, a.dst_im, a.flags, z0);
        store_elem<false>(a.dst, doff + a.vs + k * a.os_k, a.dst_im, a.flags, z1);
        if (k != 0 && 2 * k != m) {
            /* mirror k' = m-k: A' = Y[m-k], B' = Y[2m-k], C' = conj Y[m+k], D' = conj Y[k];
               w_n^(-s(m-k)) = i^s conj(w_s) */
            cplx v1 = c_mpi(c_make(w1.x, -w1.y));
            cplx v2 = c_make(-w2.x, w2.y);
            cplx v3 = c_mni(c_make(w3.x, -w3.y));
            c2r4_combine(Y1, Y2, c_make(Ykm.x, -Ykm.y), c_make(Yk.x, -Yk.y), v1, v2, v3, &z0, &z1);
            store_elem<false>(a.dst, doff + (m - k) * a.os_k, a.dst_im, a.flags, z0);
            store_elem<false>(a.dst, doff + a.vs + (m - k) * a.os_k, a.dst_im, a.flags, z1);
        }
    }
}

/* the transpose of r2c_post4_fast_kernel: interleaved half spectrum in, Z_0[k], Z_1[k] side by side out */
template <bool NT>
__global__ void __launch_bounds__(256) c2r_pre4_fast_kernel(const Real4Fast a) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= a.npair) return;
    const unsigned m = a.m;
    const double *s = a.src + (i64)blockIdx.y * a.sbatch;
    double *d = a.dst + (i64)blockIdx.y * a.dbatch;
    cplx w1 = tw2(a.tw_lo, a.tw_hi, a.tw_shift, (i64)k);
    cplx Yk = ld_cplx<NT>(s + 2 * (i64)k), Ykm = ld_cplx<NT>(s + 2 * ((i64)k + m));
    cplx Y2 = ld_cplx<NT>(s + 2 * (2 * (i64)m - k)), Y1 = ld_cplx<NT>(s + 2 * ((i64)m - k));
    if (k == 0) { Yk.y = 0.0; Y2.y = 0.0; }
    cplx w2 = c_mul(w1, w1), w3 = c_mul(w2, w1);
    cplx z0, z1;
    c2r4_combine(Yk, Ykm, c_make(Y2.x, -Y2.y), c_make(Y1.x, -Y1.y), w1, w2, w3, &z0, &z1);
    st_cplx<false>(d + 4 * (i64)k, z0);
    st_cplx<false>(d + 4 * (i64)k + 2, z1);
    if (k != 0 && 2 * k != m) {
        cplx v1 = c_mpi(c_make(w1.x, -w1.y));
        cplx v2 = c_make(-w2.x, w2.y);
        cplx v3 = c_mni(c_make(w3.x, -w3.y));
        c2r4_combine(Y1, Y2, c_make(Ykm.x, -Ykm.y), c_make(Yk.x, -Yk.y), v1, v2, v3, &z0, &z1);
        st_cplx<false>(d + 4 * ((i64)m - k), z0);
        st_cplx<false>(d + 4 * ((i64)m - k) + 2, z1);
    }
}

/* Rader: P[k] = A[k] * Omega[k]; P[0] += x0; Y[0] = x0 + A[0]
   (reference rader_apply A.c:4218-4240) */
struct RaderArgs {
    double *work;        /* [vec][p-1] complex, contiguous */
    const double *x0;    /* [vec] complex */
    double *dst;         /* where Y[0] goes */
    i64 dst_im;
    i64 pm1, nvec, total;
    i64 dn[FFTW_AMD_MAX_DIMS], dos[FFTW_AMD_MAX_DIMS];
    const cplx *omega;
    int ndims, flags;
};

__global__ void __launch_bounds__(256) rader_mul_kernel(const RaderArgs a) {
    i64 gid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    i64 stride = (i64)gridDim.x * blockDim.x;
    for (; gid < a.total; gid += stride) {
        i64 k = gid % a.pm1;
        i64 v = gid / a.pm1;
        cplx *w = reinterpret_cast<cplx *>(a.work) + v * a.pm1;
        cplx A = w[k];
        cplx P = c_mul(A, a.omega[k]);
        if (k == 0) {
            cplx x0 = reinterpret_cast<const cplx *>(a.x0)[v];
            P = c_add(P, x0);
            i64 rest = v, doff = 0;
            for (int d = 0; d < a.ndims; ++d) {
                i64 idx = rest % a.dn[d];
                rest /= a.dn[d];
                doff += idx * a.dos[d];
            }
            store_elem<false>(a.dst, doff, a.dst_im, a.flags, c_add(x0, A));
        }
        w[k] = P;
    }
}

/* half spectrum Y[0..n/2] -> full Hermitian spectrum F[0..n-1] (odd-n c2r) */
__global__ void __launch_bounds__(256) herm_expand_kernel(const CopyArgs a) {
    for (i64 vb = blockIdx.x; vb < a.e.nvb; vb += gridDim.x) {
        i64 k, soff, doff;
        if (!elem_index(a.e, vb, &k, &soff, &doff)) continue;
        i64 half = a.K / 2;
        i64 ks = (k <= half) ? k : a.K - k;
        cplx v = load_elem<false>(a.src, soff + ks * a.is_k, a.src_im, 0);
        if (k > half) v.y = -v.y;
        if (k == 0 || (2 * k == a.K)) v.y = 0.0;
        store_elem<false>(a.dst, doff + k * a.os_k, a.dst_im, a.flags, v);
    }
}

/* ---- host side: the form of a step ------------------------------------------------------------------------ */
/* r2r length n from the inner real-DFT length N of a fused step */
static i64 r2r_len_of(int mode, i64 N) {
    if (mode == FFTW_AMD_R2R_POST_E00) return N / 2 + 1;
    if (mode == FFTW_AMD_R2R_POST_O00) return N / 2 - 1;
    return N;
}

/* The streaming-rows layout of the fast forms: the batch is the only loop and fits gridDim.y, and on each side that
   the kernel accesses 16 bytes at a time the rows start 16-byte aligned an even number of doubles apart. */
static bool streaming_rows(const fftw_amd_step_desc *d, const StepGeom &g, i64 cn, bool src_side, bool dst_side) {
    return d->ndims == 1 && d->batch_dim == 0 && d->kpos == 0 && cn > 0 && cn < 65536 &&
           (!src_side || (g.src16 && g.dis_even)) && (!dst_side || (g.dst16 && g.dos_even));
}

static const int swap_mask = FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT;
static int real2_form(const fftw_amd_step_desc *d, const StepGeom &g, i64 cn) {
    const bool r2c = d->kind == FFTW_AMD_STEP_R2C_POST;
    const int r2r = d->variant, twmul = d->tile > 0 ? d->tile : 1;
    const i64 is_k = d->is_l, os_k = d->os_l, h = d->aux_n / 2, rn = r2r_len_of(r2r, d->aux_n);
    /* the two DCT forms test one side only: their other side is a row of reals, accessed one double at a time */
    if (r2c && (r2r == FFTW_AMD_R2R_POST_E10 || r2r == FFTW_AMD_R2R_POST_O10) &&
        twmul == 4 && d->src_im == 1 && is_k == 2 && os_k == 1 && rn == 2 * h && h >= 4 && h % 2 == 0 &&
        rn < (1LL << 31) && streaming_rows(d, g, cn, true, false) &&
        !(d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_CONJ_OUT)))
        return FA_ELEM_POST2_DCT;
    if (!r2c && (r2r == FFTW_AMD_R2R_PRE_E01 || r2r == FFTW_AMD_R2R_PRE_O01) &&
        twmul == 4 && d->dst_im == 1 && os_k == 2 && is_k == 1 && rn == 2 * h && h >= 4 && h % 2 == 0 &&
        rn < (1LL << 31) && streaming_rows(d, g, cn, false, true) &&
        !(d->flags & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_CONJ_OUT | FFTW_AMD_F_REAL_OUT)))
        return FA_ELEM_PRE2_DCT;
    if (r2r == 0 && twmul == 1 && d->src_im == 1 && d->dst_im == 1 && is_k == 2 && os_k == 2 &&
        !(d->flags & swap_mask) && h >= 2 && h < (1LL << 30) && streaming_rows(d, g, cn, true, true))
        return r2c ? FA_ELEM_POST2_FAST : FA_ELEM_PRE2_FAST;
    return r2c ? FA_ELEM_POST2 : FA_ELEM_PRE2;
}

static int real4_form(const fftw_amd_step_desc *d, const StepGeom &g, i64 cn) {
    const bool r2c = d->kind == FFTW_AMD_STEP_R2C_POST4;
    const int r2r = d->variant, twmul = d->tile > 0 ? d->tile : 1;
    const i64 zs = r2c ? d->is_l : d->os_l, ys = r2c ? d->os_l : d->is_l;   /* Z side / Y side strides */
    const i64 vs = d->aux_valid, m = d->aux_n / 4;
    if (r2r == 0 && twmul == 1 && d->src_im == 1 && d->dst_im == 1 && zs == 4 && ys == 2 && vs == 2 &&
        !(d->flags & swap_mask) && m >= 2 && m < (1LL << 30) && streaming_rows(d, g, cn, true, true))
        return r2c ? FA_ELEM_POST4_FAST : FA_ELEM_PRE4_FAST;
    return r2c ? FA_ELEM_POST4 : FA_ELEM_PRE4;
}

static int r2r_form(const fftw_amd_step_desc *d, const StepGeom &g, i64 cn) {
    const int mode = d->variant;
    const i64 is_k = d->is_l, os_k = d->os_l, n = d->aux_n;
    if ((mode == FFTW_AMD_R2R_PRE_E10 || mode == FFTW_AMD_R2R_PRE_O10) && is_k == 1 && os_k == 2 &&
        d->dst_im == 1 && n >= 8 && n % 4 == 0 && n < (1LL << 31) && streaming_rows(d, g, cn, true, true))
        return FA_ELEM_R2R_SHUFFLE;
    if ((mode == FFTW_AMD_R2R_POST_E01 || mode == FFTW_AMD_R2R_POST_O01) && is_k == 2 && d->src_im == 1 &&
        os_k == 1 && n >= 8 && n % 4 == 0 && n < (1LL << 31) && streaming_rows(d, g, cn, true, true))
        return FA_ELEM_R2R_UNSHUFFLE;
    return FA_ELEM_R2R;
}

/* g: fa_step_geom of the chunk, of which src16, dst16, dis_even and dos_even are read */
static int elem_form(const fftw_amd_step_desc *d, const StepGeom &g, i64 cn) {
    switch (d->kind) {
    case FFTW_AMD_STEP_COPY:
        if (d->variant == FFTW_AMD_K_TRANSPOSE) return FA_ELEM_TRANSPOSE;
        return (d->flags & (FFTW_AMD_F_PERM_SRC | FFTW_AMD_F_PERM_DST)) ? FA_ELEM_COPY_1 : FA_ELEM_COPY_4;
    case FFTW_AMD_STEP_HERM_EXPAND: return FA_ELEM_HERM;
    case FFTW_AMD_STEP_R2C_POST:
    case FFTW_AMD_STEP_C2R_PRE:     return real2_form(d, g, cn);
    case FFTW_AMD_STEP_R2C_POST4:
    case FFTW_AMD_STEP_C2R_PRE4:    return real4_form(d, g, cn);
    case FFTW_AMD_STEP_R2R:         return r2r_form(d, g, cn);
    case FFTW_AMD_STEP_RADER_MUL:   return FA_ELEM_RADER_MUL;
    default:                        return FA_ELEM_NONE;
    }
}

extern "C" int fa_hip_elem_form(const fftw_amd_step_desc *d, int src_mis, int dst_mis, long long cn) {
    StepGeom g = {};                                /* the forms read these four fields only */
    g.src16 = src_mis % 16 == 0; g.dst16 = dst_mis % 16 == 0;
    g.dis_even = g.dos_even = true;
    for (int i = 0; i < d->ndims; ++i) { if (d->dim_is[i] % 2) g.dis_even = false; if (d->dim_os[i] % 2) g.dos_even = false; }
    return elem_form(d, g, cn);
}

/* ---- host side: argument fillers and the launchers ------------------------------------------------------------ */
#define FA_LAUNCH_NT(K, nt, grid, st, a)                                                                      \
    do { if (nt) hipLaunchKernelGGL(K<true>, grid, dim3(256), 0, st, a);                                      \
         else hipLaunchKernelGGL(K<false>, grid, dim3(256), 0, st, a); } while (0)

/* index space of an element-wise step (ElemIdx): the dims of the chunk, the transform index of extent K at position kpos.
   Returns 0 when there is nothing to do.  If the inner part would not fit 32 bits the transform index simply goes first. */
static int elem_fill(ElemIdx *e, const fftw_amd_step_desc *d, const StepGeom &g, i64 K, int kpos, dim3 *grid) {
    const int bd = d->batch_dim;
    for (int i = 0; i < FFTW_AMD_MAX_DIMS; ++i) { e->dn[i] = g.dn[i]; e->dis[i] = g.dis[i]; e->dos[i] = g.dos[i]; }
    e->ndims = g.ndims;
    if (kpos < 0) kpos = 0;
    if (kpos > g.ndims) kpos = g.ndims;
    if (bd >= 0 && kpos > bd) kpos = bd;          /* the batch loop stays outside */
    for (;;) {
        unsigned long long inner = (unsigned long long)K;
        bool ok = K > 0 && K < 0x7fffffffLL;
        for (int i = 0; i < kpos && ok; ++i) {
            if (e->dn[i] <= 0 || e->dn[i] >= 0x7fffffffLL) { ok = false; break; }
            inner *= (unsigned long long)e->dn[i];
            if (inner >= 0xffffff00ULL) ok = false;
        }
        if (ok) { e->inner = (unsigned)inner; break; }
        if (kpos == 0) return 0;                  /* K itself out of range: nothing sane to launch */
        kpos = 0;
    }
    e->kpos = kpos;
    e->K = (unsigned)K;
    e->nblk = (e->inner + 255u) / 256u;
    i64 nvb = e->nblk;
    for (int i = kpos; i < g.ndims; ++i) {
        if (e->dn[i] <= 0) return 0;
        nvb *= e->dn[i];
    }
    e->nvb = nvb;
    i64 blocks = nvb;
    if (blocks > 256 * 64) blocks = 256 * 64;     /* the kernels loop over virtual blocks beyond that */
    *grid = dim3((unsigned)blocks, 1, 1);
    return nvb > 0;
}

/* what the general kernels' arguments share: addresses and strides of the transform index; the twiddle tables */
template <class A> static void io_fill(A *a, const fftw_amd_step_desc *d, const StepGeom &g) {
    a->src = g.src; a->dst = g.dst;
    a->src_im = d->src_im; a->dst_im = d->dst_im;
    a->is_k = d->is_l; a->os_k = d->os_l;
}
template <class A> static void tw_fill(A *a, const fftw_amd_step_desc *d, void *const *tables) {
    a->tw_lo = (tables && d->tw_lo >= 0) ? (const cplx *)tables[d->tw_lo] : NULL;
    a->tw_hi = (tables && d->tw_hi >= 0) ? (const cplx *)tables[d->tw_hi] : NULL;
    a->tw_shift = tables ? d->tw_shift : 0;
}
/* RealArgs / Real4Args */
template <class A> static void real_fill(A *ra, const fftw_amd_step_desc *d, const StepGeom &g, void *const *tables, i64 npair) {
    io_fill(ra, d, g);
    tw_fill(ra, d, tables);
    ra->npair = npair;
    ra->r2r = d->variant;
    ra->twmul = d->tile > 0 ? d->tile : 1;
    ra->rn = r2r_len_of(d->variant, d->aux_n);
    ra->flags = d->flags;
}
/* what the streaming forms' arguments share (streaming_rows holds), and their grid: nitems work-items per row */
template <class F> static dim3 fast_fill(F *f, const fftw_amd_step_desc *d, const StepGeom &g, void *const *tables, i64 nitems) {
    f->src = g.src; f->dst = g.dst; f->sbatch = g.dis[0]; f->dbatch = g.dos[0];
    tw_fill(f, d, tables);
    return dim3((unsigned)((nitems + 255) / 256), (unsigned)g.dn[0], 1);
}
/* arguments and grid of the four DCT streaming forms: rows of n reals, nitems work-items each, odd = the RODFT twin
   of the form's mode; tables == NULL for the two shuffles, which use no twiddles */
static dim3 dct_fast_fill(DctFast *f, const fftw_amd_step_desc *d, const StepGeom &g, void *const *tables, i64 n, i64 nitems, int odd_mode) {
    f->n = (unsigned)n; f->nitems = (unsigned)nitems;
    f->odd = d->variant == odd_mode;
    return fast_fill(f, d, g, tables, nitems);
}

int fa_launch_copy(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st) {
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    const int form = elem_form(d, g, cn);
    if (form == FA_ELEM_TRANSPOSE) {
        /* no other executor: a transposition step the tile kernels cannot take is an internal error */
        if (!fa_launch_transpose(d, bufs, cs, cn, st)) return 0;
        fprintf(stderr, "fftw3_amd: internal error: transposition step in an unsupported layout\n");
        return -1;
    }
    CopyArgs ca;
    dim3 grid;
    io_fill(&ca, d, g);
    ca.K = d->aux_n; ca.Kvalid = d->aux_valid;
    ca.flags = d->flags;
    ca.tab = (d->table >= 0) ? (const cplx *)tables[d->table] : NULL;
    ca.perm = (d->table2 >= 0) ? (const i64 *)tables[d->table2] : NULL;
    if (!elem_fill(&ca.e, d, g, d->aux_n, 0, &grid)) return 0;
    if (form == FA_ELEM_HERM) {
        hipLaunchKernelGGL(herm_expand_kernel, grid, dim3(256), 0, st, ca);
    } else if (form == FA_ELEM_COPY_1) {
        if (grid.x >= 8) grid.x &= ~7u;          /* rows stay on one XCD: a grid of whole rounds of the eight */
        hipLaunchKernelGGL(copy_kernel<1>, grid, dim3(256), 0, st, ca);
    } else {
        const i64 ngroups = (ca.e.nvb + 3) / 4;
        if ((i64)grid.x > ngroups) grid.x = (unsigned)ngroups;
        hipLaunchKernelGGL(copy_kernel<4>, grid, dim3(256), 0, st, ca);
    }
    return 0;
}

int fa_launch_real2(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st) {
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    const int form = elem_form(d, g, cn);
    const i64 h = d->aux_n / 2, npair = h / 2 + 1;
    if (form == FA_ELEM_POST2_DCT) {     /* DCT-II / DST-II: streaming untangle + epilogue */
        DctFast f;
        const dim3 grid = dct_fast_fill(&f, d, g, tables, 2 * h, npair, FFTW_AMD_R2R_POST_O10);
        hipLaunchKernelGGL(dct2_untangle_fast_kernel, grid, dim3(256), 0, st, f);
        return 0;
    }
    if (form == FA_ELEM_PRE2_DCT) {      /* DCT-III / DST-III: streaming prologue + tangle */
        DctFast f;
        const dim3 grid = dct_fast_fill(&f, d, g, tables, 2 * h, npair, FFTW_AMD_R2R_PRE_O01);
        hipLaunchKernelGGL(dct3_tangle_fast_kernel, grid, dim3(256), 0, st, f);
        return 0;
    }
    if (form == FA_ELEM_POST2_FAST || form == FA_ELEM_PRE2_FAST) {   /* the layout of the large 1-D plans (see r2c_post_fast_kernel) */
        Real2Fast f;
        const dim3 grid = fast_fill(&f, d, g, tables, npair);
        f.h = (unsigned)h; f.npair = (unsigned)npair;
        if (form == FA_ELEM_POST2_FAST) FA_LAUNCH_NT(r2c_post_fast_kernel, d->flags & FFTW_AMD_F_NT_OUT, grid, st, f);
        else FA_LAUNCH_NT(c2r_pre_fast_kernel, d->flags & FFTW_AMD_F_NT_IN, grid, st, f);
        return 0;
    }
    RealArgs ra;
    dim3 grid;
    real_fill(&ra, d, g, tables, npair);
    ra.h = h;
    if (!elem_fill(&ra.e, d, g, npair, d->kpos, &grid)) return 0;
    if (form == FA_ELEM_POST2) hipLaunchKernelGGL(r2c_post_kernel, grid, dim3(256), 0, st, ra);
    else hipLaunchKernelGGL(c2r_pre_kernel, grid, dim3(256), 0, st, ra);
    return 0;
}

int fa_launch_real4(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st) {
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    const int form = elem_form(d, g, cn);
    const i64 m = d->aux_n / 4, npair = m / 2 + 1;
    if (form == FA_ELEM_POST4_FAST || form == FA_ELEM_PRE4_FAST) {   /* the layout of the large 1-D plans (see r2c_post4_fast_kernel) */
        Real4Fast f;
        const dim3 grid = fast_fill(&f, d, g, tables, npair);
        f.m = (unsigned)m; f.npair = (unsigned)npair;
        if (form == FA_ELEM_POST4_FAST) FA_LAUNCH_NT(r2c_post4_fast_kernel, d->flags & FFTW_AMD_F_NT_OUT, grid, st, f);
        else FA_LAUNCH_NT(c2r_pre4_fast_kernel, d->flags & FFTW_AMD_F_NT_IN, grid, st, f);
        return 0;
    }
    Real4Args ra;
    dim3 grid;
    real_fill(&ra, d, g, tables, npair);
    ra.vs = d->aux_valid;            /* distance between the two quarter-length vectors */
    ra.m = m;
    if (!elem_fill(&ra.e, d, g, npair, d->kpos, &grid)) return 0;
    if (form == FA_ELEM_POST4) hipLaunchKernelGGL(r2c_post4_kernel, grid, dim3(256), 0, st, ra);
    else hipLaunchKernelGGL(c2r_pre4_kernel, grid, dim3(256), 0, st, ra);
    return 0;
}

int fa_launch_r2r(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st) {
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    const int form = elem_form(d, g, cn);
    if (form == FA_ELEM_R2R_SHUFFLE || form == FA_ELEM_R2R_UNSHUFFLE) {
        DctFast f;
        const dim3 grid = dct_fast_fill(&f, d, g, NULL, d->aux_n, d->aux_n / 4,
                                        form == FA_ELEM_R2R_SHUFFLE ? FFTW_AMD_R2R_PRE_O10 : FFTW_AMD_R2R_POST_O01);
        if (form == FA_ELEM_R2R_SHUFFLE) FA_LAUNCH_NT(dct2_shuffle_fast_kernel, d->flags & FFTW_AMD_F_NT_IN, grid, st, f);
        else FA_LAUNCH_NT(dct3_unshuffle_fast_kernel, d->flags & FFTW_AMD_F_NT_OUT, grid, st, f);
        return 0;
    }
    R2RArgs ra;
    dim3 grid;
    io_fill(&ra, d, g);
    tw_fill(&ra, d, tables);
    ra.n = d->aux_n; ra.K = d->aux_valid;
    ra.mode = d->variant;
    if (!elem_fill(&ra.e, d, g, ra.K, d->kpos, &grid)) return 0;
    hipLaunchKernelGGL(r2r_kernel, grid, dim3(256), 0, st, ra);
    return 0;
}

/* work is deliberately NOT advanced by the chunk (scratch is reused per chunk), so g.src is not what it wants: work
   and x0 keep their own base arithmetic; Y[0] goes to g.dst over the loop dims g.dn / g.dos */
int fa_launch_rader_mul(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st) {
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    RaderArgs ra;
    i64 nvec = 1;
    for (int i = 0; i < FFTW_AMD_MAX_DIMS; ++i) { ra.dn[i] = g.dn[i]; ra.dos[i] = g.dos[i]; }
    for (int i = 0; i < d->ndims; ++i) nvec *= ra.dn[i];
    ra.work = bufs[d->src_buf] + d->src_base;
    ra.x0 = bufs[d->aux_buf] + d->aux_base;
    ra.dst = g.dst;
    ra.dst_im = d->dst_im;
    ra.pm1 = d->aux_n;
    ra.nvec = nvec; ra.total = nvec * ra.pm1;
    ra.omega = (const cplx *)tables[d->table];
    ra.ndims = d->ndims; ra.flags = d->flags;
    if (ra.total <= 0) return 0;
    i64 blocks = (ra.total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;    /* grid-stride beyond that */
    hipLaunchKernelGGL(rader_mul_kernel, dim3((unsigned)blocks, 1, 1), dim3(256), 0, st, ra);
    return 0;
}
