/*
 * kernels.hip -- the generic LDS pass kernels, the launchers of the 1024-point register pass and the step dispatcher
 * (element-wise steps: kernels_elem.hip; runtime wrappers: fa_hip.hip).  No rocFFT/hipFFT, no MFMA: batched FFT
 * passes are HBM-bound vector-FMA work.  What the kernel replaces in the reference (fftw/fftw_api.c, "A.c"):
 *   pass_generic_kernel  <- the leaf executors and the Cooley-Tukey twiddle
 *       step: vrank_geq1_apply A.c:4627, ct_apply_dit A.c:2078, direct_apply
 *       A.c:3182, dftw_direct_apply A.c:2315, dftw_generic A.c:2730-2903 and
 *       the large-radix dftw_genericbuf A.c:2905-3109 (two-level twiddles,
 *       A.c:18920-18941), with the n1/t1 codelets replaced by butterflies.h.
 */
#include <string.h>
#include "common.hpp"

#include "pass1024.hpp"
#include "launch.hpp"

/* ------------------------------------------------------------------------ */
/* generic LDS pass kernel (runtime radices)                                 */
/* ------------------------------------------------------------------------ */

struct PassArgs {
    const double *src;
    double *dst;
    i64 src_im, dst_im;
    i64 is_l, os_l;
    i64 dn[FFTW_AMD_MAX_DIMS], dis[FFTW_AMD_MAX_DIMS], dos[FFTW_AMD_MAX_DIMS], dtw[FFTW_AMD_MAX_DIMS];
    const cplx *wL;
    const cplx *tw_lo;
    const cplx *tw_hi;
    i64 tw_n;
    i64 ntiles;
    int tw_shift;
    int L, nrad;
    int rad[FFTW_AMD_MAX_RADICES];
    int ndims, T, ld, flags;
    int in_t_fast, out_t_fast;
    int lo_n;              /* inner tile component (1: none); T counts lo_n * hi entries */
    i64 lo_is, lo_os;
};

template <int R>
FA_DEV void stockham_stage(const cplx *A, cplx *B, const cplx *wL, int L, int ld, int Tcur,
                           int Ns, int tid, int nth) {
    const int m = L / R;
    const int nb = m * Tcur;
    const int twstep = L / (Ns * R);
    for (int b = tid; b < nb; b += nth) {
        int j = b / Tcur, t = b - j * Tcur;
        int k = j % Ns;
        cplx x[R];
#pragma unroll
        for (int i = 0; i < R; ++i) x[i] = A[(j + i * m) * ld + t];
        if (Ns > 1) {
#pragma unroll
            for (int i = 1; i < R; ++i) x[i] = c_mulc(x[i], wL[i * k * twstep]);
        }
        Bfly<R>::run(x);
        int o = (j - k) * R + k;
#pragma unroll
        for (int q = 0; q < R; ++q) B[(o + q * Ns) * ld + t] = x[q];
    }
}

/* any prime radix p: O(p^2) DFT straight out of LDS (reference generic_apply,
   A.c:3428-3448, plays this role for primes without a codelet) */
FA_DEV void stockham_stage_prime(const cplx *A, cplx *B, const cplx *wL, int L, int ld, int Tcur,
                                 int Ns, int p, int tid, int nth) {
    const int m = L / p;
    const int nb = m * Tcur;
    const int twstep = L / (Ns * p);
    const int pstep = L / p;
    for (int b = tid; b < nb; b += nth) {
        int j = b / Tcur, t = b - j * Tcur;
        int k = j % Ns;
        int o = (j - k) * p + k;
        for (int q = 0; q < p; ++q) {
            cplx acc = c_make(0.0, 0.0);
            int iq = 0;
            for (int i = 0; i < p; ++i) {
                cplx xi = A[(j + i * m) * ld + t];
                if (Ns > 1) xi = c_mulc(xi, wL[i * k * twstep]);
                xi = c_mulc(xi, wL[iq * pstep]);
                acc = c_add(acc, xi);
                iq += q;
                if (iq >= p) iq -= p;
            }
            B[(o + q * Ns) * ld + t] = acc;
        }
    }
}

template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256)
pass_generic_kernel(const PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fa_lds_raw[];
    cplx *A = reinterpret_cast<cplx *>(fa_lds_raw);
    cplx *B = A + (size_t)a.L * a.ld;

    const int tid = threadIdx.x, nth = blockDim.x;
    i64 blk = (i64)blockIdx.x + (i64)blockIdx.y * gridDim.x;
    i64 tile = blk % a.ntiles;
    i64 rest = blk / a.ntiles;
    i64 soff = 0, doff = 0, twb = 0;
    for (int d = 1; d < a.ndims; ++d) {
        i64 idx = rest % a.dn[d];
        rest /= a.dn[d];
        soff += idx * a.dis[d];
        doff += idx * a.dos[d];
        twb += idx * a.dtw[d];
    }
    const int Thi = a.T / a.lo_n;
    const i64 t0 = tile * Thi;
    const int Tcur = (int)((a.dn[0] - t0 < Thi) ? (a.dn[0] - t0) : Thi) * a.lo_n;
    const int L = a.L, ld = a.ld;
    const int total = L * Tcur;
    const bool tw_in = a.tw_n && (a.flags & FFTW_AMD_F_TW_IN);

    /* ---- load tile into LDS, coalesced along whichever index is contiguous */
    for (int e = tid; e < total; e += nth) {
        int l, t;
        if (a.in_t_fast) { l = e / Tcur; t = e - l * Tcur; }
        else             { t = e / L;    l = e - t * L; }
        const int thi = t / a.lo_n, tlo = t - thi * a.lo_n;
        i64 addr = soff + (i64)l * a.is_l + (t0 + thi) * a.dis[0] + tlo * a.lo_is;
        cplx v = load_elem<VIN>(a.src, addr, a.src_im, a.flags);
        if (tw_in) {
            i64 m = (i64)l * (twb + (t0 + thi) * a.dtw[0]);
            v = c_mulc(v, tw2(a.tw_lo, a.tw_hi, a.tw_shift, m));
        }
        A[l * ld + t] = v;
    }
    __syncthreads();

    /* ---- Stockham autosort stages, ping-pong between the two LDS images */
    int Ns = 1;
    for (int s = 0; s < a.nrad; ++s) {
        const int r = a.rad[s];
        switch (r) {
        case 2:  stockham_stage<2>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 3:  stockham_stage<3>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 4:  stockham_stage<4>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 5:  stockham_stage<5>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 7:  stockham_stage<7>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 8:  stockham_stage<8>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 11: stockham_stage<11>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 13: stockham_stage<13>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        case 16: stockham_stage<16>(A, B, a.wL, L, ld, Tcur, Ns, tid, nth); break;
        default: stockham_stage_prime(A, B, a.wL, L, ld, Tcur, Ns, r, tid, nth); break;
        }
        Ns *= r;
        cplx *tmp = A; A = B; B = tmp;
        __syncthreads();
    }

    /* ---- inter-pass twiddle (conj: forward) and store */
    for (int e = tid; e < total; e += nth) {
        int l, t;
        if (a.out_t_fast) { l = e / Tcur; t = e - l * Tcur; }
        else              { t = e / L;    l = e - t * L; }
        cplx v = A[l * ld + t];
        const int thi = t / a.lo_n, tlo = t - thi * a.lo_n;
        if (a.tw_n && !tw_in) {
            i64 m = (i64)l * (twb + (t0 + thi) * a.dtw[0]);
            v = c_mulc(v, tw2(a.tw_lo, a.tw_hi, a.tw_shift, m));
        }
        i64 addr = doff + (i64)l * a.os_l + (t0 + thi) * a.dos[0] + tlo * a.lo_os;
        store_elem<VOUT>(a.dst, addr, a.dst_im, a.flags, v);
    }
}

/* ------------------------------------------------------------------------ */
/* generic LDS pass kernel, in-place form: ONE LDS image (64 KiB for a        */
/* 4096-element tile) so that two workgroups share a CU.  A stage reads all  */
/* of an item's butterflies into registers, synchronises, and writes them    */
/* back to their autosort positions.  Radices with a register butterfly only */
/* (2,3,4,5,7,8,11,13,16); tiles with a larger prime stage use the ping-pong */
/* kernel above.                                                             */
/* ------------------------------------------------------------------------ */
template <int R>
FA_DEV void inplace_stage(cplx *A, const cplx *wL, int L, int ld, int Tcur, int Ns, int tid) {
    constexpr int NB = (4096 / R + 255) / 256;      /* butterflies per item, worst case */
    const int m = L / R;
    const int nb = m * Tcur;
    const int twstep = L / (Ns * R);
    cplx x[NB][R];
    int pos[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int b = u * 256 + tid;
        pos[u] = -1;
        if (b < nb) {
            int j = b / Tcur, t = b - j * Tcur;
            int k = j % Ns;
#pragma unroll
            for (int i = 0; i < R; ++i) x[u][i] = A[(j + i * m) * ld + t];
            if (Ns > 1) {
#pragma unroll
                for (int i = 1; i < R; ++i) x[u][i] = c_mulc(x[u][i], wL[i * k * twstep]);
            }
            Bfly<R>::run(x[u]);
            pos[u] = ((j - k) * R + k) * ld + t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (pos[u] >= 0) {
#pragma unroll
            for (int q = 0; q < R; ++q) A[pos[u] + q * Ns * ld] = x[u][q];
        }
    }
    __syncthreads();
}

template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256, 2)
pass_inplace_kernel(const PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fa_lds_raw[];
    cplx *A = reinterpret_cast<cplx *>(fa_lds_raw);
    const int tid = threadIdx.x, nth = blockDim.x;
    i64 blk = (i64)blockIdx.x + (i64)blockIdx.y * gridDim.x;
    i64 tile = blk % a.ntiles;
    i64 rest = blk / a.ntiles;
    i64 soff = 0, doff = 0, twb = 0;
    for (int d = 1; d < a.ndims; ++d) {
        i64 idx = rest % a.dn[d];
        rest /= a.dn[d];
        soff += idx * a.dis[d];
        doff += idx * a.dos[d];
        twb += idx * a.dtw[d];
    }
    const int Thi = a.T / a.lo_n;
    const i64 t0 = tile * Thi;
    const int Tcur = (int)((a.dn[0] - t0 < Thi) ? (a.dn[0] - t0) : Thi) * a.lo_n;
    const int L = a.L, ld = a.ld;
    const int total = L * Tcur;
    const bool tw_in = a.tw_n && (a.flags & FFTW_AMD_F_TW_IN);

    for (int e = tid; e < total; e += nth) {
        int l, t;
        if (a.in_t_fast) { l = e / Tcur; t = e - l * Tcur; }
        else             { t = e / L;    l = e - t * L; }
        const int thi = t / a.lo_n, tlo = t - thi * a.lo_n;
        i64 addr = soff + (i64)l * a.is_l + (t0 + thi) * a.dis[0] + tlo * a.lo_is;
        cplx v = load_elem<VIN>(a.src, addr, a.src_im, a.flags);
        if (tw_in) {
            i64 m = (i64)l * (twb + (t0 + thi) * a.dtw[0]);
            v = c_mulc(v, tw2(a.tw_lo, a.tw_hi, a.tw_shift, m));
        }
        A[l * ld + t] = v;
    }
    __syncthreads();

    int Ns = 1;
    for (int s = 0; s < a.nrad; ++s) {
        const int r = a.rad[s];
        switch (r) {
        case 2:  inplace_stage<2>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 3:  inplace_stage<3>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 4:  inplace_stage<4>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 5:  inplace_stage<5>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 7:  inplace_stage<7>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 8:  inplace_stage<8>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 11: inplace_stage<11>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        case 13: inplace_stage<13>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        default: inplace_stage<16>(A, a.wL, L, ld, Tcur, Ns, tid); break;
        }
        Ns *= r;
    }

    for (int e = tid; e < total; e += nth) {
        int l, t;
        if (a.out_t_fast) { l = e / Tcur; t = e - l * Tcur; }
        else              { t = e / L;    l = e - t * L; }
        cplx v = A[l * ld + t];
        const int thi = t / a.lo_n, tlo = t - thi * a.lo_n;
        if (a.tw_n && !tw_in) {
            i64 m = (i64)l * (twb + (t0 + thi) * a.dtw[0]);
            v = c_mulc(v, tw2(a.tw_lo, a.tw_hi, a.tw_shift, m));
        }
        i64 addr = doff + (i64)l * a.os_l + (t0 + thi) * a.dos[0] + tlo * a.lo_os;
        store_elem<VOUT>(a.dst, addr, a.dst_im, a.flags, v);
    }
}

/* ------------------------------------------------------------------------ */
/* host side                                                                 */
/* ------------------------------------------------------------------------ */

template <bool VIN, bool VOUT>
static void launch_pass_variant(const PassArgs &pa, dim3 grid, size_t lds, hipStream_t st) {
    static int nth = 0;
    if (!nth) { const char *e = getenv("FFTW_AMD_GENERIC_THREADS"); nth = e ? atoi(e) : 256; if (nth < 64 || nth > 256) nth = 256; }
    fa_launch_lds<pass_generic_kernel<VIN, VOUT>>(grid, dim3(nth), lds, 160 * 1024, st, pa);
}

template <bool IN_T, bool OUT_T, int HAS_TW>
static void launch_p1024_variant(const P1024Args &pa, dim3 grid, hipStream_t st) {
    const size_t lds = FA_P1024_LDS_DOUBLES * sizeof(double);
    fa_launch_lds<pass1024_kernel<IN_T, OUT_T, HAS_TW>>(grid, dim3(256), lds, lds, st, pa);
}

/* arguments of the register-resident 1024-point pass for one step and chunk; returns 1 if the step
   does not qualify (caller falls through to the generic kernel), 0 and *nblocks_out == 0 for an empty launch */
static int fill_p1024(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                      i64 cs, i64 cn, P1024Args &pa, i64 *nblocks_out, bool *in_t, bool *out_t, int *tw) {
    if (d->L != 1024 || d->src_im != 1 || d->dst_im != 1 ||
        (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT)))
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
    pa.lo_sh = 0; pa.lo_is = d->tile_lo_is; pa.lo_os = d->tile_lo_os;
    pa.dbg = NULL;
    pa.order = FA_P1024_ORD_EIGHTH;
    if (d->tile_lo_n > 1) {
        if (d->tile_lo_n != 2 && d->tile_lo_n != 4) return 1;
        pa.lo_sh = d->tile_lo_n == 2 ? 1 : 2;
        if (!g.even_lo()) return 1;
    }
    pa.ntiles = (pa.dn[0] + (8 >> pa.lo_sh) - 1) / (8 >> pa.lo_sh);
    const StepBlocks nb = fa_step_blocks(pa);
    if (nb.too_large()) return 1;
    *nblocks_out = nb.empty() ? 0 : nb.n;
    *in_t = pa.dn[0] > 1 && iabs64(pa.dis[0]) <= iabs64(pa.is_l);
    *out_t = pa.dn[0] > 1 && iabs64(pa.dos[0]) <= iabs64(pa.os_l);
    *tw = d->tw_n == 0 ? 0 : ((d->flags & FFTW_AMD_F_TW_IN) ? 2 : 1);
    return 0;
}

/* launches of the two forms of the 1024-point pass since the library was loaded (fftw_amd_p1024_launches) */
static std::atomic<long long> g_p1024_full{0}, g_p1024_general{0};

extern "C" int fftw_amd_p1024_tile_order(int order, long long nblocks, long long *place) {
    if (nblocks < 1 || nblocks > 0x7fffffffLL || order < 0 || order >= FA_P1024_ORD_FORMS) return 0;
    for (long long b = 0; place && b < nblocks; ++b) place[b] = (long long)p1024_order((unsigned)b, (unsigned)nblocks, order);
    return FA_P1024_ORD_FORMS;
}

extern "C" void fftw_amd_p1024_launches(long long *full, long long *general) {
    if (full) *full = g_p1024_full.load();
    if (general) *general = g_p1024_general.load();
}

/* The full-tile form (pass1024_full_kernel) applies when every tile of the launch holds 8 sequences, the step asks
   for nothing but a cache policy and (at most) the input twiddle, and an element's byte offset inside its tile fits
   31 bits on either side. */
static bool p1024_full_ok(const P1024Args &pa, int tw) {
    if (tw == 1 || pa.lo_sh != 0 || pa.dn[0] % 8 != 0) return false;
    if (pa.flags & ~(FFTW_AMD_F_NT_IN | FFTW_AMD_F_NT_OUT | FFTW_AMD_F_TW_IN | FFTW_AMD_F_P1024_EIGHTHS)) return false;
    const i64 lim = 0x7fffffffLL / 8 - 2;      /* in doubles */
    /* negative strides, and offsets that do not fit, keep the general kernel */
    if (pa.is_l <= 0 || pa.os_l <= 0 || pa.dis[0] < 0 || pa.dos[0] < 0) return false;
    if (pa.is_l > lim / 1023 || pa.os_l > lim / 1023 || pa.dis[0] > lim / 7 || pa.dos[0] > lim / 7) return false;   /* no overflow below */
    if (1023 * pa.is_l + 7 * pa.dis[0] > lim || 1023 * pa.os_l + 7 * pa.dos[0] > lim) return false;
    return true;
}

template <bool IN_T, bool OUT_T, int HAS_TW>
static void launch_p1024_full(const P1024Args &pa, dim3 grid, hipStream_t st) {
    const size_t lds = FA_P1024_LDS_DOUBLES * sizeof(double);
    const bool nti = (pa.flags & FFTW_AMD_F_NT_IN) != 0, nto = (pa.flags & FFTW_AMD_F_NT_OUT) != 0;
    if (nti && nto) fa_launch_lds<pass1024_full_kernel<IN_T, OUT_T, HAS_TW, true, true>>(grid, dim3(256), lds, lds, st, pa);
    else if (nti) fa_launch_lds<pass1024_full_kernel<IN_T, OUT_T, HAS_TW, true, false>>(grid, dim3(256), lds, lds, st, pa);
    else if (nto) fa_launch_lds<pass1024_full_kernel<IN_T, OUT_T, HAS_TW, false, true>>(grid, dim3(256), lds, lds, st, pa);
    else fa_launch_lds<pass1024_full_kernel<IN_T, OUT_T, HAS_TW, false, false>>(grid, dim3(256), lds, lds, st, pa);
}

static int launch_p1024(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                        i64 cs, i64 cn, hipStream_t st) {
    P1024Args pa;
    i64 nblocks = 0;
    bool in_t, out_t;
    int tw;
    if (fill_p1024(d, bufs, tables, cs, cn, pa, &nblocks, &in_t, &out_t, &tw)) return 1;
    if (nblocks <= 0) return 0;
    const dim3 grid((unsigned)nblocks, 1, 1);
    /* the skewed order goes to the passes whose input side is the strided one (the column pass of the two-pass plans:
       128-byte segments at a row pitch on both sides); with contiguous rows on the input side no order measured a
       gain over the eighths (profiles/r08_p1024_tile_order.txt) */
    if (in_t && !(d->flags & FFTW_AMD_F_P1024_EIGHTHS)) pa.order = FA_P1024_ORD_SKEW;
    if (p1024_full_ok(pa, tw)) {
#define FA_P1024_FULL(I, O, W) if (in_t == I && out_t == O && tw == W) { g_p1024_full.fetch_add(1); launch_p1024_full<I, O, W>(pa, grid, st); return 0; }
        FA_P1024_FULL(true, true, 0)   FA_P1024_FULL(true, true, 2)
        FA_P1024_FULL(false, true, 0)  FA_P1024_FULL(false, true, 2)
        FA_P1024_FULL(true, false, 0)  FA_P1024_FULL(true, false, 2)
        FA_P1024_FULL(false, false, 0) FA_P1024_FULL(false, false, 2)
#undef FA_P1024_FULL
    }
#define FA_P1024_CASE(I, O, W) if (in_t == I && out_t == O && tw == W) { g_p1024_general.fetch_add(1); launch_p1024_variant<I, O, W>(pa, grid, st); return 0; }
    FA_P1024_CASE(true, true, 0)  FA_P1024_CASE(true, true, 1)  FA_P1024_CASE(true, true, 2)
    FA_P1024_CASE(false, true, 0) FA_P1024_CASE(false, true, 1) FA_P1024_CASE(false, true, 2)
    FA_P1024_CASE(true, false, 0) FA_P1024_CASE(true, false, 1) FA_P1024_CASE(true, false, 2)
    FA_P1024_CASE(false, false, 0) FA_P1024_CASE(false, false, 1) FA_P1024_CASE(false, false, 2)
#undef FA_P1024_CASE
    return 1;
}

/* one tile of a launch described by `a`, block id `b0` of `nb` (XCD-contiguous order) */
template <bool IN_T, bool OUT_T, int HAS_TW>
FA_DEV void p1024_block(const P1024Args &a, unsigned b0, unsigned nb, double *plane) {
    unsigned blk = (nb & 7) ? b0 : (b0 & 7) * (nb >> 3) + (b0 >> 3);
    const unsigned nt = (unsigned)a.ntiles;
    unsigned rest = blk / nt;
    const unsigned tile = blk - rest * nt;
    i64 soff = 0, doff = 0, twb = 0;
    for (int d = 1; d < a.ndims; ++d) {
        const unsigned dn = (unsigned)a.dn[d];
        const unsigned q = rest / dn, idx = rest - q * dn;
        rest = q;
        soff += (i64)idx * a.dis[d];
        doff += (i64)idx * a.dos[d];
        twb += (i64)idx * a.dtw[d];
    }
    const i64 t0 = (i64)tile * 8;
    P1024Tile t;
    t.lo_sh = 0; t.lo_is = 0; t.lo_os = 0;
    t.src = a.src + soff + t0 * a.dis[0];
    t.dst = a.dst + doff + t0 * a.dos[0];
    t.is_l = a.is_l; t.os_l = a.os_l;
    t.dis0 = a.dis[0]; t.dos0 = a.dos[0];
    t.dtw0 = a.dtw[0]; t.q0 = twb + t0 * a.dtw[0];
    t.w1024 = a.w1024; t.tw_lo = a.tw_lo; t.tw_hi = a.tw_hi; t.tw_shift = a.tw_shift;
    t.Tcur = (int)((a.dn[0] - t0 < 8) ? (a.dn[0] - t0) : 8);
    t.flags = a.flags;
    t.dbg = NULL;
    p1024_tile<IN_T, OUT_T, HAS_TW, 0>(t, plane, threadIdx.x);
}

/* blocks [0, n2): row pass with input twiddle (pass 2 of the previous chunk); blocks [n2, n2 + n1):
   column pass (pass 1 of this chunk).  See fa_hip_launch_pair1024. */
__global__ void __launch_bounds__(256, 2)
pass1024_pair_kernel(const P1024Args a2, const P1024Args a1, const unsigned n2, const unsigned n1) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    if (blockIdx.x < n2) p1024_block<false, true, 2>(a2, blockIdx.x, n2, plane);
    else p1024_block<true, true, 0>(a1, blockIdx.x - n2, n1, plane);
}

/* The two passes of the batched N = 1024 x 1024 plan in ONE launch per chunk: first the tiles of
   pass 2 of the previous chunk, then the tiles of pass 1 of this chunk (pass1024.hpp,
   pass1024_pair_kernel).  Workgroups are dispatched in order, so pass 1 of chunk c fills the slots
   that the tail of pass 2 of chunk c-1 leaves idle: one dependent launch boundary per chunk instead
   of two.  Either half may be empty (first / last launch).  Returns 1 when the steps are not the
   (column pass without twiddle, row pass with input twiddle) pair the kernel is built for. */
extern "C" int fa_hip_launch_pair1024(const fftw_amd_step_desc *d_second, double *const *bufs_second,
                                      long long cs2, long long cn2,
                                      const fftw_amd_step_desc *d_first, double *const *bufs_first,
                                      long long cs1, long long cn1, void *const *tables, void *stream) {
    P1024Args a2, a1;
    i64 n2 = 0, n1 = 0;
    bool i2 = false, o2 = true, i1 = true, o1 = true;
    int w2 = 2, w1 = 0;
    memset((void *)&a2, 0, sizeof(a2));
    memset((void *)&a1, 0, sizeof(a1));
    if (cn2 > 0 && fill_p1024(d_second, bufs_second, tables, cs2, cn2, a2, &n2, &i2, &o2, &w2)) return 1;
    if (cn1 > 0 && fill_p1024(d_first, bufs_first, tables, cs1, cn1, a1, &n1, &i1, &o1, &w1)) return 1;
    if ((cn2 > 0 && (i2 || !o2 || w2 != 2 || a2.lo_sh)) || (cn1 > 0 && (!i1 || !o1 || w1 != 0 || a1.lo_sh))) return 1;
    if (n1 + n2 <= 0) return 0;
    if (n1 + n2 > 0x7fffffffLL) return 1;
    const size_t lds = FA_P1024_LDS_DOUBLES * sizeof(double);
    g_p1024_general.fetch_add(1);
    fa_launch_lds<pass1024_pair_kernel>(dim3((unsigned)(n1 + n2)), dim3(256), lds, lds, (hipStream_t)stream,
                                        a2, a1, (unsigned)n2, (unsigned)n1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { fprintf(stderr, "fftw3_amd: pair launch failed: %s\n", hipGetErrorString(e)); return -1; }
    return 0;
}

static int launch_pass(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                       i64 cs, i64 cn, hipStream_t st) {
    PassArgs pa;
    if (d->flags & (FFTW_AMD_F_R2C_ROWS | FFTW_AMD_F_C2R_ROWS)) return fa_launch_r2crows(d, bufs, tables, cs, cn, st);
    if (d->flags & FFTW_AMD_F_REAL_DEC) {
        /* the last trip of a two-trip r2c: one executor (kernels_r3tw.hip), planned only where it applies */
        if (fa_launch_pass3tw(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: real-decimated rows step with an unsupported layout\n");
        abort();
    }
    if (d->flags & FFTW_AMD_F_REAL_DEC_C2R) {
        /* the first trip of a two-trip c2r: likewise one executor, no fallback */
        if (fa_launch_pass3tw(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: c2r-decimated rows step with an unsupported layout\n");
        abort();
    }
    if (d->variant == FFTW_AMD_K_IMG2D) {
        /* whole small images in one trip: one executor (kernels_img.hip), planned only where it applies */
        if (fa_launch_img2d(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: small-image step %d x %d with an unsupported layout\n", d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_IMG2DL) {
        /* the same with an extent above 32 (kernels_imgl.hip) */
        if (fa_launch_img2dl(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: image step %d x %d with an unsupported layout\n", d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_IMG2DW) {
        /* the same with an extent of 128, one tile per 512-item workgroup (kernels_imgw.hip) */
        if (fa_launch_img2dw(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: wide-image step %d x %d with an unsupported layout\n", d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_IMG2DR) {
        /* whole small real images, r2c or c2r (kernels_imgr.hip) */
        if (fa_launch_img2dr(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: real-image step %d x %d with an unsupported layout\n", d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_IMG2DLR) {
        /* the same with an extent above 32 (kernels_imglr.hip) */
        if (fa_launch_img2dlr(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: real-image step %d x %d with an unsupported layout\n", d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_VOL3D) {
        /* whole small volumes in one trip (kernels_vol.hip) */
        if (fa_launch_vol3d(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: small-volume step %d x %d x %d with an unsupported layout\n", (int)d->aux_n, d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_VOL3DR) {
        /* whole small real volumes, r2c or c2r (kernels_volr.hip) */
        if (fa_launch_vol3dr(d, bufs, tables, cs, cn, st) == 0) return 0;
        fprintf(stderr, "fftw3_amd: internal error: real-volume step %d x %d x %d with an unsupported layout\n", (int)d->aux_n, d->tile_lo_n, d->L);
        return -1;
    }
    if (d->variant == FFTW_AMD_K_P1024 && launch_p1024(d, bufs, tables, cs, cn, st) == 0) return 0;
    if (d->variant == FFTW_AMD_K_BLUE) return fa_launch_blue(d, bufs, tables, cs, cn, st);
    if (d->variant == FFTW_AMD_K_R1 && fa_launch_pass1r(d, bufs, tables, cs, cn, st) == 0) return 0;
    if (d->variant == FFTW_AMD_K_RR && fa_launch_passrr(d, bufs, tables, cs, cn, st) == 0) return 0;
    if (d->variant == FFTW_AMD_K_R3 && d->L > 8192 && d->L < 16384 && fa_launch_pass3gw(d, bufs, tables, cs, cn, st) == 0) return 0;
    if (d->variant == FFTW_AMD_K_R3 && d->L > 1024 && d->L <= 2048 && fa_launch_pass3tw(d, bufs, tables, cs, cn, st) == 0) return 0;
    if (d->variant == FFTW_AMD_K_R3 && (fa_launch_pass3s(d, bufs, tables, cs, cn, st) == 0 ||
                                        fa_launch_pass3g(d, bufs, tables, cs, cn, st) == 0 ||
                                        fa_launch_pass3t(d, bufs, tables, cs, cn, st) == 0)) return 0;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    fa_copy_dims(pa, g);
    pa.src_im = d->src_im;
    pa.dst_im = d->dst_im;
    pa.is_l = d->is_l;
    pa.os_l = d->os_l;
    pa.wL = (d->table >= 0) ? (const cplx *)tables[d->table] : NULL;
    pa.tw_n = d->tw_n;
    pa.tw_shift = d->tw_shift;
    pa.tw_lo = d->tw_n ? (const cplx *)tables[d->tw_lo] : NULL;
    pa.tw_hi = d->tw_n ? (const cplx *)tables[d->tw_hi] : NULL;
    pa.L = d->L;
    pa.nrad = d->nradices;
    for (int i = 0; i < FFTW_AMD_MAX_RADICES; ++i) pa.rad[i] = (i < d->nradices) ? d->radices[i] : 1;
    pa.T = d->tile;
    pa.lo_n = d->tile_lo_n > 1 ? d->tile_lo_n : 1;
    pa.lo_is = d->tile_lo_is; pa.lo_os = d->tile_lo_os;
    while (pa.T > pa.lo_n && (i64)d->L * (pa.T | 1) > 5120) pa.T -= pa.lo_n;   /* tile of a tuned variant may not fit here */
    if (pa.T < pa.lo_n) pa.T = pa.lo_n;
    pa.T -= pa.T % pa.lo_n;
    pa.ld = (pa.T > 1) ? (pa.T | 1) : 1;
    pa.flags = d->flags;
    pa.ntiles = (pa.dn[0] + pa.T / pa.lo_n - 1) / (pa.T / pa.lo_n);
    /* a stride-0 dim cannot be the coalescing index */
    pa.in_t_fast = (pa.dn[0] > 1 && iabs64(pa.dis[0]) <= iabs64(pa.is_l)) || pa.L == 1;
    pa.out_t_fast = (pa.dn[0] > 1 && iabs64(pa.dos[0]) <= iabs64(pa.os_l)) || pa.L == 1;

    const StepBlocks nb = fa_step_blocks(pa);
    if (nb.empty()) return 0;
    dim3 grid = nb.grid();
    if (nb.too_large()) {
        /* split over y; the kernel recombines.  nblocks must factor: use 65535-ish rows */
        unsigned gy = (unsigned)((nb.n + 0x3fffffffLL) / 0x40000000LL);
        while (nb.n % gy) ++gy;
        grid = dim3((unsigned)(nb.n / gy), gy, 1);
    }
    size_t lds = (size_t)2 * pa.L * pa.ld * sizeof(cplx);
    if (lds > 160 * 1024) {
        fprintf(stderr, "fftw3_amd: internal error: pass tile needs %zu B of LDS\n", lds);
        return -1;
    }
    /* 16-byte vector access when the element is an aligned interleaved pair */
    const bool vin = d->src_im == 1 && !(d->flags & FFTW_AMD_F_REAL_IN) && g.src16 && g.is_l_even && g.dis_even && g.lo_is_even;
    const bool vout = d->dst_im == 1 && !(d->flags & FFTW_AMD_F_REAL_OUT) && g.dst16 && g.os_l_even && g.dos_even && g.lo_os_even;
    {
        /* all radices have register butterflies and the tile is at most 4096
           elements: the single-image kernel (two workgroups per CU) */
        static int inplace_mode = -1;
        bool small_radices = true;
        if (inplace_mode < 0) { const char *e = getenv("FFTW_AMD_INPLACE"); inplace_mode = e ? atoi(e) : 1; }
        for (int i = 0; i < d->nradices; ++i)
            if (d->radices[i] > 16 || d->radices[i] == 6 || d->radices[i] == 9 || d->radices[i] == 10 ||
                d->radices[i] == 12 || d->radices[i] == 14 || d->radices[i] == 15) small_radices = false;
        /* ping-pong images that fit twice on a CU need no help; larger tiles take the single image */
        if (inplace_mode && small_radices && (i64)pa.L * pa.T <= 4096 && lds > 80 * 1024) {
            const size_t lds1 = (size_t)pa.L * pa.ld * sizeof(cplx);
            if (vin && vout) fa_launch_lds<pass_inplace_kernel<true, true>>(grid, dim3(256), lds1, 160 * 1024, st, pa);
            else if (vin) fa_launch_lds<pass_inplace_kernel<true, false>>(grid, dim3(256), lds1, 160 * 1024, st, pa);
            else if (vout) fa_launch_lds<pass_inplace_kernel<false, true>>(grid, dim3(256), lds1, 160 * 1024, st, pa);
            else fa_launch_lds<pass_inplace_kernel<false, false>>(grid, dim3(256), lds1, 160 * 1024, st, pa);
            return 0;
        }
    }
    if (vin && vout) launch_pass_variant<true, true>(pa, grid, lds, st);
    else if (vin) launch_pass_variant<true, false>(pa, grid, lds, st);
    else if (vout) launch_pass_variant<false, true>(pa, grid, lds, st);
    else launch_pass_variant<false, false>(pa, grid, lds, st);
    return 0;
}

static int launch_step_kind(const fftw_amd_step_desc *d, double *const *bufs,
                            void *const *tables, long long cs, long long cn, hipStream_t st) {
    switch (d->kind) {
    case FFTW_AMD_STEP_PASS:        return launch_pass(d, bufs, tables, cs, cn, st);
    case FFTW_AMD_STEP_COPY:
    case FFTW_AMD_STEP_HERM_EXPAND: return fa_launch_copy(d, bufs, tables, cs, cn, st);
    case FFTW_AMD_STEP_R2C_POST:
    case FFTW_AMD_STEP_C2R_PRE:     return fa_launch_real2(d, bufs, tables, cs, cn, st);
    case FFTW_AMD_STEP_R2C_POST4:
    case FFTW_AMD_STEP_C2R_PRE4:    return fa_launch_real4(d, bufs, tables, cs, cn, st);
    case FFTW_AMD_STEP_R2R:         return fa_launch_r2r(d, bufs, tables, cs, cn, st);
    case FFTW_AMD_STEP_RADER_MUL:   return fa_launch_rader_mul(d, bufs, tables, cs, cn, st);
    }
    fprintf(stderr, "fftw3_amd: unknown step kind %d\n", d->kind);
    return -1;
}

/* A launch that the runtime refuses (bad grid / LDS configuration, missing code object) leaves
   no trace unless hipGetLastError is asked: without this check the step would "succeed" and the
   output would silently keep its old contents. */
extern "C" int fa_hip_launch_step(const fftw_amd_step_desc *d, double *const *bufs,
                                  void *const *tables, long long cs, long long cn,
                                  void *stream) {
    int r = launch_step_kind(d, bufs, tables, cs, cn, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "fftw3_amd: kernel launch of step kind %d (L=%d, variant %d) failed: %s\n",
                d->kind, d->L, d->variant, hipGetErrorString(e));
        return -1;
    }
    return r;
}
