/*
 * kernels_slab.hip -- device code of the distributed 1-D transform (slab1d.c): the twiddle between its column and
 * row transforms, indexed by GLOBAL position, and the pitch limit its exchanges are checked against at plan time.
 *
 * The six-step pipeline leaves device r with the column block W[r] = [n0][w] of the global [n0][n1] image, columns
 * c0 ... c0 + w - 1; element (k0, c) must be multiplied by w_n^(k0 (c0 + c)).  n reaches 2^31 and beyond, so no
 * table as long as the data (FFTW_AMD_F_MUL_TABLE) is possible: the factor comes from the two-level table of
 * common.hpp (tw2: lo[m & (2^shift - 1)] * hi[m >> shift], 2^shift ~ sqrt n, about 1.5 MiB at n = 2^31 -- resident
 * in every XCD's L2).  Tables hold (cos, sin)(2 pi m / n); the forward sign conjugates the product.
 */
#include "common.hpp"

/* elements per work-item: U independent 16-byte load -> multiply -> store chains (copy_kernel's U = 4), the U
   elements of an item 256 apart so that every access instruction of a wave covers 1 KiB of contiguous data */
#define FA_SLAB_TW_U 4

struct SlabTwArgs {
    double *p;
    i64 total;            /* rows * width */
    i64 width, row_stride, c0;
    const cplx *lo, *hi;
    int shift, conj;
};

/* HBM-bound streaming pass, in place: 32 bytes of traffic per element, the two table loads hit L2 */
__global__ void __launch_bounds__(256) slab_twiddle_kernel(const SlabTwArgs a) {
    const i64 per = 256 * FA_SLAB_TW_U;
    const i64 nchunks = (a.total + per - 1) / per;
    for (i64 j = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x); j < nchunks; j += gridDim.x) {
        const i64 base = j * per + threadIdx.x;
        i64 k0[FA_SLAB_TW_U], c[FA_SLAB_TW_U];
        bool ok[FA_SLAB_TW_U];
        cplx v[FA_SLAB_TW_U];
        if (a.total <= 0xffffffffLL) {
            /* 32-bit element index: one unsigned division per element instead of a 64-bit one */
            const unsigned wd = (unsigned)a.width;
#pragma unroll
            for (int u = 0; u < FA_SLAB_TW_U; ++u) {
                const i64 e = base + u * 256;
                ok[u] = e < a.total;
                const unsigned e32 = ok[u] ? (unsigned)e : 0u, q = e32 / wd;
                k0[u] = q;
                c[u] = e32 - q * wd;
            }
        } else {
#pragma unroll
            for (int u = 0; u < FA_SLAB_TW_U; ++u) {
                const i64 e = base + u * 256;
                ok[u] = e < a.total;
                const i64 e64 = ok[u] ? e : 0, q = e64 / a.width;
                k0[u] = q;
                c[u] = e64 - q * a.width;
            }
        }
#pragma unroll
        for (int u = 0; u < FA_SLAB_TW_U; ++u)
            if (ok[u]) v[u] = ld_cplx<false>(a.p + 2 * (k0[u] * a.row_stride + c[u]));
#pragma unroll
        for (int u = 0; u < FA_SLAB_TW_U; ++u) {
            if (!ok[u]) continue;
            cplx t = tw2(a.lo, a.hi, a.shift, k0[u] * (a.c0 + c[u]));
            if (a.conj) t.y = -t.y;
            st_cplx<false>(a.p + 2 * (k0[u] * a.row_stride + c[u]), c_mul(v[u], t));
        }
    }
}

extern "C" int fa_hip_slab_twiddle(double *p, long long rows, long long width, long long row_stride, long long c0,
                                   long long n, int sign, const void *lo, const void *hi, int shift, void *stream) {
    /* every exponent k0 (c0 + c) stays below n, so hi[m >> shift] stays inside its ceil(n / 2^shift) entries */
    if (!p || rows < 0 || width < 0 || row_stride < width || c0 < 0 || shift < 0 || shift > 40 || n <= 0) return 1;
    if (rows == 0 || width == 0) return 0;
    if ((rows - 1) > 0 && (c0 + width - 1) > (n - 1) / (rows - 1)) return 1;
    SlabTwArgs a;
    a.p = p;
    a.total = rows * width;
    a.width = width;
    a.row_stride = row_stride;
    a.c0 = c0;
    a.lo = (const cplx *)lo;
    a.hi = (const cplx *)hi;
    a.shift = shift;
    a.conj = sign == FFTW_FORWARD;
    const i64 nchunks = (a.total + 256 * FA_SLAB_TW_U - 1) / (256 * FA_SLAB_TW_U);
    const unsigned grid = (unsigned)(nchunks < (1 << 20) ? nchunks : (1 << 20));   /* grid-stride beyond 2^30 elements */
    hipLaunchKernelGGL(slab_twiddle_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    FA_CHECK(hipGetLastError());
    return 0;
}

/* largest row pitch (bytes) hipMemcpy2D* accepts on device dev; 0 when unknown */
extern "C" size_t fa_hip_max_pitch(int dev) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxPitch, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return v > 0 ? (size_t)v : 0;
}

/*
 * The transposing exchange of the TRANSPOSED_IN / TRANSPOSED_OUT slab plans (slab.c): one launch per receiving
 * device, a permuted block copy of 16-byte elements
 *
 *     src_g[a][b][i]  ->  dst[b][a0(g) + a][i]         a < A(g), b < B(g), i < I
 *
 * for up to FA_HIP_SLAB_TR_MAXSRC sources handed over by value (peers are read through peer access, every store is local).
 * Two regimes.  I < 8: a real transposition through LDS, so that both global sides move whole contiguous runs -- a
 * tile is T x T x I elements (T = 32 for I = 1, else 16), loaded as T source rows of T I contiguous elements and
 * stored as T destination rows of T I contiguous elements, i.e. runs of 512 B and more wherever the block has them.
 * The LDS image is [T][T + 1][I]: a row pitch of (T + 1) I elements keeps the 16-byte slot (a / 16 mod 16) of the
 * transposed read at (lane + const) mod 16 inside every destination row, so the 16-lane groups of ds_read_b128 hit 16
 * different slots; the row-wise ds_write_b128 is contiguous per 8-lane group.  (For I = 3, 5, 6, 7 a 32-lane half
 * that straddles two destination rows can meet a 2-way conflict; I = 1, 2, 4 never do.)  I >= 8: runs of I elements
 * are at least 128 B on both sides already, lanes run along (b, i) of one source row, no LDS.
 * Work units are numbered source by source (u0 = first unit of a source, nb = units per a-row); the unit -> source
 * search and the unit -> (row, column) division are uniform over the workgroup.  All offsets are 64-bit.
 */
#define FA_SLAB_TR_U 4

struct SlabTrSrc {
    const double *p;
    i64 doff, A, B, sa, sb;   /* destination offset of element (0, 0, 0); extents; source strides (elements) */
    i64 u0;                   /* first work unit */
    i64 nb;                   /* work units per a-row (tile kernel: per row of tiles) */
};
struct SlabTrArgs {
    double *dst;
    i64 da, db, I, total;     /* destination strides of a and b (elements), run length, number of work units */
    int nsrc;
    SlabTrSrc s[FA_HIP_SLAB_TR_MAXSRC];
};

FA_DEV int slab_tr_find(const SlabTrArgs &a, i64 u) {
    int k = 0;
    while (k + 1 < a.nsrc && u >= a.s[k + 1].u0) ++k;
    return k;
}

template <int I, bool NT>
__global__ void __launch_bounds__(256) slab_transpose_tile_kernel(const SlabTrArgs a) {
    constexpr int T = I == 1 ? 32 : 16;
    constexpr int ROW = T * I;            /* elements per tile row, on either side */
    constexpr int PITCH = (T + 1) * I;
    constexpr int PER = T * ROW / 256;
    __shared__ cplx tile[T * PITCH];
    for (i64 u = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x); u < a.total; u += gridDim.x) {
        const int k = slab_tr_find(a, u);
        const double *sp = a.s[k].p;
        const i64 A = a.s[k].A, B = a.s[k].B, sa = a.s[k].sa, sb = a.s[k].sb;
        const i64 t = u - a.s[k].u0, ta = t / a.s[k].nb, tb = t - ta * a.s[k].nb;
        const i64 a0 = ta * T, b0 = tb * T;
        double *dp = a.dst + 2 * (a.s[k].doff + b0 * a.db + a0 * a.da);
        sp += 2 * (a0 * sa + b0 * sb);
        cplx v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {   /* rows along a, lanes along (b, i) */
            const int e = (int)threadIdx.x + j * 256, r = e / ROW, c = e - r * ROW, b = c / I, i = c - b * I;
            v[j] = c_make(0.0, 0.0);
            if (a0 + r < A && b0 + b < B) v[j] = ld_cplx<NT>(sp + 2 * (r * sa + b * sb + i));
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = (int)threadIdx.x + j * 256, r = e / ROW, c = e - r * ROW;
            tile[r * PITCH + c] = v[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {   /* rows along b, lanes along (a, i) */
            const int e = (int)threadIdx.x + j * 256, r = e / ROW, c = e - r * ROW, q = c / I, i = c - q * I;
            const cplx w = tile[q * PITCH + r * I + i];
            if (a0 + q < A && b0 + r < B) st_cplx<NT>(dp + 2 * (r * a.db + q * a.da + i), w);
        }
        __syncthreads();
    }
}

template <bool NT>
__global__ void __launch_bounds__(256) slab_transpose_direct_kernel(const SlabTrArgs a) {
    const unsigned I = (unsigned)a.I;
    for (i64 u = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x); u < a.total; u += gridDim.x) {
        const int k = slab_tr_find(a, u);
        const i64 t = u - a.s[k].u0, ar = t / a.s[k].nb, ch = t - ar * a.s[k].nb;
        const unsigned row = (unsigned)(a.s[k].B * a.I);        /* B I < 2^31: checked by the launcher */
        const i64 sb = a.s[k].sb;
        const double *sp = a.s[k].p + 2 * (ar * a.s[k].sa);
        double *dp = a.dst + 2 * (a.s[k].doff + ar * a.da);
        cplx v[FA_SLAB_TR_U];
        unsigned b[FA_SLAB_TR_U], i[FA_SLAB_TR_U];
        bool ok[FA_SLAB_TR_U];
#pragma unroll
        for (int j = 0; j < FA_SLAB_TR_U; ++j) {
            const unsigned c = (unsigned)ch * (256u * FA_SLAB_TR_U) + threadIdx.x + j * 256u;
            ok[j] = c < row;
            b[j] = ok[j] ? c / I : 0u;
            i[j] = ok[j] ? c - b[j] * I : 0u;
            if (ok[j]) v[j] = ld_cplx<NT>(sp + 2 * ((i64)b[j] * sb + i[j]));
        }
#pragma unroll
        for (int j = 0; j < FA_SLAB_TR_U; ++j)
            if (ok[j]) st_cplx<NT>(dp + 2 * ((i64)b[j] * a.db + i[j]), v[j]);
    }
}

template <int I> static void slab_tr_launch_tile(const SlabTrArgs &a, unsigned grid, bool nt, hipStream_t st) {
    if (nt) hipLaunchKernelGGL((slab_transpose_tile_kernel<I, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((slab_transpose_tile_kernel<I, false>), dim3(grid), dim3(256), 0, st, a);
}

extern "C" int fa_hip_slab_transpose(void *dst, long long da, long long db, long long I, int nsrc,
                                     const fa_slab_tr_src *src, int nt, void *stream) {
    SlabTrArgs a;
    i64 units = 0;
    bool runs = true;                     /* every contiguous run of the launch is at least one 128-byte line */
    if (!dst || !src || nsrc < 1 || nsrc > FA_HIP_SLAB_TR_MAXSRC || I < 1 || I > 0x7fffffffLL || da < I || db < I) return 1;
    const int T = I == 1 ? 32 : 16;
    a.dst = (double *)dst;
    a.da = da; a.db = db; a.I = I;
    a.nsrc = 0;
    for (int k = 0; k < nsrc; ++k) {
        const fa_slab_tr_src *s = &src[k];
        if (s->A < 0 || s->B < 0 || s->dst_off < 0 || s->B > 0x7fffffffLL / I) return 1;
        if (s->A == 0 || s->B == 0) continue;
        if (!s->src || s->sb < I || s->sa < I) return 1;
        SlabTrSrc &d = a.s[a.nsrc++];
        d.p = (const double *)s->src;
        d.doff = s->dst_off; d.A = s->A; d.B = s->B; d.sa = s->sa; d.sb = s->sb;
        d.u0 = units;
        if (I < 8) {
            d.nb = (s->B + T - 1) / T;
            units += ((s->A + T - 1) / T) * d.nb;
            runs = runs && s->A * I >= 8 && s->B * I >= 8;
        } else {
            d.nb = (s->B * I + 256 * FA_SLAB_TR_U - 1) / (256 * FA_SLAB_TR_U);
            units += s->A * d.nb;
        }
    }
    if (a.nsrc == 0) return 0;
    a.total = units;
    /* nt = 0 / 1 forces the choice.  nt < 0 (the plans): plain accesses unless FFTW_AMD_NT=2 forces the nontemporal
       ones, and then only when every run is at least one 128-byte line long (run LENGTH: rows of odd length, nc = 513,
       start off a line boundary and share their end lines with the neighbouring run).  The size rule of the planner's
       mark_streaming_accesses does not carry over: measured (profiles/r06_slab_transposed.txt), launches of 1 - 2 GiB
       run 3 - 16 % SLOWER with nontemporal accesses, launches of 128 - 512 MiB 0 - 8 % faster, and the destination is
       read again at once by the next local plan */
    static int policy = -1;
    if (policy < 0) { const char *e = getenv("FFTW_AMD_NT"); policy = e ? atoi(e) : 1; }
    const bool use_nt = nt < 0 ? (policy == 2 && runs) : nt != 0;
    const unsigned grid = (unsigned)(units < (1 << 22) ? units : (1 << 22));
    hipStream_t st = (hipStream_t)stream;
    if (I >= 8) {
        if (use_nt) hipLaunchKernelGGL(slab_transpose_direct_kernel<true>, dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(slab_transpose_direct_kernel<false>, dim3(grid), dim3(256), 0, st, a);
    } else switch ((int)I) {
        case 1: slab_tr_launch_tile<1>(a, grid, use_nt, st); break;
        case 2: slab_tr_launch_tile<2>(a, grid, use_nt, st); break;
        case 3: slab_tr_launch_tile<3>(a, grid, use_nt, st); break;
        case 4: slab_tr_launch_tile<4>(a, grid, use_nt, st); break;
        case 5: slab_tr_launch_tile<5>(a, grid, use_nt, st); break;
        case 6: slab_tr_launch_tile<6>(a, grid, use_nt, st); break;
        default: slab_tr_launch_tile<7>(a, grid, use_nt, st); break;
    }
    FA_CHECK(hipGetLastError());
    return 0;
}
