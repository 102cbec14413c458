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
