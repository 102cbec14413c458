/*
 * launch.hpp -- host side shared by the launchers of the HIP units: the loop geometry of one step and batch chunk
 * (fa_step_geom), the launch of a kernel with dynamic LDS (fa_launch_lds) and the launchers' cross-unit prototypes:
 * the pass launchers, and fa_launch_copy / _real2 / _real4 / _r2r / _rader_mul of kernels_elem.hip (kernels.hip calls them).
 */
#ifndef FA_LAUNCH_HPP
#define FA_LAUNCH_HPP

#include <atomic>
#include <type_traits>
#include "common.hpp"

/* The loop dims of a step for the batch chunk [cs, cs + cn): padded to FFTW_AMD_MAX_DIMS (n = 1, strides 0), the
   batch dim cut to the chunk, src / dst advanced to it.  The predicates are what the kernels on 16-byte interleaved
   pairs need; each launcher tests the ones it needs and decides itself what a failure means. */
struct StepGeom {
    i64 dn[FFTW_AMD_MAX_DIMS], dis[FFTW_AMD_MAX_DIMS], dos[FFTW_AMD_MAX_DIMS], dtw[FFTW_AMD_MAX_DIMS];
    int ndims;
    double *src, *dst;
    bool src16, dst16;              /* 16-byte aligned */
    bool dis_even, dos_even;        /* every loop stride even */
    bool is_l_even, os_l_even;      /* the transform-index strides even */
    bool lo_is_even, lo_os_even;    /* the inner tile strides (tile_lo_is / tile_lo_os) even */

    bool aligned() const { return src16 && dst16; }
    bool even_dims() const { return dis_even && dos_even; }
    bool even_l() const { return is_l_even && os_l_even; }
    bool even_lo() const { return lo_is_even && lo_os_even; }
};

static inline StepGeom fa_step_geom(const fftw_amd_step_desc *d, double *const *bufs, i64 cs, i64 cn) {
    StepGeom g;
    const int bd = d->batch_dim;
    i64 sbase = d->src_base, dbase = d->dst_base;
    for (int i = 0; i < FFTW_AMD_MAX_DIMS; ++i) {
        g.dn[i] = (i < d->ndims) ? d->dim_n[i] : 1;
        g.dis[i] = (i < d->ndims) ? d->dim_is[i] : 0;
        g.dos[i] = (i < d->ndims) ? d->dim_os[i] : 0;
        g.dtw[i] = (i < d->ndims) ? d->dim_tw[i] : 0;
    }
    if (bd >= 0) {
        sbase += chunk_adv(d->src_buf, cs, d->dim_is[bd]);
        dbase += chunk_adv(d->dst_buf, cs, d->dim_os[bd]);
        g.dn[bd] = cn;
    }
    g.ndims = d->ndims;
    g.src = bufs[d->src_buf] + sbase;
    g.dst = bufs[d->dst_buf] + dbase;
    g.src16 = (uintptr_t)g.src % 16 == 0;
    g.dst16 = (uintptr_t)g.dst % 16 == 0;
    g.dis_even = g.dos_even = true;
    for (int i = 0; i < d->ndims; ++i) {
        if (g.dis[i] % 2) g.dis_even = false;
        if (g.dos[i] % 2) g.dos_even = false;
    }
    g.is_l_even = d->is_l % 2 == 0;
    g.os_l_even = d->os_l % 2 == 0;
    g.lo_is_even = d->tile_lo_is % 2 == 0;
    g.lo_os_even = d->tile_lo_os % 2 == 0;
    return g;
}

/* Workgroups of a tile kernel's launch: one per tile of dim 0 and index of the other loop dims.  The tile kernels
   take one-dimensional grids only. */
struct StepBlocks {
    i64 n;
    bool empty() const { return n <= 0; }
    bool too_large() const { return n > 0x7fffffffLL; }
    dim3 grid() const { return dim3((unsigned)n, 1, 1); }
};

template <class A> static inline StepBlocks fa_step_blocks(const A &a) {
    i64 n = a.ntiles;
    for (int i = 1; i < a.ndims; ++i) n *= a.dn[i];
    return StepBlocks{n};
}

/* loop dims and base pointers into a kernel's arguments, the twiddle strides too where the kernel has them */
template <class A, class = void> struct fa_has_dtw : std::false_type {};
template <class A> struct fa_has_dtw<A, decltype((void)A::dtw)> : std::true_type {};

template <class A> static inline void fa_copy_dims(A &a, const StepGeom &g) {
    for (int i = 0; i < FFTW_AMD_MAX_DIMS; ++i) {
        a.dn[i] = g.dn[i];
        a.dis[i] = g.dis[i];
        a.dos[i] = g.dos[i];
        if constexpr (fa_has_dtw<A>::value) a.dtw[i] = g.dtw[i];
    }
    a.ndims = g.ndims;
    a.src = g.src;
    a.dst = g.dst;
}

/* Launch of kernel K with `lds` bytes of dynamic LDS.  Its MaxDynamicSharedMemorySize attribute is set to attr_bytes
   before the first launch on each device.  Function attributes are per device: the "set" flag is a bit mask over the
   device ordinals, so that a process that drives several GPUs (sharded plans, one host thread per device) sets them
   on each.  Setting twice is harmless; the bit is published after the attribute, so no thread can launch on a device
   before the attribute is there. */
static inline unsigned fa_dev_bit(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return 1u << (dev & 31);
}

template <auto K, class... A>
static void fa_launch_lds(dim3 grid, dim3 block, size_t lds, size_t attr_bytes, hipStream_t st, const A &...a) {
    static std::atomic<unsigned> attr_set{0};
    if (!(attr_set.load(std::memory_order_acquire) & fa_dev_bit())) {
        FA_CHECK(hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_bytes));
        attr_set.fetch_or(fa_dev_bit(), std::memory_order_release);
    }
    hipLaunchKernelGGL(K, grid, block, lds, st, a...);
}

/* ---- launchers called from another unit: 0 = launched (or nothing to do), 1 = not applicable ---------------- */

struct P1024Args;
struct P3SArgs;
struct R2CRArgs;
struct BlueArgs;

/* one step and batch chunk */
int fa_launch_passrr(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_rr.hip */
int fa_launch_pass3s(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);
int fa_launch_r2crows3(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);
int fa_launch_pass3g(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_r3.hip */
int fa_launch_pass3t(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);
int fa_launch_r2crows(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);
int fa_launch_pass3gw(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);  /* kernels_r3w.hip */
int fa_launch_pass3tw(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);  /* kernels_r3tw.hip */
int fa_launch_blue(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);     /* kernels_blue.hip */
int fa_launch_pass1r(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_r1.hip */
int fa_launch_r2crows1(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);
int fa_launch_img2d(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);    /* kernels_img.hip */
int fa_launch_img2dl(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_imgl.hip */
int fa_launch_img2dw(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_imgw.hip */
int fa_launch_img2dr(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_imgr.hip */
int fa_launch_img2dlr(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);  /* kernels_imglr.hip */
int fa_launch_vol3d(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);    /* kernels_vol.hip */
int fa_launch_vol3dr(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);   /* kernels_volr.hip */
/* kernels_sq.hip: FFTW_AMD_F_LO_DFT steps (rows + a DFT across the rows of a tile) */
int fa_launch_lo_dft(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);

/* kernels_elem.hip: the element-wise steps, one launcher per step kind (0 = launched or nothing to do, -1 = error) */
int fa_launch_copy(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);       /* COPY, HERM_EXPAND */
int fa_launch_real2(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);      /* R2C_POST, C2R_PRE */
int fa_launch_real4(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);      /* R2C_POST4, C2R_PRE4 */
int fa_launch_r2r(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);
int fa_launch_rader_mul(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, i64 cs, i64 cn, hipStream_t st);

/* kernels_tr.hip: transposition steps (FFTW_AMD_STEP_COPY of variant FFTW_AMD_K_TRANSPOSE) */
int fa_launch_transpose(const fftw_amd_step_desc *d, double *const *bufs, i64 cs, i64 cn, hipStream_t st);

/* kernels_rr1.hip, kernels_rr2.hip: the upper two thirds of rr_menu.inc (rr_dispatch.hpp) */
int fa_dispatch_rr_part1(int L, const P1024Args &pa, dim3 grid, hipStream_t st, bool in_t, bool out_t, int tw);
int fa_dispatch_rr_part2(int L, const P1024Args &pa, dim3 grid, hipStream_t st, bool in_t, bool out_t, int tw);
/* one length of the fused real rows; arguments and grid filled by fa_launch_r2crows / fa_launch_r2crows3 */
int fa_launch_r2crows2m(int L, const R2CRArgs &ra, dim3 grid, hipStream_t st, bool inverse);   /* kernels_r2cm.hip */
int fa_launch_r2crows3g(int L, const P3SArgs &pa, dim3 grid, hipStream_t st, bool inverse);    /* kernels_r3r.hip */
int fa_launch_r2crows3gw(int L, const P3SArgs &pa, dim3 grid, hipStream_t st, bool inverse);   /* kernels_r3w.hip */
/* kernels_bluew.hip: padded lengths 8193 ... 16384, 512 work-items per row */
int fa_hip_bluew_nb(int need);
int fa_hip_bluew_has(int nb);
int fa_launch_bluew(int nb, const BlueArgs &ba, dim3 grid, hipStream_t st);

extern "C" {
int fa_hip_r3w_has(int L);              /* kernels_r3w.hip: 1 when L is a wide menu length */
int fa_hip_r2c_rows3gw_has(int L);      /* kernels_r3w.hip: the 512-item real forms for half lengths above 8192 */
int fa_hip_r3tw_tile(int L);            /* kernels_r3tw.hip: the 512-item strided forms */
int fa_hip_r2c_rows3g_tile(int L);      /* kernels_r3r.hip: the mixed-radix lengths of r3r_menu.inc */
}

#endif /* FA_LAUNCH_HPP */
