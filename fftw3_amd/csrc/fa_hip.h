/*
 * fa_hip.h -- the thin C ABI between the C host planner (api.c / planner.c)
 * and the HIP translation units (runtime wrappers: fa_hip.hip, step dispatcher:
 * kernels.hip).  Plain C types only.
 */
#ifndef FA_HIP_H
#define FA_HIP_H

#include <stddef.h>
#include "fftw3_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int   fa_hip_device_count(void);
/* sequences per tile of the two-stage register kernel for length L, 0 if there is none */
int   fa_hip_rr_tile(int L);
int   fa_hip_r3t_tile(int L);  /* sequences per tile of the strided three-stage kernel, 0: none */
int   fa_hip_r3tw_rdec(int L); /* 1: the length has the real-decimated rows form (FFTW_AMD_F_REAL_DEC) */
int   fa_hip_r3tw_cdec(int L); /* 1: the length has the c2r-decimated rows form (FFTW_AMD_F_REAL_DEC_C2R) */
int   fa_hip_r2c_rows_tile(int L);  /* rows per tile of the fused real-rows kernel for half length L, 0: none */
int   fa_hip_r2c_rows1_tile(int L);  /* ... of the one-stage real-rows kernel (dense rows, half length 2 ... 32), 0: none */
int   fa_hip_r2c_rows2m_tile(int L); /* ... of the mixed-radix two-stage lengths (plain r2c / c2r, half length 72 ... 648), 0: none */
int   fa_hip_r2c_rows3_tile(int L); /* ... of its three-stage form (plain r2c / c2r, half length 2048 ... 8192), 0: none */
int   fa_hip_r3_tile(int L);   /* rows per tile of the three-stage rows kernel for length L, 0: none */
int   fa_hip_blue_nb(int need);  /* smallest padded length >= need of the one-kernel Bluestein, 0: none */
int   fa_hip_blue_tile(int nb);  /* its rows per tile */
int   fa_hip_r1_tile(int L);   /* rows per tile of the one-stage rows kernel (L = 2 ... 32), 0: none */
int   fa_hip_img2d_tile(int n0, int n1);  /* images per tile of the one-trip small-image kernel (img2d_menu.inc), 0: none */
int   fa_hip_img2dl_tile(int n0, int n1); /* the same for the kernel of extents above 32 (img2dl_menu.inc), 0: none */
int   fa_hip_img2dw_tile(int n0, int n1); /* the same for the 512-item kernel of an extent of 128 (img2dw_menu.inc), 0: none */
int   fa_hip_img2dr_tile(int n0, int n1, int fwd); /* ... of the small real-image kernels, r2c (fwd) or c2r (img2dr_menu.inc), 0: none */
int   fa_hip_img2dlr_tile(int n0, int n1, int fwd); /* ... of the real-image kernels of extents above 32, r2c (fwd) or c2r (img2dlr_menu.inc), 0: none */
int   fa_hip_vol3d_tile(int n0, int n1, int n2);   /* volumes per tile of the one-trip small-volume kernel (vol3d_menu.inc), 0: none */
int   fa_hip_vol3dr_tile(int n0, int n1, int n2, int fwd); /* ... of the small real-volume kernels, r2c (fwd) or c2r (vol3dr_menu.inc), 0: none */
int   fa_hip_vol3dr_lds(int n0, int n1, int n2, int fwd, int *st); /* their LDS bytes; st[0 ... 3]: row and plane stride of the two layouts (pass3dr.hpp), 0: none */
int   fa_hip_vol3d_lds(int n0, int n1, int n2, int *s, int *sp); /* its LDS bytes, row and plane stride in doubles (pass3d.hpp), 0: none */
/* The kernel form that an element-wise step takes (kernels_elem.hip) for a batch chunk of cn transforms whose
   source / destination addresses are src_mis / dst_mis bytes past a 16-byte boundary.  Needs no device. */
enum fa_elem_form {
    FA_ELEM_COPY_1, FA_ELEM_COPY_4, FA_ELEM_HERM, FA_ELEM_POST2_DCT, FA_ELEM_PRE2_DCT, FA_ELEM_POST2_FAST, FA_ELEM_PRE2_FAST,
    FA_ELEM_POST2, FA_ELEM_PRE2, FA_ELEM_POST4_FAST, FA_ELEM_PRE4_FAST, FA_ELEM_POST4, FA_ELEM_PRE4, FA_ELEM_R2R_SHUFFLE,
    FA_ELEM_R2R_UNSHUFFLE, FA_ELEM_R2R, FA_ELEM_RADER_MUL, FA_ELEM_TRANSPOSE, FA_ELEM_NONE   /* NONE: not an element-wise step */
};
int   fa_hip_elem_form(const fftw_amd_step_desc *desc, int src_mis, int dst_mis, long long cn);
void *fa_hip_malloc(size_t nbytes);
void  fa_hip_free(void *p);
void *fa_hip_host_malloc(size_t nbytes);  /* pinned; NULL when no device runtime */
int   fa_hip_host_free(void *p);          /* 0 when p was not a pinned allocation */
/* 1: device-accessible pointer (hipMalloc / managed / registered), 0: plain host */
int   fa_hip_is_device_ptr(const void *p);
int   fa_hip_ptr_device(const void *p);   /* owning device of a device allocation, -1 otherwise */
void  fa_hip_memcpy_h2d(void *dst, const void *src, size_t nbytes, void *stream);
void  fa_hip_memcpy_d2h(void *dst, const void *src, size_t nbytes, void *stream);
void  fa_hip_memset(void *dst, int v, size_t nbytes, void *stream);
void  fa_hip_stream_sync(void *stream);
void *fa_hip_event_create(void);
void  fa_hip_event_record(void *ev, void *stream);
float fa_hip_event_elapsed_ms(void *start, void *stop);   /* both must have completed */
void  fa_hip_event_destroy(void *ev);
void *fa_hip_stream_create(void);                   /* non-blocking stream */
void  fa_hip_stream_destroy(void *stream);
void  fa_hip_stream_wait_event(void *stream, void *ev);
int   fa_hip_get_device(void);
void  fa_hip_set_device(int dev);                   /* of the calling host thread */
int   fa_hip_enable_peer(int dev, int peer);        /* 0: dev may address peer's memory */
void  fa_hip_memcpy_peer(void *dst, int dst_dev, const void *src, int src_dev, size_t nbytes, void *stream);
/* 2-D device-to-device copy (rows of `width` bytes, `height` of them), source and destination possibly on different
   devices with peer access; asynchronous on `stream` (a stream of the current device) */
void  fa_hip_memcpy2d_peer(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, void *stream);
size_t fa_hip_max_pitch(int dev);               /* largest pitch (bytes) of a 2-D copy on dev, 0: unknown */

/* Distributed 1-D transform (slab1d.c, kernels_slab.hip): in place, element (k0, c) of the rows x width block at p
   (complex values, rows row_stride apart) times w^(k0 (c0 + c)), w = exp(sign 2 pi i / n), from the two-level table
   lo[m & (2^shift - 1)] * hi[m >> shift] of (cos, sin)(2 pi m / n) (device pointers).  Every exponent must stay
   below n.  Returns 0 when launched on stream, 1 on invalid arguments. */
int   fa_hip_slab_twiddle(double *p, long long rows, long long width, long long row_stride, long long c0,
                          long long n, int sign, const void *lo, const void *hi, int shift, void *stream);

/* Transposing exchange of the TRANSPOSED slab layouts (slab.c, kernels_slab.hip): one launch on `stream` (a stream
   of the device that owns dst) that copies, for every source k < nsrc <= FA_HIP_SLAB_TR_MAXSRC,
       dst[dst_off + b * db + a * da + i] = src[a * sa + b * sb + i]      a < A, b < B, i < I
   in 16-byte complex elements (sources on peers are read through peer access).  I < 8 goes through an LDS tile
   transposition, I >= 8 is copied directly.  nt: 1 / 0 nontemporal accesses on / off, -1 the library's policy (off unless
   FFTW_AMD_NT=2 and every run is at least 128 bytes long).
   Returns 0 when launched (or when there is nothing to move), 1 on arguments it cannot run. */
#define FA_HIP_SLAB_TR_MAXSRC 32
typedef struct {
    const void *src;
    long long dst_off, A, B, sa, sb;
} fa_slab_tr_src;
int   fa_hip_slab_transpose(void *dst, long long da, long long db, long long I, int nsrc,
                            const fa_slab_tr_src *src, int nt, void *stream);

/* Launch one step.  bufs[i] is the device base pointer of buffer id i, tables[i]
   the device pointer of table id i.  (chunk_start, chunk_n) select the slice
   of the batch loop when desc->batch_dim >= 0.  Returns 0 on success. */
int fa_hip_launch_step(const fftw_amd_step_desc *desc, double *const *bufs,
                       void *const *tables, long long chunk_start, long long chunk_n,
                       void *stream);

/* One launch holding pass 2 (d_second) of one chunk and pass 1 (d_first) of the next one of the
   batched 1024 x 1024 plan; either half may be empty (cn == 0).  1: the steps are not that pair. */
int fa_hip_launch_pair1024(const fftw_amd_step_desc *d_second, double *const *bufs_second,
                           long long cs2, long long cn2,
                           const fftw_amd_step_desc *d_first, double *const *bufs_first,
                           long long cs1, long long cn1, void *const *tables, void *stream);

#ifdef __cplusplus
}
#endif
#endif
