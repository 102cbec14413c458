/*
 * slab1d.c -- ONE long one-dimensional complex transform spread over several GPUs of a node, behind the C ABI.
 *
 * Mirror of the reference's distributed 1-D solver (fftw/mpi/dft-rank1.c; entry points fftw_mpi_local_size_1d /
 * fftw_mpi_plan_dft_1d of fftw/mpi/fftw3-mpi.h:97-138, FFTW_MPI_SCRAMBLED_IN / _OUT of fftw3-mpi.h:212-213), with the
 * communicator replaced by a list of devices of one process, on the machinery of slab.c (block rule, per-device
 * streams and events, peer-to-peer hipMemcpy2DAsync exchanges, column-block local plans).
 *
 * n = n0 n1 with P | n0 and P | n1 (P devices), w = n1 / P, h = n0 / P.  The input read as [n0][n1] (x[n1 j0 + j1]),
 * the output as [n1][n0] (X[k0 + n0 k1]); in normal order device g holds elements [g n / P, (g + 1) n / P) of both:
 *
 *   1  exchange: device r gathers the columns j1 in [r w, (r + 1) w) of every device's rows    in[g] -> W[r]  [n0][w]
 *      (SCRAMBLED_IN: none -- step 2 reads in[r] as [w][n0] and writes W[r] transposed)
 *   2  every device r: w transforms of length n0 down W[r] (stride w)                           W[r] in place
 *   3  every device r: W[r][k0][c] *= w_n^(k0 (r w + c))  (kernels_slab.hip)                    W[r] in place
 *   4  exchange: device g gathers the rows k0 in block g of every W[r]                          W[r] -> out[g] [h][n1]
 *   5  every device g: h transforms of length n1 along the rows of out[g]                       out[g] -> T[g] [n1][h]
 *      (SCRAMBLED_OUT: in place, and the plan ends here)
 *   6  exchange: device g gathers the rows k1 in block g of every T[d], at column d h            T[d] -> out[g] [w][n0]
 *
 * Every local transform is an ordinary guru64 plan of this library made with its device current and bound to that
 * device's stream; every copy runs on the receiving device's stream behind an event of the sending one.
 */
#include <stdio.h>
#include <stdlib.h>
#include "fa_plan.h"
#include "fa_hip.h"

struct fa_slab1d {
    int ndev, devs[FA_SLAB_MAXDEV], sign;
    unsigned scr;                                     /* FFTW_AMD_SLAB_SCRAMBLED_IN / _OUT of the flags */
    long long n, n0, n1, h, w;
    int shift;                                        /* two-level twiddle table: 2^shift + ceil(n / 2^shift) entries */
    fftw_complex *in[FA_SLAB_MAXDEV], *out[FA_SLAB_MAXDEV];
    fftw_complex *W[FA_SLAB_MAXDEV], *T[FA_SLAB_MAXDEV];   /* owned: [n0][w], [n1][h] (T in normal-out mode only) */
    void *tlo[FA_SLAB_MAXDEV], *thi[FA_SLAB_MAXDEV];       /* owned: the twiddle table on every device */
    fftw_plan cols[FA_SLAB_MAXDEV], rows[FA_SLAB_MAXDEV];
    void *stream[FA_SLAB_MAXDEV];
    void *ev_cols[FA_SLAB_MAXDEV], *ev_rows[FA_SLAB_MAXDEV], *ev_done[FA_SLAB_MAXDEV];
    int ran;                                          /* ev_done holds the end of a previous execution */
};

#define FA_SLAB_SCR (FFTW_AMD_SLAB_SCRAMBLED_IN | FFTW_AMD_SLAB_SCRAMBLED_OUT)

static int slab1d_has_kernel(long long L) {
    return L <= 0x7fffffffLL && (fa_hip_r3_tile((int)L) > 0 || fa_hip_rr_tile((int)L) > 0);
}

/* The split rule of the header: among the n = n0 n1 with P | n0 and P | n1, the ones whose ratio max / min is at
   most 4 x the smallest ratio; of those the one with the most lengths that have register kernels, then the
   smallest ratio, then the larger n0.  BACKWARD takes the FORWARD split swapped.  0: found. */
static int slab1d_split(long long n, int P, int sign, long long *pn0, long long *pn1) {
    long long d, best0 = 0;
    double rmin = 0.0, brat = 0.0;
    int pass, bk = -1;
    if (n <= 0 || P < 1 || n % ((long long)P * P)) return -1;
    for (pass = 0; pass < 2; ++pass) {
        for (d = 1; d <= n / d; ++d) {
            long long c[2], k;
            int i;
            if (n % d) continue;
            c[0] = d; c[1] = n / d;
            for (i = 0; i < 2; ++i) {
                const long long n0 = c[i], n1 = n / n0;
                const double rat = (double)(n0 > n1 ? n0 : n1) / (double)(n0 > n1 ? n1 : n0);
                if (n0 % P || n1 % P) continue;
                if (pass == 0) {
                    if (rmin == 0.0 || rat < rmin) rmin = rat;
                    continue;
                }
                if (rat > 4.0 * rmin) continue;
                k = slab1d_has_kernel(n0) + slab1d_has_kernel(n1);
                if (k > bk || (k == bk && (rat < brat || (rat == brat && n0 > best0)))) {
                    bk = (int)k; brat = rat; best0 = n0;
                }
            }
        }
        if (rmin == 0.0) return -1;
    }
    if (sign == FFTW_BACKWARD) { *pn0 = n / best0; *pn1 = best0; }
    else { *pn0 = best0; *pn1 = n / best0; }
    return 0;
}

int fftw_amd_slab_split_1d(long long n, int ndev, int sign, long long *n0, long long *n1) {
    long long a, b;
    if (ndev < 1 || ndev > FA_SLAB_MAXDEV || (sign != FFTW_FORWARD && sign != FFTW_BACKWARD)) return -1;
    if (slab1d_split(n, ndev, sign, &a, &b)) return -1;
    if (n0) *n0 = a;
    if (n1) *n1 = b;
    return 0;
}

/* fftw_mpi_local_size_1d (fftw3-mpi.h:97-100): every device holds n / P elements of the input and of the output,
   device g the ones from g n / P on (of the natural or of the scrambled order) */
long long fftw_amd_slab_local_size_1d(long long n, int ndev, int g, int sign, unsigned flags,
                                      long long *local_ni, long long *local_i_start,
                                      long long *local_no, long long *local_o_start) {
    long long n0, n1, b;
    (void)flags;
    if (g < 0 || g >= ndev || fftw_amd_slab_split_1d(n, ndev, sign, &n0, &n1)) return -1;
    b = n / ndev;
    if (local_ni) *local_ni = b;
    if (local_i_start) *local_i_start = b * g;
    if (local_no) *local_no = b;
    if (local_o_start) *local_o_start = b * g;
    return b;
}

void fa_slab1d_destroy(struct fa_slab1d *d) {
    int g, cur;
    if (!d) return;
    cur = fa_hip_device_count() > 0 ? fa_hip_get_device() : -1;
    for (g = 0; g < d->ndev; ++g) {
        if (cur >= 0) fa_hip_set_device(d->devs[g]);
        if (d->stream[g]) fa_hip_stream_sync(d->stream[g]);
    }
    for (g = 0; g < d->ndev; ++g) {
        if (cur >= 0) fa_hip_set_device(d->devs[g]);
        if (d->rows[g]) fftw_destroy_plan(d->rows[g]);
        if (d->cols[g]) fftw_destroy_plan(d->cols[g]);
        if (d->W[g]) fa_hip_free(d->W[g]);
        if (d->T[g]) fa_hip_free(d->T[g]);
        if (d->tlo[g]) fa_hip_free(d->tlo[g]);
        if (d->thi[g]) fa_hip_free(d->thi[g]);
        if (d->ev_cols[g]) fa_hip_event_destroy(d->ev_cols[g]);
        if (d->ev_rows[g]) fa_hip_event_destroy(d->ev_rows[g]);
        if (d->ev_done[g]) fa_hip_event_destroy(d->ev_done[g]);
        if (d->stream[g]) fa_hip_stream_destroy(d->stream[g]);
    }
    if (cur >= 0) fa_hip_set_device(cur);
    free(d);
}

/* one local plan: a single transform dimension and a single loop, any strides (64-bit) */
static fftw_plan slab1d_local(long long len, long long is, long long os, long long howmany, long long idist,
                              long long odist, fftw_complex *i, fftw_complex *o, int sign, unsigned flags) {
    fftw_iodim64 dim, loop;
    dim.n = len; dim.is = is; dim.os = os;
    loop.n = howmany; loop.is = idist; loop.os = odist;
    return fftw_plan_guru64_dft(1, &dim, 1, &loop, i, o, sign, flags);
}

/* fftw_mpi_plan_dft_1d (fftw3-mpi.h:130-133) */
struct fftw_amd_slab_plan_s *fftw_amd_slab_plan_dft_1d(long long n, int ndev, const int *devs,
                                                       fftw_complex *const *in, fftw_complex *const *out,
                                                       int sign, unsigned flags) {
    /* without a device (CPU test tier: plan inspection only) the owned buffers are a placeholder address */
    static fftw_complex placeholder[1] __attribute__((aligned(64)));
    struct fa_slab1d *d;
    struct fftw_amd_slab_plan_s *p;
    int g, h, ndevices = fa_hip_device_count(), saved = -1;
    const size_t z = sizeof(fftw_complex);
    double *hlo = NULL, *hhi = NULL;
    long long nlo = 0, nhi = 0, m;
    if (ndev < 1 || ndev > FA_SLAB_MAXDEV || !in || !out) return NULL;
    d = (struct fa_slab1d *)calloc(1, sizeof(*d));
    if (!d) return NULL;
    if (fftw_amd_slab_split_1d(n, ndev, sign, &d->n0, &d->n1)) { free(d); return NULL; }
    d->ndev = ndev; d->sign = sign; d->n = n;
    d->scr = flags & FA_SLAB_SCR;
    flags &= ~(unsigned)FA_SLAB_SCR;
    d->h = d->n0 / ndev; d->w = d->n1 / ndev;
    for (g = 0; g < ndev; ++g) {
        d->devs[g] = devs ? devs[g] : g;
        if (d->devs[g] < 0 || (ndevices > 0 && d->devs[g] >= ndevices)) {
            fprintf(stderr, "fftw3_amd: slab plan names device %d, but only %d are visible\n", d->devs[g], ndevices);
            free(d);
            return NULL;
        }
        d->in[g] = in[g]; d->out[g] = out[g];
        if (!in[g] || !out[g]) { free(d); return NULL; }
    }
    if (ndevices > 0) {
        /* what would otherwise only fail inside execute: a device pair without peer access, a pitch over the limit
           (the widest pitch is a whole row of n0 or n1 elements) */
        for (g = 0; g < ndev; ++g) {
            const size_t maxp = fa_hip_max_pitch(d->devs[g]);
            const long long wide = d->n0 > d->n1 ? d->n0 : d->n1;
            if (maxp && (unsigned long long)wide > maxp / z) {
                fprintf(stderr, "fftw3_amd: 1-d slab plan: a row of %lld elements exceeds the copy pitch limit\n", wide);
                free(d);
                return NULL;
            }
            for (h = 0; h < ndev; ++h)
                if (d->devs[g] != d->devs[h] && fa_hip_enable_peer(d->devs[g], d->devs[h])) {
                    fprintf(stderr, "fftw3_amd: 1-d slab plan: device %d cannot access device %d\n", d->devs[g], d->devs[h]);
                    free(d);
                    return NULL;
                }
        }
        /* the twiddle table of step 3 (as planner.c's tab_tw2), built once on the host from fa_cexp */
        while (((long long)1 << (2 * d->shift)) < n) ++d->shift;
        nlo = (long long)1 << d->shift;
        nhi = (n + nlo - 1) / nlo;
        hlo = (double *)malloc((size_t)nlo * z);
        hhi = (double *)malloc((size_t)nhi * z);
        if (!hlo || !hhi) { free(hlo); free(hhi); free(d); return NULL; }
        for (m = 0; m < nlo; ++m) fa_cexp(m, n, hlo + 2 * m);
        for (m = 0; m < nhi; ++m) fa_cexp(m << d->shift, n, hhi + 2 * m);
        saved = fa_hip_get_device();
    }
    for (g = 0; g < ndev; ++g) {
        fftw_complex *W, *T;
        if (saved >= 0) {
            fa_hip_set_device(d->devs[g]);
            d->stream[g] = fa_hip_stream_create();
            d->ev_cols[g] = fa_hip_event_create();
            d->ev_rows[g] = fa_hip_event_create();
            d->ev_done[g] = fa_hip_event_create();
            d->W[g] = (fftw_complex *)fa_hip_malloc((size_t)(n / ndev) * z);
            if (!d->W[g]) goto fail;
            if (!(d->scr & FFTW_AMD_SLAB_SCRAMBLED_OUT)) {
                d->T[g] = (fftw_complex *)fa_hip_malloc((size_t)(n / ndev) * z);
                if (!d->T[g]) goto fail;
            }
            d->tlo[g] = fa_hip_malloc((size_t)nlo * z);
            d->thi[g] = fa_hip_malloc((size_t)nhi * z);
            if (!d->tlo[g] || !d->thi[g]) goto fail;
            fa_hip_memcpy_h2d(d->tlo[g], hlo, (size_t)nlo * z, d->stream[g]);
            fa_hip_memcpy_h2d(d->thi[g], hhi, (size_t)nhi * z, d->stream[g]);
            fa_hip_stream_sync(d->stream[g]);
        }
        W = d->W[g] ? d->W[g] : placeholder;
        T = d->T[g] ? d->T[g] : placeholder;
        /* step 2: w columns of length n0, in place down W (or from in[g] read as [w][n0] into W) */
        if (d->scr & FFTW_AMD_SLAB_SCRAMBLED_IN)
            d->cols[g] = slab1d_local(d->n0, 1, d->w, d->w, d->n0, 1, in[g], W, sign, flags);
        else
            d->cols[g] = slab1d_local(d->n0, d->w, d->w, d->w, 1, 1, W, W, sign, flags);
        /* step 5: h rows of length n1, in place (SCRAMBLED_OUT) or into T read as [n1][h] */
        if (d->scr & FFTW_AMD_SLAB_SCRAMBLED_OUT)
            d->rows[g] = slab1d_local(d->n1, 1, 1, d->h, d->n1, d->n1, out[g], out[g], sign, flags);
        else
            d->rows[g] = slab1d_local(d->n1, 1, d->h, d->h, d->n1, 1, out[g], T, sign, flags);
        if (!d->cols[g] || !d->rows[g]) goto fail;
        if (saved >= 0) {
            fftw_amd_plan_set_stream(d->cols[g], d->stream[g]);
            fftw_amd_plan_set_stream(d->rows[g], d->stream[g]);
        }
    }
    if (saved >= 0) fa_hip_set_device(saved);
    free(hlo);
    free(hhi);
    p = fa_slab_wrap1d(d, ndev);
    if (!p) fa_slab1d_destroy(d);
    return p;
fail:
    if (saved >= 0) fa_hip_set_device(saved);
    free(hlo);
    free(hhi);
    fa_slab1d_destroy(d);
    return NULL;
}

/* enqueues everything and returns (fftw_amd_slab_sync waits) */
void fa_slab1d_execute(struct fa_slab1d *d) {
    const size_t z = sizeof(fftw_complex);
    const long long h = d->h, w = d->w;
    int g, r, saved;
    if (fa_hip_device_count() <= 0) {
        fprintf(stderr, "fftw3_amd: no HIP device available: a slab plan cannot execute (no CPU fallback)\n");
        abort();
    }
    saved = fa_hip_get_device();
    for (r = 0; r < d->ndev; ++r) {
        fa_hip_set_device(d->devs[r]);
        /* in[], W[r] and T[r] are read or rewritten below: the previous execution must be over on every device */
        for (g = 0; g < d->ndev && d->ran; ++g) fa_hip_stream_wait_event(d->stream[r], d->ev_done[g]);
        /* 1: the column block r of every device's rows */
        for (g = 0; g < d->ndev && !(d->scr & FFTW_AMD_SLAB_SCRAMBLED_IN); ++g)
            fa_hip_memcpy2d_peer(d->W[r] + g * h * w, (size_t)w * z, d->in[g] + r * w, (size_t)d->n1 * z,
                                 (size_t)w * z, (size_t)h, d->stream[r]);
        /* 2, 3: columns, twiddle */
        fftw_execute(d->cols[r]);
        if (fa_hip_slab_twiddle((double *)d->W[r], d->n0, w, w, r * w, d->n, d->sign, d->tlo[r], d->thi[r], d->shift,
                                d->stream[r])) {
            fprintf(stderr, "fftw3_amd: internal error: 1-d slab twiddle rejected its arguments\n");
            abort();
        }
        fa_hip_event_record(d->ev_cols[r], d->stream[r]);
    }
    for (g = 0; g < d->ndev; ++g) {
        fa_hip_set_device(d->devs[g]);
        /* 4: the rows of block g of every W[r].  Waiting for every device's columns also puts the first write of
           out[g] behind every read of in[] (exchange 1 / the SCRAMBLED_IN columns), which covers in == out */
        for (r = 0; r < d->ndev; ++r) {
            fa_hip_stream_wait_event(d->stream[g], d->ev_cols[r]);
            fa_hip_memcpy2d_peer(d->out[g] + r * w, (size_t)d->n1 * z, d->W[r] + g * h * w, (size_t)w * z,
                                 (size_t)w * z, (size_t)h, d->stream[g]);
        }
        /* 5: rows */
        fftw_execute(d->rows[g]);
        fa_hip_event_record(d->ev_rows[g], d->stream[g]);
    }
    for (g = 0; g < d->ndev; ++g) {
        fa_hip_set_device(d->devs[g]);
        /* 6: the rows k1 of block g of every T[e]; the only reader of out[g], step 5, ran before on this stream */
        for (r = 0; r < d->ndev && !(d->scr & FFTW_AMD_SLAB_SCRAMBLED_OUT); ++r) {
            fa_hip_stream_wait_event(d->stream[g], d->ev_rows[r]);
            fa_hip_memcpy2d_peer(d->out[g] + r * h, (size_t)d->n0 * z, d->T[r] + g * w * h, (size_t)h * z,
                                 (size_t)h * z, (size_t)w, d->stream[g]);
        }
        fa_hip_event_record(d->ev_done[g], d->stream[g]);
    }
    d->ran = 1;
    fa_hip_set_device(saved);
}

void fa_slab1d_sync(struct fa_slab1d *d) {
    int g, saved;
    if (fa_hip_device_count() <= 0) return;
    saved = fa_hip_get_device();
    for (g = 0; g < d->ndev; ++g) {
        fa_hip_set_device(d->devs[g]);
        fa_hip_stream_sync(d->stream[g]);
    }
    fa_hip_set_device(saved);
}

fftw_plan fa_slab1d_local_plan(const struct fa_slab1d *d, int g, int which) {
    if (g < 0 || g >= d->ndev) return NULL;
    return which ? d->cols[g] : d->rows[g];
}
