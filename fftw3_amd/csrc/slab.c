/*
 * slab.c -- ONE two- or three-dimensional complex transform spread over several GPUs of a node, behind the C ABI.
 *
 * Mirror of the reference's distributed-memory layer for the c2c case (fftw/mpi/fftw3-mpi.h:74-215:
 * fftw_mpi_local_size_2d / _3d, fftw_mpi_plan_dft_2d / _3d, fftw_mpi_execute_dft), with the MPI communicator
 * replaced by a list of devices of one process and the per-rank pointers by arrays of per-device pointers.  The
 * data distribution is the reference's: slabs along the first dimension by the block rule
 * (fftw/mpi/block.c:39-50: device g owns rows [g * ceil(n0 / P), ...)), normal order in, normal order out.
 *
 * Pipeline (the transposed-layout pipeline of fftw/mpi/dft-rank-geq2-transposed.c, with the global transposes
 * of fftw/mpi/transpose-alltoall.c done as peer-to-peer 2-D copies over xGMI -- no pack / unpack passes, and no
 * local transposes either: the second local transform simply runs down the strided first dimension):
 *
 *   1  every device g: transform over the trailing dimension(s) of its rows          in[g]  -> out[g]
 *   2  exchange: the column block of device r of every device's rows                 out[g] -> W[r]   ([n0][w_r])
 *   3  every device r: transforms of length n0 down its column block (stride w_r)    W[r] in place
 *   4  exchange back: rows of device g from every column block                       W[r]   -> out[g]
 *
 * with R = n1 (or n1 * n2) elements per row, column blocks cut on n1 by the same block rule (w_r = local_n1(r) *
 * n2).  Every local transform is an ordinary plan of this library created with its device current; every copy is
 * a hipMemcpy2DAsync on the receiving device's stream behind an event of the sending one.  One host thread
 * enqueues everything; fftw_amd_slab_sync waits.  fftw3_amd/slab.py is the multi-process form of the same layer
 * (torch.distributed in the place of MPI; r2r and howmany > 1 live there).
 *
 * Real data (fftw_mpi_plan_dft_r2c_2d / _3d, _c2r_*): the rows plan of step 1 is the local r2c into out[g] seen as
 * complex [local_n0][n1'][rest] (n1' x rest = the complex trailing dimensions, last one n_last / 2 + 1), steps 2 - 4
 * run on that complex shape; c2r runs steps 2 - 4 from in[g] into out[g] seen as complex and the local c2r last, in
 * place.
 *
 * TRANSPOSED_OUT / TRANSPOSED_IN (fftw3-mpi.h:214-215): the transposed layout of device r is [local_n1(r)][n0][rest].
 *   OUT:   trailing plan in[g] -> W[g];  TRANSPOSING exchange W[g] -> out[r];  length-n0 plan in place in out[r]
 *   IN:    length-n0 plan in[g] -> W[g]; transposing exchange W[g] -> out[r];  trailing plan in place in out[r]
 *   both:  length-n0 plan in[g] -> W[g]; exchange W -> out; trailing plan out[r] -> W[r]; exchange W -> out
 * The transposing exchange is one kernel launch per receiving device (fa_hip_slab_transpose, kernels_slab.hip): it
 * delivers every block already transposed, so the length-n0 transforms of a rank-2 problem run along contiguous rows.
 *
 * Every pipeline is a list of stages -- local plans, 2-D copies, transposing launches -- with the block moves of an
 * exchange kept as a list of ops (fftw_amd_slab_exchange_ops reports it); one executor walks the list.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fa_plan.h"
#include "fa_hip.h"

enum { SLAB_LOCAL = 0, SLAB_COPY = 1, SLAB_TRANSPOSE = 2 };
enum { SLAB_C2C = 0, SLAB_R2C = 1, SLAB_C2R = 2 };
enum { BUF_IN = 0, BUF_OUT = 1, BUF_W = 2 };
#define SLAB_MAXSTAGE 5
#define SLAB_TBITS (FFTW_AMD_SLAB_TRANSPOSED_IN | FFTW_AMD_SLAB_TRANSPOSED_OUT)

/* dst[doff + a dsa + b dsb + i] = src[soff + a ssa + b ssb + i] in complex elements, a < A, b < B, i < I */
struct slab_op {
    int sbuf, sdev, dbuf, ddev;
    long long soff, doff, A, B, I, ssa, ssb, dsa, dsb;
};

struct slab_stage {
    int kind;
    fftw_plan *plan;        /* SLAB_LOCAL: the plans of the devices (rows or cols below) */
    struct slab_op *ops;    /* exchanges: the moves, ordered by destination device */
    int nops;
    int producer;           /* exchanges: every move waits for this stage's event of its source device */
    int hazard;             /* the stage starts behind this stage's events of EVERY device (-1: none) */
    int after_last;         /* ... and behind the previous execution's last exchange on every device */
    void *ev[FA_SLAB_MAXDEV];
};

struct fftw_amd_slab_plan_s {
    int ndev, devs[FA_SLAB_MAXDEV];
    long long n0, n1, inner, R;                       /* rows, split dimension, elements per n1 entry, R = n1 * inner */
    long long lo0[FA_SLAB_MAXDEV], ln0[FA_SLAB_MAXDEV];   /* rows of device g */
    long long lo1[FA_SLAB_MAXDEV], ln1[FA_SLAB_MAXDEV];   /* its block of n1 */
    fftw_complex *buf[3][FA_SLAB_MAXDEV];             /* BUF_IN, BUF_OUT: the caller's; BUF_W: owned */
    fftw_plan rows[FA_SLAB_MAXDEV], cols[FA_SLAB_MAXDEV];   /* trailing-dimension plan, length-n0 plan */
    void *stream[FA_SLAB_MAXDEV];
    struct slab_stage st[SLAB_MAXSTAGE];
    int nst, last_x;                                   /* last_x: the last exchange stage */
    int ran;                                           /* its events hold the end of a previous execution */
    struct fa_slab1d *d1;                              /* a 1-D plan (slab1d.c): everything above unused but ndev */
};

/* block rule of fftw/mpi/block.c:39-50 (default block = ceil(n / P)) */
static void slab_block(long long n, int P, int g, long long *lo, long long *len) {
    long long blk = (n + P - 1) / P, a = blk * g, b = blk * (g + 1);
    if (a > n) a = n;
    if (b > n) b = n;
    *lo = a;
    *len = b - a;
}

/* fftw_mpi_local_size_2d / _3d (fftw3-mpi.h:98-108): rows [*local_0_start, + *local_n0) of device g of ndev; the
   return value is the number of complex elements its in / out arrays must hold */
long long fftw_amd_slab_local_size(int rank, const long long *n, int ndev, int g, long long *local_n0, long long *local_0_start) {
    long long lo = 0, len = 0, rest = 1;
    int i;
    if (rank < 2 || rank > 3 || !n || ndev < 1 || g < 0 || g >= ndev) return -1;
    for (i = 1; i < rank; ++i) rest *= n[i];
    slab_block(n[0], ndev, g, &lo, &len);
    if (local_n0) *local_n0 = len;
    if (local_0_start) *local_0_start = lo;
    return len * rest;
}

/* fftw_mpi_local_size_2d / _3d_transposed (fftw3-mpi.h:100-111): also the block of the second dimension; the array
   must hold whichever of the two layouts is larger */
long long fftw_amd_slab_local_size_transposed(int rank, const long long *n, int ndev, int g,
                                              long long *local_n0, long long *local_0_start,
                                              long long *local_n1, long long *local_1_start) {
    long long lo0 = 0, ln0 = 0, lo1 = 0, ln1 = 0, rest, a, b;
    if (rank < 2 || rank > 3 || !n || ndev < 1 || g < 0 || g >= ndev) return -1;
    rest = rank == 3 ? n[2] : 1;
    slab_block(n[0], ndev, g, &lo0, &ln0);
    slab_block(n[1], ndev, g, &lo1, &ln1);
    if (local_n0) *local_n0 = ln0;
    if (local_0_start) *local_0_start = lo0;
    if (local_n1) *local_n1 = ln1;
    if (local_1_start) *local_1_start = lo1;
    a = ln0 * n[1] * rest;
    b = ln1 * n[0] * rest;
    return a > b ? a : b;
}

void fftw_amd_destroy_slab_plan(struct fftw_amd_slab_plan_s *p) {
    int g, s, cur;
    if (!p) return;
    if (p->d1) { fa_slab1d_destroy(p->d1); free(p); return; }
    cur = fa_hip_device_count() > 0 ? fa_hip_get_device() : -1;
    for (g = 0; g < p->ndev; ++g) {
        if (cur >= 0) fa_hip_set_device(p->devs[g]);
        if (p->stream[g]) fa_hip_stream_sync(p->stream[g]);
    }
    for (g = 0; g < p->ndev; ++g) {
        if (cur >= 0) fa_hip_set_device(p->devs[g]);
        if (p->rows[g]) fftw_destroy_plan(p->rows[g]);
        if (p->cols[g]) fftw_destroy_plan(p->cols[g]);
        if (p->buf[BUF_W][g]) fa_hip_free(p->buf[BUF_W][g]);
        for (s = 0; s < SLAB_MAXSTAGE; ++s)
            if (p->st[s].ev[g]) fa_hip_event_destroy(p->st[s].ev[g]);
        if (p->stream[g]) fa_hip_stream_destroy(p->stream[g]);
    }
    for (s = 0; s < SLAB_MAXSTAGE; ++s) free(p->st[s].ops);
    if (cur >= 0) fa_hip_set_device(cur);
    free(p);
}

static struct slab_stage *slab_add_stage(struct fftw_amd_slab_plan_s *p, int kind, fftw_plan *plan, int producer, int hazard, int after_last) {
    struct slab_stage *s = &p->st[p->nst];
    s->kind = kind;
    s->plan = plan;
    s->producer = producer;
    s->hazard = hazard;
    s->after_last = after_last;
    if (kind != SLAB_LOCAL) {
        p->last_x = p->nst;
        s->ops = (struct slab_op *)calloc((size_t)p->ndev * (size_t)p->ndev, sizeof(struct slab_op));
        if (!s->ops) return NULL;
    }
    p->nst++;
    return s;
}

/* exchange of the normal-order pipeline as 2-D copies: to_cols = 1 the column block of device r of every device's
   rows (sbuf on g, [local_n0][R]) -> W[r] = [n0][w_r]; to_cols = 0 the way back into dbuf */
static int slab_add_copies(struct fftw_amd_slab_plan_s *p, int to_cols, int buf, int producer, int hazard, int after_last) {
    struct slab_stage *s = slab_add_stage(p, SLAB_COPY, NULL, producer, hazard, after_last);
    int d, e;
    if (!s) return -1;
    for (d = 0; d < p->ndev; ++d)
        for (e = 0; e < p->ndev; ++e) {
            const int g = to_cols ? e : d, r = to_cols ? d : e;      /* g: owner of the rows, r: of the column block */
            const long long w = p->ln1[r] * p->inner;
            struct slab_op *o = &s->ops[s->nops];
            if (p->ln0[g] <= 0 || w <= 0) continue;
            o->A = p->ln0[g]; o->B = 1; o->I = w;
            o->ddev = d; o->sdev = e;
            if (to_cols) {
                o->sbuf = buf; o->soff = p->lo1[r] * p->inner; o->ssa = p->R;
                o->dbuf = BUF_W; o->doff = p->lo0[g] * w; o->dsa = w;
            } else {
                o->sbuf = BUF_W; o->soff = p->lo0[g] * w; o->ssa = w;
                o->dbuf = buf; o->doff = p->lo1[r] * p->inner; o->dsa = p->R;
            }
            o->ssb = o->dsb = w;
            s->nops++;
        }
    return 0;
}

/* transposing exchange: to_t = 1 from the normal layout [local_n0(g)][n1][inner] (sbuf on g) into the transposed one
   [local_n1(r)][n0][inner] (dbuf on r), to_t = 0 from the transposed layout of g into the normal one of r */
static int slab_add_transpose(struct fftw_amd_slab_plan_s *p, int to_t, int sbuf, int dbuf, int producer, int hazard) {
    struct slab_stage *s = slab_add_stage(p, SLAB_TRANSPOSE, NULL, producer, hazard, 0);
    int r, g;
    if (!s) return -1;
    for (r = 0; r < p->ndev; ++r)
        for (g = 0; g < p->ndev; ++g) {
            struct slab_op *o = &s->ops[s->nops];
            o->sbuf = sbuf; o->sdev = g; o->dbuf = dbuf; o->ddev = r;
            o->I = p->inner;
            o->ssb = o->dsa = p->inner;
            if (to_t) {
                o->A = p->ln0[g]; o->B = p->ln1[r];
                o->soff = p->lo1[r] * p->inner; o->ssa = p->R;
                o->doff = p->lo0[g] * p->inner; o->dsb = p->n0 * p->inner;
            } else {
                o->A = p->ln1[g]; o->B = p->ln0[r];
                o->soff = p->lo0[r] * p->inner; o->ssa = p->n0 * p->inner;
                o->doff = p->lo1[g] * p->inner; o->dsb = p->R;
            }
            if (o->A > 0 && o->B > 0) s->nops++;
        }
    return 0;
}

/* without a device (CPU test tier: plan inspection only) plans on owned buffers are made on a placeholder address */
static fftw_complex slab_placeholder[1];
static fftw_complex *slab_w(const struct fftw_amd_slab_plan_s *p, int g) {
    return p->buf[BUF_W][g] ? p->buf[BUF_W][g] : slab_placeholder;
}

/* the trailing-dimension plan of device g, i -> o: c2c over n1 (x inner) of its local_n0 rows, or the local r2c /
   c2r of the logical size nl[1] (x nl[2]) in FFTW's padded layout */
static fftw_plan slab_trailing_plan(const struct fftw_amd_slab_plan_s *p, int kind, int rank, const long long *nl, int g,
                                    void *i, void *o, int sign, unsigned flags) {
    int nn[2], re[2], ce[2];
    const int nc = (int)(nl[rank - 1] / 2 + 1);
    if (kind == SLAB_C2C) {
        nn[0] = (int)p->n1; nn[1] = (int)p->inner;
        return fftw_plan_many_dft(rank - 1, nn, (int)p->ln0[g], (fftw_complex *)i, NULL, 1, (int)p->R,
                                  (fftw_complex *)o, NULL, 1, (int)p->R, sign, flags);
    }
    nn[0] = (int)nl[1]; nn[1] = rank == 3 ? (int)nl[2] : 0;
    if (rank == 3) { re[0] = ce[0] = (int)nl[1]; re[1] = 2 * nc; ce[1] = nc; }
    else { re[0] = 2 * nc; ce[0] = nc; }
    if (kind == SLAB_R2C)
        return fftw_plan_many_dft_r2c(rank - 1, nn, (int)p->ln0[g], (double *)i, re, 1, (int)(2 * p->R),
                                      (fftw_complex *)o, ce, 1, (int)p->R, flags);
    return fftw_plan_many_dft_c2r(rank - 1, nn, (int)p->ln0[g], (fftw_complex *)i, ce, 1, (int)p->R,
                                  (double *)o, re, 1, (int)(2 * p->R), flags);
}

/* the length-n0 plan of device g over the transposed layout [local_n1(g)][n0][inner], i -> o */
static fftw_plan slab_n0_plan(const struct fftw_amd_slab_plan_s *p, int g, fftw_complex *i, fftw_complex *o, int sign, unsigned flags) {
    fftw_iodim64 dim, loop[2];
    dim.n = p->n0; dim.is = dim.os = p->inner;
    loop[0].n = p->ln1[g]; loop[0].is = loop[0].os = p->n0 * p->inner;
    loop[1].n = p->inner; loop[1].is = loop[1].os = 1;
    return fftw_plan_guru64_dft(1, &dim, p->inner > 1 ? 2 : 1, loop, i, o, sign, flags);
}

static struct fftw_amd_slab_plan_s *slab_make(int kind, int rank, const long long *n, int ndev, const int *devs,
                                              void *const *in, void *const *out, int sign, unsigned flags) {
    struct fftw_amd_slab_plan_s *p;
    const int tin = (flags & FFTW_AMD_SLAB_TRANSPOSED_IN) != 0, tout = (flags & FFTW_AMD_SLAB_TRANSPOSED_OUT) != 0;
    const unsigned lflags = flags & ~SLAB_TBITS;
    int g, h, s, ndevices = fa_hip_device_count(), saved;
    long long nc;
    if (rank < 2 || rank > 3 || !n || ndev < 1 || ndev > FA_SLAB_MAXDEV || !in || !out) return NULL;
    if (n[0] <= 0 || n[1] <= 0 || (rank == 3 && n[2] <= 0) || (sign != FFTW_FORWARD && sign != FFTW_BACKWARD)) return NULL;
    if (n[0] > 0x7fffffffLL || n[1] > 0x7fffffffLL || (rank == 3 && (n[2] > 0x7fffffffLL || n[1] * n[2] > 0x7fffffffLL))) return NULL;
    if ((kind == SLAB_R2C && tin) || (kind == SLAB_C2R && tout)) return NULL;
    nc = n[rank - 1] / 2 + 1;
    if (kind != SLAB_C2C && rank == 3 && 2 * n[1] * nc > 0x7fffffffLL) return NULL;
    p = (struct fftw_amd_slab_plan_s *)calloc(1, sizeof(*p));
    if (!p) return NULL;
    p->ndev = ndev;
    p->n0 = n[0];
    if (kind == SLAB_C2C) { p->n1 = n[1]; p->inner = rank == 3 ? n[2] : 1; }
    else { p->n1 = rank == 3 ? n[1] : nc; p->inner = rank == 3 ? nc : 1; }
    p->R = p->n1 * p->inner;
    for (g = 0; g < ndev; ++g) {
        p->devs[g] = devs ? devs[g] : g;
        if (ndevices > 0 && (p->devs[g] < 0 || p->devs[g] >= ndevices)) {
            fprintf(stderr, "fftw3_amd: slab plan names device %d, but only %d are visible\n", p->devs[g], ndevices);
            free(p);
            return NULL;
        }
        slab_block(p->n0, ndev, g, &p->lo0[g], &p->ln0[g]);
        slab_block(p->n1, ndev, g, &p->lo1[g], &p->ln1[g]);
        p->buf[BUF_IN][g] = (fftw_complex *)in[g]; p->buf[BUF_OUT][g] = (fftw_complex *)out[g];
        if (((tin ? p->ln1[g] : p->ln0[g]) > 0 && !in[g]) || ((tout ? p->ln1[g] : p->ln0[g]) > 0 && !out[g])) { free(p); return NULL; }
        /* with both bits out[g] is also the landing place of the first exchange, in the normal layout */
        if (tin && tout && p->ln0[g] > 0 && !out[g]) { free(p); return NULL; }
    }
    /* the pipeline */
    if (!tin && !tout) {
        const int x = kind == SLAB_C2R ? BUF_IN : BUF_OUT;
        if (!slab_add_stage(p, SLAB_LOCAL, kind == SLAB_C2R ? NULL : p->rows, -1, -1, 0)) goto nomem;   /* 1: rows */
        if (slab_add_copies(p, 1, x, 0, -1, 1)) goto nomem;      /* 2: W[r] is rewritten: behind the last execution's exchange 4 */
        if (!slab_add_stage(p, SLAB_LOCAL, p->cols, -1, -1, 0)) goto nomem;                             /* 3: columns */
        if (slab_add_copies(p, 0, BUF_OUT, 2, 1, 0)) goto nomem; /* 4: out[g] must no longer be read by exchange 2 */
        if (kind == SLAB_C2R && !slab_add_stage(p, SLAB_LOCAL, p->rows, -1, -1, 0)) goto nomem;        /* local c2r, in place */
    } else {
        /* W[g] is rewritten by the first plan: behind the last execution's last exchange, which reads it everywhere */
        if (!slab_add_stage(p, SLAB_LOCAL, tin ? p->cols : p->rows, -1, -1, 1)) goto nomem;
        if (slab_add_transpose(p, !tin, BUF_W, BUF_OUT, 0, -1)) goto nomem;
        if (tin && tout) {
            if (!slab_add_stage(p, SLAB_LOCAL, p->rows, -1, 1, 0)) goto nomem;    /* out[r] -> W[r], which exchange 1 reads */
            if (slab_add_transpose(p, 1, BUF_W, BUF_OUT, 2, -1)) goto nomem;
        } else if (!slab_add_stage(p, SLAB_LOCAL, tin ? p->rows : p->cols, -1, -1, 0)) goto nomem;
    }
    saved = ndevices > 0 ? fa_hip_get_device() : -1;
    for (g = 0; g < ndev; ++g) {
        const long long w = p->ln1[g] * p->inner;
        const long long a = p->ln0[g] * p->R, b = p->ln1[g] * p->n0 * p->inner;
        const long long wsize = (!tin && !tout) ? p->n0 * w : (tin && tout) ? (a > b ? a : b) : tin ? b : a;
        if (saved >= 0) fa_hip_set_device(p->devs[g]);
        if (saved >= 0) {
            p->stream[g] = fa_hip_stream_create();
            for (s = 0; s < p->nst; ++s) p->st[s].ev[g] = fa_hip_event_create();
            for (h = 0; h < ndev; ++h)
                if (fa_hip_enable_peer(p->devs[g], p->devs[h]) && p->devs[g] != p->devs[h]) {
                    fprintf(stderr, "fftw3_amd: slab plan: device %d cannot access device %d\n", p->devs[g], p->devs[h]);
                    goto fail;
                }
            if (wsize > 0) {
                p->buf[BUF_W][g] = (fftw_complex *)fa_hip_malloc((size_t)wsize * sizeof(fftw_complex));
                if (!p->buf[BUF_W][g]) goto fail;
            }
        }
        if (!tin && !tout) {
            if (p->ln0[g] > 0) {
                /* step 1: the trailing dimension(s) of every local row (c2r: the last step, in place in out[g]) */
                p->rows[g] = slab_trailing_plan(p, kind, rank, n, g, kind == SLAB_C2R ? out[g] : in[g], out[g], sign, flags);
                if (!p->rows[g]) goto fail;
            }
            if (w > 0) {
                /* step 3: length-n0 transforms down the column block [n0][w], in place */
                int nn[1];
                fftw_complex *wp = slab_w(p, g);
                nn[0] = (int)p->n0;
                p->cols[g] = fftw_plan_many_dft(1, nn, (int)w, wp, NULL, (int)w, 1, wp, NULL, (int)w, 1, sign, flags);
                if (!p->cols[g]) goto fail;
            }
        } else {
            if (p->ln0[g] > 0) {
                /* OUT: in[g] -> W[g]; IN: in place in out[g] behind the exchange; both: out[g] -> W[g] */
                void *i = tin ? out[g] : in[g], *o = tout ? (void *)slab_w(p, g) : out[g];
                p->rows[g] = slab_trailing_plan(p, kind, rank, n, g, i, o, sign, lflags);
                if (!p->rows[g]) goto fail;
            }
            if (p->ln1[g] > 0) {
                /* IN: in[g] -> W[g]; OUT only: in place in out[g] behind the exchange */
                p->cols[g] = slab_n0_plan(p, g, tin ? (fftw_complex *)in[g] : (fftw_complex *)out[g],
                                          tin ? slab_w(p, g) : (fftw_complex *)out[g], sign, lflags);
                if (!p->cols[g]) goto fail;
            }
        }
        if (saved >= 0 && p->rows[g]) fftw_amd_plan_set_stream(p->rows[g], p->stream[g]);
        if (saved >= 0 && p->cols[g]) fftw_amd_plan_set_stream(p->cols[g], p->stream[g]);
    }
    if (saved >= 0) fa_hip_set_device(saved);
    return p;
fail:
    if (saved >= 0) fa_hip_set_device(saved);
nomem:
    fftw_amd_destroy_slab_plan(p);
    return NULL;
}

/* fftw_mpi_plan_dft_2d / _3d (fftw3-mpi.h:141-152): in[g] / out[g] are device arrays on devs[g] holding its rows,
   local_n0(g) x n1 (x n2) complex values in row-major order (with a TRANSPOSED bit: that side in the transposed
   layout, and both arrays of fftw_amd_slab_local_size_transposed elements); in == out (per device) is allowed.  NULL
   on invalid arguments, when a named device does not exist, or when a local plan / buffer cannot be made. */
struct fftw_amd_slab_plan_s *fftw_amd_slab_plan_dft(int rank, const long long *n, int ndev, const int *devs,
                                                    fftw_complex *const *in, fftw_complex *const *out,
                                                    int sign, unsigned flags) {
    return slab_make(SLAB_C2C, rank, n, ndev, devs, (void *const *)in, (void *const *)out, sign, flags);
}

/* fftw_mpi_plan_dft_r2c_2d / _3d (fftw3-mpi.h:167-176): n is the logical real size */
struct fftw_amd_slab_plan_s *fftw_amd_slab_plan_dft_r2c(int rank, const long long *n, int ndev, const int *devs,
                                                        double *const *in, fftw_complex *const *out, unsigned flags) {
    return slab_make(SLAB_R2C, rank, n, ndev, devs, (void *const *)in, (void *const *)out, FFTW_FORWARD, flags);
}

/* fftw_mpi_plan_dft_c2r_2d / _3d (fftw3-mpi.h:178-187): unnormalised; the complex input may be overwritten */
struct fftw_amd_slab_plan_s *fftw_amd_slab_plan_dft_c2r(int rank, const long long *n, int ndev, const int *devs,
                                                        fftw_complex *const *in, double *const *out, unsigned flags) {
    return slab_make(SLAB_C2R, rank, n, ndev, devs, (void *const *)in, (void *const *)out, FFTW_BACKWARD, flags);
}

static void slab_internal_error(const char *what) {
    fprintf(stderr, "fftw3_amd: internal error: %s\n", what);
    abort();
}

/* fftw_mpi_execute_dft on the plan's own arrays: enqueues everything and returns (fftw_amd_slab_sync waits).  Stage
   by stage, every device's part on its own stream: local plans; copies on the receiver's stream, each behind the
   sender's event; one transposing launch per receiver behind the events of all its senders. */
void fftw_amd_slab_execute(struct fftw_amd_slab_plan_s *p) {
    int g, h, s, k, saved;
    if (!p) return;
    if (p->d1) { fa_slab1d_execute(p->d1); return; }
    if (fa_hip_device_count() <= 0) {
        fprintf(stderr, "fftw3_amd: no HIP device available: a slab plan cannot execute (no CPU fallback)\n");
        abort();
    }
    saved = fa_hip_get_device();
    for (s = 0; s < p->nst; ++s) {
        struct slab_stage *st = &p->st[s];
        for (g = 0; g < p->ndev; ++g) {
            fa_slab_tr_src src[FA_SLAB_MAXDEV];
            const struct slab_op *first = NULL;
            int nsrc = 0;
            fa_hip_set_device(p->devs[g]);
            for (h = 0; h < p->ndev && st->after_last && p->ran; ++h) fa_hip_stream_wait_event(p->stream[g], p->st[p->last_x].ev[h]);
            for (h = 0; h < p->ndev && st->hazard >= 0; ++h) fa_hip_stream_wait_event(p->stream[g], p->st[st->hazard].ev[h]);
            if (st->kind == SLAB_LOCAL) {
                if (st->plan && st->plan[g]) fftw_execute(st->plan[g]);
            } else for (k = 0; k < st->nops; ++k) {
                const struct slab_op *o = &st->ops[k];
                if (o->ddev != g) continue;
                fa_hip_stream_wait_event(p->stream[g], p->st[st->producer].ev[o->sdev]);
                if (st->kind == SLAB_COPY) {
                    fa_hip_memcpy2d_peer(p->buf[o->dbuf][g] + o->doff, (size_t)o->dsa * sizeof(fftw_complex),
                                         p->buf[o->sbuf][o->sdev] + o->soff, (size_t)o->ssa * sizeof(fftw_complex),
                                         (size_t)o->I * sizeof(fftw_complex), (size_t)o->A, p->stream[g]);
                } else {
                    if (!first) first = o;
                    src[nsrc].src = p->buf[o->sbuf][o->sdev] + o->soff;
                    src[nsrc].dst_off = o->doff;
                    src[nsrc].A = o->A; src[nsrc].B = o->B; src[nsrc].sa = o->ssa; src[nsrc].sb = o->ssb;
                    nsrc++;
                }
            }
            if (nsrc && fa_hip_slab_transpose(p->buf[first->dbuf][g], first->dsa, first->dsb, first->I, nsrc, src, -1, p->stream[g]))
                slab_internal_error("the transposing exchange of a slab plan was refused by its launcher");
            fa_hip_event_record(st->ev[g], p->stream[g]);
        }
    }
    p->ran = 1;
    fa_hip_set_device(saved);
}

void fftw_amd_slab_sync(struct fftw_amd_slab_plan_s *p) {
    int g, saved;
    if (!p || fa_hip_device_count() <= 0) return;
    if (p->d1) { fa_slab1d_sync(p->d1); return; }
    saved = fa_hip_get_device();
    for (g = 0; g < p->ndev; ++g) {
        fa_hip_set_device(p->devs[g]);
        fa_hip_stream_sync(p->stream[g]);
    }
    fa_hip_set_device(saved);
}

/* one execution between device events on every device's stream (tools/perf) */
int fftw_amd_slab_execute_timed(struct fftw_amd_slab_plan_s *p, double *ms) {
    void *e0[FA_SLAB_MAXDEV], *e1[FA_SLAB_MAXDEV];
    int g, saved;
    double worst = 0.0;
    if (!p || p->d1 || !ms || fa_hip_device_count() <= 0) return -1;
    fftw_amd_slab_sync(p);
    saved = fa_hip_get_device();
    for (g = 0; g < p->ndev; ++g) {
        fa_hip_set_device(p->devs[g]);
        e0[g] = fa_hip_event_create();
        e1[g] = fa_hip_event_create();
        fa_hip_event_record(e0[g], p->stream[g]);
    }
    fftw_amd_slab_execute(p);
    for (g = 0; g < p->ndev; ++g) {
        fa_hip_set_device(p->devs[g]);
        fa_hip_event_record(e1[g], p->stream[g]);
    }
    fftw_amd_slab_sync(p);
    for (g = 0; g < p->ndev; ++g) {
        const double t = (double)fa_hip_event_elapsed_ms(e0[g], e1[g]);
        fa_hip_set_device(p->devs[g]);
        if (t > worst) worst = t;
        fa_hip_event_destroy(e0[g]);
        fa_hip_event_destroy(e1[g]);
    }
    fa_hip_set_device(saved);
    *ms = worst;
    return 0;
}

int fftw_amd_slab_num_devices(const fftw_amd_slab_plan p) { return p ? p->ndev : 0; }
fftw_plan fftw_amd_slab_local_plan(const fftw_amd_slab_plan p, int g, int which) {
    if (!p || g < 0 || g >= p->ndev) return NULL;
    if (p->d1) return fa_slab1d_local_plan(p->d1, g, which);
    return which ? p->cols[g] : p->rows[g];
}

int fftw_amd_slab_exchange_ops(const fftw_amd_slab_plan p, int which, long long *ops, int cap) {
    int s, k;
    if (!p || which < 0 || (cap > 0 && !ops)) return -1;
    if (p->d1) return 0;
    for (s = 0; s < p->nst; ++s) {
        const struct slab_stage *st = &p->st[s];
        if (st->kind == SLAB_LOCAL || which-- > 0) continue;
        for (k = 0; k < st->nops && k < cap; ++k) {
            const struct slab_op *o = &st->ops[k];
            long long *v = ops + (size_t)k * FFTW_AMD_SLAB_OP_LEN;
            v[0] = o->sbuf; v[1] = o->sdev; v[2] = o->soff; v[3] = o->dbuf; v[4] = o->ddev; v[5] = o->doff;
            v[6] = o->A; v[7] = o->B; v[8] = o->I; v[9] = o->ssa; v[10] = o->ssb; v[11] = o->dsa; v[12] = o->dsb;
        }
        return st->nops;
    }
    return -1;
}

int fftw_amd_slab_block_transpose(fftw_complex *dst, long long da, long long db, long long I, int nsrc,
                                  const long long *desc, int nt, void *stream) {
    fa_slab_tr_src src[FA_SLAB_MAXDEV];
    int k;
    if (fa_hip_device_count() <= 0) return -1;
    if (!desc || nsrc < 1 || nsrc > FA_SLAB_MAXDEV) return 1;
    for (k = 0; k < nsrc; ++k) {
        src[k].src = (const void *)(size_t)desc[6 * k];
        src[k].dst_off = desc[6 * k + 1];
        src[k].A = desc[6 * k + 2]; src[k].B = desc[6 * k + 3]; src[k].sa = desc[6 * k + 4]; src[k].sb = desc[6 * k + 5];
    }
    return fa_hip_slab_transpose(dst, da, db, I, nsrc, src, nt < 0 ? -1 : nt != 0, stream);
}

struct fftw_amd_slab_plan_s *fa_slab_wrap1d(struct fa_slab1d *d, int ndev) {
    struct fftw_amd_slab_plan_s *p = (struct fftw_amd_slab_plan_s *)calloc(1, sizeof(*p));
    if (!p) return NULL;
    p->ndev = ndev;
    p->d1 = d;
    return p;
}
