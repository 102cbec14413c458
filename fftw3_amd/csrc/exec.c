/*
 * exec.c -- the executor: brings a built plan (planner.c) onto the device, chooses its chunk schedule once, stages
 * plain host arrays and enqueues the plan's steps chunk by chunk.
 *
 * A plan runs its batch in chunks of p->chunk transforms, by one of four schedules (FA_SCHED_*, fa_plan.h), chosen by
 * choose_schedule when the plan is set up and stored in p->sched; everything below switches on that tag.  Host arrays
 * go through the host_io context: staged whole around the launches, or chunk by chunk on two copy streams.
 *
 * It talks to the device only through fa_hip.h, so it runs on a CPU against a recording fake of those calls:
 * tools/trace/exec_trace.c, tests/test_exec_trace.py.
 */
#include <stdio.h>
#include <stdlib.h>
#include "fa_plan.h"
#include "fa_hip.h"

typedef struct fftw_plan_s plan;

static i64 chunk_count(const plan *p) { return (p->batch + p->chunk - 1) / p->chunk; }
/* transforms in chunk c: the last one may be ragged */
static i64 chunk_len(const plan *p, i64 c) {
    const i64 left = p->batch - c * p->chunk;
    return left < p->chunk ? left : p->chunk;
}
static int has_side_streams(const plan *p) { return p->sched == FA_SCHED_PIPE || p->sched == FA_SCHED_LANES; }

/* ---------------------------------------------------------------- set-up */

static plan *make_c2c_1d_contig(i64 n) {
    plan *q = fa_plan_new();
    q->type = FA_C2C;
    q->sign = FFTW_FORWARD;
    q->rank = 1;
    q->dims[0].n = n; q->dims[0].is = 2; q->dims[0].os = 2;
    q->hrank = 0;
    if (fa_build(q)) { fa_plan_free(q); return NULL; }
    return q;
}

static int upload_tables(plan *p) {
    int i;
    for (i = 0; i < p->ntabs; ++i) {
        fa_table *t = &p->tabs[i];
        size_t bytes = (size_t)t->len * (t->kind == FA_TAB_PERM ? sizeof(i64) : 2 * sizeof(double));
        if (t->dev) continue;
        t->dev = fa_hip_malloc(bytes);
        if (!t->dev) return -1;
        if (t->kind == FA_TAB_DFT_OF) continue;    /* second sweep */
        fa_hip_memcpy_h2d(t->dev, t->host, bytes, p->stream);
    }
    fa_hip_stream_sync(p->stream);
    for (i = 0; i < p->ntabs; ++i) {
        fa_table *t = &p->tabs[i];
        if (t->kind != FA_TAB_DFT_OF) continue;
        {
            /* the convolution kernel is itself a DFT: compute it with a
               nested plan on the device, keep a host copy for introspection */
            plan *q = make_c2c_1d_contig(t->n);
            size_t bytes = (size_t)t->len * 2 * sizeof(double);
            if (!q) return -1;
            q->stream = p->stream;
            fa_run(q, (double *)p->tabs[t->src].dev, (double *)p->tabs[t->src].dev + 1,
                   (double *)t->dev, (double *)t->dev + 1);
            if (!t->host) t->host = malloc(bytes);
            fa_hip_memcpy_d2h(t->host, t->dev, bytes, p->stream);
            fa_hip_stream_sync(p->stream);
            fa_plan_free(q);
        }
    }
    return 0;
}

/* Sets p->sched, the scratch slots and lanes that go with it, and creates the schedule's streams and events. */
static void choose_schedule(plan *p) {
    /* batched 1024 x 1024: pass 2 of chunk c-1 and pass 1 of chunk c share a launch (two scratch slots) */
    static int pair_mode = -1;     /* FFTW_AMD_PAIR=0 switches it off */
    int i;
    if (pair_mode < 0) { const char *e = getenv("FFTW_AMD_PAIR"); pair_mode = e ? atoi(e) : 1; }
    p->sched = FA_SCHED_SERIAL;
    p->nslots = 1;
    p->lanes = 1;
    if (pair_mode && !p->cfg.pipeline && p->cfg.lanes <= 1 && p->nsteps == 2 && p->nbufs == 3 && p->chunk > 0 && p->chunk < p->batch &&
        !p->single_chunk &&
        p->steps[0].kind == FFTW_AMD_STEP_PASS && p->steps[1].kind == FFTW_AMD_STEP_PASS &&
        p->steps[0].variant == FFTW_AMD_K_P1024 && p->steps[1].variant == FFTW_AMD_K_P1024 &&
        p->steps[0].src_buf == 0 && p->steps[0].dst_buf == 2 && p->steps[1].src_buf == 2 && p->steps[1].dst_buf == 1 &&
        p->steps[0].tw_n == 0 && p->steps[1].tw_n != 0 && (p->steps[1].flags & FFTW_AMD_F_TW_IN) &&
        p->steps[0].tile_lo_n <= 1 && p->steps[1].tile_lo_n <= 1 &&
        p->steps[0].batch_dim >= 0 && p->steps[1].batch_dim >= 0) {
        p->sched = FA_SCHED_PAIR;
        p->nslots = 2;
    }
    /* chunk pipeline: worth it when there are several chunks of >= 2 steps */
    if (p->sched == FA_SCHED_SERIAL && p->chunk > 0 && p->nsteps >= 2 && chunk_count(p) >= 3 &&
        !p->single_chunk && p->cfg.pipeline) {
        i64 per = 0;
        for (i = 2; i < p->nbufs; ++i) per += p->buf_reals[i];
        if (per > 0 && (size_t)per * sizeof(double) * 3 <= ((size_t)8 << 30)) {
            p->sched = FA_SCHED_PIPE;
            p->nslots = 3;
            p->split = p->nsteps / 2;
            p->pstream[0] = fa_hip_stream_create();
            p->pstream[1] = fa_hip_stream_create();
            for (i = 0; i < 4; ++i) { p->ev_a[i] = fa_hip_event_create(); p->ev_b[i] = fa_hip_event_create(); }
            p->ev_begin = fa_hip_event_create();
            p->ev_end[0] = fa_hip_event_create();
            p->ev_end[1] = fa_hip_event_create();
        }
    }
    /* chunk lanes: chunk c runs all its steps, in order, on stream c % lanes in scratch slot c % lanes; the
       lanes share the machine, so the tail of one lane's launch overlaps the other lane's next launch and
       no dependency crosses the lanes */
    if (p->sched == FA_SCHED_SERIAL && p->cfg.lanes > 1 && p->chunk > 0 && p->nsteps >= 2 && p->nbufs > 2 &&
        !p->single_chunk && chunk_count(p) >= 2) {
        i64 nch = chunk_count(p), per = 0;
        for (i = 2; i < p->nbufs; ++i) per += p->buf_reals[i];
        /* a chunk whose scratch is beyond the budget anyway (one transform with hundreds of MB of scratch: two of
           them in flight leave nothing on the die) gains nothing from a second lane and loses to the doubled
           footprint -- cfg4, n = 15 375 360, 246 MB of scratch per transform: 67.0 ms serial, 71 ... 76 ms with two
           lanes; one 4096 x 4096 image (256 MiB): 14.7 serial, 14.5 with two (tools/perf/perf_lanes_gate.sh) */
        if ((size_t)per * sizeof(double) > p->cfg.chunk_bytes) nch = 0;
        p->lanes = p->cfg.lanes > FA_MAXLANES ? FA_MAXLANES : p->cfg.lanes;
        if (p->lanes > nch) p->lanes = nch > 0 ? (int)nch : 1;
        p->nslots = p->lanes;
        if (p->lanes > 1) {
            p->sched = FA_SCHED_LANES;
            for (i = 0; i < p->lanes; ++i) { p->pstream[i] = fa_hip_stream_create(); p->ev_end[i] = fa_hip_event_create(); }
            p->ev_begin = fa_hip_event_create();
        }
    }
}

int fa_device_init(plan *p) {
    int i;
    if (p->dev_ready) return 0;
    if (fa_hip_device_count() <= 0) {
        fprintf(stderr, "fftw3_amd: no HIP device available: this executor has no CPU "
                        "fallback; fftw_execute cannot run\n");
        return -1;
    }
    if (upload_tables(p)) return -1;
    choose_schedule(p);
    for (i = 2; i < p->nbufs; ++i)
        if (!p->dbuf[i]) {
            p->dbuf[i] = (double *)fa_hip_malloc((size_t)p->buf_reals[i] * sizeof(double) * (size_t)p->nslots);
            if (!p->dbuf[i]) return -1;
        }
    p->dev_ready = 1;
    return 0;
}

/* The device half of fa_plan_free: everything fa_device_init and the executions created. */
void fa_exec_release(plan *p) {
    /* device resources may exist without dev_ready (fa_device_init gave up half way: out of device memory) */
    int i, any = p->dev_ready || p->stage_in || p->stage_out || p->hstream[0] || has_side_streams(p);
    for (i = 0; i < p->ntabs && !any; ++i) any = p->tabs[i].dev != NULL;
    for (i = 2; i < p->nbufs && !any; ++i) any = p->dbuf[i] != NULL;
    if (!any) return;
    fa_hip_stream_sync(p->stream);
    for (i = 0; i < p->ntabs; ++i) fa_hip_free(p->tabs[i].dev);
    for (i = 2; i < p->nbufs; ++i) fa_hip_free(p->dbuf[i]);
    fa_hip_free(p->stage_in);
    fa_hip_free(p->stage_out);
    if (p->hstream[0]) fa_hip_stream_destroy(p->hstream[0]);
    if (p->hstream[1]) fa_hip_stream_destroy(p->hstream[1]);
    if (p->sched == FA_SCHED_PIPE)
        for (i = 0; i < 4; ++i) { fa_hip_event_destroy(p->ev_a[i]); fa_hip_event_destroy(p->ev_b[i]); }
    if (has_side_streams(p)) {
        fa_hip_event_destroy(p->ev_begin);
        for (i = 0; i < FA_MAXLANES; ++i) {
            if (p->ev_end[i]) fa_hip_event_destroy(p->ev_end[i]);
            if (p->pstream[i]) fa_hip_stream_destroy(p->pstream[i]);
        }
    }
}

/* ------------------------------------------------------------- host arrays */

/* How a host array is laid out in its device staging buffer.  Offsets count doubles relative to
   the pointer of the "real" part; im is the caller's real -> imaginary distance. */
typedef struct {
    int two;        /* 1: two packed planes of `span` doubles each, 0: one span [lo, hi] covering both parts */
    i64 lo, hi;     /* touched offsets (two: of each plane; one span: of both parts together) */
    i64 span;
    i64 im_dev;     /* real -> imaginary distance inside the staging buffer */
} stage_layout;

static stage_layout stage_layout_of(i64 lo, i64 hi, i64 im) {
    stage_layout L;
    L.span = hi - lo + 1;
    L.two = im != 0 && llabs(im) >= L.span;
    if (L.two) {
        L.lo = lo; L.hi = hi;
        L.im_dev = im > 0 ? L.span : -L.span;
    } else {
        L.lo = im < 0 ? lo + im : lo;
        L.hi = im > 0 ? hi + im : hi;
        L.span = L.hi - L.lo + 1;
        L.im_dev = im;
    }
    return L;
}
static size_t stage_bytes(const stage_layout *L) { return (size_t)L->span * (L->two ? 2 : 1) * sizeof(double); }
/* device address that plays the role of the caller's real-part pointer */
static double *stage_origin(const stage_layout *L, double *st) {
    return st - L->lo + ((L->two && L->im_dev < 0) ? L->span : 0);
}
static void stage_h2d(const stage_layout *L, double *st, const double *re, i64 im, void *stream) {
    double *o = stage_origin(L, st);
    if (L->two) {
        fa_hip_memcpy_h2d(o + L->lo, re + L->lo, (size_t)L->span * sizeof(double), stream);
        fa_hip_memcpy_h2d(o + L->im_dev + L->lo, re + im + L->lo, (size_t)L->span * sizeof(double), stream);
    } else {
        fa_hip_memcpy_h2d(o + L->lo, re + L->lo, (size_t)L->span * sizeof(double), stream);
    }
}
static void stage_d2h(const stage_layout *L, double *st, double *re, i64 im, void *stream) {
    double *o = stage_origin(L, st);
    if (L->two) {
        fa_hip_memcpy_d2h(re + L->lo, o + L->lo, (size_t)L->span * sizeof(double), stream);
        fa_hip_memcpy_d2h(re + im + L->lo, o + L->im_dev + L->lo, (size_t)L->span * sizeof(double), stream);
    } else {
        fa_hip_memcpy_d2h(re + L->lo, o + L->lo, (size_t)L->span * sizeof(double), stream);
    }
}

static double *stage_buf(double **slot, size_t *have, size_t need) {
    if (*have < need) {
        fa_hip_free(*slot);
        *slot = (double *)fa_hip_malloc(need);
        if (!*slot) {
            fprintf(stderr, "fftw3_amd: no device memory to stage the host arrays of this execution\n");
            abort();
        }
        *have = need;
    }
    return *slot;
}

/* The arrays of one execution as the device sees them.  Device arrays pass through.  Plain host arrays are staged
   through device copies (slow path, PCIe): whole around the launches, or -- `piped` -- chunk by chunk on the plan's two
   copy streams, hstream[0] up and hstream[1] down. */
typedef struct {
    double *ri, *ro;            /* the caller's arrays */
    double *din, *dout;         /* their device views */
    i64 in_im, out_im;          /* re -> im distances on the device, what the steps of this call get */
    i64 out_im_host;            /* the caller's, on the output side */
    int in_host, out_host, inplace, piped;
    stage_layout Lin, Lout;
    i64 ibs, obs, ispan, ospan; /* piped: batch strides and one transform's span on both sides */
    void **ev_in, **ev_out;     /* piped: chunk c is on the device / its download may start */
} host_io;

/* A split array whose imaginary plane lies beyond the real one (|im| >= span: typically two separate allocations,
   the usual fftw_plan_guru_split_dft call) is staged as two packed planes -- never as one span from the lower to the
   upper plane, which would read and write whatever the caller keeps between the two allocations. */
static void io_layouts(const plan *p, host_io *h, double *ii, double *io) {
    stage_layout *Lin = &h->Lin, *Lout = &h->Lout;
    *Lin = stage_layout_of(p->in_lo, p->in_hi, h->in_im);
    *Lout = stage_layout_of(p->out_lo, p->out_hi, h->out_im);
    h->inplace = h->in_host && h->out_host && h->ro == h->ri &&
                 (io == ii || FA_REAL_OUT(p->type) || FA_REAL_IN(p->type));
    if (!h->inplace) return;
    /* both views share one staging image: same plane layout, union of the spans */
    if (Lin->two != Lout->two || (Lin->two && (Lin->lo != Lout->lo || Lin->hi != Lout->hi || Lin->im_dev != Lout->im_dev))) {
        fprintf(stderr, "fftw3_amd: in-place execution on host arrays whose input and output views have "
                        "different split layouts is not supported\n");
        abort();
    }
    if (!Lin->two) {
        if (Lout->lo < Lin->lo) Lin->lo = Lout->lo;
        if (Lout->hi > Lin->hi) Lin->hi = Lout->hi;
        Lin->span = Lin->hi - Lin->lo + 1;
        Lout->lo = Lin->lo; Lout->hi = Lin->hi; Lout->span = Lin->span;
    }
}

/* Host pipeline: a batch that is dense on both sides (every transform's span below the batch stride) and
   runs in several chunks is staged chunk by chunk on two copy streams -- upload of chunk c+1, compute of
   chunk c and download of chunk c-1 overlap, so an unmodified host caller sees max(H2D, D2H) of the PCIe
   link instead of their sum plus the compute.  Everything else is staged whole. */
static void io_admit_pipe(plan *p, host_io *h) {
    h->piped = 0;
    h->ev_in = h->ev_out = NULL;
    if (h->in_host && h->out_host && !h->inplace && !h->Lin.two && !h->Lout.two && p->hrank == 1 && !p->prof_ms &&
        p->chunk > 0 && p->chunk < p->batch && !p->single_chunk && p->sched != FA_SCHED_PIPE) {
        const i64 B = p->batch, ibs = p->hdims[0].is, obs = p->hdims[0].os;
        const i64 it_span = h->Lin.span - (B - 1) * ibs, ot_span = h->Lout.span - (B - 1) * obs;   /* one transform's span */
        static int hp_mode = -1;        /* FFTW_AMD_HOST_PIPELINE=0 switches it off */
        if (hp_mode < 0) { const char *e = getenv("FFTW_AMD_HOST_PIPELINE"); hp_mode = e ? atoi(e) : 1; }
        if (hp_mode && ibs > 0 && obs > 0 && it_span > 0 && ot_span > 0 && it_span <= ibs && ot_span <= obs &&
            h->Lout.span == p->out_written) {
            h->piped = 1;
            h->ibs = ibs; h->obs = obs; h->ispan = it_span; h->ospan = ot_span;
            if (!p->hstream[0]) { p->hstream[0] = fa_hip_stream_create(); p->hstream[1] = fa_hip_stream_create(); }
            h->ev_in = (void **)calloc((size_t)chunk_count(p), sizeof(void *));
            h->ev_out = (void **)calloc((size_t)chunk_count(p), sizeof(void *));
        }
    }
}

/* piped: the uploads are queued now, in chunk order, behind whatever the caller's stream already holds */
static void io_upload_chunks(plan *p, host_io *h) {
    i64 c;
    void *e0 = fa_hip_event_create();
    fa_hip_event_record(e0, p->stream);
    fa_hip_stream_wait_event(p->hstream[0], e0);
    fa_hip_stream_wait_event(p->hstream[1], e0);
    fa_hip_event_destroy(e0);
    for (c = 0; c < chunk_count(p); ++c) {
        const i64 lo = h->Lin.lo + c * p->chunk * h->ibs, len = (chunk_len(p, c) - 1) * h->ibs + h->ispan;
        fa_hip_memcpy_h2d(h->din + lo, h->ri + lo, (size_t)len * sizeof(double), p->hstream[0]);
        h->ev_in[c] = fa_hip_event_create();
        fa_hip_event_record(h->ev_in[c], p->hstream[0]);
    }
}

/* Decides how the arrays of this call reach the device, allocates the staging buffers and queues the uploads. */
static void io_begin(plan *p, host_io *h, double *ri, double *ii, double *ro, double *io) {
    h->ri = h->din = ri;
    h->ro = h->dout = ro;
    h->in_im = FA_REAL_IN(p->type) ? 0 : ii - ri;
    h->out_im = FA_REAL_OUT(p->type) ? 0 : io - ro;
    h->out_im_host = 0;
    h->in_host = !fa_hip_is_device_ptr(ri);
    h->out_host = !fa_hip_is_device_ptr(ro);
    io_layouts(p, h, ii, io);
    io_admit_pipe(p, h);
    if (h->in_host) {
        double *st = stage_buf(&p->stage_in, &p->stage_in_bytes, stage_bytes(&h->Lin));
        h->din = stage_origin(&h->Lin, st);
        if (h->piped) io_upload_chunks(p, h);
        else stage_h2d(&h->Lin, st, ri, h->in_im, p->stream);
        h->in_im = h->Lin.im_dev;
    }
    if (h->out_host) {
        if (h->inplace) {
            h->dout = h->din;
        } else {
            double *st = stage_buf(&p->stage_out, &p->stage_out_bytes, stage_bytes(&h->Lout));
            /* gaps between output elements must survive the round trip */
            if ((i64)(stage_bytes(&h->Lout) / sizeof(double)) != p->out_written)
                stage_h2d(&h->Lout, st, ro, h->out_im, p->stream);
            h->dout = stage_origin(&h->Lout, st);
        }
        h->out_im_host = h->out_im;
        h->out_im = h->Lout.im_dev;
    }
}

/* chunk c is on the device before `stream` goes on */
static void io_chunk_ready(const host_io *h, i64 c, void *stream) {
    if (h->piped) fa_hip_stream_wait_event(stream, h->ev_in[c]);
}

/* chunk c is complete on `stream`: download it while the next launches run */
static void io_chunk_done(plan *p, host_io *h, i64 c, void *stream) {
    if (h->piped) {
        const i64 lo = h->Lout.lo + c * p->chunk * h->obs, len = (chunk_len(p, c) - 1) * h->obs + h->ospan;
        h->ev_out[c] = fa_hip_event_create();
        fa_hip_event_record(h->ev_out[c], stream);
        fa_hip_stream_wait_event(p->hstream[1], h->ev_out[c]);
        fa_hip_memcpy_d2h(h->ro + lo, h->dout + lo, (size_t)len * sizeof(double), p->hstream[1]);
    }
}

static void io_end(plan *p, host_io *h) {
    if (h->piped) {
        i64 c;
        fa_hip_stream_sync(p->stream);
        fa_hip_stream_sync(p->hstream[1]);
        for (c = 0; c < chunk_count(p); ++c) {
            if (h->ev_in[c]) fa_hip_event_destroy(h->ev_in[c]);
            if (h->ev_out[c]) fa_hip_event_destroy(h->ev_out[c]);
        }
        free(h->ev_in);
        free(h->ev_out);
        return;
    }
    if (h->out_host) stage_d2h(&h->Lout, h->inplace ? p->stage_in : p->stage_out, h->ro, h->out_im_host, p->stream);
    if (h->in_host || h->out_host) fa_hip_stream_sync(p->stream);
}

/* ---------------------------------------------------------------- schedules */

/* step i with the re/im distances of this call: split-array callers may pass different ones per call, and staged host
   planes lie at a distance of their own.  Both ends of a step count: a plan of rank >= 2 runs its later axes in place on
   the output array (buf1 -> buf1), a c2r plan may run its leading axes in place on the input (buf0 -> buf0). */
static fftw_amd_step_desc step_for_call(const plan *p, int i, i64 in_im, i64 out_im) {
    fftw_amd_step_desc d = p->steps[i];
    if (!FA_REAL_IN(p->type)) {
        if (d.src_buf == 0 && d.src_im == p->in_im) d.src_im = in_im;
        if (d.dst_buf == 0 && d.dst_im == p->in_im) d.dst_im = in_im;
    }
    if (!FA_REAL_OUT(p->type)) {
        if (d.src_buf == 1 && d.src_im == p->out_im) d.src_im = out_im;
        if (d.dst_buf == 1 && d.dst_im == p->out_im) d.dst_im = out_im;
    }
    return d;
}

/* bufs with the scratch buffers moved to scratch slot `slot` */
static void slot_bufs(const plan *p, double *const *bufs, int slot, double **sb) {
    int i;
    sb[0] = bufs[0];
    sb[1] = bufs[1];
    for (i = 2; i < p->nbufs; ++i) sb[i] = bufs[i] + (i64)slot * p->buf_reals[i];
}

/* FA_SCHED_PAIR.  Launch k: pass 2 of chunk k-1 (scratch slot (k-1) & 1) + pass 1 of chunk k (slot k & 1).  A profiled
   execution times every launch under step 0, with a sync per launch.  Returns 1 when the kernel refuses the first
   launch (not the pair it is built for) and nothing has run. */
static int run_pair(plan *p, host_io *h, double *const *bufs, void *const *tabs) {
    const i64 nchunks = chunk_count(p);
    const fftw_amd_step_desc d1 = step_for_call(p, 0, h->in_im, h->out_im), d2 = step_for_call(p, 1, h->in_im, h->out_im);
    i64 k;
    for (k = 0; k <= nchunks; ++k) {
        double *sb1[FA_MAXBUF], *sb2[FA_MAXBUF];
        const i64 cn1 = k < nchunks ? chunk_len(p, k) : 0, cn2 = k > 0 ? chunk_len(p, k - 1) : 0;
        void *e0 = NULL, *e1 = NULL;
        int refused;
        slot_bufs(p, bufs, (int)(k & 1), sb1);
        slot_bufs(p, bufs, (int)((k + 1) & 1), sb2);
        if (p->prof_ms) { e0 = fa_hip_event_create(); e1 = fa_hip_event_create(); fa_hip_event_record(e0, p->stream); }
        if (k < nchunks) io_chunk_ready(h, k, p->stream);
        refused = fa_hip_launch_pair1024(&d2, sb2, (k - 1) * p->chunk, cn2, &d1, sb1, k * p->chunk, cn1, tabs, p->stream);
        if (refused && k > 0) abort();
        if (!refused && k > 0) io_chunk_done(p, h, k - 1, p->stream);
        if (p->prof_ms) {
            fa_hip_event_record(e1, p->stream);
            fa_hip_stream_sync(p->stream);
            if (!refused) { p->prof_ms[0] += (double)fa_hip_event_elapsed_ms(e0, e1); p->prof_launches[0] += 1; }
            fa_hip_event_destroy(e0);
            fa_hip_event_destroy(e1);
        }
        if (refused) return 1;
    }
    return 0;
}

/* the HIP events of a profiled execution: a pair around every launch, on the stream the launch runs on */
typedef struct { void **ev; i64 n; } prof_events;

static void prof_mark(prof_events *t, void *stream) {
    if (!t->ev) return;
    t->ev[t->n] = fa_hip_event_create();
    fa_hip_event_record(t->ev[t->n++], stream);
}

/* after the execution has drained: launch l of the chunk loop is step l % nsteps */
static void prof_collect(plan *p, prof_events *t) {
    i64 l;
    if (!t->ev) return;
    fa_hip_stream_sync(p->stream);
    for (l = 0; 2 * l < t->n; ++l) {
        p->prof_ms[l % p->nsteps] += (double)fa_hip_event_elapsed_ms(t->ev[2 * l], t->ev[2 * l + 1]);
        p->prof_launches[l % p->nsteps] += 1;
        fa_hip_event_destroy(t->ev[2 * l]);
        fa_hip_event_destroy(t->ev[2 * l + 1]);
    }
    free(t->ev);
}

/* The steps of chunk c in scratch slot `slot`.  Serial and lanes: all on `home`.  Pipeline: stage A (steps
   [0, split)) on pstream[0] and stage B on pstream[1], ordered per slot by the events ev_a / ev_b. */
static void launch_chunk(plan *p, const host_io *h, double *const *sb, void *const *tabs, i64 c, int slot, void *home,
                         prof_events *prof) {
    const int pipe = p->sched == FA_SCHED_PIPE;
    int i;
    for (i = 0; i < p->nsteps; ++i) {
        const fftw_amd_step_desc d = step_for_call(p, i, h->in_im, h->out_im);
        void *st = pipe ? p->pstream[i < p->split ? 0 : 1] : home;
        /* stage A reuses a slot only after stage B of its previous user is done */
        if (pipe && i == 0 && c >= p->nslots) fa_hip_stream_wait_event(st, p->ev_b[slot]);
        if (pipe && i == p->split) fa_hip_stream_wait_event(st, p->ev_a[slot]);
        prof_mark(prof, st);
        if (fa_hip_launch_step(&d, sb, tabs, c * p->chunk, chunk_len(p, c), st)) abort();
        prof_mark(prof, st);
        if (pipe && i == p->split - 1) fa_hip_event_record(p->ev_a[slot], st);
        if (pipe && i == p->nsteps - 1) fa_hip_event_record(p->ev_b[slot], st);
    }
}

/* FA_SCHED_SERIAL, _PIPE and _LANES: one pass over the chunks.  Chunk c works in scratch slot c % nslots (serial: slot
   0); it arrives and completes on its lane's stream (lanes) or on the caller's.  Profiled executions keep the lanes:
   the HIP events around a launch sit on the lane's own stream and time the launch as it really runs, beside the other
   lane's (rocprofv3's kernel durations see the same). */
static void run_chunks(plan *p, host_io *h, double *const *bufs, void *const *tabs) {
    const i64 nchunks = chunk_count(p);
    const int nside = p->sched == FA_SCHED_PIPE ? 2 : (p->sched == FA_SCHED_LANES ? p->lanes : 0);
    prof_events prof = { NULL, 0 };
    i64 c;
    int i;
    if (p->prof_ms) prof.ev = (void **)malloc(sizeof(void *) * (size_t)(2 * nchunks * p->nsteps));
    if (nside) {
        /* the side streams start after everything already queued on the caller's stream */
        fa_hip_event_record(p->ev_begin, p->stream);
        for (i = 0; i < nside; ++i) fa_hip_stream_wait_event(p->pstream[i], p->ev_begin);
    }
    for (c = 0; c < nchunks; ++c) {
        const int slot = p->sched == FA_SCHED_SERIAL ? 0 : (int)(c % p->nslots);
        void *home = p->sched == FA_SCHED_LANES ? p->pstream[slot] : p->stream;
        double *sb[FA_MAXBUF];
        slot_bufs(p, bufs, slot, sb);
        io_chunk_ready(h, c, home);
        launch_chunk(p, h, sb, tabs, c, slot, home, &prof);
        io_chunk_done(p, h, c, home);
    }
    /* the caller's stream continues after the side streams have drained */
    for (i = 0; i < nside; ++i) {
        fa_hip_event_record(p->ev_end[i], p->pstream[i]);
        fa_hip_stream_wait_event(p->stream, p->ev_end[i]);
    }
    prof_collect(p, &prof);
}

/* ------------------------------------------------------------------ driver */

static void fa_run_locked(plan *p, double *ri, double *ii, double *ro, double *io) {
    double *bufs[FA_MAXBUF];
    void *tabs[FA_MAXTAB];
    host_io h;
    int i;

    if (p->batch == 0) return;
    if (fa_device_init(p)) abort();

    io_begin(p, &h, ri, ii, ro, io);
    bufs[0] = h.din;
    bufs[1] = h.dout;
    for (i = 2; i < p->nbufs; ++i) bufs[i] = p->dbuf[i];
    for (i = 0; i < p->ntabs; ++i) tabs[i] = p->tabs[i].dev;
    /* not the pair the kernel is built for: ordinary launches, in this execution and from now on (the two scratch
       slots stay allocated) */
    if (p->sched == FA_SCHED_PAIR && run_pair(p, &h, bufs, tabs)) p->sched = FA_SCHED_SERIAL;
    if (p->sched != FA_SCHED_PAIR) run_chunks(p, &h, bufs, tabs);
    io_end(p, &h);
}

/* serialised per plan: concurrent fftw_execute calls on one plan are legal in the
   reference (A.c:433, re-entrant executors) but here they share scratch and streams */
void fa_run(plan *p, double *ri, double *ii, double *ro, double *io) {
    pthread_mutex_lock(&p->lock);
    /* New-array execution on arrays aligned differently from the plan's own (a caller error by FFTW's rules,
       fftw3.h "new-array execute"): the plan may hold steps whose kernels rely on the 16-byte alignment it
       saw at planning time and have no other executor.  Run the FFTW_UNALIGNED twin instead -- same problem,
       same tables' values, only kernels that serve every alignment -- rather than abort() inside a library. */
    if (!(p->flags & FFTW_UNALIGNED) && p->ri && p->ro && p->batch > 0 &&
        ((((size_t)ri ^ (size_t)p->ri) | ((size_t)ii ^ (size_t)p->ii) | ((size_t)ro ^ (size_t)p->ro) | ((size_t)io ^ (size_t)p->io)) & 15)) {
        if (!p->alt) p->alt = fa_unaligned_twin(p);
        if (p->alt) {
            p->alt->stream = p->stream;
            fa_run_locked(p->alt, ri, ii, ro, io);
            pthread_mutex_unlock(&p->lock);
            return;
        }
    }
    fa_run_locked(p, ri, ii, ro, io);
    pthread_mutex_unlock(&p->lock);
}

/* One execution on the plan's own arrays with a HIP event pair around every
   launch (on the stream the kernels run on).  ms[i] / launches[i] accumulate
   the time and the number of launches of step i (p->prof_ms / p->prof_launches, set under the plan's lock, never
   process-wide: another plan's execute on another thread must not see them).  Returns the step count. */
int fftw_amd_execute_profiled(fftw_plan p, double *ms, long long *launches, int cap) {
    int i;
    if (!p || cap < p->nsteps) return -1;
    for (i = 0; i < p->nsteps; ++i) { ms[i] = 0.0; launches[i] = 0; }
    pthread_mutex_lock(&p->lock);
    p->prof_ms = ms;
    p->prof_launches = launches;
    fa_run_locked(p, p->ri, p->ii, p->ro, p->io);
    p->prof_ms = NULL;
    p->prof_launches = NULL;
    pthread_mutex_unlock(&p->lock);
    return p->nsteps;
}
