/*
 * planner.c -- the static GPU planner: turns a DFT problem (dims + strides)
 * into a short list of kernel launches ("steps").
 *
 * It replaces the reference's search-based planner (ifftw_mkplan,
 * fftw/fftw_api.c:15300-15426) and restates the *structure* of the solvers it
 * would have picked:
 *   - Cooley-Tukey n = L1*L2*...  (ct_mkplan A.c:2183-2202)  -> fa_emit_ct
 *   - vector / rank loops (vrank_geq1 A.c:4627, rank_geq2 A.c:4435) -> loop
 *     dims carried by every step and executed by the kernel grid
 *   - Rader (A.c:4187-4261) and Bluestein (A.c:1642-1688) for sizes with a
 *     prime factor the LDS kernel has no stage for
 *   - rdft2 via half-length complex DFT + untangle (ct_hc2c A.c:5579-5590)
 * A CPU cost model is meaningless on the GPU, so there is no search: the
 * decomposition is a function of n and of which index is contiguous.
 *
 * Planning only: the plan object, its tables, fa_build and fa_sprint.  Bringing a plan onto the device and running
 * it is exec.c.
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fa_plan.h"
#include "fa_hip.h"

typedef struct fftw_plan_s plan;

/* scratch per chunk: what one chunk writes between two passes must still be in the 256 MiB
   Infinity Cache when the next pass reads it.  Round 3 (tests/micro/mall_probe.hip, profiles/r03_mall_probe.txt):
   the two-pass 2^20 plan as pure data movement takes 10.0 us per transform as serial launches over 256 MiB
   chunks, and 8.2 us when chunk c runs on stream c % 2 with 96 ... 128 MiB of scratch per chunk (two lanes,
   256 MiB of scratch in flight): the tail of one lane's launch is filled by the other lane's, and the
   reuse distance of a scratch line is a few transforms instead of a whole 1 GiB launch pair. */
#define FA_DEFAULT_CHUNK_BYTES ((size_t)128 << 20)
/* Where the planner reads the environment -- the block that ends with nt_policy() below, and nowhere else:
     fa_default_cfg    the tunables of fa_cfg, into the plan's own copy when the plan is created (fa_plan_new);
     fa_read_knobs     the test switches of fa_knobs, into the plan's own copy at the top of every fa_build;
     transposes_enabled, nt_policy
                       FFTW_AMD_NO_TRANSPOSE and FFTW_AMD_NT, once per process, at their first use.
   Process-wide planner state is therefore those two settings and the documented setter below (read and written
   atomically); everything else a plan is built from lives in the plan, so threads that plan with different settings
   do not see each other's, and the builds of one fa_build (a dry run, up to two sized runs) see one environment. */
static size_t g_chunk_bytes = FA_DEFAULT_CHUNK_BYTES;

void fftw_amd_set_chunk_bytes(size_t nbytes) {
    __atomic_store_n(&g_chunk_bytes, nbytes ? nbytes : FA_DEFAULT_CHUNK_BYTES, __ATOMIC_RELAXED);
}

static i64 iabs(i64 v) { return v < 0 ? -v : v; }
static int is_pow2(i64 n) { return (n & (n - 1)) == 0; }

/* The opt-in plan families (fa_plan.h), in the order the FFTW_MEASURE search tries them.  Why each is off under
   FFTW_ESTIMATE, what it takes and what was measured is said once, at its emitter: emit_r2c_decimated and
   emit_c2r_decimated, emit_real_image (real_img and real_imgl), emit_real_volume, emit_vol3d, emit_vol_planes,
   emit_images (img_wide). */
#define T_REAL (1u << FA_R2C | 1u << FA_C2R)
#define T_C2C  (1u << FA_C2C)
const fa_family fa_family_table[FA_NFAMILIES] = {
    { "FFTW_AMD_REAL_DEC",   offsetof(fa_cfg, real_dec),     16, T_REAL, 0, FA_ACCEPT_ANY },
    { "FFTW_AMD_REAL_IMG",   offsetof(fa_cfg, real_img),     32, T_REAL, 0, FA_ACCEPT_ANY },
    { "FFTW_AMD_REAL_VOL",   offsetof(fa_cfg, real_vol),    128, T_REAL, 3, FFTW_AMD_K_VOL3DR },
    { "FFTW_AMD_REAL_IMGL",  offsetof(fa_cfg, real_imgl),   256, T_REAL, 2, FFTW_AMD_K_IMG2DLR },
    { "FFTW_AMD_VOL3D",      offsetof(fa_cfg, vol3d),        64, T_C2C,  3, FFTW_AMD_K_VOL3D },
    { "FFTW_AMD_VOL_PLANES", offsetof(fa_cfg, vol_planes),  512, T_C2C,  3, FA_ACCEPT_PLANES },
    { "FFTW_AMD_IMG_WIDE",   offsetof(fa_cfg, img_wide),   1024, T_C2C,  2, FFTW_AMD_K_IMG2DW },
};

fa_cfg fa_default_cfg(void) {
    fa_cfg c;
    const char *e;
    int i;
    c.chunk_bytes = __atomic_load_n(&g_chunk_bytes, __ATOMIC_RELAXED);
    c.pipeline = 0;       /* two-stream chunk pipeline: off under FFTW_ESTIMATE (each kernel then owns the machine and
                             its launch duration is its roofline), a FFTW_MEASURE candidate, FFTW_AMD_PIPELINE=1 */
    c.lmax_multi = 1024;
    c.small_tiles = 1;
    c.long_first = 0;
    c.tile_elems = 0;
    c.lanes = 2;
    e = getenv("FFTW_AMD_CHUNK_BYTES");
    if (e && atoll(e) > 0) c.chunk_bytes = (size_t)atoll(e);
    e = getenv("FFTW_AMD_SMALL_TILES");
    if (e) c.small_tiles = atoi(e);
    e = getenv("FFTW_AMD_TILE_ELEMS");
    if (e) c.tile_elems = atoll(e);
    e = getenv("FFTW_AMD_LONG_FIRST");
    if (e) c.long_first = atoi(e);
    e = getenv("FFTW_AMD_PIPELINE");
    if (e) c.pipeline = atoi(e);
    e = getenv("FFTW_AMD_LMAX_MULTI");
    if (e && atoll(e) >= 16) c.lmax_multi = (int)atoll(e);
    e = getenv("FFTW_AMD_LANES");
    if (e && atoi(e) >= 1 && atoi(e) <= FA_MAXLANES) c.lanes = atoi(e);
    for (i = 0; i < FA_NFAMILIES; ++i) {
        e = getenv(fa_family_table[i].env);
        fa_family_set(&c, &fa_family_table[i], e && atoi(e) != 0);
    }
    return c;
}

/* The test switches (fa_knobs).  PRESENT: the int at `off` is 1 when the variable exists, whatever it holds -- the
   rule these hooks have always had.  LENS: the split that FFTW_AMD_FORCE_LENS="L1,L2,..." fixes for the axis whose
   length is the product (tests/test_gpu_menu.py reaches every kernel variant with it). */
enum { KNOB_PRESENT, KNOB_LENS, KNOB_P1024_ORDER };
static const struct { const char *name; size_t off; int rule; } g_knob_table[] = {
    { "FFTW_AMD_NO_TUNED",       offsetof(fa_knobs, no_tuned),       KNOB_PRESENT },
    { "FFTW_AMD_NO_3S",          offsetof(fa_knobs, no_3s),          KNOB_PRESENT },
    { "FFTW_AMD_NO_R1",          offsetof(fa_knobs, no_r1),          KNOB_PRESENT },
    { "FFTW_AMD_NO_BLUE_ROWS",   offsetof(fa_knobs, no_blue_rows),   KNOB_PRESENT },
    { "FFTW_AMD_NO_NARROW",      offsetof(fa_knobs, no_narrow),      KNOB_PRESENT },
    { "FFTW_AMD_NO_SPLIT_COSTS", offsetof(fa_knobs, no_split_costs), KNOB_PRESENT },
    { "FFTW_AMD_NO_LO_DFT",      offsetof(fa_knobs, no_lo_dft),      KNOB_PRESENT },
    { "FFTW_AMD_NO_IMG2D",       offsetof(fa_knobs, no_img2d),       KNOB_PRESENT },
    { "FFTW_AMD_NO_R2CROWS",     offsetof(fa_knobs, no_r2crows),     KNOB_PRESENT },
    { "FFTW_AMD_R2R_UNFUSED",    offsetof(fa_knobs, r2r_unfused),    KNOB_PRESENT },
    { "FFTW_AMD_NO_RADIX4",      offsetof(fa_knobs, no_radix4),      KNOB_PRESENT },
    { "FFTW_AMD_FORCE_RADIX4",   offsetof(fa_knobs, force_radix4),   KNOB_PRESENT },
    { "FFTW_AMD_FORCE_LENS",     offsetof(fa_knobs, force_lens),     KNOB_LENS },
    { "FFTW_AMD_P1024_ORDER",    offsetof(fa_knobs, p1024_order),    KNOB_P1024_ORDER },
};

static void fa_read_knobs(fa_knobs *k) {
    size_t i;
    memset(k, 0, sizeof(*k));
    for (i = 0; i < sizeof(g_knob_table) / sizeof(g_knob_table[0]); ++i) {
        const char *c = getenv(g_knob_table[i].name);
        if (g_knob_table[i].rule == KNOB_PRESENT) {
            *(int *)((char *)k + g_knob_table[i].off) = c != NULL;
            continue;
        }
        if (g_knob_table[i].rule == KNOB_P1024_ORDER) {
            k->p1024_order = (c && atoi(c) >= 0) ? atoi(c) : FA_P1024_ORDER_DEFAULT;
            continue;
        }
        /* at most FA_MAXPASS entries are read (what follows them is not looked at); an entry below 1 or anything
           but a comma between two entries voids the list, and so does a single entry */
        k->force_prod = 1;
        while (c && *c && k->n_force_lens < FA_MAXPASS) {
            char *end;
            long long v = strtoll(c, &end, 10);
            if (end == c || v < 1 || (*end && *end != ',')) { k->n_force_lens = 0; break; }
            k->force_lens[k->n_force_lens++] = v;
            k->force_prod *= v;
            c = (*end == ',') ? end + 1 : end;
        }
        if (k->n_force_lens < 2) k->n_force_lens = 0;
    }
}

/* FFTW_AMD_NO_TRANSPOSE=1 keeps every copy on the element-wise kernels (measurements: tools/perf/perf_transpose.py).
   Read once per process, as documented and tested (tests/test_gpu_footprint.py runs it in a child for that reason):
   fa_match_transpose takes no plan, and api.c calls it outside fa_build too */
static int transposes_enabled(void) {
    static int on = -1;
    if (on < 0) { const char *e = getenv("FFTW_AMD_NO_TRANSPOSE"); on = !(e && atoi(e)); }
    return on;
}

/* FFTW_AMD_NT, the cache policy of mark_streaming_accesses: 0 never, 1 by size (default), 2 always.  Read once per
   process */
static int nt_policy(void) {
    static int policy = -1;
    if (policy < 0) { const char *e = getenv("FFTW_AMD_NT"); policy = e ? atoi(e) : 1; }
    return policy;
}

/* ------------------------------------------------------------------ plan */

plan *fa_plan_new(void) {
    plan *p = (plan *)calloc(1, sizeof(plan));
    if (!p) return NULL;
    p->nbufs = 2;
    p->in_im = p->out_im = 1;
    p->cfg = fa_default_cfg();
    pthread_mutex_init(&p->lock, NULL);
    return p;
}

static void plan_reset_build(plan *p) {
    int i;
    free(p->steps);
    p->steps = NULL;
    p->nsteps = p->cap_steps = 0;
    for (i = 0; i < p->ntabs; ++i) free(p->tabs[i].host);
    memset(p->tabs, 0, sizeof(p->tabs));
    p->ntabs = 0;
    p->nbufs = 2;
    memset(p->buf_reals, 0, sizeof(p->buf_reals));
    memset(p->buf_busy, 0, sizeof(p->buf_busy));
    p->failed = 0;
    p->est_flops = 0;
}

void fa_plan_free(plan *p) {
    int i;
    if (!p) return;
    if (p->alt) { fa_plan_free(p->alt); p->alt = NULL; }
    fa_exec_release(p);        /* the device half: tables, scratch, staging, streams and events (exec.c) */
    for (i = 0; i < p->ntabs; ++i) free(p->tabs[i].host);
    free(p->steps);
    pthread_mutex_destroy(&p->lock);
    free(p);
}

/* ---------------------------------------------------------------- tables */

static int tab_find(plan *p, int kind, i64 n, i64 aux) {
    int i;
    for (i = 0; i < p->ntabs; ++i)
        if (p->tabs[i].kind == kind && p->tabs[i].n == n && p->tabs[i].aux == aux) return i;
    return -1;
}

static int tab_new(plan *p, int kind, i64 n, i64 aux, i64 len, size_t elem) {
    fa_table *t;
    if (p->ntabs >= FA_MAXTAB) { p->failed = 1; return 0; }
    t = &p->tabs[p->ntabs];
    t->kind = kind;
    t->n = n;
    t->aux = aux;
    t->len = len;
    t->src = -1;
    t->host = len ? calloc((size_t)len, elem) : NULL;
    t->dev = NULL;
    return p->ntabs++;
}

static int tab_stage(plan *p, i64 L) {
    int id = tab_find(p, FA_TAB_STAGE, L, 0);
    double *h;
    i64 m;
    if (id >= 0) return id;
    id = tab_new(p, FA_TAB_STAGE, L, 0, L, 2 * sizeof(double));
    h = (double *)p->tabs[id].host;
    for (m = 0; m < L; ++m) fa_cexp(m, L, h + 2 * m);
    return id;
}

/* w^m = lo[m & (2^s - 1)] * hi[m >> s], both factors exact table entries:
   the reference's sqrt(n) scheme for large radix steps
   (fftw/fftw_api.c:18989-19011, rotate A.c:18920-18941) */
static void tab_tw2(plan *p, i64 n, int *lo, int *hi, int *shift) {
    int s = 0, id;
    i64 m, nlo, nhi;
    double *h;
    while (((i64)1 << (2 * s)) < n) ++s;
    nlo = (i64)1 << s;
    nhi = (n + nlo - 1) / nlo;
    *shift = s;
    id = tab_find(p, FA_TAB_TW_LO, n, s);
    if (id < 0) {
        id = tab_new(p, FA_TAB_TW_LO, n, s, nlo, 2 * sizeof(double));
        h = (double *)p->tabs[id].host;
        for (m = 0; m < nlo; ++m) fa_cexp(m, n, h + 2 * m);
    }
    *lo = id;
    id = tab_find(p, FA_TAB_TW_HI, n, s);
    if (id < 0) {
        id = tab_new(p, FA_TAB_TW_HI, n, s, nhi, 2 * sizeof(double));
        h = (double *)p->tabs[id].host;
        for (m = 0; m < nhi; ++m) fa_cexp(m << s, n, h + 2 * m);
    }
    *hi = id;
}

/* Bluestein chirp w[k] = exp(+i pi k^2 / n), k^2 reduced mod 2n first
   (reference bluestein_sequence, fftw/fftw_api.c:1598-1611) */
static int tab_chirp(plan *p, i64 n, i64 nb) {
    int id = tab_find(p, FA_TAB_CHIRP, n, nb);
    double *h;
    i64 k;
    if (id >= 0) return id;
    id = tab_new(p, FA_TAB_CHIRP, n, nb, nb, 2 * sizeof(double));
    h = (double *)p->tabs[id].host;
    for (k = 0; k < n; ++k) fa_cexp(fa_mulmod(k, k, 2 * n), 2 * n, h + 2 * k);
    return id;
}

static int tab_dft_of(plan *p, int src, i64 n) {
    int id = tab_find(p, FA_TAB_DFT_OF, n, src);
    if (id >= 0) return id;
    id = tab_new(p, FA_TAB_DFT_OF, n, src, n, 2 * sizeof(double));
    free(p->tabs[id].host);
    p->tabs[id].host = NULL;
    p->tabs[id].src = src;
    return id;
}

/* DFT_nb( w[0], w[1..n-1], 0.., w[n-1..1] ) / nb  (A.c:1624-1639) */
static int tab_blue_kernel(plan *p, i64 n, i64 nb) {
    int seq = tab_find(p, FA_TAB_BLUE_SEQ, n, nb);
    if (seq < 0) {
        double *h, w[2];
        i64 k;
        seq = tab_new(p, FA_TAB_BLUE_SEQ, n, nb, nb, 2 * sizeof(double));
        h = (double *)p->tabs[seq].host;
        for (k = 0; k < n; ++k) {
            fa_cexp(fa_mulmod(k, k, 2 * n), 2 * n, w);
            h[2 * k] = w[0] / (double)nb;
            h[2 * k + 1] = w[1] / (double)nb;
            if (k) {
                h[2 * (nb - k)] = h[2 * k];
                h[2 * (nb - k) + 1] = h[2 * k + 1];
            }
        }
    }
    return tab_dft_of(p, seq, nb);
}

/* perm[k] = g^k mod p (inverse = 0) or g^-k mod p (inverse = 1), k in [0, p-1) */
static int tab_perm(plan *p, i64 pr, int inverse) {
    int id = tab_find(p, FA_TAB_PERM, pr, inverse);
    i64 *h, g, x, k;
    if (id >= 0) return id;
    id = tab_new(p, FA_TAB_PERM, pr, inverse, pr - 1, sizeof(i64));
    h = (i64 *)p->tabs[id].host;
    g = fa_find_generator(pr);
    if (inverse) g = fa_power_mod(g, pr - 2, pr);
    x = 1;
    for (k = 0; k < pr - 1; ++k) {
        h[k] = x;
        x = fa_mulmod(x, g, pr);
    }
    return id;
}

/* Omega = DFT_{p-1}( exp(-2 pi i g^-j / p) / (p-1) )   (rader_mkomega A.c:4139-4167) */
static int tab_rader_kernel(plan *p, i64 pr) {
    int seq = tab_find(p, FA_TAB_RADER_SEQ, pr, 0);
    if (seq < 0) {
        int pi = tab_perm(p, pr, 1);
        const i64 *perm = (const i64 *)p->tabs[pi].host;
        double *h, w[2];
        i64 j;
        seq = tab_new(p, FA_TAB_RADER_SEQ, pr, 0, pr - 1, 2 * sizeof(double));
        h = (double *)p->tabs[seq].host;
        for (j = 0; j < pr - 1; ++j) {
            fa_cexp(perm[j], pr, w);
            h[2 * j] = w[0] / (double)(pr - 1);
            h[2 * j + 1] = -w[1] / (double)(pr - 1);
        }
    }
    return tab_dft_of(p, seq, pr - 1);
}

/* --------------------------------------------------------------- buffers */

static int buf_acquire(plan *p, i64 reals) {
    int i;
    for (i = 2; i < p->nbufs; ++i)
        if (!p->buf_busy[i]) {
            p->buf_busy[i] = 1;
            if (p->buf_reals[i] < reals) p->buf_reals[i] = reals;
            return i;
        }
    if (p->nbufs >= FA_MAXBUF) { p->failed = 1; return 2; }
    i = p->nbufs++;
    p->buf_busy[i] = 1;
    p->buf_reals[i] = reals;
    return i;
}

static void buf_release(plan *p, int id) { p->buf_busy[id] = 0; }

/* ----------------------------------------------------------------- steps */

static fftw_amd_step_desc *new_step(plan *p, int kind) {
    fftw_amd_step_desc *s;
    if (p->nsteps == p->cap_steps) {
        p->cap_steps = p->cap_steps ? 2 * p->cap_steps : 16;
        p->steps = (fftw_amd_step_desc *)realloc(p->steps, sizeof(*s) * (size_t)p->cap_steps);
    }
    s = &p->steps[p->nsteps++];
    memset(s, 0, sizeof(*s));
    s->kind = kind;
    s->table = s->table2 = -1;
    s->tw_lo = s->tw_hi = -1;
    s->batch_dim = -1;
    s->aux_buf = -1;
    s->tile = 1;
    s->tile_lo_n = 1;
    s->variant = FFTW_AMD_K_GENERIC;
    return s;
}

static void step_set_locs(fftw_amd_step_desc *s, fa_loc src, fa_loc dst) {
    s->src_buf = src.buf; s->src_base = src.base; s->src_im = src.im;
    s->dst_buf = dst.buf; s->dst_base = dst.base; s->dst_im = dst.im;
}

typedef struct { i64 n, is, os, tw; int is_batch; } sdim;

/* put dims into the step; returns -1 if they do not fit */
static int step_set_dims(plan *p, fftw_amd_step_desc *s, const sdim *d, int nd, int tile_idx) {
    int i, k = 0;
    if (tile_idx >= 0) {
        s->dim_n[0] = d[tile_idx].n; s->dim_is[0] = d[tile_idx].is;
        s->dim_os[0] = d[tile_idx].os; s->dim_tw[0] = d[tile_idx].tw;
        if (d[tile_idx].is_batch) s->batch_dim = 0;
        k = 1;
    }
    for (i = 0; i < nd; ++i) {
        if (i == tile_idx) continue;
        if (d[i].n == 1 && !d[i].is_batch) continue;
        if (k >= FFTW_AMD_MAX_DIMS) { p->failed = 1; return -1; }
        s->dim_n[k] = d[i].n; s->dim_is[k] = d[i].is;
        s->dim_os[k] = d[i].os; s->dim_tw[k] = d[i].tw;
        if (d[i].is_batch) s->batch_dim = k;
        ++k;
    }
    s->ndims = k;
    return 0;
}


/* Order the loops of an element-wise step by their stride on the user side (by_dst: the
   destination, else the source), the batch loop last, and return how many of them are
   faster than the transform index of stride kstride (step.kpos).  Extent-1 loops drop out
   here so that the count matches what step_set_dims keeps. */
static int order_dims_kpos(sdim *d, int *nd_io, int by_dst, i64 kstride) {
    sdim t[FA_MAXLOOPS + 1], b;
    int nd = *nd_io, cnt = 0, i, j, have_b = 0, kpos = 0;
    for (i = 0; i < nd; ++i) {
        i64 key;
        if (d[i].is_batch) { b = d[i]; have_b = 1; continue; }
        if (d[i].n == 1) continue;
        key = iabs(by_dst ? d[i].os : d[i].is);
        for (j = cnt - 1; j >= 0 && iabs(by_dst ? t[j].os : t[j].is) > key; --j) t[j + 1] = t[j];
        t[j + 1] = d[i];
        ++cnt;
    }
    for (i = 0; i < cnt; ++i) if (iabs(by_dst ? t[i].os : t[i].is) < iabs(kstride)) kpos = i + 1;
    if (have_b) t[cnt++] = b;
    memcpy(d, t, sizeof(sdim) * (size_t)cnt);
    *nd_io = cnt;
    return kpos;
}

/* One batched length-L DFT pass.  dims: every index other than the transform
   index.  The tile dim is the one whose stride makes global access widest. */
static void emit_pass(plan *p, fa_loc src, fa_loc dst, i64 L, i64 is_l, i64 os_l,
                      const sdim *dims, int nd, i64 tw_n, int flags) {
    fftw_amd_step_desc *s = new_step(p, FFTW_AMD_STEP_PASS);
    int i, best = -1, pair = -1;
    i64 best_cost = 0, T;
    const i64 INF = (i64)1 << 60;
    sdim dummy, dims_local[FFTW_AMD_MAX_DIMS + FA_MAXLOOPS];
    /* the pair loop of interleaved vectors is reserved for the inner tile component */
    for (i = 0; i < nd; ++i)
        if (dims[i].n == 2 && !dims[i].is_batch && dims[i].tw == 0 &&
            (iabs(dims[i].is) == 2 || iabs(dims[i].os) == 2) &&
            (dims[i].is % 2) == 0 && (dims[i].os % 2) == 0) { pair = i; break; }
    if (L * 3 > FA_LDS_ELEMS || FA_TILE_ELEMS / L < 2) pair = -1;   /* a tile must hold both members */
    for (i = 0; i < nd; ++i) {
        i64 ci, co, cost;
        if (dims[i].n <= 1 || i == pair) continue;
        ci = dims[i].is ? iabs(dims[i].is) : INF;
        co = dims[i].os ? iabs(dims[i].os) : INF;
        if (L > 1 && iabs(is_l) < ci) ci = iabs(is_l);
        if (L > 1 && iabs(os_l) < co) co = iabs(os_l);
        cost = ci + co;
        if (best < 0 || cost < best_cost ||
            (cost == best_cost && dims[i].n > dims[best].n)) {
            best = i;
            best_cost = cost;
        }
    }
    /* a two-element loop whose stride is one complex on either side (the two
       interleaved vectors of a radix-4 real transform) becomes the inner
       component of the tile dim: its pairs then share 32-byte accesses */
    if (best < 0 && pair >= 0) { best = pair; pair = -1; }   /* nothing else to tile over */
    {
        sdim rest[FFTW_AMD_MAX_DIMS + FA_MAXLOOPS];
        int lo = pair, k2 = 0;
        if (lo >= 0) {
            int nb = best;
            s->tile_lo_n = 2;
            s->tile_lo_is = dims[lo].is;
            s->tile_lo_os = dims[lo].os;
            for (i = 0; i < nd; ++i) {
                if (i == lo) { if (i < best) --nb; continue; }
                rest[k2++] = dims[i];
            }
            memcpy((void *)dims_local, rest, sizeof(sdim) * (size_t)k2);
            dims = dims_local;
            nd = k2;
            best = nb;
        }
    }
    step_set_locs(s, src, dst);
    s->flags = flags;
    s->L = (int)L;
    s->is_l = is_l;
    s->os_l = os_l;
    s->nradices = fa_radices(L, s->radices);
    if (s->nradices < 0) { p->failed = 1; return; }
    if (L > 1) s->table = tab_stage(p, L);
    if (best < 0) {
        /* no loop with extent > 1: a dummy tile dim keeps the kernel uniform,
           any batch dim of extent 1 still rides along as a loop */
        sdim tmp[FFTW_AMD_MAX_DIMS + 1];
        memset(&dummy, 0, sizeof(dummy));
        dummy.n = 1;
        tmp[0] = dummy;
        for (i = 0; i < nd && i < FFTW_AMD_MAX_DIMS; ++i) tmp[i + 1] = dims[i];
        step_set_dims(p, s, tmp, nd + 1, 0);
    } else {
        step_set_dims(p, s, dims, nd, best);
    }
    T = FA_TILE_ELEMS / L;
    /* Small tiles for the LDS kernels: about 1024 elements per workgroup (32 KiB of
       ping-pong LDS, 4-5 workgroups per CU) hide the latencies of the stage loop far
       better than one 128 KiB workgroup -- measured 1.46 -> 2.30 TB/s for n = 1000,
       0.96 -> 1.35 TB/s for n = 5000.  Strided passes keep 8
       sequences (128-byte segments).  small_tiles = 0 (a FFTW_MEASURE candidate) keeps
       the 4096-element tiles.  The register kernels set their own tile below. */
    {
        i64 elems = p->cfg.tile_elems > 0 ? p->cfg.tile_elems : (p->cfg.small_tiles ? 1024 : FA_TILE_ELEMS);
        i64 cap = elems / L, floor_t = (iabs(is_l) <= 2 && iabs(os_l) <= 2) ? 1 : 8;
        if (cap < floor_t) cap = floor_t;
        if (T > cap) T = cap;
    }
    if (T < 1) T = 1;
    if (T > s->dim_n[0] * s->tile_lo_n) T = s->dim_n[0] * s->tile_lo_n;
    /* the LDS row is padded to an odd width (T | 1): both images must fit 160 KiB */
    while (T > 1 && L * (T | 1) > FA_LDS_ELEMS) --T;
    T -= T % s->tile_lo_n;
    if (T < 1) T = 1;
    s->tile = (int)T;
    if (src.im == 1 && dst.im == 1 && !(flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT)) &&
        !p->knobs.no_tuned) {
        if (L == 1024) {
            s->variant = FFTW_AMD_K_P1024;  /* register-resident radix-32x32, 8 sequences per tile */
            s->tile = 8;
            if (p->knobs.p1024_order == 0) s->flags |= FFTW_AMD_F_P1024_EIGHTHS;
        } else if (L <= 32 && fa_hip_r1_tile((int)L) > 0 && is_l == 2 && os_l == 2 && tw_n == 0 && s->tile_lo_n == 1 &&
                   s->dim_is[0] == 2 * L && s->dim_os[0] == 2 * L && s->dim_n[0] >= 256 && !p->knobs.no_r1) {
            s->variant = FFTW_AMD_K_R1;     /* dense rows of a short length: one butterfly per row (pass1r.hpp) */
            s->tile = fa_hip_r1_tile((int)L);
        } else if (fa_hip_r3_tile((int)L) > 0 && is_l == 2 && os_l == 2 && tw_n == 0 && s->tile_lo_n == 1 &&
                   (L == 2048 || L == 4096 || L == 8192 || L == 16384 || s->dim_n[0] * 2 >= fa_hip_r3_tile((int)L))) {
            s->variant = FFTW_AMD_K_R3;     /* three-stage register kernel, whole contiguous rows */
            s->tile = fa_hip_r3_tile((int)L);
        } else if (fa_hip_rr_tile((int)L) > 0 && s->dim_n[0] * s->tile_lo_n * 4 >= fa_hip_rr_tile((int)L) &&
                   (s->tile_lo_n == 1 || is_pow2(L))) {
            s->variant = FFTW_AMD_K_RR;     /* two-stage register kernel */
            s->tile = fa_hip_rr_tile((int)L);
        } else if (fa_hip_r3t_tile((int)L) > 0 && s->tile_lo_n == 1 && s->dim_n[0] * 4 >= fa_hip_r3t_tile((int)L)) {
            s->variant = FFTW_AMD_K_R3;     /* three-stage register kernel, column / transposed form */
            s->tile = fa_hip_r3t_tile((int)L);
        }
    }
    s->tw_n = tw_n;
    if (tw_n) tab_tw2(p, tw_n, &s->tw_lo, &s->tw_hi, &s->tw_shift);
    {
        double work = (double)L;
        for (i = 0; i < s->ndims; ++i) work *= (double)s->dim_n[i];
        if (L > 1) p->est_flops += 5.0 * work * log2((double)L);
        if (tw_n) p->est_flops += 6.0 * work;
    }
}

static void emit_copy(plan *p, int kind, fa_loc src, fa_loc dst, i64 K, i64 Kvalid,
                      i64 is_k, i64 os_k, const sdim *dims, int nd, int flags,
                      int table, int table2) {
    fftw_amd_step_desc *s = new_step(p, kind);
    step_set_locs(s, src, dst);
    s->flags = flags;
    s->is_l = is_k;
    s->os_l = os_k;
    s->aux_n = K;
    s->aux_valid = Kvalid;
    s->table = table;
    s->table2 = table2;
    step_set_dims(p, s, dims, nd, -1);
}

/* ------------------------------------------------------- transpositions */

int fa_match_transpose(const fa_dim *l, int nl, i64 unit, fa_transp *t) {
    int ti, i, a, b;
    if (!transposes_enabled()) return 0;
    for (i = 0; i < nl; ++i) if (l[i].n < 1 || (l[i].n > 1 && (l[i].is <= 0 || l[i].os <= 0))) return 0;
    /* with an inner tuple loop first (a loop of unit stride on both sides, at most 8 doubles), then without */
    for (ti = 0; ti <= nl; ++ti) {
        const int tl = ti < nl ? ti : -1;
        i64 vl = unit;
        int best = -1, ba = -1, bb = -1;
        if (tl >= 0) {
            if (l[tl].n < 2 || l[tl].is != unit || l[tl].os != unit || l[tl].n * unit > 8) continue;
            vl = l[tl].n * unit;
        }
        for (a = 0; a < nl; ++a)
            for (b = 0; b < nl; ++b) {
                int score;
                if (a == b || a == tl || b == tl) continue;
                if (l[a].os != vl || l[b].is != vl) continue;
                if (l[a].is < l[b].n * vl || l[b].os < l[a].n * vl) continue;
                score = (l[a].n > 1) + (l[b].n > 1);
                if (score > best) { best = score; ba = a; bb = b; }
            }
        if (best < 0) continue;
        t->n0 = l[ba].n; t->lds = l[ba].is;
        t->n1 = l[bb].n; t->ldd = l[bb].os;
        t->vl = vl;
        t->nb = 0;
        for (i = 0; i < nl; ++i) {
            if (i == ba || i == bb || i == tl || l[i].n == 1) continue;
            if (t->nb >= FFTW_AMD_MAX_DIMS - 2 || t->nb >= FA_MAXLOOPS) return 0;
            /* a batch loop is an OUTER loop: it steps over a whole matrix on both sides (a third loop interleaved
               with the matrix is a permutation of three loops, which stays on the element-wise kernels) */
            if (l[i].is < (t->n0 - 1) * t->lds + t->n1 * vl || l[i].os < (t->n1 - 1) * t->ldd + t->n0 * vl) return 0;
            t->b[t->nb++] = l[i];
        }
        return 1;
    }
    return 0;
}

int fa_transp_inplace_ok(const fa_transp *t) {
    i64 n[FA_MAXLOOPS + 2], st[FA_MAXLOOPS + 2];
    int i, j, k = 0;
    if (t->n0 != t->n1 || t->lds != t->ldd) return 0;
    n[k] = t->n1; st[k++] = t->vl;
    n[k] = t->n0; st[k++] = t->lds;
    for (i = 0; i < t->nb; ++i) {
        if (t->b[i].is != t->b[i].os) return 0;
        n[k] = t->b[i].n; st[k++] = t->b[i].is;
    }
    for (i = 1; i < k; ++i)                       /* by stride; every loop must step over the whole of the previous one */
        for (j = i; j > 0 && st[j] < st[j - 1]; --j) {
            i64 x = st[j]; st[j] = st[j - 1]; st[j - 1] = x;
            x = n[j]; n[j] = n[j - 1]; n[j - 1] = x;
        }
    for (i = 1; i < k; ++i) if (n[i] > 1 && st[i] < n[i - 1] * st[i - 1]) return 0;
    return 1;
}

/* One transposition step (kernels_tr.hip).  The fields mean what they mean for every copy: the tuple is the copy's
   own index (aux_n elements), the two matrix loops and the batch loops are its dims.  All extents are the whole
   problem's: plans that hold such a step run in one chunk. */
static void emit_transpose(plan *p, fa_loc src, fa_loc dst, const fa_transp *t, i64 unit, int inplace) {
    fftw_amd_step_desc *s = new_step(p, FFTW_AMD_STEP_COPY);
    int i;
    src.im = dst.im = unit == 2 ? 1 : 0;
    step_set_locs(s, src, dst);
    s->flags = (unit == 1 ? (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT) : 0) | (inplace ? FFTW_AMD_F_PAIR_SWAP : 0);
    s->is_l = s->os_l = unit;
    s->aux_n = s->aux_valid = t->vl / unit;
    s->variant = FFTW_AMD_K_TRANSPOSE;
    s->tile = t->vl == unit ? 32 : 16;
    s->dim_n[0] = t->n0; s->dim_is[0] = t->lds; s->dim_os[0] = t->vl;
    s->dim_n[1] = t->n1; s->dim_is[1] = t->vl;  s->dim_os[1] = t->ldd;
    for (i = 0; i < t->nb; ++i) {
        s->dim_n[2 + i] = t->b[i].n; s->dim_is[2 + i] = t->b[i].is; s->dim_os[2 + i] = t->b[i].os;
    }
    s->ndims = 2 + t->nb;
}

/* interleaved complex data the 16-byte kernels of a c2c problem can take: the planner's arrays aligned.  (The
   launcher itself takes any alignment: a new-array execution may still pass an offset array.) */
static int transp_layout_ok(const plan *p, fa_loc src, fa_loc dst) {
    if (p->type == FA_R2R) return 1;
    if (p->type != FA_C2C || src.im != 1 || dst.im != 1 || (src.base % 2) || (dst.base % 2)) return 0;
    if ((src.buf == 0 || dst.buf == 0) && ((size_t)p->ri % 16)) return 0;
    if ((src.buf == 1 || dst.buf == 1) && ((size_t)p->ro % 16)) return 0;
    return 1;
}

/* ------------------------------------------------------------- one axis */

static void fa_emit_axis(plan *p, const fa_axis *ax);

/* the loops of an axis as step dims d[0 ... nloops); lis / los: the loop strides on the two sides when a side is a
   scratch image, NULL = the axis's own .is / .os.  Returns the count, so a caller that put nd dims of its own first
   (a twiddled one, say) appends with nd += loop_sdims(..., d + nd). */
static int loop_sdims(const fa_axis *ax, const i64 *lis, const i64 *los, sdim *d) {
    int i;
    for (i = 0; i < ax->nloops; ++i) {
        d[i].n = ax->loops[i].n;
        d[i].is = lis ? lis[i] : ax->loops[i].is;
        d[i].os = los ? los[i] : ax->loops[i].os;
        d[i].tw = 0;
        d[i].is_batch = (i == ax->batch_loop);
    }
    return ax->nloops;
}

/* dense scratch layout for an axis: batch loop outermost, then the remaining
   indices in the order of their source strides, innermost stride 2 (one
   interleaved complex).  Returns total doubles; fills axis and loop strides. */
static i64 scratch_layout_u(const fa_axis *ax, i64 n_axis, i64 unit, i64 *ts_axis, i64 *ts_loop) {
    int order[FA_MAXLOOPS + 1], cnt = 0, i, j;
    i64 key[FA_MAXLOOPS + 1], stride = unit;
    /* index -1 denotes the axis itself; it comes first so that it wins ties (callers pass
       is = 1 to ask for the axis innermost, and a loop of real data may have stride 1 too) */
    order[cnt] = -1;
    key[cnt] = iabs(ax->is);
    ++cnt;
    for (i = 0; i < ax->nloops; ++i) {
        if (i == ax->batch_loop) continue;
        order[cnt] = i;
        key[cnt] = iabs(ax->loops[i].is);
        ++cnt;
    }
    /* insertion sort ascending by source stride: smallest stride innermost */
    for (i = 1; i < cnt; ++i) {
        int o = order[i];
        i64 k = key[i];
        for (j = i - 1; j >= 0 && key[j] > k; --j) { order[j + 1] = order[j]; key[j + 1] = key[j]; }
        order[j + 1] = o;
        key[j + 1] = k;
    }
    for (i = 0; i < cnt; ++i) {
        if (order[i] < 0) { *ts_axis = stride; stride *= n_axis; }
        else { ts_loop[order[i]] = stride; stride *= ax->loops[order[i]].n; }
    }
    if (ax->batch_loop >= 0) {
        ts_loop[ax->batch_loop] = stride;
        stride *= ax->loops[ax->batch_loop].n;
    }
    return stride;
}

/* A scratch image of n_axis complex numbers per sequence over the loops of `ax`, acquired: its location, axis stride
   *ts and loop strides lts[].  axis_key ranks the axis among the loops' source strides: 1 = the axis innermost.
   The caller releases it: buf_release(p, z.buf). */
static fa_loc scratch_image(plan *p, const fa_axis *ax, i64 axis_key, i64 n_axis, i64 *ts, i64 *lts) {
    fa_axis lay = *ax;
    fa_loc z = { 0, 0, 1 };
    lay.is = axis_key;
    z.buf = buf_acquire(p, scratch_layout_u(&lay, n_axis, 2, ts, lts));
    return z;
}

/* Cooley-Tukey over k >= 2 passes through a scratch image:
   pass i < k : length-L_i DFTs down columns of the [L_i][M_i] view, times
               w_{L_i M_i}^(k_i j);   last pass: length-L_k DFTs along rows,
   written transposed so the output is in natural order. */
static void emit_ct(plan *p, const fa_axis *ax, const i64 *lens, int k) {
    i64 M[FA_MAXPASS + 1], Pf[FA_MAXPASS + 1];
    i64 ts, lts[FA_MAXLOOPS];
    sdim d[FFTW_AMD_MAX_DIMS + FA_MAXLOOPS];
    fa_loc tmp;
    int i, j, nd;

    /* M[i] = product of the lengths after pass i, Pf[i] = product before it */
    M[k - 1] = 1;
    for (i = k - 2; i >= 0; --i) M[i] = M[i + 1] * lens[i + 1];
    Pf[0] = 1;
    for (i = 1; i < k; ++i) Pf[i] = Pf[i - 1] * lens[i - 1];

    tmp = scratch_image(p, ax, ax->is, ax->n, &ts, lts);

    for (i = 0; i < k; ++i) {
        int flags = 0;
        nd = 0;
        if (i == 0) {
            /* source -> scratch */
            d[nd].n = M[0]; d[nd].is = ax->is; d[nd].os = ts; d[nd].tw = 1; d[nd].is_batch = 0; ++nd;
            nd += loop_sdims(ax, NULL, lts, d + nd);
            flags = ax->flags_in & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_REAL_IN);
            /* two passes: the twiddle w_n^(k_0 j) is applied by the last pass on
               its input (index j along the row, k_0 = which row) */
            emit_pass(p, ax->src, tmp, lens[0], M[0] * ax->is, M[0] * ts, d, nd,
                      k == 2 ? 0 : ax->n, flags);
        } else if (i < k - 1) {
            /* scratch -> scratch, in place */
            d[nd].n = M[i]; d[nd].is = ts; d[nd].os = ts; d[nd].tw = 1; d[nd].is_batch = 0; ++nd;
            for (j = 0; j < i; ++j) {
                d[nd].n = lens[j]; d[nd].is = M[j] * ts; d[nd].os = M[j] * ts;
                d[nd].tw = 0; d[nd].is_batch = 0; ++nd;
            }
            nd += loop_sdims(ax, lts, lts, d + nd);
            emit_pass(p, tmp, tmp, lens[i], M[i] * ts, M[i] * ts, d, nd, lens[i] * M[i], 0);
        } else {
            /* scratch -> destination, digits reversed into natural order */
            for (j = 0; j < k - 1; ++j) {
                d[nd].n = lens[j]; d[nd].is = M[j] * ts; d[nd].os = Pf[j] * ax->os;
                d[nd].tw = (k == 2) ? 1 : 0; d[nd].is_batch = 0; ++nd;
            }
            nd += loop_sdims(ax, lts, NULL, d + nd);
            flags = ax->flags_out & (FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_OUT);
            if (k == 2) flags |= FFTW_AMD_F_TW_IN;
            emit_pass(p, tmp, ax->dst, lens[k - 1], ts, Pf[k - 1] * ax->os, d, nd,
                      k == 2 ? ax->n : 0, flags);
        }
    }
    buf_release(p, tmp.buf);
}

/* Bluestein: y[k] = conj(w_k) * ( (x conj(w)) (*) w )[k], the convolution by
   two DFTs of the smooth size nb >= 2n-1  (reference A.c:1642-1688) */
static void emit_bluestein(plan *p, const fa_axis *ax) {
    i64 n = ax->n, nb = fa_next_smooth(2 * n - 1);
    i64 wts, lts[FA_MAXLOOPS];
    int chirp = tab_chirp(p, n, nb);
    int kern = tab_blue_kernel(p, n, nb);
    int j, nd;
    fa_loc w = scratch_image(p, ax, 1, nb, &wts, lts);     /* work image [loops][nb], axis innermost */
    sdim d[FA_MAXLOOPS];
    fa_axis sub;

    nd = loop_sdims(ax, NULL, lts, d);
    emit_copy(p, FFTW_AMD_STEP_COPY, ax->src, w, nb, n, ax->is, wts, d, nd,
              (ax->flags_in & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_REAL_IN)) | FFTW_AMD_F_MUL_CONJ,
              chirp, -1);

    memset(&sub, 0, sizeof(sub));
    sub.n = nb; sub.is = wts; sub.os = wts; sub.src = w; sub.dst = w;
    sub.nloops = ax->nloops; sub.batch_loop = ax->batch_loop;
    for (j = 0; j < ax->nloops; ++j) {
        sub.loops[j].n = ax->loops[j].n; sub.loops[j].is = lts[j]; sub.loops[j].os = lts[j];
    }
    fa_emit_axis(p, &sub);

    for (j = 0; j < nd; ++j) d[j].is = d[j].os;
    emit_copy(p, FFTW_AMD_STEP_COPY, w, w, nb, nb, wts, wts, d, nd, FFTW_AMD_F_MUL_TABLE, kern, -1);

    sub.flags_in = FFTW_AMD_F_SWAP_IN;
    sub.flags_out = FFTW_AMD_F_SWAP_OUT;
    fa_emit_axis(p, &sub);

    for (j = 0; j < ax->nloops; ++j) { d[j].is = lts[j]; d[j].os = ax->loops[j].os; }
    emit_copy(p, FFTW_AMD_STEP_COPY, w, ax->dst, n, n, wts, ax->os, d, nd,
              (ax->flags_out & (FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_OUT)) | FFTW_AMD_F_MUL_CONJ,
              chirp, -1);
    buf_release(p, w.buf);
}

/* Rader for a prime p: a cyclic convolution of length p-1 over the
   multiplicative group (reference rader_apply A.c:4187-4261) */
static void emit_rader(plan *p, const fa_axis *ax) {
    i64 pr = ax->n, m = pr - 1;
    i64 wts, lts[FA_MAXLOOPS], xts, xlts[FA_MAXLOOPS];
    int pf = tab_perm(p, pr, 0), pinv = tab_perm(p, pr, 1);
    int omega = tab_rader_kernel(p, pr);
    int j, nd;
    fa_loc w = scratch_image(p, ax, 1, m, &wts, lts), x0 = scratch_image(p, ax, 1, 1, &xts, xlts);
    sdim d[FA_MAXLOOPS];
    fa_axis sub;
    fftw_amd_step_desc *s;

    nd = loop_sdims(ax, NULL, lts, d);
    /* a[k] = x[g^k] */
    emit_copy(p, FFTW_AMD_STEP_COPY, ax->src, w, m, m, ax->is, wts, d, nd,
              (ax->flags_in & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_REAL_IN)) | FFTW_AMD_F_PERM_SRC,
              -1, pf);
    /* x0 */
    for (j = 0; j < nd; ++j) d[j].os = xlts[j];
    emit_copy(p, FFTW_AMD_STEP_COPY, ax->src, x0, 1, 1, ax->is, xts, d, nd,
              ax->flags_in & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_REAL_IN), -1, -1);

    memset(&sub, 0, sizeof(sub));
    sub.n = m; sub.is = wts; sub.os = wts; sub.src = w; sub.dst = w;
    sub.nloops = ax->nloops; sub.batch_loop = ax->batch_loop;
    for (j = 0; j < ax->nloops; ++j) {
        sub.loops[j].n = ax->loops[j].n; sub.loops[j].is = lts[j]; sub.loops[j].os = lts[j];
    }
    fa_emit_axis(p, &sub);

    /* pointwise product, DC fix-ups, Y[0].  The kernel walks vectors in the
       scratch order, which is the order of dims given here. */
    s = new_step(p, FFTW_AMD_STEP_RADER_MUL);
    step_set_locs(s, w, ax->dst);
    s->aux_buf = x0.buf; s->aux_base = 0;
    s->aux_n = m;
    s->table = omega;
    s->flags = ax->flags_out & (FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_OUT);
    {
        /* dims sorted by scratch stride ascending so that the linear vector
           index equals the scratch vector index */
        sdim sd[FA_MAXLOOPS];
        int order[FA_MAXLOOPS], a, b, t;
        for (j = 0; j < ax->nloops; ++j) order[j] = j;
        for (a = 0; a < ax->nloops; ++a)
            for (b = a + 1; b < ax->nloops; ++b)
                if (lts[order[b]] < lts[order[a]]) { t = order[a]; order[a] = order[b]; order[b] = t; }
        for (j = 0; j < ax->nloops; ++j) {
            int o = order[j];
            sd[j].n = ax->loops[o].n; sd[j].is = lts[o]; sd[j].os = ax->loops[o].os;
            sd[j].tw = 0; sd[j].is_batch = (o == ax->batch_loop);
        }
        /* keep extent-1 dims out but the vector numbering intact: extent 1
           contributes a factor of 1 */
        step_set_dims(p, s, sd, ax->nloops, -1);
    }

    sub.flags_in = FFTW_AMD_F_SWAP_IN;
    sub.flags_out = FFTW_AMD_F_SWAP_OUT;
    fa_emit_axis(p, &sub);

    /* Y[g^-k] = c[k] */
    for (j = 0; j < ax->nloops; ++j) { d[j].is = lts[j]; d[j].os = ax->loops[j].os; }
    emit_copy(p, FFTW_AMD_STEP_COPY, w, ax->dst, m, m, wts, ax->os, d, nd,
              (ax->flags_out & (FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_OUT)) | FFTW_AMD_F_PERM_DST,
              -1, pinv);
    buf_release(p, x0.buf);
    buf_release(p, w.buf);
}

static int rows_alias_ok(const plan *p, const fa_axis *ax, fa_loc a, fa_loc b);

/* May a contiguous axis longer than FA_LMAX_SINGLE run as ONE trip of a register rows kernel?  Such a step has
   no LDS-kernel fallback (the row does not fit the runtime-radix kernel), so everything the rows kernel needs is
   settled here, at plan time: interleaved unit-stride rows, 16-byte aligned user arrays and even loop strides,
   rows that map onto themselves when the transform is in place, no two-level tile dim, no FFTW_UNALIGNED. */
static int long_rows_ok(const plan *p, const fa_axis *ax) {
    int j, rows = 0;
    if (ax->is != 2 || ax->os != 2 || ax->src.im != 1 || ax->dst.im != 1) return 0;
    if ((ax->flags_in | ax->flags_out) & ~(FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT)) return 0;
    if (!rows_alias_ok(p, ax, ax->src, ax->dst)) return 0;
    for (j = 0; j < ax->nloops; ++j) {
        if ((ax->loops[j].is % 2) || (ax->loops[j].os % 2)) return 0;
        if (ax->loops[j].n == 2 && (iabs(ax->loops[j].is) == 2 || iabs(ax->loops[j].os) == 2)) return 0;
        if (ax->loops[j].n > 1) rows = 1;
    }
    if (!rows) return 0;
    if ((ax->src.base % 2) || (ax->dst.base % 2)) return 0;
    if (ax->src.buf == 0 && ((size_t)p->ri % 16)) return 0;
    if (ax->src.buf == 1 && ((size_t)p->ro % 16)) return 0;
    if (ax->dst.buf == 0 && ((size_t)p->ri % 16)) return 0;
    if (ax->dst.buf == 1 && ((size_t)p->ro % 16)) return 0;
    return 1;
}

/* Bluestein for interleaved unit-stride rows whose padded length fits one workgroup: the whole algorithm in ONE
   kernel (pass3b.hpp).  The padded length comes from a ladder (blue_menu.inc); when its first entry >= 2n - 1 is
   more than 1.35 x that (short lengths: the ladder starts at 539) the step-by-step plan with its tighter
   nb = next smooth number is kept.  Like the long rows the step has no fallback, so the same plan-time conditions
   apply (long_rows_ok).  1 = emitted. */
static int emit_bluestein_rows(plan *p, const fa_axis *ax) {
    i64 need = 2 * ax->n - 1;
    int nb, j;
    sdim d[FA_MAXLOOPS];
    fftw_amd_step_desc *s;
    if (p->knobs.no_tuned || p->knobs.no_3s || p->knobs.no_blue_rows) return 0;
    if (ax->n < 2 || need > 16384 || ax->nloops == 0) return 0;
    nb = fa_hip_blue_nb((int)need);
    if (nb <= 0 || (double)nb > 1.35 * (double)need) return 0;
    if (!long_rows_ok(p, ax)) return 0;
    emit_pass(p, ax->src, ax->dst, nb, 2, 2, d, loop_sdims(ax, NULL, NULL, d), 0,
              (ax->flags_in & FFTW_AMD_F_SWAP_IN) | (ax->flags_out & FFTW_AMD_F_SWAP_OUT));
    if (p->failed) return 1;
    s = &p->steps[p->nsteps - 1];
    if (s->tile_lo_n != 1) { p->failed = 1; return 1; }
    s->variant = FFTW_AMD_K_BLUE;
    s->tile = fa_hip_blue_tile(nb);
    s->aux_n = ax->n;
    s->tw_lo = tab_chirp(p, ax->n, nb);
    s->tw_hi = tab_blue_kernel(p, ax->n, nb);
    /* emit_pass counted 5 nb log2 nb once; the kernel runs the stages twice plus three pointwise products */
    {
        double rows = 1.0;
        for (j = 0; j < ax->nloops; ++j) rows *= (double)ax->loops[j].n;
        p->est_flops += rows * (5.0 * (double)nb * log2((double)nb) + 18.0 * (double)nb);
    }
    return 1;
}

/* ---- how an axis is split into passes: axis_split and its three stages.  They decide and emit nothing. */

/* interleaved complex data on both sides of the axis, no real side: what the tuned complex kernels take */
static int plain_complex_axis(const fa_axis *ax) {
    return ax->src.im == 1 && ax->dst.im == 1 &&
           !((ax->flags_in | ax->flags_out) & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT));
}

/* unit-stride rows of a length the three-stage rows kernel does in one trip */
static int rows3_layout_ok(const plan *p, const fa_axis *ax) {
    return fa_hip_r3_tile((int)ax->n) > 0 && iabs(ax->is) == 2 && iabs(ax->os) == 2 && plain_complex_axis(ax) &&
           !p->knobs.no_3s;
}

/* Stage 1: the longest length the axis may run as ONE pass.  The order of the rules is behaviour: later ones
   overwrite what earlier ones set. */
static i64 single_pass_cap(const plan *p, const fa_axis *ax, int contiguous) {
    const i64 n = ax->n;
    const int tuned = !p->knobs.no_tuned;
    /* A strided axis keeps tiles at least 8 wide so that global access stays
       in 128-byte segments; a contiguous axis may fill the tile by itself. */
    i64 lmax1 = contiguous ? FA_LMAX_SINGLE : FA_TILE_ELEMS / 8;
    /* a strided axis with a register kernel of its own length needs no split either */
    if (!contiguous && n <= 1024 && tuned && fa_has_register_kernel(n)) lmax1 = 1024;
    /* ... and neither does a strided axis of 1025 ... 2048 points with a narrow-tile three-stage kernel
       (4 ... 7 sequences per tile, 64 ... 112-byte segments, ~3 TB/s): the 1080 of a 1080 x 1920 image */
    if (!contiguous && n > 1024 && n <= 2048 && ax->nloops > 0 && tuned && !p->knobs.no_narrow &&
        fa_hip_r3t_tile((int)n) > 0 && plain_complex_axis(ax))
        lmax1 = 2048;
    /* powers of two above 1024 run faster as two register-kernel passes than
       as one LDS-sized pass (measured: 4096-point rows 0.8 TB/s vs ~5 TB/s per pass) */
    if (contiguous && n > 1024 && is_pow2(n) && ax->nloops > 0 && tuned) {
        /* ... except contiguous rows of 2048 / 4096: the three-stage kernel does them in one */
        int rows3s = rows3_layout_ok(p, ax);
        /* 8192: one row per workgroup (32 x 16 x 16), one trip instead of 128 x 64 in two; 16384: one row per
           512-item workgroup (pass3w.hpp) */
        if (rows3s && n > FA_LMAX_SINGLE) rows3s = n <= 16384 && long_rows_ok(p, ax);
        if (!rows3s) lmax1 = 1024;
        else if (n > lmax1) lmax1 = n;
    }
    if (ax->nloops == 0 && !contiguous) lmax1 = FA_LMAX_SINGLE;
    /* 4096 < n < 16384 with a three-stage rows kernel (one row per workgroup; above 8192 the 512-item kernels of
       kernels_r3w.hip): one trip instead of two, under the same plan-time conditions as the 8192-point rows (no
       LDS-kernel fallback at that length) */
    if (contiguous && n > FA_LMAX_SINGLE && n < 16384 && !is_pow2(n) && ax->nloops > 0 && tuned && !p->knobs.no_3s &&
        fa_hip_r3_tile((int)n) > 0 && long_rows_ok(p, ax))
        lmax1 = n;
    /* 1024 < n <= 4096 that is not a power of two: two register-kernel passes (each near
       the copy rate) beat one pass of the LDS kernel (1.3-1.8 TB/s) whenever both halves of
       a balanced split have a register kernel -- measured n = 3000: 1.27 vs 2.4 TB/s --
       unless the three-stage rows kernel does the whole length in one trip */
    if (contiguous && n > 1024 && n <= lmax1 && !is_pow2(n) && ax->nloops > 0 && tuned && !rows3_layout_ok(p, ax)) {
        i64 l2[FA_MAXPASS];
        if (fa_factor_passes_pref(n, 2, 1, 1024, l2, fa_has_register_kernel) == 2 &&
            fa_has_register_kernel(l2[0]) && fa_has_register_kernel(l2[1]))
            lmax1 = 1024;
    }
    return lmax1;
}

/* Stage 2: n = L1 x L2 with 1024 < L1 <= 2048 in TWO trips instead of the three the factoriser found: the strided
   three-stage kernel of such a length works on tiles of 4 ... 7 columns (64 ... 112-byte segments, ~3.2 TB/s) --
   slower per trip than the 128-byte kernels, but two trips beat three (2^21 = 2048 x 1024: 7.9 vs 11.2 ms per 8 GiB;
   with BOTH lengths above 1024 the two slow trips only tie with three fast ones, so that is not done).
   (The narrow-tile kernel takes interleaved complex data on 16-byte aligned arrays only -- the same conditions as
   for a strided axis in single_pass_cap; with split or unaligned arrays its pass would fall to the runtime-radix
   LDS kernel with a 1 ... 2 column tile, far slower than the three-pass plan.)  1 and lens[0 .. 2) when two trips
   win. */
static int two_trip_split(const plan *p, const fa_axis *ax, i64 *lens) {
    /* cost per GiB of a pass (the units of split_costs.inc): narrow-tile first pass 0.34 (2048-point: 5.33 ms
       per 16 GiB), the partner as LAST pass from the table (1024: 0.18, the cfg2 pass; 1000: 0.20); the
       three-pass alternative from the same table (powers of two: 0.68, measured 2^21 ... 2^24) */
    const i64 n = ax->n;
    i64 L1, bestL1 = 0, l3[FA_MAXPASS];
    double best2 = 1e30, est3 = 0.68;
    if (ax->nloops == 0 || p->knobs.no_tuned || p->knobs.no_narrow || !plain_complex_axis(ax) ||
        (p->flags & FFTW_UNALIGNED) || p->cfg.lmax_multi < 1024)
        return 0;
    if (!is_pow2(n)) {
        double c3 = fa_mixed_three_pass_split(n, l3);
        if (c3 > 0.0) est3 = c3;
    }
    for (L1 = 2048; L1 > 1024; --L1) {
        i64 L2 = n / L1;
        double c1, c2;
        if (n % L1 || fa_hip_r3t_tile((int)L1) <= 0 || L2 < 96) continue;
        /* round 3: the 512-item kernels of r3tw_menu.inc (8 ... 15 sequences per tile) are cheaper first passes
           than the narrow tiles, and serve as LAST pass too (rows in, transposed store, twiddle on the input):
           both lengths above 1024, e.g. 2^22 = 2048 x 2048 in 3.8 instead of 5.4 ms per 4 GiB */
        c1 = fa_wide_pass_cost(L1, 0);
        if (c1 <= 0.0) c1 = 0.34;
        if (L2 > 1024) {
            c2 = L2 <= 2048 ? fa_wide_pass_cost(L2, 1) : 0.0;
            if (c2 <= 0.0 || fa_wide_pass_cost(L1, 0) <= 0.0) continue;
        } else {
            if (!fa_has_register_kernel(L2)) continue;
            c2 = L2 == 1024 ? 0.18 : (L2 == 1000 ? 0.20 : fa_split_cost_measured(L2, 2));
        }
        if (c2 <= 0.0) continue;                  /* no measurement for that partner: do not guess */
        if (c1 + c2 < best2) { best2 = c1 + c2; bestL1 = L1; }
    }
    if (!bestL1 || !(best2 < 0.95 * est3)) return 0;
    lens[0] = bestL1;
    lens[1] = n / bestL1;
    return 1;
}

/* Stage 3: the k lengths of a contiguous axis by the measured split model for that k, where there is one (split.c).
   The models know lengths up to 1024: with a smaller cap (the FFTW_MEASURE candidate lmax_multi = 512,
   FFTW_AMD_LMAX_MULTI) the balanced split of fa_factor_passes_pref, which honours it, stays. */
static void measured_split(const plan *p, const fa_axis *ax, int k, i64 *lens) {
    if (p->cfg.lmax_multi < 1024 || p->knobs.no_tuned) return;
    if (k == 3 && is_pow2(ax->n)) fa_pow2_three_pass_split(ax->n, lens);
    else if (k == 3 && !p->knobs.no_split_costs) fa_mixed_three_pass_split(ax->n, lens);
    else if (k == 2 && ax->nloops > 0 && lens[0] <= 1024 && lens[1] <= 1024 && !p->knobs.no_split_costs)
        fa_mixed_two_pass_split(ax->n, lens);
}

/* The split of an LDS-able axis into passes: returns k and lens[0 .. k); 1 = one pass, 0 = no split (Bluestein).
   contiguous: the axis may fill a tile by itself. */
static int axis_split(const plan *p, const fa_axis *ax, int contiguous, i64 *lens) {
    int k = fa_factor_passes_pref(ax->n, FA_MAXPASS, single_pass_cap(p, ax, contiguous),
                                  contiguous ? p->cfg.lmax_multi : FA_TILE_ELEMS / 8, lens,
                                  p->knobs.no_tuned ? NULL : fa_has_register_kernel);
    int a, b;
    if (contiguous) {
        if (k == 3 && two_trip_split(p, ax, lens)) k = 2;
        measured_split(p, ax, k, lens);
    }
    /* test hook FFTW_AMD_FORCE_LENS (fa_read_knobs): the axis whose length is the product takes that split */
    if (p->knobs.n_force_lens && p->knobs.force_prod == ax->n) {
        k = p->knobs.n_force_lens;
        for (a = 0; a < k; ++a) lens[a] = p->knobs.force_lens[a];
    }
    /* longest sub-transform first (FFTW_MEASURE candidate) */
    if (p->cfg.long_first)
        for (a = 0; a < k; ++a)
            for (b = a + 1; b < k; ++b)
                if (lens[b] > lens[a]) { i64 t = lens[a]; lens[a] = lens[b]; lens[b] = t; }
    return k;
}

static void fa_emit_axis(plan *p, const fa_axis *ax) {
    i64 lens[FA_MAXPASS];
    sdim d[FA_MAXLOOPS];
    int k;

    if (p->failed) return;

    if (!fa_lds_able(ax->n)) {
        if (emit_bluestein_rows(p, ax)) return;
        if (fa_is_prime(ax->n) && fa_lds_able(ax->n - 1)) emit_rader(p, ax);
        else emit_bluestein(p, ax);
        return;
    }
    k = axis_split(p, ax, (iabs(ax->is) <= 2 && iabs(ax->os) <= 2) || ax->dense, lens);
    if (k == 0) {
        /* e.g. a prime factor between lmax and FA_PRIME_LDS_MAX cannot happen;
           sizes that do not split fall back to Bluestein */
        emit_bluestein(p, ax);
        return;
    }
    if (k == 1) {
        emit_pass(p, ax->src, ax->dst, ax->n, ax->is, ax->os, d, loop_sdims(ax, NULL, NULL, d), 0,
                  (ax->flags_in & (FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_REAL_IN)) |
                  (ax->flags_out & (FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_OUT)));
        return;
    }
    if (ax->nloops + k > FFTW_AMD_MAX_DIMS) { p->failed = 1; return; }
    emit_ct(p, ax, lens, k);
}

/* ------------------------------------------------------- whole problems */

/* merge loop b into loop a when b is exactly a's inner continuation */
static int merge_loops(fa_dim *l, int n, int *batch) {
    int changed = 1;
    while (changed) {
        int a, b;
        changed = 0;
        for (a = 0; a < n && !changed; ++a)
            for (b = 0; b < n && !changed; ++b) {
                if (a == b || a == *batch || b == *batch) continue;
                if (l[a].is == l[b].n * l[b].is && l[a].os == l[b].n * l[b].os) {
                    int i;
                    l[b].n *= l[a].n;
                    for (i = a; i + 1 < n; ++i) l[i] = l[i + 1];
                    if (*batch > a) --*batch;
                    --n;
                    changed = 1;
                }
            }
    }
    return n;
}

/* loops for transforming `axis` of a rank-r array: the other transform dims
   plus the howmany dims.  use_os: source strides are the output strides. */
static int collect_loops(const plan *p, const fa_dim *dims, int rank, int axis,
                         const i64 *ext_override, int use_os, fa_axis *ax) {
    int i, n = 0;
    ax->batch_loop = -1;
    for (i = 0; i < rank; ++i) {
        if (i == axis) continue;
        if (n >= FA_MAXLOOPS) return -1;
        ax->loops[n].n = ext_override ? ext_override[i] : dims[i].n;
        ax->loops[n].is = use_os ? dims[i].os : dims[i].is;
        ax->loops[n].os = dims[i].os;
        ++n;
    }
    for (i = 0; i < p->hrank; ++i) {
        if (n >= FA_MAXLOOPS) return -1;
        ax->loops[n].n = (i == 0) ? p->chunk : p->hdims[i].n;
        ax->loops[n].is = use_os ? p->hdims[i].os : p->hdims[i].is;
        ax->loops[n].os = p->hdims[i].os;
        if (i == 0) ax->batch_loop = n;
        ++n;
    }
    n = merge_loops(ax->loops, n, &ax->batch_loop);
    ax->nloops = n;
    return 0;
}


/* A two-dimensional transform n0 x n1 whose rows (n1 = 2048 or 4096 points, contiguous) have a one-trip rows
   kernel holding T whole rows per tile, and whose strided axis is n0 = T x L0 with 1024 < n0 <= 4096 and L0 <= 1024
   a register-kernel length, in TWO full-rate trips (pass3q.hpp, pass3s.hpp XROW): the strided axis is split
   Cooley-Tukey over the row index r = s + T r' --
     trip 1  the ordinary strided L0-point pass of every row class s (128-byte segments), twiddle w_n0^(s k') on
             the output, stored as [k'][s][c]: the T rows that belong together are adjacent
     trip 2  tiles k' of T rows: the row transforms and the DFT of length T across the rows in the same registers,
             X[k' + L0 q] = sum_s w_T^(s q) DFT_n1(Y_s[k'])
   Round 2 ran 4096 x 4096 as rows + 64 x 64 columns (three trips, 23 %) and strided axes of 1025 ... 2048 points on
   the narrow-tile kernel (64-byte segments, 3.2 TB/s).  The last step has no other executor, so everything it
   needs is settled here: interleaved unit-stride rows, 16-byte aligned arrays, even strides, at most one batch
   loop, no FFTW_UNALIGNED.  1 = emitted. */
static int emit_rows_lo_dft(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out) {
    const fa_dim *col = &p->dims[0], *row = &p->dims[1];
    sdim d[3];
    int nd, sbuf;
    i64 N1, N0, T = 0, L0, img, chunk = p->hrank ? p->chunk : 1;
    fftw_amd_step_desc *st;
    if (p->rank != 2 || p->hrank > 1 || p->knobs.no_tuned || p->knobs.no_lo_dft || p->knobs.no_3s) return 0;
    N1 = row->n; N0 = col->n;
    if ((N1 != 2048 && N1 != 4096) || N0 <= 1024 || N0 > 4096) return 0;
    if (N1 == 4096 && N0 <= 2048 && N0 % 2 == 0 && fa_has_register_kernel(N0 / 2)) T = 2;      /* pass3s<16>, XROW */
    else if (N0 % 4 == 0 && fa_has_register_kernel(N0 / 4)) T = 4;                             /* pass3q / pass3s<8>, XROW */
    if (!T) return 0;
    L0 = N0 / T;
    if (row->is != 2 || row->os != 2 || in.im != 1 || out.im != 1) return 0;
    if (col->is < 2 * N1 || col->os < 2 * N1 || (col->is % 2) || (col->os % 2)) return 0;
    if (p->flags & FFTW_UNALIGNED) return 0;
    if (((size_t)p->ri % 16) || ((size_t)p->ro % 16)) return 0;
    if (p->hrank && ((p->hdims[0].is % 2) || (p->hdims[0].os % 2))) return 0;
    if (fa_hip_r3_tile((int)N1) <= 0) return 0;
    img = N0 * N1 * 2;
    sbuf = buf_acquire(p, chunk * img);
    {
        /* trip 1: L0-point column pass of every row class s, twiddle w_n0^(s k') on the output */
        fa_loc scr = { sbuf, 0, 1 };
        d[0].n = N1; d[0].is = 2;       d[0].os = 2;      d[0].tw = 0; d[0].is_batch = 0;    /* columns c */
        d[1].n = T;  d[1].is = col->is; d[1].os = 2 * N1; d[1].tw = 1; d[1].is_batch = 0;    /* row class s */
        nd = 2;
        if (p->hrank) { d[2].n = chunk; d[2].is = p->hdims[0].is; d[2].os = img; d[2].tw = 0; d[2].is_batch = 1; nd = 3; }
        emit_pass(p, in, scr, L0, T * col->is, T * 2 * N1, d, nd, N0, sw_in);
        if (p->failed) return 1;
        /* trip 2: tiles k' of T rows: DFT-n1 along every row and DFT-T across them */
        d[0].n = L0; d[0].is = T * 2 * N1; d[0].os = col->os; d[0].tw = 0; d[0].is_batch = 0;
        nd = 1;
        if (p->hrank) { d[1].n = chunk; d[1].is = img; d[1].os = p->hdims[0].os; d[1].tw = 0; d[1].is_batch = 1; nd = 2; }
        emit_pass(p, scr, out, N1, 2, 2, d, nd, 0, sw_out);
        if (p->failed) return 1;
        st = &p->steps[p->nsteps - 1];
        st->tile_lo_n = (int)T;
        st->tile_lo_is = 2 * N1;
        st->tile_lo_os = L0 * col->os;
        st->flags |= FFTW_AMD_F_LO_DFT;
        st->variant = FFTW_AMD_K_R3;
        st->tile = (int)T;
        p->est_flops += 5.0 * (double)(N0 * N1) * (double)chunk * (T == 4 ? 2.0 : 1.0);     /* the radix-T stage */
    }
    buf_release(p, sbuf);
    return 1;
}

/* A batch of small two-dimensional transforms n0 x n1 on dense contiguous images, in ONE trip: a workgroup takes T
   whole images and does both axes in registers, where the axis-by-axis plan crosses HBM twice.  Two kernel families:
   both extents at most 32, a pair of img2d_menu.inc, one butterfly per axis (FFTW_AMD_K_IMG2D, pass2d.hpp); extents in
   {16, 32, 40, 48, 64} with at least one above 32, a pair of img2dl_menu.inc, two register stages on an axis of 40, 48
   or 64 points (FFTW_AMD_K_IMG2DL, pass2dl.hpp), whose intra-axis twiddles w_n^(a d) come from the stage tables of the
   axes: table (row axis) and table2 (column axis), which no executor of a pass without tw_n reads otherwise.  The
   steps have no other executor, so everything they need is settled here: rank 2, interleaved arrays, dense rows and
   images, at most one howmany loop (mk_guru drops the extent-1 ones) that steps over exactly one image on both sides,
   16-byte aligned arrays, no FFTW_UNALIGNED.  No scratch, in place or out of place.  fa_hip_img2d_tile and
   fa_hip_img2dl_tile are the only sources of what the kernels cover.  FFTW_AMD_NO_IMG2D=1 (no whole images in one
   trip) restores the two-trip plans for both.  A third family, off under FFTW_ESTIMATE (cfg.img_wide,
   FFTW_AMD_IMG_WIDE=1, a FFTW_MEASURE candidate): 128 x 128, 64 x 128 and 128 x 64, a pair of img2dw_menu.inc, one tile
   of 16384 elements per 512-item workgroup (FFTW_AMD_K_IMG2DW, pass2dw.hpp; both axes two stages, both tables; its
   tile query is fa_hip_img2dw_tile), under the same layout rule and the same two switches.  emit_images, below its
   two helpers: 1 = emitted. */

/* images per tile of a family's kernel for n0 x n1 (0: none) */
static int image_tile(int variant, i64 n0, i64 n1) {
    if (n0 > 128 || n1 > 128) return 0;
    if (variant == FFTW_AMD_K_IMG2D) return fa_hip_img2d_tile((int)n0, (int)n1);
    if (variant == FFTW_AMD_K_IMG2DL) return fa_hip_img2dl_tile((int)n0, (int)n1);
    return fa_hip_img2dw_tile((int)n0, (int)n1);
}

/* the step itself: nimg dense images n0 x n1 one after another, T per workgroup; the loop over them is the batch
   loop of the plan (is_batch) or a loop of its own */
static int emit_image_step(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out, int variant, i64 n0, i64 n1, int T,
                           i64 nimg, int is_batch) {
    const i64 img = 2 * n0 * n1;
    fftw_amd_step_desc *s;
    sdim d;
    s = new_step(p, FFTW_AMD_STEP_PASS);
    step_set_locs(s, in, out);
    s->flags = sw_in | sw_out | FFTW_AMD_F_LO_DFT;
    s->L = (int)n1;
    s->is_l = 2;
    s->os_l = 2;
    s->nradices = fa_radices(n1, s->radices);
    if (s->nradices < 0) { p->failed = 1; return 1; }
    s->tile_lo_n = (int)n0;
    s->tile_lo_is = 2 * n1;
    s->tile_lo_os = 2 * n1;
    d.n = nimg; d.is = img; d.os = img; d.tw = 0; d.is_batch = is_batch;
    step_set_dims(p, s, &d, 1, 0);
    s->tile = T;
    s->variant = variant;
    if (variant != FFTW_AMD_K_IMG2D) {
        if (n1 > 32) s->table = tab_stage(p, n1);
        if (n0 > 32) s->table2 = tab_stage(p, n0);
    }
    p->est_flops += 5.0 * (double)(n0 * n1) * (double)d.n * log2((double)(n0 * n1));
    return 1;
}

static int emit_images(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out, int variant) {
    const fa_dim *col = &p->dims[0], *row = &p->dims[1];
    i64 n0, n1, img;
    int T;
    if (p->rank != 2 || p->hrank > 1 || p->knobs.no_tuned || p->knobs.no_img2d) return 0;
    if (variant == FFTW_AMD_K_IMG2DW && !p->cfg.img_wide) return 0;
    n0 = col->n; n1 = row->n;
    T = image_tile(variant, n0, n1);
    if (T <= 0) return 0;
    img = 2 * n0 * n1;
    if (in.im != 1 || out.im != 1) return 0;
    if (row->is != 2 || row->os != 2 || col->is != 2 * n1 || col->os != 2 * n1) return 0;
    if (p->hrank && (p->hdims[0].is != img || p->hdims[0].os != img)) return 0;
    if (p->flags & FFTW_UNALIGNED) return 0;
    if (((size_t)p->ri % 16) || ((size_t)p->ro % 16)) return 0;
    return emit_image_step(p, in, out, sw_in, sw_out, variant, n0, n1, T, p->hrank ? p->chunk : 1, p->hrank ? 1 : 0);
}

static int emit_img2d(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out) {
    return emit_images(p, in, out, sw_in, sw_out, FFTW_AMD_K_IMG2D);
}

static int emit_img2dl(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out) {
    return emit_images(p, in, out, sw_in, sw_out, FFTW_AMD_K_IMG2DL);
}

static int emit_img2dw(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out) {
    return emit_images(p, in, out, sw_in, sw_out, FFTW_AMD_K_IMG2DW);
}

/* A batch of small three-dimensional transforms n0 x n1 x n2 on dense contiguous volumes, in ONE trip
   (FFTW_AMD_K_VOL3D, pass3d.hpp): a workgroup takes T whole volumes and does all three axes in registers, where the
   axis-by-axis plan crosses HBM three times.  The step has no other executor, so everything it needs is settled here:
   rank 3, interleaved arrays, dense rows, planes and volumes, at most one howmany loop that steps over exactly one
   volume on both sides, 16-byte aligned arrays, no FFTW_UNALIGNED.  No scratch, no tables, in place or out of place.
   fa_hip_vol3d_tile is the only source of what the kernel covers.  Off under FFTW_ESTIMATE (cfg.vol3d,
   FFTW_AMD_VOL3D=1): the numpy step interpreter of the CPU tier does not know the step, so it stays an opt-in and a
   FFTW_MEASURE candidate until that interpreter learns it.  FFTW_AMD_NO_IMG2D=1 and FFTW_AMD_NO_TUNED=1 switch it off
   like the image steps.  1 = emitted. */
static int emit_vol3d(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out) {
    const fa_dim *d0 = &p->dims[0], *d1 = &p->dims[1], *d2 = &p->dims[2];
    fftw_amd_step_desc *s;
    sdim d;
    i64 n0, n1, n2, vol;
    int T;
    if (!p->cfg.vol3d || p->rank != 3 || p->hrank > 1 || p->knobs.no_tuned || p->knobs.no_img2d) return 0;
    n0 = d0->n; n1 = d1->n; n2 = d2->n;
    if (n0 > 32 || n1 > 32 || n2 > 32) return 0;
    T = fa_hip_vol3d_tile((int)n0, (int)n1, (int)n2);
    if (T <= 0) return 0;
    vol = 2 * n0 * n1 * n2;
    if (in.im != 1 || out.im != 1) return 0;
    if (d2->is != 2 || d2->os != 2 || d1->is != 2 * n2 || d1->os != 2 * n2 || d0->is != 2 * n1 * n2 || d0->os != 2 * n1 * n2) return 0;
    if (p->hrank && (p->hdims[0].is != vol || p->hdims[0].os != vol)) return 0;
    if (p->flags & FFTW_UNALIGNED) return 0;
    if (((size_t)p->ri % 16) || ((size_t)p->ro % 16)) return 0;
    s = new_step(p, FFTW_AMD_STEP_PASS);
    step_set_locs(s, in, out);
    s->flags = sw_in | sw_out | FFTW_AMD_F_LO_DFT | FFTW_AMD_F_VOL3D;
    s->L = (int)n2;
    s->is_l = 2;
    s->os_l = 2;
    s->nradices = fa_radices(n2, s->radices);
    if (s->nradices < 0) { p->failed = 1; return 1; }
    s->tile_lo_n = (int)n1;
    s->tile_lo_is = 2 * n2;
    s->tile_lo_os = 2 * n2;
    s->aux_n = n0;
    d.n = p->hrank ? p->chunk : 1; d.is = vol; d.os = vol; d.tw = 0; d.is_batch = p->hrank ? 1 : 0;
    step_set_dims(p, s, &d, 1, 0);
    s->tile = T;
    s->variant = FFTW_AMD_K_VOL3D;
    p->est_flops += 5.0 * (double)(n0 * n1 * n2) * (double)d.n * log2((double)(n0 * n1 * n2));
    return 1;
}

/* A batch of three-dimensional transforms n0 x n1 x n2 on dense contiguous volumes in TWO trips where the
   axis-by-axis plan crosses HBM three times: the (n1, n2) planes of the chunk's volumes are one run of chunk x n0
   dense images, which one image step (FFTW_AMD_K_IMG2D, _IMG2DL or _IMG2DW, whichever tile query takes the pair)
   transforms from `in` to `out`; the first axis is then one strided pass in place on `out` through the axis emitter,
   its loops the n1 n2 contiguous columns and the batch.  The image step has no other executor, so everything it needs
   is settled here (the conditions of emit_vol3d), and whether n0 is ONE pass is decided before anything is emitted:
   in every other case the plan of the axis loop is built, step for step.  The loop over the planes is no batch dim: it
   counts planes, not volumes, and the plan -- the caller's two arrays, no scratch -- runs in one chunk
   (fa_build_steps_sized).  No scratch, in place or out of place.  Off under FFTW_ESTIMATE (cfg.vol_planes,
   FFTW_AMD_VOL_PLANES=1), a FFTW_MEASURE candidate, for the reason given at emit_vol3d; FFTW_AMD_NO_IMG2D=1 and
   FFTW_AMD_NO_TUNED=1 switch it off like the image steps.  1 = emitted. */
static int emit_vol_planes(plan *p, fa_loc in, fa_loc out, int sw_in, int sw_out) {
    static const int families[3] = { FFTW_AMD_K_IMG2D, FFTW_AMD_K_IMG2DL, FFTW_AMD_K_IMG2DW };
    const fa_dim *d0 = &p->dims[0], *d1 = &p->dims[1], *d2 = &p->dims[2];
    const i64 chunk = p->hrank ? p->chunk : 1;
    i64 n0, n1, n2, vol, lens[FA_MAXPASS];
    fa_axis ax;
    int f, T = 0, variant = 0;
    if (!p->cfg.vol_planes || p->rank != 3 || p->hrank > 1 || p->knobs.no_tuned || p->knobs.no_img2d) return 0;
    if (in.buf != 0 || out.buf != 1) return 0;
    n0 = d0->n; n1 = d1->n; n2 = d2->n;
    for (f = 0; f < 3 && T <= 0; ++f) { variant = families[f]; T = image_tile(variant, n1, n2); }
    if (T <= 0) return 0;
    vol = 2 * n0 * n1 * n2;
    if (in.im != 1 || out.im != 1) return 0;
    if (d2->is != 2 || d2->os != 2 || d1->is != 2 * n2 || d1->os != 2 * n2 || d0->is != 2 * n1 * n2 || d0->os != 2 * n1 * n2) return 0;
    if (p->hrank && (p->hdims[0].is != vol || p->hdims[0].os != vol)) return 0;
    if (p->flags & FFTW_UNALIGNED) return 0;
    if (((size_t)p->ri % 16) || ((size_t)p->ro % 16)) return 0;
    /* the first axis, in place on the output */
    memset(&ax, 0, sizeof(ax));
    ax.n = n0;
    ax.is = d0->os;
    ax.os = d0->os;
    ax.src = out;
    ax.dst = out;
    ax.flags_in = sw_in;
    ax.flags_out = sw_out;
    if (collect_loops(p, p->dims, p->rank, 0, NULL, 1, &ax)) return 0;
    if (!fa_lds_able(n0) || axis_split(p, &ax, 0, lens) != 1) return 0;
    emit_image_step(p, in, out, sw_in, sw_out, variant, n1, n2, T, chunk * n0, 0);
    if (p->failed) return 1;
    fa_emit_axis(p, &ax);
    return 1;
}

static void build_c2c_on(plan *p, fa_loc in, fa_loc out);

/* One copy src -> dst over ALL dims of the problem as loops (transform dims, then the howmany dims of the current
   chunk; strides as p->dims / p->hdims hold them now): a tiled transposition when the loops form one
   (fa_match_transpose), else the element-wise copy -- complex: a pass of length 1 on the LDS kernel, real:
   copy_kernel (reference rank0 solvers, fftw/fftw_api.c:9655-9720). */
static void emit_loops_copy(plan *p, fa_loc src, fa_loc dst, int contig_k) {
    const i64 unit = p->type == FA_R2R ? 1 : 2;
    fa_dim l[2 * FA_MAXRANK];
    fa_transp t;
    fa_axis ax;
    sdim d[FA_MAXLOOPS];
    int i, nl = 0, nd;
    for (i = 0; i < p->rank; ++i) l[nl++] = p->dims[i];
    for (i = 0; i < p->hrank; ++i) { l[nl] = p->hdims[i]; if (i == 0) l[nl].n = p->chunk; ++nl; }
    if (transp_layout_ok(p, src, dst) && fa_match_transpose(l, nl, unit, &t)) {
        emit_transpose(p, src, dst, &t, unit, 0);
        return;
    }
    memset(&ax, 0, sizeof(ax));
    if (collect_loops(p, p->dims, p->rank, -1, NULL, 0, &ax)) { p->failed = 1; return; }
    nd = loop_sdims(&ax, NULL, NULL, d);
    if (unit == 2) { emit_pass(p, src, dst, 1, 0, 0, d, nd, 0, 0); return; }
    if (contig_k) {
        /* a loop that is contiguous on both sides becomes the copy's own index: copy_kernel then gives a workgroup 256
           neighbouring elements instead of one (the plain half of an in-place plan: 16 GB/s otherwise) */
        for (i = 0; i < nd; ++i)
            if (!d[i].is_batch && d[i].is == 1 && d[i].os == 1 && d[i].n > 1 && d[i].n < 0x7fffffffLL) {
                const i64 K = d[i].n;
                d[i].n = 1;                      /* step_set_dims drops it */
                emit_copy(p, FFTW_AMD_STEP_COPY, src, dst, K, K, 1, 1, d, nd, FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT, -1, -1);
                return;
            }
    }
    emit_copy(p, FFTW_AMD_STEP_COPY, src, dst, 1, 1, 0, 0, d, nd, FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT, -1, -1);
}

/* the whole of a rank-0 problem (c2c and r2r) */
static void build_rank0(plan *p, fa_loc in, fa_loc out) {
    const i64 unit = p->type == FA_R2R ? 1 : 2;
    if (p->tr_kind == FA_TR_COPY || p->tr_kind == FA_TR_INPLACE) {
        emit_transpose(p, in, out, &p->tr, unit, p->tr_kind == FA_TR_INPLACE);
        return;
    }
    emit_loops_copy(p, in, out, 0);
}

static void build_c2c(plan *p) {
    fa_loc in = { 0, 0, p->in_im }, out = { 1, 0, p->out_im };
    if (p->tr_kind == FA_TR_AFTER) {
        /* Output strides = the transposed input strides, square (the reference's dft-ct-dif + q1 case, A.c:2204-2250,
           2596-2727): the ordinary in-place problem on the INPUT strides, in one chunk, then the in-place square
           transposition -- no more scratch than that in-place plan needs. */
        fa_dim sd[FA_MAXRANK], sh[FA_MAXRANK];
        int i;
        memcpy(sd, p->dims, sizeof(sd));
        memcpy(sh, p->hdims, sizeof(sh));
        for (i = 0; i < p->rank; ++i) p->dims[i].os = p->dims[i].is;
        for (i = 0; i < p->hrank; ++i) p->hdims[i].os = p->hdims[i].is;
        build_c2c_on(p, in, out);
        memcpy(p->dims, sd, sizeof(sd));
        memcpy(p->hdims, sh, sizeof(sh));
        if (!p->failed) emit_transpose(p, out, out, &p->tr, 2, 1);
        return;
    }
    if (p->via_scratch) {
        /* in-place with different strides on the two sides (same locations): transform into a dense row-major
           scratch image [hdims...][dims...], then copy it to the output layout -- every read of the user's array
           precedes every write (single chunk).  The reference does these problems with its in-place square
           DIF + transpose codelets or with buffers (A.c:2204-2250, 2596-2727); see api.c inplace_same_locations. */
        fa_dim sd[FA_MAXRANK], sh[FA_MAXRANK];
        fa_loc scr;
        i64 stride = 2, total;
        int i, sbuf;
        memcpy(sd, p->dims, sizeof(sd));
        memcpy(sh, p->hdims, sizeof(sh));
        for (i = p->rank - 1; i >= 0; --i) { p->dims[i].os = stride; stride *= p->dims[i].n; }
        for (i = p->hrank - 1; i >= 0; --i) {
            p->hdims[i].os = stride;
            stride *= (i == 0 ? p->chunk : p->hdims[i].n);
        }
        total = stride;
        sbuf = buf_acquire(p, total);
        scr.buf = sbuf; scr.base = 0; scr.im = 1;
        build_c2c_on(p, in, scr);
        /* the copy: all dims as loops, source = dense strides, destination = the user's output strides */
        for (i = 0; i < p->rank; ++i) p->dims[i].is = p->dims[i].os;
        for (i = 0; i < p->hrank; ++i) p->hdims[i].is = p->hdims[i].os;
        for (i = 0; i < p->rank; ++i) p->dims[i].os = sd[i].os;
        for (i = 0; i < p->hrank; ++i) p->hdims[i].os = sh[i].os;
        if (!p->failed) emit_loops_copy(p, scr, out, 0);
        memcpy(p->dims, sd, sizeof(sd));
        memcpy(p->hdims, sh, sizeof(sh));
        buf_release(p, sbuf);
        return;
    }
    build_c2c_on(p, in, out);
}

static void build_c2c_on(plan *p, fa_loc in, fa_loc out) {
    int a, first = 1;
    int sw_in = (p->sign > 0) ? FFTW_AMD_F_SWAP_IN : 0;
    int sw_out = (p->sign > 0) ? FFTW_AMD_F_SWAP_OUT : 0;
    if (p->rank == 0) {
        /* rank-0 "transform" = strided copy (reference rank0 solvers) */
        build_rank0(p, in, out);
        return;
    }
    if (emit_rows_lo_dft(p, in, out, sw_in, sw_out)) return;
    if (emit_img2d(p, in, out, sw_in, sw_out)) return;
    if (emit_img2dl(p, in, out, sw_in, sw_out)) return;
    if (emit_img2dw(p, in, out, sw_in, sw_out)) return;
    if (emit_vol3d(p, in, out, sw_in, sw_out)) return;
    if (emit_vol_planes(p, in, out, sw_in, sw_out)) return;
    for (a = p->rank - 1; a >= 0; --a) {
        fa_axis ax;
        memset(&ax, 0, sizeof(ax));
        ax.n = p->dims[a].n;
        ax.is = first ? p->dims[a].is : p->dims[a].os;
        ax.os = p->dims[a].os;
        ax.src = first ? in : out;
        ax.dst = out;
        ax.flags_in = sw_in;
        ax.flags_out = sw_out;
        if (collect_loops(p, p->dims, p->rank, a, NULL, !first, &ax)) { p->failed = 1; return; }
        fa_emit_axis(p, &ax);
        first = 0;
    }
}

/* An estimate of the passes a contiguous axis of length n needs, for the choice between the real-axis plans
   (use_radix4_real); 99 for lengths that go through Rader / Bluestein.  It is NOT axis_split: of its rules it knows
   only the first cap (FA_LMAX_SINGLE, 1024 for a tuned power of two above that) and the plain balanced
   factorisation -- no rows kernels, no register-kernel preference, no two-trip plans, no FFTW_AMD_FORCE_LENS.  The
   plans that were measured were chosen by this count, so it stays what it is. */
static int axis_pass_count(const plan *p, i64 n) {
    i64 lens[FA_MAXPASS], lmax1 = FA_LMAX_SINGLE;
    int k;
    if (!fa_lds_able(n)) return 99;
    /* (the radix-4 real plans feed strided pair data: the 3-stage row kernel does not apply) */
    if (n > 1024 && is_pow2(n) && !p->knobs.no_tuned) lmax1 = 1024;
    k = fa_factor_passes(n, FA_MAXPASS, lmax1, p->cfg.lmax_multi, lens);
    return k ? k : 99;
}

/* The quarter-length transforms of the radix-4 real plans run on PAIRS of interleaved vectors (a two-level tile dim),
   which only the power-of-two two-stage kernels and the 1024-point kernel take; a multi-pass m with another factor
   would put a pass on the runtime-radix LDS kernel (3 932 160 = 4 x 960 x 1024: 7.9 ms per 4 GiB where the half-length
   plan takes 4.3, profiles/r03_r2c_two_trip.txt).  One-pass lengths keep the old rule. */
static int radix4_passes_have_kernels(const plan *p, i64 m) {
    return axis_pass_count(p, m) <= 1 || is_pow2(m);
}

/* passes of the half-length complex transform of an r2c / c2r axis: its rows are contiguous, so a length with
   a three-stage rows kernel (up to 8192) is one pass */
static int half_axis_pass_count(const plan *p, i64 n) {
    if (n <= 16384 && !p->knobs.no_tuned && !p->knobs.no_3s && fa_hip_r3_tile((int)n) > 0) return 1;
    return axis_pass_count(p, n);
}

/* Do source and destination of a one-trip rows step alias?  The fused rows kernels read a tile
   of rows and write the same tile's results without a scratch image in between, so when both
   sides are the same user memory every row must map onto itself (FFTW's padded in-place
   layout does); otherwise the general path, which reads a whole chunk into scratch first. */
static int rows_alias_ok(const plan *p, const fa_axis *ax, fa_loc a, fa_loc b) {
    int j, same_mem;
    /* FFTW_UNALIGNED: the plan must serve arrays of any alignment through the new-array
       interface; the rows kernels rely on 16-byte alignment and have no fallback */
    if (p->flags & FFTW_UNALIGNED) return 0;
    same_mem = (a.buf == b.buf && a.buf < 2) ||
                      (a.buf < 2 && b.buf < 2 && (void *)p->ri == (void *)p->ro && p->ri != NULL);
    if (!same_mem) return 1;
    if (a.base != b.base) return 0;
    for (j = 0; j < ax->nloops; ++j)
        if (ax->loops[j].n > 1 && ax->loops[j].is != ax->loops[j].os) return 0;
    return 1;
}

/* the fused rows kernel loads 16-byte pairs and stores 16-byte complex numbers: every
   loop stride must keep that alignment, the user arrays must be 16-byte aligned, there must
   be a loop to tile over, and the tile dim must not be a two-level (pair) dim.
   hook_in / hook_out: an r2r prologue on the source / epilogue on the destination side (FFTW_AMD_R2R_*, 0 = none):
   that side is then the user's real array of any stride, which the kernel gathers from / scatters to by element */
static int real_rows_layout_ok(const plan *p, const fa_axis *ax, fa_loc src, fa_loc dst, int hook_in, int hook_out) {
    int j, rows = 0;
    if (p->knobs.no_r2crows) return 0;
    if (!rows_alias_ok(p, ax, src, dst)) return 0;
    for (j = 0; j < ax->nloops; ++j) {
        if ((!hook_in && (ax->loops[j].is % 2)) || (!hook_out && (ax->loops[j].os % 2))) return 0;
        /* emit_pass would fold such a loop into a two-level tile dim, which this kernel lacks */
        if (ax->loops[j].n == 2 && (iabs(ax->loops[j].is) == 2 || iabs(ax->loops[j].os) == 2)) return 0;
        if (ax->loops[j].n > 1) rows = 1;
    }
    if (!rows) return 0;
    if (!hook_in && src.buf == 0 && (((size_t)p->ri % 16) || (src.base % 2))) return 0;
    if (!hook_in && src.buf == 1 && (((size_t)p->ro % 16) || (src.base % 2))) return 0;
    if (!hook_out && dst.buf == 1 && (((size_t)p->ro % 16) || (dst.base % 2))) return 0;
    return 1;
}

/* rows per tile of the one-trip real-rows kernels for half length `half` (0: none): the power-of-two two-stage
   form carries the r2r hooks; its mixed-radix lengths (r2cr_menu.inc) and the three-stage form (640 ... 8192) only
   the plain r2c / c2r */
static int real_rows_tile(const plan *p, i64 half, int hooks) {
    int t;
    if (half > 16384) return 0;
    t = fa_hip_r2c_rows_tile((int)half);
    if (t > 0) return t;
    if (hooks) return 0;
    t = fa_hip_r2c_rows2m_tile((int)half);
    if (t > 0) return t;
    if (p->knobs.no_3s) return 0;
    return fa_hip_r2c_rows3_tile((int)half);
}

/* dense real rows of n = 2 half = 4 ... 64 points with at least one tile of them in a loop whose strides are exactly
   the row lengths (n reals, half + 1 complex numbers): the one-stage real-rows kernel (pass1r.hpp); 0: not this */
static int short_real_rows_tile(const plan *p, const fa_axis *ax, i64 half, int hooks, int fwd) {
    int j, t;
    if (hooks || half < 2 || half > 32 || p->knobs.no_r1) return 0;
    t = fa_hip_r2c_rows1_tile((int)half);
    if (t <= 0) return 0;
    for (j = 0; j < ax->nloops; ++j)
        if (ax->loops[j].n >= 256 && ax->loops[j].is == (fwd ? 2 * half : 2 * (half + 1)) &&
            ax->loops[j].os == (fwd ? 2 * (half + 1) : 2 * half)) return t;
    /* FFTW's padded rows (the in-place layout): 2 (half + 1) doubles per row on both sides */
    for (j = 0; j < ax->nloops; ++j)
        if (ax->loops[j].n >= 256 && ax->loops[j].is == 2 * (half + 1) && ax->loops[j].os == 2 * (half + 1)) return t;
    return 0;
}

/* rows per tile of the one-trip rows step of an r2c (fwd) / c2r axis, 0: no such kernel */
static int real_rows_tile_for(const plan *p, const fa_axis *ax, i64 half, int hooks, int fwd) {
    const int t = short_real_rows_tile(p, ax, half, hooks, fwd);
    return t > 0 ? t : real_rows_tile(p, half, hooks);
}

/* can the r2c / c2r axis emitters fuse an r2r epilogue / prologue for this length? */
static int r2r_can_fuse(const plan *p, i64 nl) { return nl >= 2 && nl % 2 == 0 && !p->knobs.r2r_unfused; }

/* Twiddle tables of a step that untangles / tangles a real transform of nl points.  Plain: modulus nl.  With a fused
   REDFT/RODFT 10/01 epilogue or prologue: the modulus-4n table serves both the r2r twiddle w_4n^k and the untangle
   twiddle w_n^k = w_4n^(4k); *mult is the index multiplier of the latter.  `sets` names the fused modes the caller
   takes for such: the untangle / tangle steps all four, a forward rows step the epilogues, a backward one the
   prologues. */
enum { TW4_POST10 = 1, TW4_PRE01 = 2 };
static void real_tw_tables(plan *p, fftw_amd_step_desc *s, i64 nl, int mode, int sets, i64 *mult) {
    const int four = ((sets & TW4_POST10) && (mode == FFTW_AMD_R2R_POST_E10 || mode == FFTW_AMD_R2R_POST_O10)) ||
                     ((sets & TW4_PRE01) && (mode == FFTW_AMD_R2R_PRE_E01 || mode == FFTW_AMD_R2R_PRE_O01));
    *mult = four ? 4 : 1;
    tab_tw2(p, *mult * nl, &s->tw_lo, &s->tw_hi, &s->tw_shift);
}

/* an untangle / tangle step with the fused r2r mode `mode` (0: none): step.variant = mode, step.tile = multiplier */
static void r2r_fuse_tables(plan *p, fftw_amd_step_desc *s, i64 nl, int mode) {
    i64 mult;
    s->variant = mode;
    real_tw_tables(p, s, nl, mode, TW4_POST10 | TW4_PRE01, &mult);
    s->tile = (int)mult;
}

/* Contiguous rows of a supported length: the half-length complex DFT and the untangle (fwd: r2crows.hpp) or the
   tangle and the backward half-length DFT in ONE trip instead of a pass plus an untangle / tangle step.  ss / ds:
   element strides of the real array a hook (real_rows_layout_ok) gathers from / scatters to.  The r2r mode fused
   with the untangle / tangle goes to aux_valid, the one the kernel does while it gathers the row (forward:
   FFTW_AMD_R2R_PRE_*) or stores it (backward: FFTW_AMD_R2R_POST_E01 / O01) to aux_buf; aux_n = n, aux_base = index
   multiplier of the untangle twiddle (real_tw_tables). */
static void emit_real_rows_step(plan *p, int fwd, i64 nl, const fa_axis *ax, fa_loc src, i64 ss, fa_loc dst, i64 ds,
                                int hook_in, int hook_out, int tile) {
    const int fused = fwd ? hook_out : hook_in, shuffle = fwd ? hook_in : hook_out;
    sdim d[FA_MAXLOOPS];
    fftw_amd_step_desc *s;
    if (fwd) src.im = 1; else dst.im = 1;          /* the real row as pairs: odd sample = imaginary part */
    emit_pass(p, src, dst, nl / 2, hook_in ? ss : 2, hook_out ? ds : 2, d, loop_sdims(ax, NULL, NULL, d), 0,
              fwd ? FFTW_AMD_F_R2C_ROWS : FFTW_AMD_F_C2R_ROWS);
    s = &p->steps[p->nsteps - 1];
    s->variant = fwd ? FFTW_AMD_K_R2C : FFTW_AMD_K_C2R;
    s->aux_buf = shuffle ? shuffle : -1;
    s->tile = tile;
    s->tile_lo_n = 1;
    s->aux_n = nl;
    s->aux_valid = fused;
    real_tw_tables(p, s, nl, fused, fwd ? TW4_POST10 : TW4_PRE01, &s->aux_base);
    p->est_flops += 8.0 * (double)(nl / 2);
}

/* the radix-4 plans of a real axis (n = 4m, two complex transforms of m points and a radix-4 untangle / tangle) are
   chosen when m needs fewer passes than n / 2; FFTW_AMD_NO_RADIX4 / FFTW_AMD_FORCE_RADIX4 override */
static int use_radix4_real(const plan *p, i64 nl, const fa_axis *ax) {
    return nl % 4 == 0 && nl >= 8 && ax->nloops < FA_MAXLOOPS && !p->knobs.no_radix4 &&
           ((axis_pass_count(p, nl / 4) < half_axis_pass_count(p, nl / 2) && radix4_passes_have_kernels(p, nl / 4)) ||
            p->knobs.force_radix4);
}

/* ---- what the two decimated plans below (emit_r2c_decimated, emit_c2r_decimated) share */

#define FA_DEC_L2 2048      /* length of the rows trip */

/* May the real axis of nl points run decimated (fwd: r2c, src real and dst complex; else c2r)?  Returns L1 = nl / L2,
   the length of the column trip, or 0.  The rows step has no fallback executor, so everything it needs is settled
   here: the kernel exists, the column trip is ONE strided pass, interleaved arrays, 16-byte alignment, even strides. */
static i64 real_dec_geometry(const plan *p, i64 nl, const fa_axis *ax, fa_loc src, fa_loc dst, int fwd) {
    const i64 L2 = FA_DEC_L2, L1 = nl / L2;
    int j;
    if (!p->cfg.real_dec || (!fwd && p->type != FA_C2R) || p->knobs.no_tuned || p->knobs.no_narrow ||
        (p->flags & FFTW_UNALIGNED) || p->cfg.lmax_multi < 1024)
        return 0;
    if (nl % L2 || !(fwd ? fa_hip_r3tw_rdec((int)L2) : fa_hip_r3tw_cdec((int)L2)) || fa_hip_r3t_tile((int)L2) < 8) return 0;
    if (L1 % 2 || L1 < 256) return 0;
    /* a register kernel of that length with 128-byte segments */
    if (!((L1 <= 1024 && fa_has_register_kernel(L1)) || (L1 <= 2048 && fa_hip_r3t_tile((int)L1) >= 8))) return 0;
    if (ax->nloops >= FA_MAXLOOPS || src.im != (fwd ? 0 : 1) || dst.im != (fwd ? 1 : 0)) return 0;
    if ((src.base % 2) || (dst.base % 2) || ((size_t)p->ro % 16)) return 0;
    /* (a c2r source may be the scratch image of the leading dims) */
    if ((fwd || src.buf < 2) && ((size_t)p->ri % 16)) return 0;
    for (j = 0; j < ax->nloops; ++j)
        if ((ax->loops[j].is % 2) || (ax->loops[j].os % 2)) return 0;
    return L1;
}

/* The column trip: complex transforms of L1 points down the columns of the real array `real` read as [L1][L2 / 2]
   pairs, into (fwd) or backward out of the scratch image z, whose L2 / 2 columns ride as one more loop. */
static fa_axis real_dec_column_axis(const fa_axis *ax, i64 L1, fa_loc real, fa_loc z, i64 zts, const i64 *lts, int fwd) {
    const i64 L2 = FA_DEC_L2;
    fa_axis c = *ax;
    const int cloop = c.nloops++;
    int j;
    real.im = 1;                       /* odd sample = imaginary part */
    c.n = L1;
    c.dense = 0;
    c.loops[cloop].n = L2 / 2;
    if (fwd) {
        c.loops[cloop].is = 2;
        c.loops[cloop].os = zts;
        for (j = 0; j < ax->nloops; ++j) c.loops[j].os = lts[j];
        c.is = L2;                     /* L2 / 2 pairs of two doubles */
        c.os = (L2 / 2) * zts;
        c.src = real;
        c.dst = z;
        c.flags_in = c.flags_out = 0;
    } else {
        c.loops[cloop].is = zts;
        c.loops[cloop].os = 2;
        for (j = 0; j < ax->nloops; ++j) c.loops[j].is = lts[j];
        c.is = (L2 / 2) * zts;
        c.os = L2;
        c.src = z;
        c.dst = real;
        c.flags_in = FFTW_AMD_F_SWAP_IN;
        c.flags_out = FFTW_AMD_F_SWAP_OUT;
    }
    return c;
}

/* is the step emitted last the rows trip as its kernel takes it: rows k1 = 0 ... L1 / 2 as the tile dim? */
static int real_dec_rows_step_ok(const plan *p, i64 L1) {
    const fftw_amd_step_desc *s = &p->steps[p->nsteps - 1];
    return s->variant == FFTW_AMD_K_R3 && s->tile == fa_hip_r3t_tile(FA_DEC_L2) && s->tile_lo_n == 1 &&
           s->dim_n[0] == L1 / 2 + 1 && s->dim_tw[0] == 1 && s->batch_dim != 0;
}

/* the end of both: 1 = emitted (or the plan failed); 0 = not this way, the steps emitted so far are taken back */
static int real_dec_end(plan *p, int ok, int n0, double flops0, int zbuf) {
    if (p->failed) return 1;
    if (!ok) { p->nsteps = n0; p->est_flops = flops0; }
    buf_release(p, zbuf);
    return ok;
}

/* A long real transform in TWO trips (round 3): n = L1 x L2 real points, decimated over the real data itself
   instead of packed into a half-length complex transform plus an untangle trip.
     trip 1   the plain complex pass of length L1 down the columns of the input read as [L1][L2 / 2] pairs
              (x[j1 L2 + 2c], x[j1 L2 + 2c + 1]) -> Z[k1][c] in scratch: the real DFTs of two columns in one
     trip 2   rows k1 = 0 ... L1 / 2: separate the two columns while loading (rows k1 and L1 - k1 of Z), twiddle,
              DFT of length L2 along the row, store X[k1 + L1 k2] and, conjugated, X[n - (k1 + L1 k2)]
              (FFTW_AMD_F_REAL_DEC, pass3t_kernel RD = 1)
   Both trips move n / 2 complex numbers in and out: 2 x the algorithmic bytes where the half-length plans need
   3 x (two passes + untangle).  2^22 = 2048 x 2048 (BASELINE cfg3), 2^21 = 1024 x 2048.
   MEASURED (tools/perf/perf_r2c_two_trip.py, profiles/r03_r2c_two_trip.txt): with the 512-item kernels (one
   workgroup per CU, ~4.5 TB/s per trip with two chunk lanes) the two trips only TIE with the three trips of the
   256-item kernels, whose scratch chunks stay in the Infinity Cache (2^22: 4.58 against 4.11 ms per 4 GiB; 2^20:
   3.98 against 4.10) -- so the plan is off under FFTW_ESTIMATE (cfg.real_dec, FFTW_AMD_REAL_DEC=1) and a candidate
   of the FFTW_MEASURE search for r2c problems.  Reference counterpart: the
   rdft2 Cooley-Tukey plan over real-data codelets (ct_hc2c_direct_apply, fftw/fftw_api.c:5831, with
   fftw/rdft_scalar/r2cf/hc2cfdft_*.c).  The last step has no fallback executor, so everything it needs is settled
   here (aligned interleaved arrays, even strides).  1 = emitted. */
static int emit_r2c_decimated(plan *p, i64 nl, const fa_axis *ax, fa_loc in, fa_loc out) {
    const i64 L2 = FA_DEC_L2, L1 = real_dec_geometry(p, nl, ax, in, out, 1);
    const int n0 = p->nsteps;
    const double flops0 = p->est_flops;
    i64 zts, lts[FA_MAXLOOPS + 1];
    fa_axis c_ax;
    fa_loc z;
    sdim d[FA_MAXLOOPS + 1];
    int ok;
    if (!L1) return 0;
    z = scratch_image(p, ax, 1, nl / 2, &zts, lts);
    c_ax = real_dec_column_axis(ax, L1, in, z, zts, lts, 1);
    fa_emit_axis(p, &c_ax);
    ok = !p->failed && p->nsteps == n0 + 1;
    if (ok) {
        d[0].n = L1 / 2 + 1; d[0].is = (L2 / 2) * zts; d[0].os = 2; d[0].tw = 1; d[0].is_batch = 0;
        emit_pass(p, z, out, L2, zts, 2 * L1, d, 1 + loop_sdims(ax, lts, NULL, d + 1), nl,
                  FFTW_AMD_F_TW_IN | FFTW_AMD_F_REAL_DEC);
        ok = !p->failed && real_dec_rows_step_ok(p, L1);
    }
    return real_dec_end(p, ok, n0, flops0, z.buf);
}

/* real -> half spectrum along one axis.  ax: the loops (.is = strides in the real
   source, .os = strides in the complex destination) and the batch loop; rs / cs:
   element strides of the transform index on the two sides, in doubles. */
/* epi: 0 = store the half spectrum as complex numbers; FFTW_AMD_R2R_POST_* = the
   untangle step applies that r2r epilogue and writes reals of stride cs instead
   (even lengths only; returns 1 when the epilogue was fused, 0 when the caller
   still has to run it on the complex result)
   ps / pim (even lengths): the real input as pairs -- sample 2j at j*ps, sample 2j+1 at
   j*ps + pim; 0 / 0 = the plain strided array (ps = 2 rs, pim = rs).  Scratch inputs of the
   r2r emitters use ps = any, pim = 1: pairs stay adjacent even when other loops are
   innermost, so the register kernels take the first pass. */
static int emit_r2c_axis(plan *p, i64 nl, const fa_axis *axp, fa_loc in, i64 rs, fa_loc out, i64 cs, int epi,
                         i64 ps, i64 pim, int pre) {
    fa_axis ax = *axp;
    i64 half = nl / 2 + 1, zts, lts[FA_MAXLOOPS + 1];
    sdim d[FA_MAXLOOPS + 1];
    fftw_amd_step_desc *s;
    fa_loc z;
    int j, nd, rows_tile;
    if (ps == 0) { ps = 2 * rs; pim = rs; }
    if (epi == 0 && pre == 0 && ps == 2 && pim == 1 && cs == 2 && emit_r2c_decimated(p, nl, &ax, in, out)) return 0;
    if (use_radix4_real(p, nl, &ax)) {
        /* n = 4m: two complex DFTs of size m on (x[4j], x[4j+1]) and (x[4j+2], x[4j+3]),
           then the radix-4 untangle -- the reference's rdft2-ct-dit/4 + hc2cfdft_4 plan,
           chosen when m needs fewer passes than n/2 (n = 2^22: m = 2^20 is 1024 x 1024) */
        i64 m = nl / 4;
        fa_axis q_ax = ax, lay;
        /* scratch [loops][v][m]: the vector index v rides as the innermost loop */
        int vloop = q_ax.nloops++;
        q_ax.loops[vloop].n = 2;
        q_ax.loops[vloop].is = ps;
        q_ax.loops[vloop].os = 0;
        lay = q_ax;
        lay.loops[vloop].is = 1;           /* the pair index is innermost: Z[k][v], like the input */
        z = scratch_image(p, &lay, 2, m, &zts, lts);
        q_ax.dense = (pim == 1 && ps == 2);
        q_ax.n = m;
        q_ax.is = 2 * ps;
        q_ax.os = zts;
        q_ax.src = in;
        q_ax.src.im = pim;
        q_ax.dst = z;
        for (j = 0; j < q_ax.nloops; ++j) q_ax.loops[j].os = lts[j];
        fa_emit_axis(p, &q_ax);

        s = new_step(p, FFTW_AMD_STEP_R2C_POST4);
        step_set_locs(s, z, out);
        s->is_l = zts;
        s->os_l = cs;
        s->aux_n = nl;
        s->aux_valid = lts[vloop];
        r2r_fuse_tables(p, s, nl, epi);
        nd = loop_sdims(&ax, lts, NULL, d);
        s->kpos = order_dims_kpos(d, &nd, 1, cs);
        step_set_dims(p, s, d, nd, -1);
        p->est_flops += 20.0 * (double)m;
        buf_release(p, z.buf);
    } else if (nl % 2 == 0 && nl >= 2 && (pre != 0 || (ps == 2 && pim == 1)) &&
               (epi != 0 || (cs == 2 && out.im == 1)) &&
               (rows_tile = real_rows_tile_for(p, &ax, nl / 2, epi || pre, 1)) > 0 &&
               real_rows_layout_ok(p, &ax, in, out, pre, epi)) {
        emit_real_rows_step(p, 1, nl, &ax, in, rs, out, cs, pre, epi, rows_tile);
    } else if (nl % 2 == 0 && nl >= 2) {
        /* z[j] = x[2j] + i x[2j+1]; Z = DFT_{n/2}(z); untangle */
        i64 h = nl / 2;
        fa_axis half_ax = ax;
        z = scratch_image(p, &ax, 1, h, &zts, lts);
        half_ax.n = h;
        half_ax.is = ps;
        half_ax.os = zts;
        half_ax.src = in;
        half_ax.src.im = pim;    /* odd sample = imaginary part */
        half_ax.dst = z;
        for (j = 0; j < ax.nloops; ++j) half_ax.loops[j].os = lts[j];
        fa_emit_axis(p, &half_ax);

        s = new_step(p, FFTW_AMD_STEP_R2C_POST);
        step_set_locs(s, z, out);
        s->is_l = zts;
        s->os_l = cs;
        s->aux_n = nl;
        r2r_fuse_tables(p, s, nl, epi);
        nd = loop_sdims(&ax, lts, NULL, d);
        s->kpos = order_dims_kpos(d, &nd, 1, cs);
        step_set_dims(p, s, d, nd, -1);
        p->est_flops += 8.0 * (double)h;
        buf_release(p, z.buf);
    } else {
        /* odd length: full complex DFT of the real sequence, keep half */
        fa_axis full_ax = ax;
        z = scratch_image(p, &ax, 1, nl, &zts, lts);
        full_ax.n = nl;
        full_ax.is = rs;
        full_ax.os = zts;
        full_ax.src = in;
        full_ax.dst = z;
        full_ax.flags_in = FFTW_AMD_F_REAL_IN;
        for (j = 0; j < ax.nloops; ++j) full_ax.loops[j].os = lts[j];
        fa_emit_axis(p, &full_ax);
        emit_copy(p, FFTW_AMD_STEP_COPY, z, out, half, half, zts, cs, d, loop_sdims(&ax, lts, NULL, d), 0, -1, -1);
        buf_release(p, z.buf);
        return 0;
    }
    return epi != 0;
}

/* A batch of small two-dimensional r2c (fwd) or c2r transforms n0 x n1 in ONE trip (FFTW_AMD_K_IMG2DR, pass2dr.hpp): a
   workgroup takes T whole real images and does both axes in registers, where the axis-by-axis plans make three trips
   (a pass, the untangle / tangle, a pass), two of them on the runtime-radix LDS kernel, through a scratch buffer.  The
   step has no other executor, so everything it needs is settled here: rank 2, at most one howmany loop that steps over
   exactly one image on both sides, the real side with element stride 1 and row pitch n1 or n1 + 2, the complex side
   interleaved with stride 2 and row pitch n1 + 2, 16-byte aligned arrays, no FFTW_UNALIGNED.  No scratch, no table;
   in place with padded rows (an image then occupies the same words on both sides).  fa_hip_img2dr_tile is the only
   source of what the kernels cover.  Off under FFTW_ESTIMATE (cfg.real_img, FFTW_AMD_REAL_IMG=1): the numpy
   interpreter of the test suite's existing files does not know the step, and those files plan such problems with
   default settings; a candidate of the FFTW_MEASURE search for r2c / c2r problems, remembered by wisdom.
   FFTW_AMD_NO_IMG2D=1 and FFTW_AMD_NO_TUNED=1 switch it off like the complex image steps.
   variant FFTW_AMD_K_IMG2DLR (pass2dlr.hpp): the same step under the same layout rule for extents in {16, 32, 40, 48,
   64} with at least one above 32, where the axis-by-axis plans make a real-row pass, the untangle / tangle and a
   strided pass through a scratch buffer.  fa_hip_img2dlr_tile is the only source of what its kernels cover.  The
   untangle / tangle twiddles are the stage table of the row axis (table, always), the intra-axis twiddles of a column
   axis of two register stages that of the column axis (table2, n0 > 32).  A knob of its own (cfg.real_imgl,
   FFTW_AMD_REAL_IMGL=1): existing tests plan 64 x 64 with FFTW_AMD_REAL_IMG=1 and interpret the plan with the base
   numpy interpreter.  1 = emitted. */
static int emit_real_image(plan *p, int fwd, int variant) {
    const fa_dim *col = &p->dims[0], *row = &p->dims[1];
    fftw_amd_step_desc *s;
    fa_loc in = { 0, 0, fwd ? 0 : p->in_im }, out = { 1, 0, fwd ? p->out_im : 0 };
    sdim d;
    i64 n0, n1, cp, rp, r_el, c_el, c_row, r_img, c_img;
    int T;
    if (!(variant == FFTW_AMD_K_IMG2DR ? p->cfg.real_img : p->cfg.real_imgl)) return 0;
    if (p->rank != 2 || p->hrank > 1 || p->knobs.no_tuned || p->knobs.no_img2d) return 0;
    n0 = col->n; n1 = row->n;
    if (n0 > 64 || n1 > 64) return 0;
    T = (variant == FFTW_AMD_K_IMG2DR) ? fa_hip_img2dr_tile((int)n0, (int)n1, fwd) : fa_hip_img2dlr_tile((int)n0, (int)n1, fwd);
    if (T <= 0) return 0;
    cp = n1 + 2;
    r_el = fwd ? row->is : row->os; c_el = fwd ? row->os : row->is;
    rp = fwd ? col->is : col->os; c_row = fwd ? col->os : col->is;
    if ((fwd ? p->out_im : p->in_im) != 1) return 0;
    if (r_el != 1 || c_el != 2 || c_row != cp || (rp != n1 && rp != cp)) return 0;
    r_img = n0 * rp; c_img = n0 * cp;
    if (p->hrank && ((fwd ? p->hdims[0].is : p->hdims[0].os) != r_img || (fwd ? p->hdims[0].os : p->hdims[0].is) != c_img)) return 0;
    if (p->flags & FFTW_UNALIGNED) return 0;
    if (((size_t)p->ri % 16) || ((size_t)p->ro % 16)) return 0;
    s = new_step(p, FFTW_AMD_STEP_PASS);
    step_set_locs(s, in, out);
    s->flags = FFTW_AMD_F_REAL_IMG | (fwd ? FFTW_AMD_F_REAL_IN : FFTW_AMD_F_REAL_OUT);
    s->L = (int)n1;
    s->is_l = fwd ? 1 : 2;
    s->os_l = fwd ? 2 : 1;
    s->nradices = fa_radices(n1, s->radices);
    if (s->nradices < 0) { p->failed = 1; return 1; }
    s->tile_lo_n = (int)n0;
    s->tile_lo_is = fwd ? rp : cp;
    s->tile_lo_os = fwd ? cp : rp;
    d.n = p->hrank ? p->chunk : 1; d.is = fwd ? r_img : c_img; d.os = fwd ? c_img : r_img; d.tw = 0; d.is_batch = p->hrank ? 1 : 0;
    step_set_dims(p, s, &d, 1, 0);
    s->tile = T;
    s->variant = variant;
    if (variant == FFTW_AMD_K_IMG2DLR) {
        s->table = tab_stage(p, n1);
        if (n0 > 32) s->table2 = tab_stage(p, n0);
    }
    p->est_flops += 2.5 * (double)(n0 * n1) * (double)d.n * log2((double)(n0 * n1));
    return 1;
}

/* A batch of small three-dimensional r2c (fwd) or c2r transforms n0 x n1 x n2 in ONE trip (FFTW_AMD_K_VOL3DR,
   pass3dr.hpp): a workgroup takes T whole real volumes and does all three axes in registers, where the axis-by-axis
   plans make one trip for the real axis, one for the untangle / tangle and one per complex axis, through a scratch
   buffer.  The step has no other executor, so everything it needs is settled here: rank 3, at most one howmany loop
   that steps over exactly one volume on both sides, the real side with element stride 1, row pitch n2 or n2 + 2, plane
   pitch n1 rows and volume pitch n0 planes, the complex side interleaved with stride 2, rows of n2 / 2 + 1 entries
   and dense planes and volumes, 16-byte aligned arrays, no FFTW_UNALIGNED.  In place only with the padded pitch (a
   volume then occupies the same words on both sides).  No scratch, no table.  fa_hip_vol3dr_tile is the only source
   of what the kernels cover.  Off under FFTW_ESTIMATE (cfg.real_vol, FFTW_AMD_REAL_VOL=1 -- a knob of its own:
   existing tests plan rank-3 real problems with FFTW_AMD_REAL_IMG=1 and interpret them with the base numpy
   interpreter, which does not know the step); a candidate of the FFTW_MEASURE search for rank-3 r2c / c2r problems,
   remembered by wisdom.  FFTW_AMD_NO_IMG2D=1 and FFTW_AMD_NO_TUNED=1 switch it off like its siblings.  1 = emitted. */
static int emit_real_volume(plan *p, int fwd) {
    const fa_dim *d0 = &p->dims[0], *d1 = &p->dims[1], *d2 = &p->dims[2];
    fftw_amd_step_desc *s;
    fa_loc in = { 0, 0, fwd ? 0 : p->in_im }, out = { 1, 0, fwd ? p->out_im : 0 };
    sdim d;
    i64 n0, n1, n2, cp, rp, r_vol, c_vol;
    int T;
    if (!p->cfg.real_vol || p->rank != 3 || p->hrank > 1 || p->knobs.no_tuned || p->knobs.no_img2d) return 0;
    n0 = d0->n; n1 = d1->n; n2 = d2->n;
    if (n0 > 32 || n1 > 32 || n2 > 32) return 0;
    T = fa_hip_vol3dr_tile((int)n0, (int)n1, (int)n2, fwd);
    if (T <= 0) return 0;
    cp = n2 + 2;
    rp = fwd ? d1->is : d1->os;
    if ((fwd ? p->out_im : p->in_im) != 1) return 0;
    if ((fwd ? d2->is : d2->os) != 1 || (fwd ? d2->os : d2->is) != 2) return 0;
    if ((rp != n2 && rp != cp) || (fwd ? d1->os : d1->is) != cp) return 0;
    if ((fwd ? d0->is : d0->os) != n1 * rp || (fwd ? d0->os : d0->is) != n1 * cp) return 0;
    r_vol = n0 * n1 * rp; c_vol = n0 * n1 * cp;
    if (p->hrank && ((fwd ? p->hdims[0].is : p->hdims[0].os) != r_vol || (fwd ? p->hdims[0].os : p->hdims[0].is) != c_vol)) return 0;
    if (p->inplace && rp != cp) return 0;
    if (p->flags & FFTW_UNALIGNED) return 0;
    if (((size_t)p->ri % 16) || ((size_t)p->ro % 16)) return 0;
    s = new_step(p, FFTW_AMD_STEP_PASS);
    step_set_locs(s, in, out);
    s->flags = FFTW_AMD_F_REAL_VOL | (fwd ? FFTW_AMD_F_REAL_IN : FFTW_AMD_F_REAL_OUT);
    s->L = (int)n2;
    s->is_l = fwd ? 1 : 2;
    s->os_l = fwd ? 2 : 1;
    s->nradices = fa_radices(n2, s->radices);
    if (s->nradices < 0) { p->failed = 1; return 1; }
    s->tile_lo_n = (int)n1;
    s->tile_lo_is = fwd ? rp : cp;
    s->tile_lo_os = fwd ? cp : rp;
    s->aux_n = n0;
    d.n = p->hrank ? p->chunk : 1; d.is = fwd ? r_vol : c_vol; d.os = fwd ? c_vol : r_vol; d.tw = 0; d.is_batch = p->hrank ? 1 : 0;
    step_set_dims(p, s, &d, 1, 0);
    s->tile = T;
    s->variant = FFTW_AMD_K_VOL3DR;
    p->est_flops += 2.5 * (double)(n0 * n1 * n2) * (double)d.n * log2((double)(n0 * n1 * n2));
    return 1;
}

/* r2c: last dim real -> half spectrum, then complex DFTs over the other dims
   on the half-spectrum array (reference rank_geq2_rdft2 A.c:10111-10282).
   p->dims[].is are strides of the REAL array (doubles), .os of the complex
   array (doubles, so 2 per complex). */
static void build_r2c(plan *p) {
    int r = p->rank, a, j;
    i64 nl = p->dims[r - 1].n, half = nl / 2 + 1;
    i64 ext[FA_MAXRANK];
    fa_loc in = { 0, 0, 0 }, out = { 1, 0, p->out_im };
    fa_axis ax;
    if (emit_real_image(p, 1, FFTW_AMD_K_IMG2DR)) return;
    if (emit_real_image(p, 1, FFTW_AMD_K_IMG2DLR)) return;
    if (emit_real_volume(p, 1)) return;
    for (j = 0; j < r; ++j) ext[j] = p->dims[j].n;
    ext[r - 1] = half;

    memset(&ax, 0, sizeof(ax));
    if (collect_loops(p, p->dims, r, r - 1, NULL, 0, &ax)) { p->failed = 1; return; }

    emit_r2c_axis(p, nl, &ax, in, p->dims[r - 1].is, out, p->dims[r - 1].os, 0, 0, 0, 0);

    for (a = r - 2; a >= 0; --a) {
        fa_axis cx;
        memset(&cx, 0, sizeof(cx));
        cx.n = p->dims[a].n;
        cx.is = cx.os = p->dims[a].os;
        cx.src = cx.dst = out;
        if (collect_loops(p, p->dims, r, a, ext, 1, &cx)) { p->failed = 1; return; }
        fa_emit_axis(p, &cx);
    }
}

/* The backward twin of emit_r2c_decimated: a long c2r transform in TWO trips, n = L1 x L2 real points.
     trip 1   rows k1 = 0 ... L1 / 2 of the half spectrum read as [L2][L1]: Y[k2] = X[k1 + L1 k2] below L2 / 2, the
              conjugate of X[(L1 - k1) + L1 (L2 - 1 - k2)] above (every index stays within 0 ... n / 2), backward DFT
              of length L2 along the row, twiddle w_n^(+k1 j2) on the output, and the rows k1 and L1 - k1 of the
              scratch image Z[k1][c] = A[k1][2c] + i A[k1][2c + 1] stored from the one result (A[L1 - k1] = conj A[k1])
              (FFTW_AMD_F_REAL_DEC_C2R, pass3t_kernel RD = 2)
     trip 2   the plain backward complex pass of length L1 down the columns of Z, which leaves the pairs
              (x[j1 L2 + 2c], x[j1 L2 + 2c + 1]) in the real output
   The three-trip plans are tangle + two passes.  Z has the r2c plan's layout (plain row-major), so trip 2 is that
   plan's trip 1 run the other way and trip 1 stores 64-byte runs, four pairs of a row per quarter wave.
   MEASURED (tools/perf/perf_c2r_two_trip.py, profiles/r04_c2r_two_trip.txt; ms per 4 GiB of output, median of 9, two chunk
   lanes, against the three-trip plan of the same binary): 2^22 4.33 against 4.17 (a tie: the ranges overlap), 2^21 3.56
   against 4.08, 2^20 3.51 against 4.14.  Per step the rows trip takes 1.7 ... 2.6 x the column pass (2^22: 5.58 and 3.22 ms
   summed over the chunks of both lanes): its 64-byte store runs are the next lever; neither remedy (a stage-C owner map
   with d1 fastest, a scratch layout blocked in c) has been built or measured.  Off under
   FFTW_ESTIMATE like its twin (cfg.real_dec, FFTW_AMD_REAL_DEC=1), a candidate of the FFTW_MEASURE search for c2r
   problems, remembered by wisdom through the same bit.  r2r problems whose inner transform is a c2r keep their plans
   (no prologue / epilogue fusion here).  The plan never writes its input.  Reference counterpart: ct_hc2c backward
   (fftw/fftw_api.c:5551-5603, fftw/rdft_scalar/r2cb/hc2cbdft_*.c).  The first step has no fallback executor, so
   everything it needs is settled here.  1 = emitted. */
static int emit_c2r_decimated(plan *p, i64 nl, const fa_axis *ax, fa_loc cur, fa_loc out) {
    const i64 L2 = FA_DEC_L2, L1 = real_dec_geometry(p, nl, ax, cur, out, 0);
    const int n0 = p->nsteps;
    const double flops0 = p->est_flops;
    i64 zts, lts[FA_MAXLOOPS + 1];
    fa_axis c_ax;
    fa_loc z;
    sdim d[FA_MAXLOOPS + 1];
    int ok;
    if (!L1) return 0;
    z = scratch_image(p, ax, 1, nl / 2, &zts, lts);
    d[0].n = L1 / 2 + 1; d[0].is = 2; d[0].os = (L2 / 2) * zts; d[0].tw = 1; d[0].is_batch = 0;
    emit_pass(p, cur, z, L2, 2 * L1, zts, d, 1 + loop_sdims(ax, NULL, lts, d + 1), nl,
              FFTW_AMD_F_SWAP_IN | FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_DEC_C2R);
    ok = !p->failed && real_dec_rows_step_ok(p, L1);
    if (ok) {
        c_ax = real_dec_column_axis(ax, L1, out, z, zts, lts, 0);
        fa_emit_axis(p, &c_ax);
        ok = !p->failed && p->nsteps == n0 + 2;
    }
    return real_dec_end(p, ok, n0, flops0, z.buf);
}

/* half spectrum -> real along one axis (unnormalised backward).  ax: the loops
   (.is = strides in the complex source `cur`, .os = strides in the real
   destination); cs / rs: element strides of the transform index, in doubles. */
/* pro: 0 = `cur` holds the half spectrum as complex numbers; FFTW_AMD_R2R_PRE_* =
   `cur` is the user's real r2r input of stride cs and the tangle step applies
   that prologue while loading (even lengths only, see r2r_can_fuse)
   ps / pim: pair geometry of the real output, as in emit_r2c_axis */
static void emit_c2r_axis(plan *p, i64 nl, const fa_axis *axp, fa_loc cur, i64 cs, fa_loc out, i64 rs, int pro,
                          i64 ps, i64 pim, int post) {
    fa_axis ax = *axp;
    i64 zts, lts[FA_MAXLOOPS + 1];
    sdim d[FA_MAXLOOPS + 1];
    fftw_amd_step_desc *s;
    fa_loc z;
    int j, nd, rows_tile;
    if (ps == 0) { ps = 2 * rs; pim = rs; }
    if (pro == 0 && post == 0 && ps == 2 && pim == 1 && cs == 2 && emit_c2r_decimated(p, nl, &ax, cur, out)) return;
    if (use_radix4_real(p, nl, &ax)) {
        /* transpose of the radix-4 r2c plan: tangle into two quarter-length
           spectra, two backward complex DFTs of size m straight into the real array */
        i64 m = nl / 4;
        fa_axis q_ax = ax, lay;
        int vloop = q_ax.nloops++;
        q_ax.loops[vloop].n = 2;
        q_ax.loops[vloop].is = 0;
        q_ax.loops[vloop].os = ps;
        lay = q_ax;
        lay.loops[vloop].is = 1;
        z = scratch_image(p, &lay, 2, m, &zts, lts);
        q_ax.dense = (pim == 1 && ps == 2);

        s = new_step(p, FFTW_AMD_STEP_C2R_PRE4);
        step_set_locs(s, cur, z);
        s->is_l = cs;
        s->os_l = zts;
        s->aux_n = nl;
        s->aux_valid = lts[vloop];
        r2r_fuse_tables(p, s, nl, pro);
        nd = loop_sdims(&ax, NULL, lts, d);
        s->kpos = order_dims_kpos(d, &nd, 0, cs);
        step_set_dims(p, s, d, nd, -1);

        q_ax.n = m;
        q_ax.is = zts;
        q_ax.os = 2 * ps;
        q_ax.src = z;
        q_ax.dst = out;
        q_ax.dst.im = pim;
        q_ax.flags_in = FFTW_AMD_F_SWAP_IN;
        q_ax.flags_out = FFTW_AMD_F_SWAP_OUT;
        for (j = 0; j < q_ax.nloops; ++j) q_ax.loops[j].is = lts[j];
        fa_emit_axis(p, &q_ax);
        buf_release(p, z.buf);
    } else if (nl % 2 == 0 && nl >= 2 && (post != 0 || (ps == 2 && pim == 1)) &&
               (pro != 0 || (cs == 2 && cur.im == 1)) &&
               (rows_tile = real_rows_tile_for(p, &ax, nl / 2, pro || post, 0)) > 0 &&
               real_rows_layout_ok(p, &ax, cur, out, pro, post)) {
        emit_real_rows_step(p, 0, nl, &ax, cur, cs, out, rs, pro, post, rows_tile);
    } else if (nl % 2 == 0 && nl >= 2) {
        fa_axis half_ax = ax;
        z = scratch_image(p, &ax, 1, nl / 2, &zts, lts);

        s = new_step(p, FFTW_AMD_STEP_C2R_PRE);
        step_set_locs(s, cur, z);
        s->is_l = cs;
        s->os_l = zts;
        s->aux_n = nl;
        r2r_fuse_tables(p, s, nl, pro);
        nd = loop_sdims(&ax, NULL, lts, d);
        s->kpos = order_dims_kpos(d, &nd, 0, cs);
        step_set_dims(p, s, d, nd, -1);

        half_ax.n = nl / 2;
        half_ax.is = zts;
        half_ax.os = ps;
        half_ax.src = z;
        half_ax.dst = out;
        half_ax.dst.im = pim;
        half_ax.flags_in = FFTW_AMD_F_SWAP_IN;
        half_ax.flags_out = FFTW_AMD_F_SWAP_OUT;
        for (j = 0; j < ax.nloops; ++j) half_ax.loops[j].is = lts[j];
        fa_emit_axis(p, &half_ax);
        buf_release(p, z.buf);
    } else {
        fa_axis full_ax = ax;
        z = scratch_image(p, &ax, 1, nl, &zts, lts);
        emit_copy(p, FFTW_AMD_STEP_HERM_EXPAND, cur, z, nl, nl, cs, zts, d, loop_sdims(&ax, NULL, lts, d), 0, -1, -1);
        full_ax.n = nl;
        full_ax.is = zts;
        full_ax.os = rs;
        full_ax.src = z;
        full_ax.dst = out;
        full_ax.flags_in = FFTW_AMD_F_SWAP_IN;
        /* backward by the swap identity: the real result is the imaginary
           slot of the swapped output, so swap on store and keep the real part */
        full_ax.flags_out = FFTW_AMD_F_SWAP_OUT | FFTW_AMD_F_REAL_OUT;
        for (j = 0; j < ax.nloops; ++j) full_ax.loops[j].is = lts[j];
        fa_emit_axis(p, &full_ax);
        buf_release(p, z.buf);
    }
}

/* c2r: complex backward DFTs over the leading dims (into scratch, so the
   caller's input survives), then half spectrum -> real along the last dim.
   p->dims[].is: strides of the complex array, .os: of the real array. */
static void build_c2r(plan *p) {
    int r = p->rank, a, j;
    i64 nl = p->dims[r - 1].n, half = nl / 2 + 1;
    i64 ext[FA_MAXRANK];
    fa_loc in = { 0, 0, p->in_im }, out = { 1, 0, 0 };
    fa_loc cur = in;
    fa_dim cdims[FA_MAXRANK];     /* current layout of the half-spectrum array */
    fa_dim chd[FA_MAXRANK];
    int cbuf = -1;
    fa_axis ax;

    if (emit_real_image(p, 0, FFTW_AMD_K_IMG2DR)) return;
    if (emit_real_image(p, 0, FFTW_AMD_K_IMG2DLR)) return;
    if (emit_real_volume(p, 0)) return;
    for (j = 0; j < r; ++j) { ext[j] = p->dims[j].n; cdims[j] = p->dims[j]; cdims[j].os = p->dims[j].is; }
    ext[r - 1] = half;
    for (j = 0; j < p->hrank; ++j) { chd[j] = p->hdims[j]; chd[j].os = p->hdims[j].is; }

    if (r > 1) {
        /* dense scratch for the half spectrum: [batch][d0]...[half] */
        i64 stride = 2, total;
        fa_dim sd[FA_MAXRANK], sh[FA_MAXRANK];
        plan view;
        int first = 1;
        for (j = r - 1; j >= 0; --j) { sd[j].n = ext[j]; sd[j].os = stride; stride *= ext[j]; }
        for (j = p->hrank - 1; j >= 1; --j) { sh[j].n = p->hdims[j].n; sh[j].os = stride; stride *= p->hdims[j].n; }
        if (p->hrank) { sh[0].n = p->hdims[0].n; sh[0].os = stride; stride *= p->chunk; }
        total = stride;
        cbuf = buf_acquire(p, total);
        /* leading dims: in -> scratch for the first, in place afterwards */
        for (a = r - 2; a >= 0; --a) {
            fa_axis cx;
            fa_dim td[FA_MAXRANK];
            memset(&cx, 0, sizeof(cx));
            for (j = 0; j < r; ++j) {
                td[j].n = ext[j];
                td[j].is = first ? p->dims[j].is : sd[j].os;
                td[j].os = sd[j].os;
            }
            view = *p;
            for (j = 0; j < p->hrank; ++j) {
                view.hdims[j].is = first ? p->hdims[j].is : sh[j].os;
                view.hdims[j].os = sh[j].os;
            }
            cx.n = p->dims[a].n;
            cx.is = td[a].is;
            cx.os = td[a].os;
            cx.src = first ? in : (fa_loc){ cbuf, 0, 1 };
            cx.dst = (fa_loc){ cbuf, 0, 1 };
            cx.flags_in = FFTW_AMD_F_SWAP_IN;
            cx.flags_out = FFTW_AMD_F_SWAP_OUT;
            if (collect_loops(&view, td, r, a, ext, 0, &cx)) { p->failed = 1; return; }
            fa_emit_axis(p, &cx);
            first = 0;
        }
        cur = (fa_loc){ cbuf, 0, 1 };
        for (j = 0; j < r; ++j) { cdims[j].is = sd[j].os; }
        for (j = 0; j < p->hrank; ++j) chd[j].is = sh[j].os;
    }

    /* loops of the last-dim c2r: source strides = current complex layout,
       destination strides = the real output array */
    memset(&ax, 0, sizeof(ax));
    {
        plan view = *p;
        fa_dim td[FA_MAXRANK];
        for (j = 0; j < r; ++j) { td[j].n = p->dims[j].n; td[j].is = cdims[j].is; td[j].os = p->dims[j].os; }
        for (j = 0; j < p->hrank; ++j) { view.hdims[j].is = chd[j].is; view.hdims[j].os = p->hdims[j].os; }
        if (collect_loops(&view, td, r, r - 1, NULL, 0, &ax)) { p->failed = 1; return; }
    }

    emit_c2r_axis(p, nl, &ax, cur, cdims[r - 1].is, out, p->dims[r - 1].os, 0, 0, 0, 0);
    if (cbuf >= 0) buf_release(p, cbuf);
}


/* ------------------------------------------------------------------ r2r */
/* One r2r axis = PRE step (user reals -> inner input), an inner real or complex
   DFT on scratch, POST step (inner output -> user reals).  The reference gets the
   same transforms from R2HC/HC2R children with pre/post loops around them:
   reodft010e-r2hc (fftw/fftw_api.c:12465-12660), redft00e-r2hc-pad (:11932-11965),
   rodft00e-r2hc-pad (:14012-14050), reodft11e-radix2 (:13362-13640), reodft11e-r2hc-odd
   (:13097-13230), dht-r2hc (:6365-6387).  Derivations of the index maps: DESIGN.md
   section 9. */

static fftw_amd_step_desc *emit_r2r_step(plan *p, int mode, i64 n, i64 K, i64 twmod,
                                         fa_loc src, i64 is_k, fa_loc dst, i64 os_k,
                                         const fa_axis *ax, const i64 *lis, const i64 *los,
                                         int order_by_dst) {
    fftw_amd_step_desc *s = new_step(p, FFTW_AMD_STEP_R2R);
    sdim d[FA_MAXLOOPS + 1];
    int cnt = loop_sdims(ax, lis, los, d);
    s->variant = mode;
    step_set_locs(s, src, dst);
    s->is_l = is_k;
    s->os_l = os_k;
    s->aux_n = n;
    s->aux_valid = K;
    if (twmod) tab_tw2(p, twmod, &s->tw_lo, &s->tw_hi, &s->tw_shift);
    /* flatten order: smallest user-side stride fastest, the batch loop last */
    s->kpos = order_dims_kpos(d, &cnt, order_by_dst, order_by_dst ? os_k : is_k);
    step_set_dims(p, s, d, cnt, -1);
    p->est_flops += 4.0 * (double)K;
    return s;
}

/* ax: loops with .is = user source strides, .os = user destination strides */
static void emit_r2r_axis(plan *p, int kind, i64 n, const fa_axis *axp, fa_loc in, i64 rs,
                          fa_loc out, i64 os) {
    enum { IN_R2C, IN_C2R, IN_C2C };
    int pre = 0, post = 0, inner = IN_R2C, j, nl = axp->nloops, fuse_pre = 0, fuse_post = 0, rows_pre = 0, rows_post = 0;
    i64 N = n, cntA = 0, unitA = 1, cntB = 0, unitB = 1, twmod = 0, Kpre = 0, Kpost = 0;
    i64 lis_user[FA_MAXLOOPS], los_user[FA_MAXLOOPS], ltsA[FA_MAXLOOPS], ltsB[FA_MAXLOOPS];
    i64 tsA = 0, tsB = 0, psA = 0, pimA = 0, psB = 0, pimB = 0;
    int abuf = -1, bbuf = -1, pairA = 0, pairB = 0;
    fa_loc A = { -1, 0, 1 }, B = { -1, 0, 1 };
    fa_axis lay, iax;
    for (j = 0; j < nl; ++j) { lis_user[j] = axp->loops[j].is; los_user[j] = axp->loops[j].os; }

    switch (kind) {
    case FFTW_R2HC: post = FFTW_AMD_R2R_POST_R2HC; goto via_r2c;
    case FFTW_DHT:  post = FFTW_AMD_R2R_POST_DHT;
    via_r2c:
        inner = IN_R2C; N = n; cntB = n / 2 + 1; unitB = 2; Kpost = n / 2 + 1;
        break;
    case FFTW_HC2R:
        pre = FFTW_AMD_R2R_PRE_HC2R; inner = IN_C2R; N = n; cntA = n / 2 + 1; unitA = 2; Kpre = n / 2 + 1;
        break;
    case FFTW_REDFT10: pre = FFTW_AMD_R2R_PRE_E10; post = FFTW_AMD_R2R_POST_E10; goto makhoul_f;
    case FFTW_RODFT10: pre = FFTW_AMD_R2R_PRE_O10; post = FFTW_AMD_R2R_POST_O10;
    makhoul_f:
        inner = IN_R2C; N = n; cntA = n; unitA = 1; cntB = n / 2 + 1; unitB = 2;
        Kpre = (n + 1) / 2; Kpost = n / 2 + 1; twmod = 4 * n;
        break;
    case FFTW_REDFT01: pre = FFTW_AMD_R2R_PRE_E01; post = FFTW_AMD_R2R_POST_E01; goto makhoul_b;
    case FFTW_RODFT01: pre = FFTW_AMD_R2R_PRE_O01; post = FFTW_AMD_R2R_POST_O01;
    makhoul_b:
        inner = IN_C2R; N = n; cntA = n / 2 + 1; unitA = 2; cntB = n; unitB = 1;
        Kpre = n / 2 + 1; Kpost = (n + 1) / 2; twmod = 4 * n;
        break;
    case FFTW_REDFT00:
        if (n < 2) { p->failed = 1; return; }
        pre = FFTW_AMD_R2R_PRE_E00; post = FFTW_AMD_R2R_POST_E00;
        inner = IN_R2C; N = 2 * (n - 1); cntA = N; unitA = 1; cntB = N / 2 + 1; unitB = 2;
        Kpre = N; Kpost = n;
        break;
    case FFTW_RODFT00:
        pre = FFTW_AMD_R2R_PRE_O00; post = FFTW_AMD_R2R_POST_O00;
        inner = IN_R2C; N = 2 * (n + 1); cntA = N; unitA = 1; cntB = N / 2 + 1; unitB = 2;
        Kpre = N; Kpost = n;
        break;
    case FFTW_REDFT11:
    case FFTW_RODFT11: {
        int odd = (kind == FFTW_RODFT11);
        inner = IN_C2C; twmod = 8 * n; unitA = 2;
        if (n % 2 == 0) {
            pre = odd ? FFTW_AMD_R2R_PRE_O11 : FFTW_AMD_R2R_PRE_E11;
            post = odd ? FFTW_AMD_R2R_POST_O11 : FFTW_AMD_R2R_POST_E11;
            N = n / 2; cntA = N; Kpre = N; Kpost = N;
        } else {
            pre = odd ? FFTW_AMD_R2R_PRE_O11ODD : FFTW_AMD_R2R_PRE_E11ODD;
            post = odd ? FFTW_AMD_R2R_POST_O11ODD : FFTW_AMD_R2R_POST_E11ODD;
            N = 2 * n; cntA = N; Kpre = N; Kpost = n;
        }
        break;
    }
    default:
        p->failed = 1;
        return;
    }

    /* even inner length: the untangle / tangle step of the real transform does the
       r2r post / pre processing itself, one pass over the data less */
    if (inner == IN_R2C && post && r2r_can_fuse(p, N)) { fuse_post = 1; cntB = 0; }
    /* short rows: the fused real-rows kernel also gathers the pre-processed sequence from the
       user's row itself -- the whole r2r axis is one trip */
    if (fuse_post && pre && pre != FFTW_AMD_R2R_PRE_HC2R && fa_hip_r2c_rows_tile((int)(N / 2)) > 0) {
        fa_axis tax = *axp;
        if (real_rows_layout_ok(p, &tax, in, out, pre, post)) { rows_pre = pre; cntA = 0; }
    }
    if (inner == IN_C2R && pre && r2r_can_fuse(p, N)) { fuse_pre = 1; cntA = 0; }
    /* short rows: the fused c2r rows kernel also does the DCT-III / DST-III output shuffle */
    if (fuse_pre && post && fa_hip_r2c_rows_tile((int)(N / 2)) > 0) {
        fa_axis tax = *axp;
        if (real_rows_layout_ok(p, &tax, in, out, pre, post)) { rows_post = post; cntB = 0; }
    }

    /* Real scratch sequences of even length are laid out as adjacent pairs
       (sample 2j, 2j+1) = one interleaved complex number of stride ts: whatever loops end
       up innermost, the inner real transform then reads / writes 16-byte elements and its
       first / last pass can be a register kernel.  pairA / pairB = 1 marks that layout;
       odd lengths keep a plain real stride (pair stride 2 ts, pair im ts). */
    if (cntA) {
        i64 total;
        lay = *axp;
        lay.is = rs;
        if (unitA == 1 && cntA % 2 == 0) {
            pairA = 1;
            total = scratch_layout_u(&lay, cntA / 2, 2, &tsA, ltsA);
        } else {
            total = scratch_layout_u(&lay, cntA, unitA, &tsA, ltsA);
        }
        abuf = buf_acquire(p, total);
        A.buf = abuf;
    }
    if (cntB) {
        i64 total;
        lay = *axp;
        lay.is = os;
        for (j = 0; j < nl; ++j) lay.loops[j].is = los_user[j];
        if (unitB == 1 && cntB % 2 == 0) {
            pairB = 1;
            total = scratch_layout_u(&lay, cntB / 2, 2, &tsB, ltsB);
        } else {
            total = scratch_layout_u(&lay, cntB, unitB, &tsB, ltsB);
        }
        bbuf = buf_acquire(p, total);
        B.buf = bbuf;
    }
    /* pair geometry as the steps see it: (pair stride, distance inside the pair) */
    psA = (unitA == 1) ? (pairA ? tsA : 2 * tsA) : 0;  pimA = (unitA == 1) ? (pairA ? 1 : tsA) : 0;
    psB = (unitB == 1) ? (pairB ? tsB : 2 * tsB) : 0;  pimB = (unitB == 1) ? (pairB ? 1 : tsB) : 0;

    if (pre && !fuse_pre && !rows_pre) {
        fa_loc dA = A;
        if (unitA == 1) dA.im = pimA;          /* real sequence: element j at (j >> 1) psA + (j & 1) pimA */
        emit_r2r_step(p, pre, n, Kpre, twmod, in, rs, dA, unitA == 1 ? psA : tsA, axp, lis_user, ltsA, 0);
    }

    iax = *axp;
    iax.flags_in = iax.flags_out = 0;
    iax.dense = 0;
    if (inner == IN_R2C) {
        fa_loc s = pre ? A : in;
        for (j = 0; j < nl; ++j) {
            iax.loops[j].is = (pre && !rows_pre) ? ltsA[j] : lis_user[j];
            iax.loops[j].os = fuse_post ? los_user[j] : ltsB[j];
        }
        s.im = 0;
        if (rows_pre) {
            emit_r2c_axis(p, N, &iax, in, rs, out, os, post, 0, 0, rows_pre);
            post = 0;
        } else if (fuse_post) {
            emit_r2c_axis(p, N, &iax, s, pre ? pimA : rs, out, os, post, pre ? psA : 0, pre ? pimA : 0, 0);
            post = 0;
        } else {
            emit_r2c_axis(p, N, &iax, s, pre ? pimA : rs, B, tsB, 0, pre ? psA : 0, pre ? pimA : 0, 0);
        }
    } else if (inner == IN_C2R) {
        fa_loc d = post ? B : out;
        for (j = 0; j < nl; ++j) {
            iax.loops[j].is = fuse_pre ? lis_user[j] : ltsA[j];
            iax.loops[j].os = post ? ltsB[j] : los_user[j];
        }
        d.im = 0;
        if (rows_post) {
            for (j = 0; j < nl; ++j) iax.loops[j].os = los_user[j];
            emit_c2r_axis(p, N, &iax, in, rs, out, os, pre, 0, 0, rows_post);
            post = 0;
        } else if (fuse_pre) emit_c2r_axis(p, N, &iax, in, rs, d, post ? pimB : os, pre, post ? psB : 0, post ? pimB : 0, 0);
        else emit_c2r_axis(p, N, &iax, A, tsA, d, post ? pimB : os, 0, post ? psB : 0, post ? pimB : 0, 0);
    } else {
        for (j = 0; j < nl; ++j) { iax.loops[j].is = ltsA[j]; iax.loops[j].os = ltsA[j]; }
        iax.n = N; iax.is = tsA; iax.os = tsA;
        iax.src = A; iax.dst = A;
        fa_emit_axis(p, &iax);
        B = A; tsB = tsA; unitB = 2;
        for (j = 0; j < nl; ++j) ltsB[j] = ltsA[j];
    }

    if (post) {
        fa_loc sB = B;
        if (unitB == 1) sB.im = pimB;          /* real sequence read as pairs, see above */
        emit_r2r_step(p, post, n, Kpost, twmod, sB, unitB == 1 ? psB : tsB, out, os, axp, ltsB, los_user, 1);
    }
    if (abuf >= 0) buf_release(p, abuf);
    if (bbuf >= 0) buf_release(p, bbuf);
}

/* separable r2r: every dim gets its own kind (reference problem_rdft with
   kind[] per dim, fftw/fftw_api.c:9100-9150); the first processed axis moves the
   data from the input to the output array, the others work in place there */
static void build_r2r(plan *p) {
    int a, first = 1;
    fa_loc in = { 0, 0, 0 }, out = { 1, 0, 0 };
    if (p->rank == 0 && p->via_scratch) {
        /* in place with different strides on the two sides (same locations, no square transposition): through a dense
           row-major scratch image in one chunk, as build_c2c does -- every read of the array precedes every write.
           One half is a plain contiguous copy, the other the transposition. */
        fa_dim sh[FA_MAXRANK];
        fa_loc scr;
        i64 stride = 1;
        int i, sbuf;
        memcpy(sh, p->hdims, sizeof(sh));
        for (i = p->hrank - 1; i >= 0; --i) {
            p->hdims[i].os = stride;
            stride *= (i == 0 ? p->chunk : p->hdims[i].n);
        }
        sbuf = buf_acquire(p, stride);
        scr.buf = sbuf; scr.base = 0; scr.im = 0;
        emit_loops_copy(p, in, scr, 1);
        for (i = 0; i < p->hrank; ++i) { p->hdims[i].is = p->hdims[i].os; p->hdims[i].os = sh[i].os; }
        if (!p->failed) emit_loops_copy(p, scr, out, 1);
        memcpy(p->hdims, sh, sizeof(sh));
        buf_release(p, sbuf);
        return;
    }
    if (p->rank == 0) {
        /* rank 0: strided copy of reals (reference rdft rank0 solver, fftw/fftw_api.c:9655-9720) */
        build_rank0(p, in, out);
        return;
    }
    for (a = p->rank - 1; a >= 0; --a) {
        fa_axis ax;
        memset(&ax, 0, sizeof(ax));
        if (collect_loops(p, p->dims, p->rank, a, NULL, !first, &ax)) { p->failed = 1; return; }
        emit_r2r_axis(p, p->kinds[a], p->dims[a].n, &ax, first ? in : out,
                      first ? p->dims[a].is : p->dims[a].os, out, p->dims[a].os);
        if (p->failed) return;
        first = 0;
    }
}

static void build_steps(plan *p) {
    switch (p->type) {
    case FA_C2C: build_c2c(p); break;
    case FA_R2C: build_r2c(p); break;
    case FA_C2R: build_c2r(p); break;
    case FA_R2R: build_r2r(p); break;
    default: p->failed = 1;
    }
}

/* Cache policy of the streams that touch the caller's arrays (FFTW_AMD_F_NT_IN / NT_OUT).
   An array that one execution reads once (or writes and never reads back) is moved with
   nontemporal accesses when the batch is too large to stay cached anyway: the Infinity
   Cache (256 MiB) then keeps the scratch image between two passes of a chunk instead of
   input / output lines nobody asks for again (tests/micro/membw3.hip).  Small problems keep
   plain accesses so that a consumer kernel still finds the output on chip. */
static void mark_streaming_accesses(plan *p) {
    int i, j;
    double touched = ((double)(p->in_hi - p->in_lo) + (double)(p->out_hi - p->out_lo)) * sizeof(double);
    if (nt_policy() == 0 || (nt_policy() == 1 && touched < 384.0 * 1048576.0)) return;
    for (i = 0; i < p->nsteps; ++i) {
        fftw_amd_step_desc *s = &p->steps[i];
        if (s->src_buf == 0) {
            int readers = 0;
            for (j = 0; j < p->nsteps; ++j) readers += (p->steps[j].src_buf == 0) || (p->inplace && p->steps[j].src_buf == 1);
            if (readers == 1) s->flags |= FFTW_AMD_F_NT_IN;
        }
        if (s->dst_buf == 1) {
            int later = 0;
            for (j = i + 1; j < p->nsteps; ++j)
                later += p->steps[j].src_buf == 1 || p->steps[j].aux_buf == 1 || (p->inplace && p->steps[j].src_buf == 0);
            if (!later) s->flags |= FFTW_AMD_F_NT_OUT;
        }
    }
}

static int fa_build_steps_sized(plan *p);

int fa_build(plan *p) {
    int r;
    fa_read_knobs(&p->knobs);
    r = fa_build_steps_sized(p);
    if (r == 0 && p->batch > 0) mark_streaming_accesses(p);
    return r;
}

static int fa_build_steps_sized(plan *p) {
    i64 per_elem = 0;
    int i;
    p->batch = p->hrank ? p->hdims[0].n : 1;
    if (p->batch == 0) {   /* howmany == 0: a valid plan that does nothing */
        plan_reset_build(p);
        p->chunk = 0;
        return 0;
    }
    /* dry run at one batch element to size the scratch, then pick the chunk */
    plan_reset_build(p);
    p->chunk = 1;
    build_steps(p);
    if (p->failed) return -1;
    for (i = 2; i < p->nbufs; ++i) per_elem += p->buf_reals[i];
    if (per_elem == 0 || p->batch == 1 || p->single_chunk) {
        p->chunk = p->batch;
    } else {
        i64 c = (i64)(p->cfg.chunk_bytes / ((size_t)per_elem * sizeof(double)));
        if (c < 1) c = 1;
        if (c > p->batch) c = p->batch;
        p->chunk = c;
    }
    if (p->chunk != 1) {
        plan_reset_build(p);
        build_steps(p);
        if (p->failed) return -1;
        /* a plan can turn out scratch-free only once the batch loop has more than one entry
           (the fused rows kernels need rows to tile over): then nothing limits the chunk */
        per_elem = 0;
        for (i = 2; i < p->nbufs; ++i) per_elem += p->buf_reals[i];
        if (per_elem == 0 && p->chunk != p->batch) {
            p->chunk = p->batch;
            plan_reset_build(p);
            build_steps(p);
            if (p->failed) return -1;
        }
    }
    return 0;
}

/* ------------------------------------------------------------- printing */

static const char *kind_name(int k) {
    switch (k) {
    case FFTW_AMD_STEP_PASS: return "pass";
    case FFTW_AMD_STEP_COPY: return "copy";
    case FFTW_AMD_STEP_R2C_POST: return "r2c-untangle";
    case FFTW_AMD_STEP_C2R_PRE: return "c2r-tangle";
    case FFTW_AMD_STEP_RADER_MUL: return "rader-mul";
    case FFTW_AMD_STEP_HERM_EXPAND: return "herm-expand";
    case FFTW_AMD_STEP_R2C_POST4: return "r2c-untangle4";
    case FFTW_AMD_STEP_C2R_PRE4: return "c2r-tangle4";
    case FFTW_AMD_STEP_R2R: return "r2r";
    }
    return "?";
}

/* bounded append: never writes past cap, whatever the numbers print to */
static void sapp(char *s, size_t cap, size_t *len, const char *fmt, ...) {
    va_list ap;
    int w;
    if (*len + 1 >= cap) return;
    va_start(ap, fmt);
    w = vsnprintf(s + *len, cap - *len, fmt, ap);
    va_end(ap);
    if (w < 0) return;
    *len += (size_t)w;
    if (*len >= cap) *len = cap - 1;
}

/* lisp-like dump in the spirit of the reference's fftw_print_plan
   (fftw/fftw_api.c:1046-1080) */
char *fa_sprint(const plan *p) {
    size_t cap = 256 + (size_t)p->nsteps * 512, len = 0;
    char *s = (char *)malloc(cap);
    if (!s) return NULL;
    s[0] = 0;
    int i, j;
    const char *tn = p->type == FA_C2C ? "dft" : p->type == FA_R2C ? "rdft2-r2c" : p->type == FA_C2R ? "rdft2-c2r" : "rdft-r2r";
    sapp(s, cap, &len, "(hip-%s batch=%lld chunk=%lld", tn, p->batch, p->chunk);
    for (i = 0; i < p->nsteps; ++i) {
        const fftw_amd_step_desc *d = &p->steps[i];
        if (d->kind == FFTW_AMD_STEP_COPY && d->variant == FFTW_AMD_K_TRANSPOSE)
            sapp(s, cap, &len, "\n  (%s", (d->flags & FFTW_AMD_F_PAIR_SWAP) ? "transpose-inplace" : "transpose");
        else
            sapp(s, cap, &len, "\n  (%s", kind_name(d->kind));
        if (d->kind == FFTW_AMD_STEP_PASS) {
            /* which kernel runs the pass: reg32x32 / reg2 / reg3 = register-resident
               (pass1024 / passrr / pass3s), lds = runtime-radix LDS kernel + its radices */
            sapp(s, cap, &len, "-%d/", d->L);
            if (d->variant == FFTW_AMD_K_R2C) sapp(s, cap, &len, d->aux_valid ? "r2c-rows+r2r-post" : "r2c-rows");
            else if (d->variant == FFTW_AMD_K_C2R) sapp(s, cap, &len, d->aux_valid ? (d->aux_buf > 0 ? "c2r-rows+r2r-pre+post" : "c2r-rows+r2r-pre") : "c2r-rows");
            else if (d->variant == FFTW_AMD_K_P1024) sapp(s, cap, &len, "reg32x32");
            else if (d->variant == FFTW_AMD_K_RR) sapp(s, cap, &len, "reg2");
            else if (d->variant == FFTW_AMD_K_R3 && (d->flags & FFTW_AMD_F_REAL_DEC)) sapp(s, cap, &len, "reg3+real-decimated");
            else if (d->variant == FFTW_AMD_K_R3 && (d->flags & FFTW_AMD_F_REAL_DEC_C2R)) sapp(s, cap, &len, "reg3+c2r-decimated");
            else if (d->variant == FFTW_AMD_K_R3) sapp(s, cap, &len, (d->flags & FFTW_AMD_F_LO_DFT) ? (d->tile_lo_n == 4 ? "reg3+dft4-across-rows" : "reg3+dft2-across-rows") : "reg3");
            else if (d->variant == FFTW_AMD_K_R1) sapp(s, cap, &len, "reg1");
            else if (d->variant == FFTW_AMD_K_IMG2D) sapp(s, cap, &len, "img2d-%dx%d", d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_IMG2DL) sapp(s, cap, &len, "img2dl-%dx%d", d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_IMG2DW) sapp(s, cap, &len, "img2dw-%dx%d", d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_IMG2DR) sapp(s, cap, &len, "img2d-%s-%dx%d", (d->flags & FFTW_AMD_F_REAL_IN) ? "r2c" : "c2r", d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_IMG2DLR) sapp(s, cap, &len, "img2dl-%s-%dx%d", (d->flags & FFTW_AMD_F_REAL_IN) ? "r2c" : "c2r", d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_VOL3DR) sapp(s, cap, &len, "vol3d-%s-%dx%dx%d", (d->flags & FFTW_AMD_F_REAL_IN) ? "r2c" : "c2r", (int)d->aux_n, d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_VOL3D) sapp(s, cap, &len, "vol3d-%dx%dx%d", (int)d->aux_n, d->tile_lo_n, d->L);
            else if (d->variant == FFTW_AMD_K_BLUE) sapp(s, cap, &len, "bluestein-rows n=%lld", (long long)d->aux_n);
            else {
                sapp(s, cap, &len, "lds:");
                for (j = 0; j < d->nradices; ++j)
                    sapp(s, cap, &len, "%s%d", j ? "x" : "", d->radices[j]);
            }
            sapp(s, cap, &len, " tile=%d", d->tile);
            if (d->tw_n) sapp(s, cap, &len, " tw=%lld", d->tw_n);
        } else if (d->kind == FFTW_AMD_STEP_R2R ||
                   ((d->kind == FFTW_AMD_STEP_R2C_POST || d->kind == FFTW_AMD_STEP_R2C_POST4 ||
                     d->kind == FFTW_AMD_STEP_C2R_PRE || d->kind == FFTW_AMD_STEP_C2R_PRE4) && d->variant)) {
            /* untangle / tangle steps carry the name of a fused r2r epilogue / prologue */
            static const char *mn[] = { "?", "pre-hc2r", "pre-e10", "pre-o10", "pre-e01", "pre-o01", "pre-e00",
                "pre-o00", "pre-e11", "pre-o11", "pre-e11odd", "pre-o11odd", "post-r2hc", "post-dht",
                "post-e10", "post-o10", "post-e01", "post-o01", "post-e00", "post-o00", "post-e11",
                "post-o11", "post-e11odd", "post-o11odd" };
            int m = (d->variant >= 1 && d->variant <= FFTW_AMD_R2R_POST_O11ODD) ? d->variant : 0;
            sapp(s, cap, &len, "%s%s n=%lld", d->kind == FFTW_AMD_STEP_R2R ? "-" : "+r2r-",
                                    mn[m], d->aux_n);
        } else {
            sapp(s, cap, &len, " n=%lld", d->aux_n);
        }
        sapp(s, cap, &len, " buf%d->buf%d x", d->src_buf, d->dst_buf);
        for (j = 0; j < d->ndims; ++j)
            sapp(s, cap, &len, "%s%lld", j ? "," : "", d->dim_n[j]);
        sapp(s, cap, &len, ")");
    }
    sapp(s, cap, &len, ")");
    return s;
}
