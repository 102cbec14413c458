/*
 * exec_trace.c -- runs the executor (fftw3_amd/csrc/exec.c) on a CPU against a recording fake of the runtime part of
 * fa_hip.h and prints, one line per runtime call, what an execution enqueues on which stream.
 *
 * Built like `make san-c2r`: the C sources are compiled into the program, the HIP units (host-side tile tables, which
 * planning needs) come from the ordinary library.  The functions defined here take precedence over the library's.
 * Nothing is computed and no array is touched: an allocation is an untouched malloc, and a pointer is a "device"
 * pointer exactly when it lies inside a live one.
 *
 *     exec_trace <case>        the trace of one case on stdout; exit status 1 on an imbalance (see below)
 *     exec_trace --list        the case names
 *
 * One case per process: FFTW_AMD_PAIR and FFTW_AMD_HOST_PIPELINE are read once per process.
 *
 * Normal form.  Streams are s0 (the caller's), s1, s2 ... in creation order.  Pointers are d<k>+<bytes> (k-th device
 * allocation of the process), <name>+<bytes> (a host array of the case) or ? (any other host memory: a table's host
 * copy).  An event is e<s>.<k>, the k-th record on stream s, whenever it was created.  Creation and destruction of
 * streams and events, allocation and release are not traced but counted: an execution must destroy the events it
 * creates, and nothing may be left after fftw_destroy_plan.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fftw3.h>
#include <fftw3_amd.h>
#include "fa_plan.h"
#include "fa_hip.h"

#define N20 (1 << 20)
#define MAXALLOC 256
#define MAXEV 4096
#define MAXSTREAM 32
#define MAXHOST 16

typedef struct { char *base; size_t bytes; int live; } dev_alloc;
typedef struct { int live, stream, k; } event;
typedef struct { int live, records; } stream;
typedef struct { const char *name; char *base; size_t bytes; } host_range;

static dev_alloc g_alloc[MAXALLOC];
static event g_ev[MAXEV];
static stream g_st[MAXSTREAM + 1] = { { 1, 0 } };      /* g_st[0]: the caller's stream (NULL) */
static host_range g_host[MAXHOST];
static int g_nalloc, g_nev, g_nst = 1, g_nhost, g_live_ev, g_fails;
static fftw_plan g_plan;            /* the plan whose steps name the launches */
static int g_refuse_pair;           /* the next pair launch is refused */

static void fail(const char *what) { fprintf(stderr, "exec_trace: %s\n", what); ++g_fails; }

/* page-aligned and never touched: planning looks at the alignment of the arrays */
static char *untouched(size_t nbytes) {
    void *p = NULL;
    if (posix_memalign(&p, 4096, nbytes)) { fail("out of memory"); exit(2); }
    return (char *)p;
}

/* ------------------------------------------------------------ names */

static const char *ptr_name(const void *p, char *buf) {
    const char *c = (const char *)p;
    int i;
    for (i = 0; i < g_nalloc; ++i)
        if (g_alloc[i].live && c >= g_alloc[i].base && c < g_alloc[i].base + g_alloc[i].bytes) {
            sprintf(buf, "d%d+%lld", i, (long long)(c - g_alloc[i].base));
            return buf;
        }
    for (i = 0; i < g_nhost; ++i)
        if (c >= g_host[i].base && c < g_host[i].base + g_host[i].bytes) {
            sprintf(buf, "%s+%lld", g_host[i].name, (long long)(c - g_host[i].base));
            return buf;
        }
    return "?";
}

static int stream_id(void *s) {
    int id = s ? (int)((stream *)s - g_st) : 0;
    if (id < 0 || id >= g_nst || !g_st[id].live) { fail("call on a stream that does not exist"); return 0; }
    return id;
}

static const char *event_name(void *e, char *buf) {
    event *ev = (event *)e;
    if (!ev || ev < g_ev || ev >= g_ev + g_nev || !ev->live) { fail("call on an event that does not exist"); return "e?"; }
    if (ev->k == 0) { fail("an event is used before it was recorded"); return "e?"; }
    sprintf(buf, "e%d.%d", ev->stream, ev->k);
    return buf;
}

/* index of the step in the plan (or in its unaligned twin) that desc is a patched copy of, and its buffer count */
static int step_of(const fftw_amd_step_desc *d, int *nbufs) {
    fftw_plan q;
    int i;
    for (q = g_plan; q; q = q->alt)
        for (i = 0; i < q->nsteps; ++i) {
            const fftw_amd_step_desc *s = &q->steps[i];
            if (s->kind == d->kind && s->variant == d->variant && s->src_buf == d->src_buf && s->dst_buf == d->dst_buf &&
                s->src_base == d->src_base && s->dst_base == d->dst_base && s->L == d->L && s->flags == d->flags &&
                s->tw_n == d->tw_n && s->table == d->table) {
                *nbufs = q->nbufs;
                return i;
            }
        }
    *nbufs = 2;
    return -1;
}

static void print_bufs(double *const *bufs, int nbufs) {
    char b[64];
    int i;
    for (i = 0; i < nbufs; ++i) printf(" b%d=%s", i, ptr_name(bufs[i], b));
}

/* ------------------------------------------------------------ the fake */

int fa_hip_device_count(void) { return 1; }
int fa_hip_get_device(void) { return 0; }
void fa_hip_set_device(int dev) { (void)dev; }

void *fa_hip_malloc(size_t nbytes) {
    dev_alloc *a = &g_alloc[g_nalloc];
    if (g_nalloc == MAXALLOC) { fail("too many allocations"); exit(2); }
    if (nbytes == 0) nbytes = 16;
    a->bytes = nbytes;
    a->base = untouched(nbytes);
    a->live = 1;
    ++g_nalloc;
    return a->base;
}

void fa_hip_free(void *p) {
    int i;
    if (!p) return;
    for (i = 0; i < g_nalloc; ++i)
        if (g_alloc[i].live && g_alloc[i].base == (char *)p) { g_alloc[i].live = 0; free(p); return; }
    fail("release of something that is not a live allocation");
}

int fa_hip_is_device_ptr(const void *p) {
    char b[64];
    return p && ptr_name(p, b)[0] == 'd';
}
int fa_hip_ptr_device(const void *p) { return fa_hip_is_device_ptr(p) ? 0 : -1; }

void fa_hip_memcpy_h2d(void *dst, const void *src, size_t nbytes, void *s) {
    char a[64], b[64];
    if (!fa_hip_is_device_ptr(dst) || !fa_hip_is_device_ptr((char *)dst + nbytes - 1)) fail("h2d outside an allocation");
    printf("h2d s%d %s <- %s bytes=%zu\n", stream_id(s), ptr_name(dst, a), ptr_name(src, b), nbytes);
}
void fa_hip_memcpy_d2h(void *dst, const void *src, size_t nbytes, void *s) {
    char a[64], b[64];
    if (!fa_hip_is_device_ptr(src) || !fa_hip_is_device_ptr((const char *)src + nbytes - 1)) fail("d2h outside an allocation");
    printf("d2h s%d %s <- %s bytes=%zu\n", stream_id(s), ptr_name(dst, a), ptr_name(src, b), nbytes);
}

void fa_hip_stream_sync(void *s) { printf("sync s%d\n", stream_id(s)); }

void *fa_hip_stream_create(void) {
    if (g_nst > MAXSTREAM) { fail("too many streams"); exit(2); }
    g_st[g_nst].live = 1;
    return &g_st[g_nst++];
}
void fa_hip_stream_destroy(void *s) { if (s) g_st[stream_id(s)].live = 0; else fail("the caller's stream is destroyed"); }

void *fa_hip_event_create(void) {
    if (g_nev == MAXEV) { fail("too many events"); exit(2); }
    g_ev[g_nev].live = 1;
    ++g_live_ev;
    return &g_ev[g_nev++];
}
void fa_hip_event_destroy(void *e) {
    event *ev = (event *)e;
    if (!ev || ev < g_ev || ev >= g_ev + g_nev || !ev->live) { fail("destruction of an event that does not exist"); return; }
    ev->live = 0;
    --g_live_ev;
}
void fa_hip_event_record(void *e, void *s) {
    event *ev = (event *)e;
    char b[32];
    int id = stream_id(s);
    if (!ev || ev < g_ev || ev >= g_ev + g_nev || !ev->live) { fail("record of an event that does not exist"); return; }
    ev->stream = id;
    ev->k = ++g_st[id].records;
    printf("record s%d %s\n", id, event_name(e, b));
}
void fa_hip_stream_wait_event(void *s, void *e) {
    char b[32];
    printf("wait s%d %s\n", stream_id(s), event_name(e, b));
}
float fa_hip_event_elapsed_ms(void *start, void *stop) {
    char a[32], b[32];
    printf("elapsed %s %s\n", event_name(start, a), event_name(stop, b));
    return 1.0f;
}

int fa_hip_launch_step(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables, long long cs, long long cn,
                       void *s) {
    int nbufs, i = step_of(d, &nbufs);
    (void)tables;
    printf("launch s%d step=%d kind=%d/%d cs=%lld cn=%lld", stream_id(s), i, d->kind, d->variant, cs, cn);
    print_bufs(bufs, nbufs);
    printf(" src_im=%lld dst_im=%lld\n", d->src_im, d->dst_im);
    return 0;
}

int fa_hip_launch_pair1024(const fftw_amd_step_desc *d2, double *const *bufs2, long long cs2, long long cn2,
                           const fftw_amd_step_desc *d1, double *const *bufs1, long long cs1, long long cn1,
                           void *const *tables, void *s) {
    int nbufs, i2 = step_of(d2, &nbufs), i1 = step_of(d1, &nbufs);
    (void)tables;
    if (g_refuse_pair) {
        g_refuse_pair = 0;
        printf("pair-refused s%d\n", stream_id(s));
        return 1;
    }
    printf("pair s%d step=%d cs=%lld cn=%lld", stream_id(s), i2, cs2, cn2);
    print_bufs(bufs2, 3);
    printf(" dst_im=%lld | step=%d cs=%lld cn=%lld", d2->dst_im, i1, cs1, cn1);
    print_bufs(bufs1, 3);
    printf(" src_im=%lld\n", d1->src_im);
    return 0;
}

/* ------------------------------------------------------------ what the cases are made of */

static double *host_array(const char *name, size_t doubles) {
    host_range *h = &g_host[g_nhost++];
    h->name = name;
    h->bytes = doubles * sizeof(double);
    h->base = untouched(h->bytes);
    return (double *)h->base;
}
static double *dev_array(size_t doubles) { return (double *)fftw_amd_malloc_device(doubles * sizeof(double)); }

static int g_exec, g_ev_before;
static void exec_begin(void) { printf("# execute %d\n", ++g_exec); g_ev_before = g_live_ev; }
static void exec_end(void) { if (g_live_ev != g_ev_before) fail("an execution left events behind"); }

static fftw_plan planned(fftw_plan p) {
    if (!p) { fail("no plan"); exit(2); }
    printf("# plan: %d steps, chunk %lld of %lld, paired %d, lanes %d\n", fftw_amd_plan_num_steps(p), fftw_amd_plan_chunk(p),
           fftw_amd_plan_batch(p), fftw_amd_plan_paired(p), fftw_amd_plan_lanes(p));
    return g_plan = p;
}
static fftw_plan c2c(int n, int b, double *in, double *out, int sign) {
    return planned(fftw_plan_many_dft(1, &n, b, (fftw_complex *)in, NULL, 1, n, (fftw_complex *)out, NULL, 1, n, sign, FFTW_ESTIMATE));
}
static void execute(fftw_plan p) { exec_begin(); fftw_execute(p); exec_end(); }
static void execute_dft(fftw_plan p, double *in, double *out) {
    exec_begin(); fftw_execute_dft(p, (fftw_complex *)in, (fftw_complex *)out); exec_end();
}
static void execute_profiled(fftw_plan p) {
    double ms[8];
    long long launches[8];
    int i, n;
    exec_begin();
    n = fftw_amd_execute_profiled(p, ms, launches, 8);
    exec_end();
    for (i = 0; i < n; ++i) printf("# profiled step %d: %lld launches, %g ms\n", i, launches[i], ms[i]);
}
static void destroy(fftw_plan p) { printf("# destroy\n"); g_plan = NULL; fftw_destroy_plan(p); }

/* c2c on device arrays: n, batch, chunk bytes, executions */
static void run_device(int n, int b, size_t chunk_bytes, int sign, int times) {
    double *in = dev_array(2 * (size_t)n * b), *out = dev_array(2 * (size_t)n * b);
    fftw_plan p;
    fftw_amd_set_chunk_bytes(chunk_bytes);
    p = c2c(n, b, in, out, sign);
    while (times-- > 0) execute(p);
    destroy(p);
    fftw_amd_free_device(in); fftw_amd_free_device(out);
}
/* the same on plain host arrays */
static void run_host(int n, int b, size_t chunk_bytes, int with_new_arrays) {
    double *in = host_array("in", 2 * (size_t)n * b), *out = host_array("out", 2 * (size_t)n * b);
    fftw_plan p;
    fftw_amd_set_chunk_bytes(chunk_bytes);
    p = c2c(n, b, in, out, FFTW_FORWARD);
    execute(p);
    if (with_new_arrays) execute_dft(p, host_array("in2", 2 * (size_t)n * b), host_array("out2", 2 * (size_t)n * b));
    destroy(p);
}

/* ------------------------------------------------------------ the cases */

static void serial_small(void) { run_device(4096, 4, 0, FFTW_FORWARD, 1); }
static void serial_chunks(void) { setenv("FFTW_AMD_LANES", "1", 1); run_device(65536, 11, 2 << 20, FFTW_FORWARD, 1); }
static void lanes2(void) { run_device(N20, 7, 32 << 20, FFTW_FORWARD, 2); }
static void lanes3(void) { setenv("FFTW_AMD_LANES", "3", 1); run_device(N20, 7, 32 << 20, FFTW_FORWARD, 2); }
static void lanes_inplace_new_array(void) {
    double *a = dev_array(2 * (size_t)N20 * 7), *b = dev_array(2 * (size_t)N20 * 7);
    fftw_plan p;
    fftw_amd_set_chunk_bytes(32 << 20);
    p = c2c(N20, 7, a, a, FFTW_FORWARD);
    execute(p);
    execute_dft(p, b, b);
    destroy(p);
    fftw_amd_free_device(a); fftw_amd_free_device(b);
}
static void profiled(int b) {
    double *in = dev_array(2 * (size_t)N20 * b), *out = dev_array(2 * (size_t)N20 * b);
    fftw_plan p;
    fftw_amd_set_chunk_bytes(32 << 20);
    p = c2c(N20, b, in, out, FFTW_FORWARD);
    execute_profiled(p);
    destroy(p);
    fftw_amd_free_device(in); fftw_amd_free_device(out);
}
static void lanes_profiled(void) { profiled(7); }
static void pair_forward(void) { setenv("FFTW_AMD_LANES", "1", 1); run_device(N20, 5, 32 << 20, FFTW_FORWARD, 1); }
static void pair_backward(void) { setenv("FFTW_AMD_LANES", "1", 1); run_device(N20, 5, 32 << 20, FFTW_BACKWARD, 1); }
static void pair_profiled(void) { setenv("FFTW_AMD_LANES", "1", 1); profiled(5); }
static void pair_refused(void) {
    setenv("FFTW_AMD_LANES", "1", 1);
    g_refuse_pair = 1;
    run_device(N20, 5, 32 << 20, FFTW_FORWARD, 2);
}
static void pair_off(void) {
    setenv("FFTW_AMD_LANES", "1", 1);
    setenv("FFTW_AMD_PAIR", "0", 1);
    run_device(N20, 5, 32 << 20, FFTW_FORWARD, 1);
}
static void pipeline(void) { setenv("FFTW_AMD_PIPELINE", "1", 1); run_device(N20, 9, 8 << 20, FFTW_FORWARD, 1); }

static void host_single_chunk(void) { run_host(4096, 4, 0, 0); }
static void host_inplace(void) {
    double *a = host_array("a", 2 * 4096 * 4);
    fftw_plan p = c2c(4096, 4, a, a, FFTW_FORWARD);
    execute(p);
    destroy(p);
}
static void host_strided_output(void) {
    int n = 4096;
    double *in = host_array("in", 2 * 4096 * 4), *out = host_array("out", 4 * 4096 * 4);
    fftw_plan p = planned(fftw_plan_many_dft(1, &n, 4, (fftw_complex *)in, NULL, 1, n, (fftw_complex *)out, NULL, 2, 2 * n,
                                             FFTW_FORWARD, FFTW_ESTIMATE));
    execute(p);
    destroy(p);
}
static void host_r2c(void) {
    int n = 4096;
    double *in = host_array("in", 4096 * 4), *out = host_array("out", 2 * 2049 * 4);
    fftw_plan p = planned(fftw_plan_many_dft_r2c(1, &n, 4, in, NULL, 1, n, (fftw_complex *)out, NULL, 1, n / 2 + 1, FFTW_ESTIMATE));
    execute(p);
    destroy(p);
}
/* split arrays: real and imaginary planes of 4 x 4096 doubles, 512 doubles of someone else's between them (the two
   planes are carved from one block so that their order in memory is the same in every run) */
#define PLANE (4 * 4096)
static fftw_plan split_plan(double *ri, double *ii, double *ro, double *io) {
    const fftw_iodim d = { 4096, 1, 1 }, h = { 4, 4096, 4096 };
    return planned(fftw_plan_guru_split_dft(1, &d, 1, &h, ri, ii, ro, io, FFTW_ESTIMATE));
}
static void host_two_planes(void) {
    double *in = host_array("in", 2 * PLANE + 512), *out = host_array("out", 2 * PLANE + 512);
    fftw_plan p = split_plan(in, in + PLANE + 512, out, out + PLANE + 512);
    execute(p);
    destroy(p);
}
static void host_new_array_other_distance(void) {
    double *in = host_array("in", 2 * PLANE + 512), *out = host_array("out", 2 * PLANE + 512);
    double *in2 = host_array("in2", 2 * PLANE + 512), *out2 = host_array("out2", 2 * PLANE + 512);
    fftw_plan p = split_plan(in, in + PLANE + 512, out, out + PLANE + 512);
    execute(p);
    /* imaginary planes below the real ones */
    exec_begin();
    fftw_execute_split_dft(p, in2 + PLANE + 512, in2, out2 + PLANE + 512, out2);
    exec_end();
    destroy(p);
}
static void device_new_array_other_distance(void) {
    double *in = dev_array(2 * PLANE + 512), *out = dev_array(2 * PLANE + 512);
    fftw_plan p = split_plan(in, in + PLANE, out, out + PLANE);
    execute(p);
    exec_begin();
    fftw_execute_split_dft(p, in + PLANE + 512, in, out, out + PLANE + 512);
    exec_end();
    destroy(p);
    fftw_amd_free_device(in); fftw_amd_free_device(out);
}

static void hpipe_lanes(void) { run_host(N20, 5, 32 << 20, 1); }
static void hpipe_serial(void) { setenv("FFTW_AMD_LANES", "1", 1); run_host(65536, 11, 2 << 20, 0); }
static void hpipe_pair(void) { setenv("FFTW_AMD_LANES", "1", 1); run_host(N20, 5, 32 << 20, 1); }
static void hpipe_pair_refused(void) { setenv("FFTW_AMD_LANES", "1", 1); g_refuse_pair = 1; run_host(N20, 5, 32 << 20, 1); }
static void hpipe_off(void) { setenv("FFTW_AMD_HOST_PIPELINE", "0", 1); run_host(N20, 5, 32 << 20, 0); }
static void hpipe_under_pipeline(void) { setenv("FFTW_AMD_PIPELINE", "1", 1); run_host(N20, 4, 8 << 20, 0); }

static void unaligned_twin(void) {
    double *in = dev_array(2 * 4096 * 4 + 2), *out = dev_array(2 * 4096 * 4 + 2);
    fftw_plan p = c2c(4096, 4, in, out, FFTW_FORWARD);
    execute(p);
    execute_dft(p, in + 1, out + 1);        /* 8 bytes off: the FFTW_UNALIGNED twin runs */
    execute_dft(p, in + 1, out + 1);
    destroy(p);
    fftw_amd_free_device(in); fftw_amd_free_device(out);
}
static void howmany_zero(void) {
    double *in = dev_array(2 * 4096), *out = dev_array(2 * 4096);
    fftw_plan p = c2c(4096, 0, in, out, FFTW_FORWARD);
    execute(p);
    destroy(p);
    fftw_amd_free_device(in); fftw_amd_free_device(out);
}

static const struct { const char *name; void (*run)(void); } cases[] = {
    { "serial_small", serial_small }, { "serial_chunks", serial_chunks },
    { "lanes2", lanes2 }, { "lanes3", lanes3 }, { "lanes_inplace_new_array", lanes_inplace_new_array },
    { "lanes_profiled", lanes_profiled },
    { "pair_forward", pair_forward }, { "pair_backward", pair_backward }, { "pair_profiled", pair_profiled },
    { "pair_refused", pair_refused }, { "pair_off", pair_off },
    { "pipeline", pipeline },
    { "host_single_chunk", host_single_chunk }, { "host_two_planes", host_two_planes }, { "host_inplace", host_inplace },
    { "host_strided_output", host_strided_output }, { "host_r2c", host_r2c },
    { "host_new_array_other_distance", host_new_array_other_distance },
    { "device_new_array_other_distance", device_new_array_other_distance },
    { "hpipe_lanes", hpipe_lanes }, { "hpipe_serial", hpipe_serial }, { "hpipe_pair", hpipe_pair },
    { "hpipe_pair_refused", hpipe_pair_refused }, { "hpipe_off", hpipe_off }, { "hpipe_under_pipeline", hpipe_under_pipeline },
    { "unaligned_twin", unaligned_twin }, { "howmany_zero", howmany_zero },
};
#define NCASES ((int)(sizeof(cases) / sizeof(cases[0])))

int main(int argc, char **argv) {
    int i;
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (i = 0; i < NCASES; ++i) printf("%s\n", cases[i].name);
        return 0;
    }
    for (i = 0; argc == 2 && i < NCASES; ++i)
        if (!strcmp(argv[1], cases[i].name)) {
            /* the knobs a case does not set are at their defaults, whatever the caller's environment holds */
            unsetenv("FFTW_AMD_LANES"); unsetenv("FFTW_AMD_PAIR"); unsetenv("FFTW_AMD_PIPELINE");
            unsetenv("FFTW_AMD_HOST_PIPELINE"); unsetenv("FFTW_AMD_CHUNK_BYTES");
            cases[i].run();
            for (i = 0; i < g_nalloc; ++i) if (g_alloc[i].live) { fail("a device allocation outlives its plan"); break; }
            for (i = 1; i < g_nst; ++i) if (g_st[i].live) { fail("a stream outlives its plan"); break; }
            if (g_live_ev) fail("an event outlives its plan");
            for (i = 0; i < g_nhost; ++i) free(g_host[i].base);
            fflush(stdout);
            return g_fails != 0;
        }
    fprintf(stderr, "usage: exec_trace <case> | --list\n");
    return 2;
}
