/*
 * fa_plan.h -- internal types of the host planner (C).
 */
#ifndef FA_PLAN_H
#define FA_PLAN_H

#include <stddef.h>
#include <pthread.h>
#include "fftw3.h"
#include "fftw3_amd.h"

typedef long long i64;

#define FA_MAXRANK 8
#define FA_MAXLOOPS 7
#define FA_MAXBUF 16
#define FA_MAXTAB 256
#define FA_MAXPASS 4
#define FA_MAXLANES 4

/* primes up to this get an in-LDS O(p^2) stage; larger ones go to Rader or
   Bluestein (the reference switches from its O(n^2) "generic" solver to
   Rader/Bluestein in the same spirit: fftw/fftw_api.h:1108-1114) */
#define FA_PRIME_LDS_MAX 31

/* complex elements one workgroup tile holds (two LDS images of 16 B each) */
#define FA_TILE_ELEMS 4096
#define FA_LMAX_SINGLE 4096
/* complex elements per LDS image: 160 KiB / (2 images * 16 B) */
#define FA_LDS_ELEMS 5120

enum { FA_C2C = 0, FA_R2C = 1, FA_C2R = 2, FA_R2R = 3 };
#define FA_REAL_IN(t)  ((t) == FA_R2C || (t) == FA_R2R)
#define FA_REAL_OUT(t) ((t) == FA_C2R || (t) == FA_R2R)

enum {
    FA_TAB_STAGE = 1,   /* (cos,sin)(2 pi m / n), m in [0,n) */
    FA_TAB_TW_LO,       /* two-level twiddle, low digits */
    FA_TAB_TW_HI,       /* two-level twiddle, high digits */
    FA_TAB_CHIRP,       /* Bluestein w[k] = (cos,sin)(pi k^2 / n), zero padded to nb */
    FA_TAB_BLUE_SEQ,    /* Bluestein kernel sequence c[k] / nb (time domain) */
    FA_TAB_RADER_SEQ,   /* Rader kernel sequence b[j] / (p-1) (time domain) */
    FA_TAB_DFT_OF,      /* forward DFT of table `src`, computed on the device */
    FA_TAB_PERM         /* int64 index permutation */
};

typedef struct {
    int kind;
    i64 n;          /* defining size */
    i64 aux;        /* shift (TW_*), nb (CHIRP), 0/1 = forward/inverse power (PERM) */
    i64 len;        /* entries: complex pairs, or int64s for PERM */
    int src;        /* FA_TAB_DFT_OF: table id of the time-domain sequence */
    void *host;     /* host copy (NULL for DFT_OF until the device computed it) */
    void *dev;
} fa_table;

typedef struct { i64 n, is, os; } fa_dim;

/* what FFTW_MEASURE tunes and wisdom remembers */
typedef struct {
    size_t chunk_bytes;   /* scratch per chunk */
    int pipeline;         /* two-stream chunk pipeline on/off */
    int lmax_multi;       /* longest sub-transform of a multi-pass split */
    int small_tiles;      /* half-size tiles in the generic LDS kernel */
    int long_first;       /* multi-pass splits run the longest sub-transform first */
    int lanes;            /* chunk lanes: chunk c runs all its steps on stream c % lanes, scratch slot c % lanes */
    i64 tile_elems;       /* FFTW_AMD_TILE_ELEMS: tile size of the generic LDS kernel, 0 = default (not tuned) */
    /* the opt-in plan families: 0 under FFTW_ESTIMATE; what switches each on, and for which problems, is its row of
       fa_family_table below */
    int real_dec;         /* long r2c / c2r transforms decimated over the real data, two trips */
    int real_img;         /* batches of small 2-D r2c / c2r transforms in one trip */
    int vol3d;            /* batches of small 3-D c2c transforms in one trip */
    int real_vol;         /* batches of small 3-D r2c / c2r transforms in one trip; not implied by real_img */
    int real_imgl;        /* batches of 2-D r2c / c2r transforms with an extent above 32 in one trip; nor is this one */
    int vol_planes;       /* dense 3-D c2c volumes in two trips: the (n1, n2) planes, then the first axis */
    int img_wide;         /* batches of 2-D c2c transforms with an extent of 128 in one trip; not needed by vol_planes */
} fa_cfg;

/* One row per opt-in plan family, and the only place that says what switches it on: the environment variable
   (fa_default_cfg: the field is atoi(value) != 0 when the variable is present), the bit of a wisdom record's flag
   integer, and the problems for which the FFTW_MEASURE search times one candidate with that field alone set -- after
   its base candidates, in the order of the rows (api.c: fa_measure_candidates) -- and which plan it then accepts. */
enum { FA_ACCEPT_ANY = -1, FA_ACCEPT_PLANES = -2 };
typedef struct {
    const char *env;
    size_t off;         /* of the int field in fa_cfg */
    int bit;            /* of the wisdom record */
    unsigned types;     /* problem types the search tries it for: 1 << FA_C2C | ... */
    int rank;           /* the rank it tries it for, 0 = every rank */
    int accept;         /* the candidate is timed when its plan is: FA_ACCEPT_ANY any plan that builds, FA_ACCEPT_PLANES
                           the two steps of emit_vol_planes, otherwise exactly one step of this FFTW_AMD_K_* variant */
} fa_family;
#define FA_NFAMILIES 7
__attribute__((visibility("hidden"))) extern const fa_family fa_family_table[FA_NFAMILIES];
static inline int fa_family_on(const fa_cfg *c, const fa_family *f) { return *(const int *)((const char *)c + f->off); }
static inline void fa_family_set(fa_cfg *c, const fa_family *f, int on) { *(int *)((char *)c + f->off) = on; }

/* The planner's test switches, read from the environment by fa_read_knobs at the top of every fa_build (planner.c)
   and from nowhere else: one build -- its dry run and its sized runs -- sees one snapshot.  Not part of fa_cfg:
   wisdom does not store them and a MEASURE candidate, a clone or an FFTW_UNALIGNED twin reads its own when it is
   built.  Every int is 1 when the variable is PRESENT, whatever its value (FFTW_AMD_NO_TUNED=0 switches the tuned
   kernels off). */
#define FA_P1024_ORDER_DEFAULT 1
typedef struct {
    int no_tuned, no_3s, no_r1, no_blue_rows, no_narrow, no_split_costs, no_lo_dft, no_img2d, no_r2crows;
    int r2r_unfused, no_radix4, force_radix4;
    int p1024_order;            /* FFTW_AMD_P1024_ORDER: tile order of the 1024-point pass.  The one switch that carries a
                                   number: FA_P1024_ORDER_DEFAULT when absent or negative, 0 = every XCD walks its eighth of
                                   the tile list from the start (the steps then carry FFTW_AMD_F_P1024_EIGHTHS) */
    /* FFTW_AMD_FORCE_LENS="L1,L2,...": n_force_lens >= 2 entries, all >= 1, and their product; 0 entries when the
       variable is absent, has fewer than two entries or anything but numbers and commas in it.  Entries past
       FA_MAXPASS are not read. */
    i64 force_lens[FA_MAXPASS], force_prod;
    int n_force_lens;
} fa_knobs;

typedef struct {
    int buf;
    i64 base;
    i64 im;         /* real -> imaginary distance in doubles */
} fa_loc;

typedef struct {
    i64 n;
    i64 is, os;                 /* strides of the transform index, in doubles */
    fa_loc src, dst;
    int nloops;
    fa_dim loops[FA_MAXLOOPS];
    int batch_loop;             /* index of the chunked loop or -1 */
    int flags_in, flags_out;    /* FFTW_AMD_F_* that apply at the first / last step */
    int dense;                  /* the axis interleaved with a 2-element loop is contiguous memory */
} fa_axis;

/* loops seen as a batched transposition of n0 x n1 matrices of tuples of vl contiguous doubles:
       dst[c ldd + r vl + t] = src[r lds + c vl + t],   r < n0, c < n1, t < vl,
   inside the outer loops b[0 .. nb) */
typedef struct {
    i64 n0, n1, lds, ldd, vl;
    int nb;
    fa_dim b[FA_MAXLOOPS];
} fa_transp;

/* plan.tr_kind: how the problem uses the transposition kernels (api.c decides on the caller's own loops, extent-1
   ones included) */
enum {
    FA_TR_NONE = 0,
    FA_TR_COPY,         /* rank 0, two arrays: the whole plan is one tiled transposition */
    FA_TR_INPLACE,      /* rank 0, one array, square: the whole plan is one in-place step, no scratch */
    FA_TR_AFTER         /* in-place transform whose output strides are the transposed input strides (square): the
                           ordinary in-place plan on the input strides, then the in-place step */
};

/* plan.sched: how the chunks of the batch are enqueued (exec.c: choose_schedule picks one when the plan is set up on
   the device; a plan that is not set up yet is SERIAL) */
enum {
    FA_SCHED_SERIAL = 0,    /* chunk after chunk on the caller's stream, one scratch slot */
    FA_SCHED_PAIR,          /* 1024 x 1024 plan: pass 2 of chunk c-1 and pass 1 of chunk c in one launch (fa_hip_launch_pair1024),
                               two scratch slots; becomes SERIAL when the kernel refuses the plan's first launch */
    FA_SCHED_PIPE,          /* two-stream chunk pipeline: stage A (steps [0, split)) of chunk c+1 on pstream[0] overlaps stage B
                               (steps [split, nsteps)) of chunk c on pstream[1]; three scratch slots */
    FA_SCHED_LANES          /* chunk lanes (see fa_cfg.lanes): the streams are pstream[0 .. lanes) */
};

struct fftw_plan_s {
    int type;                   /* FA_C2C / FA_R2C / FA_C2R / FA_R2R */
    int kinds[FA_MAXRANK];      /* FA_R2R: fftw_r2r_kind of every dim */
    fa_cfg cfg;
    fa_knobs knobs;             /* snapshot of the test switches this plan's steps were built under */
    int sign;
    unsigned flags;
    int rank;
    fa_dim dims[FA_MAXRANK];    /* logical transform dims, strides in doubles */
    int hrank;
    fa_dim hdims[FA_MAXRANK];
    i64 in_im, out_im;          /* imaginary offsets of the user arrays */

    fftw_amd_step_desc *steps;
    int nsteps, cap_steps;

    fa_table tabs[FA_MAXTAB];
    int ntabs;

    int nbufs;                  /* ids 0,1 = user in/out */
    i64 buf_reals[FA_MAXBUF];   /* scratch sizes in doubles */
    int buf_busy[FA_MAXBUF];
    double *dbuf[FA_MAXBUF];

    i64 batch, chunk;

    double *ri, *ii, *ro, *io;  /* arrays the plan was created on */
    i64 in_lo, in_hi, out_lo, out_hi;   /* touched offset range of the real parts */
    i64 out_written;            /* number of doubles the plan writes in the output */
    int inplace;
    int single_chunk;           /* run the whole batch as one chunk */
    int via_scratch;            /* in-place c2c or rank-0 r2r problem whose input and output strides differ (same
                                   locations): the result is built in a dense scratch image and copied to the output layout */
    int tr_kind;                /* FA_TR_* */
    fa_transp tr;

    void *stream;
    int dev_ready;
    pthread_mutex_t lock;       /* fftw_execute is thread-safe in the reference; the plan's scratch is not shareable */

    int sched;                  /* FA_SCHED_* */
    int nslots, split;          /* scratch slots (chunk c works in slot c % nslots); FA_SCHED_PIPE: first step of stage B */
    int lanes;                  /* FA_SCHED_LANES: number of lanes, 1 otherwise */
    void *pstream[FA_MAXLANES];
    void *ev_a[4], *ev_b[4], *ev_begin, *ev_end[FA_MAXLANES];
    int failed;

    /* staging for plain host pointers; hstream[0] / [1]: copy streams of the chunked host pipeline */
    void *hstream[2];
    double *stage_in, *stage_out;
    size_t stage_in_bytes, stage_out_bytes;

    double est_flops;

    struct fftw_plan_s *alt;    /* FFTW_UNALIGNED twin, built on the first new-array execution that needs it */

    double *prof_ms;            /* fftw_amd_execute_profiled: per-step sinks, NULL otherwise */
    long long *prof_launches;
};

/* hostmath.c */
void fa_cexp(i64 m, i64 n, double out[2]);
i64  fa_mulmod(i64 x, i64 y, i64 p);
i64  fa_power_mod(i64 b, i64 e, i64 p);
int  fa_prime_factors(i64 n, i64 *primes, int *mult);
int  fa_is_prime(i64 n);
i64  fa_largest_prime_factor(i64 n);
i64  fa_find_generator(i64 p);
int  fa_lds_able(i64 n);
i64  fa_next_smooth(i64 n);
int  fa_radices(i64 L, int *rad);
int  fa_factor_passes(i64 n, int max_passes, i64 lmax_single, i64 lmax_multi, i64 *lens);
int  fa_factor_passes_pref(i64 n, int max_passes, i64 lmax_single, i64 lmax_multi, i64 *lens,
                           int (*tuned)(i64));

/* planner.c */
struct fftw_plan_s *fa_plan_new(void);
void fa_plan_free(struct fftw_plan_s *p);
int  fa_build(struct fftw_plan_s *p);     /* steps from p->type/dims/hdims; 0 on success */
char *fa_sprint(const struct fftw_plan_s *p);
fa_cfg fa_default_cfg(void);
/* 1 and *t when the loops l[0 .. nl) (strides in doubles, `unit` doubles per element) are a transposition the tile
   kernels take: positive strides, an optional inner tuple loop of unit stride on both sides, one loop of tuple stride
   on the output and another of tuple stride on the input (extent-1 loops count when their strides fit), the rest
   outer batch loops that step over a whole matrix on both sides */
int fa_match_transpose(const fa_dim *l, int nl, i64 unit, fa_transp *t);
/* 1 when *t is square with equal leading dimensions, every batch loop has the same stride on both sides and the
   matrices of the batch do not overlap: the in-place step applies */
int fa_transp_inplace_ok(const fa_transp *t);

/* split.c: cost models of the multi-pass splits, pure functions of the length */
int    fa_has_register_kernel(i64 L);
void   fa_pow2_three_pass_split(i64 n, i64 *lens);
double fa_mixed_three_pass_split(i64 n, i64 *lens);     /* modelled cost of the split, -1: none */
void   fa_mixed_two_pass_split(i64 n, i64 *lens);
double fa_split_cost_measured(i64 L, int pos);          /* 0: no sample */
double fa_wide_pass_cost(i64 L, int last);              /* 0: no such kernel */

/* exec.c */
int  fa_device_init(struct fftw_plan_s *p);      /* tables, schedule, scratch; 0 on success */
/* gives back everything fa_device_init and the executions created; fa_plan_free calls it.  Hidden: the library's
   dynamic symbols stay what they were */
__attribute__((visibility("hidden"))) void fa_exec_release(struct fftw_plan_s *p);
void fa_run(struct fftw_plan_s *p, double *ri, double *ii, double *ro, double *io);

/* api.c */
struct fftw_plan_s *fa_unaligned_twin(const struct fftw_plan_s *p);

/* slab1d.c: the distributed 1-D transform; slab.c wraps it in an fftw_amd_slab_plan and dispatches to it */
#define FA_SLAB_MAXDEV 32
struct fa_slab1d;
void fa_slab1d_execute(struct fa_slab1d *d);
void fa_slab1d_sync(struct fa_slab1d *d);
void fa_slab1d_destroy(struct fa_slab1d *d);
fftw_plan fa_slab1d_local_plan(const struct fa_slab1d *d, int g, int which);
struct fftw_amd_slab_plan_s *fa_slab_wrap1d(struct fa_slab1d *d, int ndev);   /* slab.c; NULL: out of memory */

#endif
