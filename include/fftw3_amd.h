/*
 * fftw3_amd.h -- MI355X-specific additions behind the FFTW3 C ABI.
 *
 * Nothing here exists in the reference ("GPU-specific
 * additions behind the same ABI"); the names live under the fftw_amd_ prefix so
 * the stock fftw_ namespace stays clean.  All signatures are plain C: pointers,
 * sizes and an opaque stream handle (a hipStream_t passed as void*).
 */
#ifndef FFTW3_AMD_EXT_H
#define FFTW3_AMD_EXT_H

#include <stddef.h>
#include "fftw3.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of HIP devices visible to the process; 0 when there is none (the
   planners still work, fftw_execute* aborts loudly: there is no CPU fallback). */
int fftw_amd_device_count(void);

/* Device memory (hipMalloc / hipFree).  fftw_execute* accepts these pointers
   and runs on them in place of staging through PCIe.  fftw_malloc() itself
   returns pinned host memory so CPU callers keep working (staged path). */
void *fftw_amd_malloc_device(size_t nbytes);
void  fftw_amd_free_device(void *p);
/* Current device of the calling host thread (hipSetDevice / hipGetDevice) for callers without HIP headers:
   fftw_amd_malloc_device allocates on it.  fftw_amd_set_device returns -1 for a device that does not exist. */
int   fftw_amd_set_device(int device);
int   fftw_amd_get_device(void);
/* Blocking host <-> device copies (hipMemcpy), so that a C caller of the device path needs no
   HIP headers of its own. */
void  fftw_amd_memcpy_to_device(void *dst_device, const void *src_host, size_t nbytes);
void  fftw_amd_memcpy_to_host(void *dst_host, const void *src_device, size_t nbytes);

/* Bind the HIP stream (hipStream_t as void*) that fftw_execute* launches on.
   NULL restores the default stream.  Per plan. */
void fftw_amd_plan_set_stream(fftw_plan p, void *hip_stream);

/* Block until everything launched by fftw_execute*(p) has finished. */
void fftw_amd_plan_sync(fftw_plan p);

/* Bytes of device scratch the plan owns (twiddle tables + work buffers). */
size_t fftw_amd_plan_workspace_bytes(const fftw_plan p);
/* Device that holds them: a plan belongs to the device that was current (fftw_amd_set_device / hipSetDevice)
   when its planner function ran.  -1: none yet / no device; -2: allocations on more than one device (a bug). */
int fftw_amd_plan_workspace_device(const fftw_plan p);

/* Upper bound, in bytes, for the scratch that one chunk of a multi-pass plan may occupy (default
   256 MiB).  Measured on MI355X: with the caller's input and output streamed with nontemporal
   accesses, a 256 MiB scratch image written by one pass is still in the Infinity Cache when the next
   pass reads it (N = 2^20: 12.7 -> 11.4 us per transform); larger chunks lose that, smaller ones pay
   more launches (profiles/r02_chunk_nt_sweep.txt).  FFTW_MEASURE searches
   128 MiB ... 4 GiB.  0 restores the default.  Affects plans created afterwards. */
void fftw_amd_set_chunk_bytes(size_t nbytes);

/* ---- batch sharding over the GPUs of one node ----------------------
   The reference splits the vector loop of a batched plan across its workers inside the library
   (fftw/threads/dft-vrank-geq1.c:140-175, block size ceil(vl / nthr) :158-159; the same block
   rule as fftw/mpi/block.c:35-42).  Here the workers are GPUs: shard g of ndev owns the
   transforms [g*ceil(B/ndev), min(B, (g+1)*ceil(B/ndev))) of the batch, with one plan replica
   (tables + scratch), one stream and one host thread per device, and nothing exchanged inside a
   transform.  in[g] / out[g] are device pointers on device devs[g] (devs == NULL: 0..ndev-1)
   that hold shard g -- its first transform at offset 0 -- laid out exactly as
   fftw_plan_many_dft describes one batch (embed, stride, dist).  A device may appear more than
   once in devs (its shards then run on separate streams of that device). */
typedef struct fftw_amd_sharded_plan_s *fftw_amd_sharded_plan;

void fftw_amd_shard_range(long long howmany, int nshards, int g, long long *lo, long long *hi);

fftw_amd_sharded_plan fftw_amd_plan_many_dft_sharded(
    int rank, const int *n, int howmany, int ndev, const int *devs,
    fftw_complex *const *in, const int *inembed, int istride, int idist,
    fftw_complex *const *out, const int *onembed, int ostride, int odist, int sign, unsigned flags);
fftw_amd_sharded_plan fftw_amd_plan_many_dft_r2c_sharded(
    int rank, const int *n, int howmany, int ndev, const int *devs,
    double *const *in, const int *inembed, int istride, int idist,
    fftw_complex *const *out, const int *onembed, int ostride, int odist, unsigned flags);
fftw_amd_sharded_plan fftw_amd_plan_many_dft_c2r_sharded(
    int rank, const int *n, int howmany, int ndev, const int *devs,
    fftw_complex *const *in, const int *inembed, int istride, int idist,
    double *const *out, const int *onembed, int ostride, int odist, unsigned flags);

/* Enqueue every shard's transforms (asynchronous, like fftw_execute on device pointers);
   fftw_amd_sharded_sync blocks until all devices are done. */
void fftw_amd_execute_sharded(const fftw_amd_sharded_plan p);
void fftw_amd_sharded_sync(const fftw_amd_sharded_plan p);

/* All-gather of the output shards over xGMI: full[d] is a buffer on shard d's device for the
   WHOLE batch (howmany * odist elements); every shard's output lands at its place in each of
   them, ordered after the transforms (complete after fftw_amd_sharded_sync).  mode 0: RCCL
   (librccl.so, loaded once per process; ncclAllGather when the shards are equal, one ncclBroadcast per
   shard in a group when the block rule leaves a ragged tail; issued on the shards' own streams behind
   their transforms, no host-side drain) when every shard has its own device, direct peer-to-peer pushes
   otherwise; 1: force peer-to-peer; 2: RCCL or fail.  Returns 1 if RCCL moved the data, 0 for
   peer-to-peer, -1 on error.  This is the xGMI-bound part (for cfg5 each GPU
   receives 120 GB at <= 7 x 153 GB/s) and is never part of a transform's timing. */
int fftw_amd_sharded_all_gather(const fftw_amd_sharded_plan p, void *const *full, int mode);
/* The RCCL calls fftw_amd_sharded_all_gather issues (inside one group), without issuing them: 6 values per
   call -- kind (0 ncclAllGather, 1 ncclBroadcast), rank d, root (-1 for all-gather), send pointer, receive
   pointer, bytes.  Equal shards: one ncclAllGather per rank; ragged block-rule tails: one ncclBroadcast per
   non-empty shard and rank.  Returns the number of calls (ops holds at most cap of them), -1 on bad arguments. */
int fftw_amd_sharded_gather_ops(const fftw_amd_sharded_plan p, void *const *full, long long *ops, int cap);
/* Number of RCCL entry points the loader resolves (7 when librccl.so can serve the gather, else 0); opens the
   library once per process, makes no RCCL call.  FFTW_AMD_RCCL_LIB names a stand-in library. */
int fftw_amd_rccl_probe(void);

int  fftw_amd_sharded_num_shards(const fftw_amd_sharded_plan p);
int  fftw_amd_sharded_device(const fftw_amd_sharded_plan p, int g);
void fftw_amd_sharded_range(const fftw_amd_sharded_plan p, int g, long long *lo, long long *hi);
fftw_plan fftw_amd_sharded_replica(const fftw_amd_sharded_plan p, int g);   /* NULL for an empty shard */
void fftw_amd_destroy_sharded_plan(fftw_amd_sharded_plan p);

/* ---- one transform spread over the GPUs of a node in slabs ----------------------
   The c2c part of the reference's distributed-memory API (fftw/mpi/fftw3-mpi.h:74-215: fftw_mpi_local_size_2d / _3d,
   fftw_mpi_plan_dft_2d / _3d, fftw_mpi_execute_dft) with the MPI communicator replaced by a list of devices of this
   process: device g of ndev owns the rows [local_0_start, local_0_start + local_n0) of the first dimension (block
   rule of fftw/mpi/block.c:39-50), normal order in and out.  Pipeline: local transforms over the trailing
   dimension(s), exchange of column blocks (peer-to-peer 2-D copies over xGMI on the receiver's stream), local
   transforms of length n0 down the column blocks, exchange back (fftw3_amd/csrc/slab.c).  The multi-process form of
   the same layer -- r2c / c2r / r2r, TRANSPOSED_IN / OUT, torch.distributed in the place of MPI -- is
   fftw3_amd/slab.py. */
typedef struct fftw_amd_slab_plan_s *fftw_amd_slab_plan;
/* rows of device g (rank = 2 or 3, n = the logical size); returns the number of complex elements of its arrays */
long long fftw_amd_slab_local_size(int rank, const long long *n, int ndev, int g, long long *local_n0, long long *local_0_start);
/* in[g] / out[g]: device arrays on devs[g] (devs == NULL: 0..ndev-1) with local_n0(g) x n[1] (x n[2]) complex values;
   in[g] == out[g] is allowed.  NULL on invalid arguments or when a local plan / buffer cannot be made. */
fftw_amd_slab_plan fftw_amd_slab_plan_dft(int rank, const long long *n, int ndev, const int *devs,
                                          fftw_complex *const *in, fftw_complex *const *out, int sign, unsigned flags);
void fftw_amd_slab_execute(fftw_amd_slab_plan p);      /* enqueues on every device and returns */
void fftw_amd_slab_sync(fftw_amd_slab_plan p);
int  fftw_amd_slab_num_devices(const fftw_amd_slab_plan p);
fftw_plan fftw_amd_slab_local_plan(const fftw_amd_slab_plan p, int g, int which);   /* 0: rows plan, 1: column-block plan */
void fftw_amd_destroy_slab_plan(fftw_amd_slab_plan p);

/* ---- real data and the TRANSPOSED layouts of the slab plans (fftw3_amd/csrc/slab.c) ------------------------------
   fftw_mpi_local_size_2d / _3d_transposed, fftw_mpi_plan_dft_r2c_2d / _3d, fftw_mpi_plan_dft_c2r_2d / _3d and
   FFTW_MPI_TRANSPOSED_IN / _OUT of fftw/mpi/fftw3-mpi.h, devices of this process in the place of MPI ranks.  The
   results are ordinary fftw_amd_slab_plans (execute / sync / num_devices / local_plan / destroy as above).

   Sizes.  n is the LOGICAL size.  For real data nc = n[rank-1] / 2 + 1 and the complex array has the dimensions
   n[0] x nc (rank 2) or n[0] x n[1] x nc (rank 3); the real array has the same rows with 2 nc doubles each (FFTW's
   padded layout: the last 2 nc - n[rank-1] doubles of a row are padding).  Write n0 for n[0], n1' for the second
   complex dimension (n[1]; nc for rank-2 real data) and rest for the product of the complex dimensions after the
   second (1 for rank 2; n[2], or nc for real data, for rank 3).  Blocks by the block rule on n0 and on n1'.

   Layouts of device g:
   - normal:      [local_n0(g)][n1'][rest] complex; real: [local_n0(g)][n1] (x [n2]) with the padded last dimension.
   - transposed:  [local_n1(g)][n0][rest] complex, local_n1 / local_1_start the block of n1'.  Element (c, j, i) is
                  X[j][local_1_start + c][i].
   fftw_amd_slab_local_size_transposed takes the COMPLEX dimensions (the caller passes nc as the last one for real
   data, exactly as with fftw3-mpi) and returns max(local_n0 n1' rest, local_n1 n0 rest), the number of complex
   elements device g must allocate for either array of a plan with a TRANSPOSED bit (a real array: twice as many
   doubles).

   Plans.  fftw_amd_slab_plan_dft accepts the two bits in `flags`: TRANSPOSED_OUT leaves the result in the transposed
   layout, TRANSPOSED_IN expects the input in it; without them it plans and runs as before.  r2c (forward) accepts
   TRANSPOSED_OUT only, c2r (backward, unnormalised) TRANSPOSED_IN only, and c2r may overwrite its complex input.
   (void *)in[g] == (void *)out[g] is allowed everywhere.  Forward TRANSPOSED_OUT followed by backward TRANSPOSED_IN
   returns N x with two exchanges instead of four.

   Pipelines.  Normal order, real: the local r2c over the trailing dimension(s) first (c2r: last), the exchange /
   columns / exchange-back of the c2c plan on the complex shape in between.  TRANSPOSED_OUT: trailing-dimension plan
   in[g] -> W[g] (owned), ONE transposing exchange (device r pulls the block [local_n0(g)][local_n1(r)][rest] of
   every W[g] into out[r][c][local_0_start(g) + j][:], kernels_slab.hip), length-n0 plan in place in out[r] -- for
   rank 2 over contiguous rows.  TRANSPOSED_IN: the mirror image (length-n0 plan in[g] -> W[g], transposing exchange
   into out[g], trailing plan in place).  Both bits: length-n0 plan, exchange, trailing plan, exchange.
   fftw_amd_slab_local_plan(p, g, 0) is the trailing-dimension plan, (p, g, 1) the length-n0 plan.

   NULL (never a failure inside execute): bad arguments or flag combinations, rank other than 2 / 3, an extent < 1,
   a NULL array of a non-empty block, a named device that does not exist, distinct devices without peer access, a
   local plan / buffer that cannot be made.  Planning works without a device. */
#define FFTW_AMD_SLAB_TRANSPOSED_IN  (1U << 29)   /* same bits as FFTW_MPI_TRANSPOSED_IN / _OUT */
#define FFTW_AMD_SLAB_TRANSPOSED_OUT (1U << 30)
long long fftw_amd_slab_local_size_transposed(int rank, const long long *n, int ndev, int g,
                                              long long *local_n0, long long *local_0_start,
                                              long long *local_n1, long long *local_1_start);
fftw_amd_slab_plan fftw_amd_slab_plan_dft_r2c(int rank, const long long *n, int ndev, const int *devs,
                                              double *const *in, fftw_complex *const *out, unsigned flags);
fftw_amd_slab_plan fftw_amd_slab_plan_dft_c2r(int rank, const long long *n, int ndev, const int *devs,
                                              fftw_complex *const *in, double *const *out, unsigned flags);
/* The block moves of exchange `which` (0, 1: in execution order) exactly as the executor iterates them, 13 values
   each: source buffer (0 in, 1 out, 2 the plan's W), source device index, source element offset, destination
   buffer, destination device index, destination element offset, extents A, B, I, source strides of a and b,
   destination strides of a and b -- in complex elements:
       dst[doff + a dsa + b dsb + i] = src[soff + a ssa + b ssb + i],   a < A, b < B, i < I.
   Normal-order exchanges are 2-D copies (B = 1); transposing ones run as one kernel launch per destination device.
   Returns the number of moves (ops holds at most cap of them), -1 for a bad plan / exchange, 0 for a 1-D plan. */
#define FFTW_AMD_SLAB_OP_LEN 13
int fftw_amd_slab_exchange_ops(const fftw_amd_slab_plan p, int which, long long *ops, int cap);
/* fftw_amd_slab_execute between device events: waits for the plan's streams, records an event on every device's
   stream, executes, records again, synchronises; *ms = the longest event-to-event time of any device's stream.  For
   measurements (tools/perf); 0 on success, -1 for a bad or 1-D plan or without a device. */
int fftw_amd_slab_execute_timed(fftw_amd_slab_plan p, double *ms);
/* INTERNAL, for the tests and tools/perf only -- not part of the interface a caller should build on.  The
   transposing-exchange kernel by itself: nsrc blocks, 6 values each in desc (source device pointer, destination
   element offset, A, B, source strides of a and b), dst[off + b db + a da + i] = src[a sa + b sb + i]; enqueued on
   `stream` of the current device.  nt: 1 / 0 nontemporal accesses on / off, -1 the launcher's own rule (what the
   plans use).  0 when launched, 1 on arguments it cannot run, -1 without a device. */
int fftw_amd_slab_block_transpose(fftw_complex *dst, long long da, long long db, long long I, int nsrc,
                                  const long long *desc, int nt, void *stream);

/* ---- one long 1-D transform spread over the GPUs of a node (fftw3_amd/csrc/slab1d.c) -----------------------------
   The reference's distributed 1-D solver (fftw/mpi/dft-rank1.c; fftw_mpi_local_size_1d / fftw_mpi_plan_dft_1d of
   fftw/mpi/fftw3-mpi.h:97-138), devices of this process in the place of MPI ranks.  The result is an ordinary
   fftw_amd_slab_plan: fftw_amd_slab_execute / _sync / _num_devices and fftw_amd_destroy_slab_plan work on it;
   fftw_amd_slab_local_plan(p, g, 1) is device g's plan of the length-n0 columns, (p, g, 0) the one of the length-n1
   rows.  Local plans get `flags` without the two SCRAMBLED bits and are guru64 plans (local arrays > 2^31 work).

   Split.  n = n0 n1 with P | n0 and P | n1 (P = ndev); without such a split the planner returns NULL and
   local_size_1d -1 (with P = 1 every n has one).  Rule, deterministic in (n, P, sign): among the admissible splits
   whose ratio max(n0, n1) / min(n0, n1) is at most 4 times the smallest admissible ratio, take the one with the most
   lengths that have register kernels (the two- and three-stage register-resident kernels of the library), then the
   smallest ratio, then the larger n0.  BACKWARD uses the FORWARD split swapped
   (fftw_amd_slab_split_1d reports it), which is what makes the two scrambled layouts below fit together.

   Pipeline (w = n1 / P, h = n0 / P): exchange of column blocks of the input read as [n0][n1], w transforms of
   length n0 down every block, a twiddle w_n^(k0 j1) by global position (kernels_slab.hip), exchange of row blocks,
   h transforms of length n1 along the rows, and an exchange back into natural order.  Owned memory per device: two
   buffers of n / P elements (one with SCRAMBLED_OUT) and a twiddle table of about 2 sqrt(n) elements.

   Layouts (X = the transform of x):
   - normal: device g holds the elements [g n / P, (g + 1) n / P) of x in in[g] and of X in out[g], so
     local_ni = local_no = n / P.
   - SCRAMBLED_OUT: device g holds [k0 in block g of n0][k1 in 0 .. n1), row-major; element (k0, k1) is X[k0 + n0 k1].
   - SCRAMBLED_IN: in the plan's own split, device g holds [j1 in block g of n1][j0 in 0 .. n0), row-major; element
     (j1, j0) is x[n1 j0 + j1].  For a BACKWARD plan this is exactly what the FORWARD SCRAMBLED_OUT plan of the same
     n and P leaves, so FORWARD with SCRAMBLED_OUT followed by BACKWARD with SCRAMBLED_IN gives n x in normal order.
   local_size_1d reports the block [g n / P, (g + 1) n / P) of whichever order applies.

   NULL instead of a failure inside execute: ndev outside 1 ... 32, a named device that does not exist, a pair of
   distinct devices without peer access, a row pitch (n0 or n1 elements) over hipDeviceAttributeMaxPitch, or a local
   plan / buffer that cannot be made.  Planning works without a device (placeholder buffers: the plans can be
   inspected, not executed). */
#define FFTW_AMD_SLAB_SCRAMBLED_IN  (1U << 27)   /* same bits as FFTW_MPI_SCRAMBLED_IN / _OUT */
#define FFTW_AMD_SLAB_SCRAMBLED_OUT (1U << 28)
/* fftw_mpi_local_size_1d: elements device g's in / out arrays must hold; -1 when the plan would be NULL */
long long fftw_amd_slab_local_size_1d(long long n, int ndev, int g, int sign, unsigned flags,
                                      long long *local_ni, long long *local_i_start,
                                      long long *local_no, long long *local_o_start);
/* the split (n0, n1) the planner takes for (n, ndev, sign); 0 on success, -1 when there is none */
int fftw_amd_slab_split_1d(long long n, int ndev, int sign, long long *n0, long long *n1);
/* fftw_mpi_plan_dft_1d: in[g] / out[g] device arrays on devs[g] (devs == NULL: 0..ndev-1); in[g] == out[g] allowed */
fftw_amd_slab_plan fftw_amd_slab_plan_dft_1d(long long n, int ndev, const int *devs,
                                             fftw_complex *const *in, fftw_complex *const *out,
                                             int sign, unsigned flags);

/* ---- plan introspection used by the host-logic tests ------------------- */

#define FFTW_AMD_MAX_DIMS 8
#define FFTW_AMD_MAX_RADICES 16

/* One launch of the executor, as the planner built it.  Offsets and strides
   are counted in doubles (an interleaved complex array has stride 2, im = 1). */
typedef struct {
    int kind;            /* FFTW_AMD_STEP_* */
    int src_buf, dst_buf;/* 0 = plan input, 1 = plan output, 2.. = scratch */
    long long src_base, dst_base;
    long long src_im, dst_im;     /* distance from real to imaginary part */
    int flags;                    /* FFTW_AMD_F_* */
    int L;                        /* sub-transform length of a PASS */
    int nradices, radices[FFTW_AMD_MAX_RADICES];
    long long is_l, os_l;         /* stride of the transform index */
    int ndims;                    /* dims[0] is the tile dim, the rest loops */
    long long dim_n[FFTW_AMD_MAX_DIMS];
    long long dim_is[FFTW_AMD_MAX_DIMS];
    long long dim_os[FFTW_AMD_MAX_DIMS];
    long long dim_tw[FFTW_AMD_MAX_DIMS];
    long long tw_n;               /* 0: no inter-pass twiddle */
    int tw_shift, tw_lo, tw_hi;   /* two-level table: w^m = lo[m & mask] * hi[m >> shift] */
    int tile;                     /* tile width T along dims[0] */
    int batch_dim;                /* index into dims of the chunked batch loop, or -1 */
    long long aux_n;              /* kind-specific length (r2c: n, copy: K ...) */
    long long aux_valid;          /* copy: source elements beyond this read as 0 */
    int table, table2;            /* stage-twiddle / multiplier table, permutation table; -1: none */
    int aux_buf;                  /* Rader: buffer holding x[0] per vector */
    long long aux_base;
    int variant;                  /* which kernel the executor launches (FFTW_AMD_K_*) */
    /* optional inner component of the tile dim: the sequences of a tile are
       (lo, hi) pairs, lo in [0, tile_lo_n) fastest; dims[0] describes hi.
       Semantically just one more loop; it lets two interleaved vectors (radix-4
       real transforms) share 16-byte-contiguous global accesses. */
    int tile_lo_n;
    long long tile_lo_is, tile_lo_os;
    /* element-wise real-transform steps (untangle / tangle / r2r): the work items run over
       dims[0..kpos), then the pair / transform index, then the remaining dims -- the planner
       orders them by the user-side stride so that neighbouring items touch neighbouring
       memory whichever axis is transformed */
    int kpos;
} fftw_amd_step_desc;

enum {
    FFTW_AMD_STEP_PASS = 1,     /* batched length-L DFT + optional twiddle */
    FFTW_AMD_STEP_COPY = 2,     /* strided copy / pad / table multiply / permute */
    FFTW_AMD_STEP_R2C_POST = 3, /* untangle half-length complex DFT into r2c output */
    FFTW_AMD_STEP_C2R_PRE = 4,  /* inverse of the above */
    FFTW_AMD_STEP_RADER_MUL = 5,/* Rader pointwise product and DC fix-ups */
    FFTW_AMD_STEP_HERM_EXPAND = 6,/* half spectrum -> full Hermitian spectrum */
    FFTW_AMD_STEP_R2C_POST4 = 7,  /* radix-4 untangle: two quarter-length complex DFTs -> r2c output */
    FFTW_AMD_STEP_C2R_PRE4 = 8,   /* inverse of the above */
    FFTW_AMD_STEP_R2R = 9         /* r2r pre/post-processing around a real or complex DFT; variant = FFTW_AMD_R2R_* */
};

/* FFTW_AMD_STEP_R2R modes (step.variant).  aux_n = r2r length n, aux_valid =
   work items per transform, kpos = position of the transform index among the
   flattened loop indices, tw_* = two-level table of modulus 4n (01/10) or 8n (11).
   PRE_* map the user's real array into the inner transform's input, POST_* map
   the inner transform's output into the user's real array. */
enum {
    FFTW_AMD_R2R_PRE_HC2R = 1,   /* halfcomplex -> interleaved half spectrum */
    FFTW_AMD_R2R_PRE_E10, FFTW_AMD_R2R_PRE_O10,     /* even/odd index shuffle (sign flips for RODFT10) */
    FFTW_AMD_R2R_PRE_E01, FFTW_AMD_R2R_PRE_O01,     /* twiddled half spectrum for c2r */
    FFTW_AMD_R2R_PRE_E00, FFTW_AMD_R2R_PRE_O00,     /* even / odd symmetric extension */
    FFTW_AMD_R2R_PRE_E11, FFTW_AMD_R2R_PRE_O11,     /* n even: n/2 twiddled complex pairs */
    FFTW_AMD_R2R_PRE_E11ODD, FFTW_AMD_R2R_PRE_O11ODD, /* n odd: twiddle and zero-pad to 2n */
    FFTW_AMD_R2R_POST_R2HC, FFTW_AMD_R2R_POST_DHT,
    FFTW_AMD_R2R_POST_E10, FFTW_AMD_R2R_POST_O10,
    FFTW_AMD_R2R_POST_E01, FFTW_AMD_R2R_POST_O01,
    FFTW_AMD_R2R_POST_E00, FFTW_AMD_R2R_POST_O00,
    FFTW_AMD_R2R_POST_E11, FFTW_AMD_R2R_POST_O11,
    FFTW_AMD_R2R_POST_E11ODD, FFTW_AMD_R2R_POST_O11ODD
};

enum {
    FFTW_AMD_K_GENERIC = 0,     /* runtime-radix LDS kernel */
    FFTW_AMD_K_P1024 = 1,       /* register-resident radix-32x32 kernel, tile of 8 */
    FFTW_AMD_K_RR = 2,          /* register-resident two-stage kernel, L = 64..512, tile of 8192/L */
    FFTW_AMD_K_R3 = 3,          /* register-resident three-stage kernels (rows up to 8192 and of 16384 points; strided up to 2048) */
    FFTW_AMD_K_R2C = 4,         /* fused real rows -> half spectra (r2crows.hpp), with FFTW_AMD_F_R2C_ROWS */
    FFTW_AMD_K_C2R = 5,         /* fused half spectra -> real rows, with FFTW_AMD_F_C2R_ROWS */
    FFTW_AMD_K_R1 = 6,          /* one-stage register kernel: dense rows of 2 ... 32 points, one butterfly per row */
    FFTW_AMD_K_BLUE = 7,        /* Bluestein's algorithm for a whole row in one kernel (pass3b.hpp): L = padded length nb,
                                   aux_n = n, tw_lo / tw_hi = ids of the chirp and the kernel table */
    FFTW_AMD_K_TRANSPOSE = 8,   /* FFTW_AMD_STEP_COPY that is a batched transposition of n0 x n1 matrices of tuples, through
                                   LDS tiles (transpose.hpp): dims[0] = (n0, source leading dimension, vl), dims[1] =
                                   (n1, vl, destination leading dimension), dims[2 ...] the outer batch loops, the tuple of
                                   vl doubles as the copy's own index (aux_n elements at is_l = os_l).  Every field keeps
                                   the meaning it has for any other copy */
    FFTW_AMD_K_IMG2D = 9,       /* FFTW_AMD_STEP_PASS with FFTW_AMD_F_LO_DFT: whole small images in one trip (pass2d.hpp).  The
                                   step is the 2-D DFT tile_lo_n x L of dense row-major images: L = n1 columns (is_l = os_l = 2),
                                   tile_lo_n = n0 rows (tile_lo_is = tile_lo_os = 2 n1), dims[0] the loop over the images of the
                                   chunk (strides 2 n0 n1), tile = images per workgroup, no twiddle, no tables.  No fallback
                                   executor: planned only for aligned interleaved arrays */
    FFTW_AMD_K_IMG2DL = 10,     /* the same step (every field as for FFTW_AMD_K_IMG2D) for extents in {16, 32, 40, 48, 64} with at
                                   least one above 32 (pass2dl.hpp): an axis of 40, 48 or 64 points is two register stages, whose
                                   intra-axis twiddles are the stage tables `table` (row axis, L entries) and `table2` (column
                                   axis, tile_lo_n entries), -1 for an axis of one stage; tw_n = 0.  The plan owns these tables, so
                                   fftw_amd_plan_workspace_bytes is 16 bytes per entry of them; it owns no scratch buffer */
    FFTW_AMD_K_IMG2DR = 11,     /* FFTW_AMD_STEP_PASS with FFTW_AMD_F_REAL_IMG: whole small REAL images in one trip, r2c or c2r
                                   (pass2dr.hpp); see the flag for the fields.  No fallback executor */
    FFTW_AMD_K_VOL3D = 12,      /* FFTW_AMD_STEP_PASS with FFTW_AMD_F_LO_DFT and FFTW_AMD_F_VOL3D: whole small volumes in one trip
                                   (pass3d.hpp); see FFTW_AMD_F_VOL3D for the fields.  No fallback executor */
    FFTW_AMD_K_VOL3DR = 13,     /* FFTW_AMD_STEP_PASS with FFTW_AMD_F_REAL_VOL: whole small REAL volumes in one trip, r2c or c2r
                                   (pass3dr.hpp); see the flag for the fields.  No fallback executor */
    FFTW_AMD_K_IMG2DLR = 14,    /* FFTW_AMD_STEP_PASS with FFTW_AMD_F_REAL_IMG: whole REAL images with extents in {16, 32, 40, 48,
                                   64} and at least one above 32 in one trip, r2c or c2r (pass2dlr.hpp).  The same transform and
                                   every field as for FFTW_AMD_K_IMG2DR (see the flag), with two differences: `table` is the
                                   stage table of the row axis (L entries (cos, sin)(2 pi m / L); the untangle / tangle reads
                                   it) and is always present, `table2` is that of the column axis (tile_lo_n entries) and is
                                   present exactly when tile_lo_n > 32 (an axis of two register stages), -1 otherwise.  The
                                   plan owns these tables (16 bytes per entry) and no scratch buffer.  No fallback executor */
    FFTW_AMD_K_IMG2DW = 15      /* the FFTW_AMD_K_IMG2DL step (every field as for FFTW_AMD_K_IMG2D) for 128 x 128, 64 x 128 and
                                   128 x 64 images (pass2dw.hpp, 512 work-items per tile of 16384 elements): both axes are two
                                   register stages, so `table` (row axis, L entries) and `table2` (column axis, tile_lo_n
                                   entries) are both present.  In the planes plan of a rank-3 problem (the (n1, n2) planes in
                                   one trip, then the first axis in place on the output) the image step of any of the three
                                   families has dims[0] = the chunk's n0 planes per volume x volumes, and is no batch dim
                                   (batch_dim = -1): the plan has no scratch, so it runs in one chunk */
};

enum {
    FFTW_AMD_F_SWAP_IN   = 1 << 0, /* read (im,re) instead of (re,im) */
    FFTW_AMD_F_SWAP_OUT  = 1 << 1, /* write (im,re) */
    FFTW_AMD_F_REAL_IN   = 1 << 2, /* source has no imaginary part (reads as 0) */
    FFTW_AMD_F_REAL_OUT  = 1 << 3, /* store the real part only */
    FFTW_AMD_F_MUL_TABLE = 1 << 4, /* copy: multiply by table[k] */
    FFTW_AMD_F_MUL_CONJ  = 1 << 5, /* copy: multiply by conj(table[k]) */
    FFTW_AMD_F_PERM_SRC  = 1 << 6, /* copy: source index through permutation */
    FFTW_AMD_F_PERM_DST  = 1 << 7, /* copy: destination index through permutation */
    FFTW_AMD_F_CONJ_OUT  = 1 << 8, /* conjugate on store */
    FFTW_AMD_F_TW_IN     = 1 << 9, /* pass: the twiddle multiplies the INPUT element (l, q) instead of the output */
    FFTW_AMD_F_R2C_ROWS  = 1 << 10,/* pass over real pairs (src_im = 1) that also does the r2c untangle for n = 2L:
                                      stores L + 1 entries per row; tw_lo / tw_hi hold w_n^m (tw_n stays 0) */
    FFTW_AMD_F_C2R_ROWS  = 1 << 11,/* the transpose: reads L + 1 spectrum entries per row, c2r tangle, backward
                                      length-L pass, stores the real pairs (dst_im = 1) */
    FFTW_AMD_F_NT_IN     = 1 << 12,/* the source is read once per execution: nontemporal loads */
    FFTW_AMD_F_NT_OUT    = 1 << 13,/* the destination is not read again by this plan: nontemporal stores */
    FFTW_AMD_F_LO_DFT    = 1 << 14,/* pass: the inner tile component is transformed too -- a DFT of length tile_lo_n across the
                                      tile's tile_lo_n sequences (no twiddle), i.e. the step is the 2-D DFT tile_lo_n x L of every
                                      tile (pass3q.hpp: four rows of 4096 points, the last trip of a 4096 x 4096 transform) */
    FFTW_AMD_F_REAL_DEC  = 1 << 15,/* pass: the last trip of a two-trip r2c transform of n = L1 x L real points (pass3t_kernel,
                                      RD = 1).  The tile dim runs over the rows k1 = 0 ... L1 / 2 (dim_n[0] = L1 / 2 + 1) of the
                                      scratch image Z[k1][c] (rows at dim_is[0], pairs at is_l) left by the complex pass of
                                      length L1 over the real input read as pairs; row k1 is loaded as
                                      A[2c] = (Z[k1][c] + conj Z[L1-k1][c]) / 2, A[2c+1] = (Z[k1][c] - conj Z[L1-k1][c]) / 2i,
                                      multiplied by the input twiddle and transformed; output k2 < L / 2 goes to
                                      k1 dim_os[0] + k2 os_l, the others conjugated to (L1-k1) dim_os[0] + (L-1-k2) os_l
                                      (not for k1 = 0 and L1 / 2, whose second halves repeat their first; X[n / 2] comes from
                                      row 0).  No fallback executor: planned only for aligned interleaved arrays */
    FFTW_AMD_F_PAIR_SWAP = 1 << 16,/* transposition step (FFTW_AMD_K_TRANSPOSE) of a square matrix onto itself (source and
                                      destination are the same array, equal leading dimensions): workgroups exchange the tile
                                      pairs (ti, tj) / (tj, ti) in place, no scratch.  As for every copy, all reads happen
                                      before any write of the same word */
    FFTW_AMD_F_REAL_IMG  = 1 << 18,/* pass of variant FFTW_AMD_K_IMG2DR: the whole 2-D r2c (with FFTW_AMD_F_REAL_IN) or c2r (with
                                      FFTW_AMD_F_REAL_OUT) transform of real images of tile_lo_n = n0 rows x L = n1 real columns,
                                      n1 even, both at most 32 (variant FFTW_AMD_K_IMG2DLR: the same step for extents up to 64,
                                      with the stage tables described there).  dims[0] is the loop over the images of the chunk,
                                      tile = images per workgroup, tw_n = 0, table = table2 = -1, no swap flags.  The complex side is the
                                      dense half spectrum: n0 rows of n1 / 2 + 1 interleaved entries (im = 1, entries 2 apart,
                                      rows n1 + 2 doubles apart, images n0 (n1 + 2) apart); the real side has im = 0, elements 1
                                      apart, rows `pitch` = n1 or n1 + 2 doubles apart and images n0 pitch apart.
                                      r2c: src_im = 0, is_l = 1, tile_lo_is = pitch, dim_is[0] = n0 pitch; dst_im = 1, os_l = 2,
                                      tile_lo_os = n1 + 2, dim_os[0] = n0 (n1 + 2);
                                      Y[k0][k1] = sum x[j0][j1] w_n0^(j0 k0) w_n1^(j1 k1) for k1 = 0 ... n1 / 2.
                                      c2r: the same fields with the sides exchanged (src_im = 1, is_l = 2, tile_lo_is = n1 + 2,
                                      dst_im = 0, os_l = 1, tile_lo_os = pitch).  First the backward DFT of length n0 down each
                                      of the n1 / 2 + 1 columns, then the 1-D c2r of length n1 along each row, which reads the
                                      imaginary parts of its entries 0 and n1 / 2 as 0 (half spectra need not be Hermitian).
                                      With pitch = n1 + 2 an image occupies the same words on both sides and the step may run
                                      in place: every word of an image is read before any is written.  The padding words of
                                      padded real rows are never written.  Planned only for aligned arrays */
    FFTW_AMD_F_VOL3D     = 1 << 19,/* pass of variant FFTW_AMD_K_VOL3D (always with FFTW_AMD_F_LO_DFT): the step is the 3-D DFT
                                      aux_n x tile_lo_n x L of dense row-major interleaved volumes n0 x n1 x n2, every extent at
                                      most 32 and at most 8192 points: L = n2 (is_l = os_l = 2), tile_lo_n = n1 (rows
                                      tile_lo_is = tile_lo_os = 2 n2 doubles apart), aux_n = n0 (planes 2 n1 n2 doubles apart),
                                      Y[k0][k1][k2] = sum x[j0][j1][j2] w_n0^(j0 k0) w_n1^(j1 k1) w_n2^(j2 k2).
                                      dims[0] is the loop over the volumes of the chunk (strides 2 n0 n1 n2 on both sides),
                                      tile = volumes per workgroup, tw_n = 0, table = table2 = -1, src_im = dst_im = 1.
                                      Backward transforms carry FFTW_AMD_F_SWAP_IN and _SWAP_OUT, both or neither.  Every word
                                      of a volume is read before any is written, so the step may run in place.  No fallback
                                      executor: planned only for aligned interleaved arrays */
    FFTW_AMD_F_REAL_VOL  = 1 << 20,/* pass of variant FFTW_AMD_K_VOL3DR: the whole 3-D r2c (with FFTW_AMD_F_REAL_IN) or c2r (with
                                      FFTW_AMD_F_REAL_OUT) transform of real row-major volumes of aux_n = n0 planes x tile_lo_n =
                                      n1 rows x L = n2 real columns, n2 even, every extent at most 32.  dims[0] is the loop over
                                      the volumes of the chunk, tile = volumes per workgroup, tw_n = 0, table = table2 = -1, no
                                      swap flags, neither FFTW_AMD_F_LO_DFT nor FFTW_AMD_F_VOL3D.  The complex side is the dense
                                      half spectrum: n0 x n1 rows of n2 / 2 + 1 interleaved entries (im = 1, entries 2 apart,
                                      rows n2 + 2 doubles apart, planes n1 (n2 + 2) apart, volumes n0 n1 (n2 + 2) apart); the
                                      real side has im = 0, elements 1 apart, rows `pitch` = n2 or n2 + 2 doubles apart, planes
                                      n1 pitch apart and volumes n0 n1 pitch apart.
                                      r2c: src_im = 0, is_l = 1, tile_lo_is = pitch, dim_is[0] = n0 n1 pitch; dst_im = 1,
                                      os_l = 2, tile_lo_os = n2 + 2, dim_os[0] = n0 n1 (n2 + 2);
                                      Y[k0][k1][k2] = sum x[j0][j1][j2] w_n0^(j0 k0) w_n1^(j1 k1) w_n2^(j2 k2), k2 = 0 ... n2 / 2.
                                      c2r: the same fields with the sides exchanged (src_im = 1, is_l = 2, tile_lo_is = n2 + 2,
                                      dst_im = 0, os_l = 1, tile_lo_os = pitch).  First the backward DFTs of length n0 and n1
                                      over the two leading axes for each of the n2 / 2 + 1 columns, then the 1-D c2r of length
                                      n2 along each row, which reads the imaginary parts of its entries 0 and n2 / 2 as 0 (half
                                      spectra need not be Hermitian).
                                      With pitch = n2 + 2 a volume occupies the same words on both sides and the step may run
                                      in place: every word of a volume is read before any is written.  The padding words of
                                      padded real rows are never written.  Planned only for aligned arrays */
    FFTW_AMD_F_P1024_EIGHTHS = 1 << 21,/* pass of variant FFTW_AMD_K_P1024, set under FFTW_AMD_P1024_ORDER=0 only: every XCD walks
                                      its eighth of a launch's tile list from the start in the column launches too (tile order
                                      0 of fftw_amd_p1024_tile_order); without it XCD x starts x odd steps into its eighth
                                      (order 1).  Which workgroup computes which tile, nothing else */
    FFTW_AMD_F_REAL_DEC_C2R = 1 << 17 /* pass: the FIRST trip of a two-trip c2r transform of n = L1 x L real points (pass3t_kernel,
                                      RD = 2), the backward twin of FFTW_AMD_F_REAL_DEC.  The source is the half spectrum
                                      X[0 ... n / 2], entry k at k1 dim_is[0] + k2 is_l for k = k1 + L1 k2 (so is_l = L1 dim_is[0]).
                                      The tile dim runs over the rows k1 = 0 ... L1 / 2 (dim_n[0] = L1 / 2 + 1, dim_tw[0] = 1).
                                      Row k1 is loaded as Y[k2] = X[k1 + L1 k2] for k2 < L / 2 and
                                      Y[k2] = conj X[(L1 - k1) + L1 (L - 1 - k2)] for k2 >= L / 2, the imaginary parts of X[0] and
                                      X[n / 2] read as 0; it is transformed backward (the step carries FFTW_AMD_F_SWAP_IN and
                                      _SWAP_OUT like every backward pass) and multiplied by the twiddle on the OUTPUT index:
                                      A[k1][j2] = w_n^(+k1 j2) sum_k2 Y[k2] w_L^(+k2 j2).  The destination is the scratch image
                                      Z of L1 rows (at dim_os[0]) of L / 2 complex pairs (at os_l), plain row-major:
                                      Z[k1][c] = A[k1][2c] + i A[k1][2c+1] and, for 0 < k1 < L1 / 2,
                                      Z[L1-k1][c] = conj A[k1][2c] + i conj A[k1][2c+1]; the rows k1 = 0 and L1 / 2 are their own
                                      mirrors and store Z[k1][c] = Re A[k1][2c] + i Re A[k1][2c+1] only.  Every word of the rows
                                      0 ... L1 - 1 is written once, nothing else is, and the source is never written.  The
                                      backward complex pass of length L1 down the columns of Z then leaves the pairs
                                      (x[j1 L + 2c], x[j1 L + 2c + 1]).  No fallback executor: planned only for aligned
                                      interleaved arrays */
};

int fftw_amd_plan_num_steps(const fftw_plan p);
int fftw_amd_plan_get_step(const fftw_plan p, int i, fftw_amd_step_desc *out);
/* how many batch elements one chunk processes, and the total batch */
long long fftw_amd_plan_chunk(const fftw_plan p);
long long fftw_amd_plan_batch(const fftw_plan p);
/* 1 when the executor runs both passes of a two-pass plan in one launch per chunk (pass 2 of chunk
   c-1 followed by pass 1 of chunk c); fftw_amd_execute_profiled then reports every launch under step 0.
   Known once the plan has been set up on a device. */
int fftw_amd_plan_paired(const fftw_plan p);
/* Chunk lanes of a multi-pass plan (round 3): chunk c of the batch runs ALL its steps, in order, on stream
   c % lanes in scratch slot c % lanes; the lanes share the chip, so the tail of one lane's launch is filled by
   the other lane's next one and a chunk's scratch is re-read while it is still in the Infinity Cache
   (default 2 lanes x 128 MiB of scratch; FFTW_AMD_LANES=1 restores serial chunks, and with them the pair
   launches above).  The lanes fork from and join the plan's stream (fftw_amd_plan_set_stream) inside every
   fftw_execute*.  1 for single-chunk, one-step and oversized-chunk plans.  Known once the plan is set up. */
int fftw_amd_plan_lanes(const fftw_plan p);
/* Launches of the register-resident 1024-point pass since the library was loaded, by form: `full` counts the
   full-tile kernel (every tile of the launch holds 8 sequences, no re / im swap, no output twiddle), `general`
   everything else, pair launches included.  Either pointer may be NULL.
   DEBUG / INTROSPECTION ONLY: a hook for the test suite and profiling scripts, not part of the stable ABI; it may
   change or go away without notice. */
void fftw_amd_p1024_launches(long long *full, long long *general);
/* The same kind of hook: place[b], b < nblocks, receives the place in the tile list (tile = place % tiles of the tile
   dim, the loop dims from the quotient) that workgroup b of a launch of `nblocks` workgroups takes under tile order
   `order`, evaluated on the host by the function the kernels call; place may be NULL.  Returns the number of orders the
   library has (0 ... orders - 1), or 0 on arguments no launch has. */
int fftw_amd_p1024_tile_order(int order, long long nblocks, long long *place);
/* host copy of table `id` as interleaved doubles; returns its length in
   doubles (writes at most cap doubles). */
long long fftw_amd_plan_table(const fftw_plan p, int id, double *dst, long long cap);

/* Execute once on the plan's own arrays with a HIP event pair around every
   kernel launch, on the stream the kernels run on.  ms[i] receives the summed
   duration of step i over all chunks, launches[i] how often it was launched.
   Returns the number of steps, -1 if cap is too small. */
int fftw_amd_execute_profiled(fftw_plan p, double *ms, long long *launches, int cap);

/* Host-side numerics exported for the tests (no device needed). */
void fftw_amd_cexp(long long m, long long n, double out[2]);  /* (cos, sin)(2 pi m / n) */
long long fftw_amd_find_generator(long long p);
long long fftw_amd_power_mod(long long b, long long e, long long p);
int fftw_amd_factor_passes(long long n, int max_passes, long long *lens);

#ifdef __cplusplus
}
#endif
#endif
