/*
 * pass3dr.hpp -- one-trip 3-D r2c and c2r transforms of small real volumes: T whole volumes of R0 x R1 x R2 reals
 * (row-major, R2 fastest and even, every extent at most 32) per workgroup, all three axes in registers.  The real
 * twins of pass3d.hpp, put together from its three-stage scheme and the real-data steps of pass2dr.hpp: the same
 * butterflies (RB<R>), padded planes, the same store in the order of the run; no twiddle appears anywhere, so there is
 * no table.  Below H = R2 / 2, M0 = R0 / 2 + 1 (integer division) and -k = ((R0 - k0) % R0, (R1 - k1) % R1).
 *
 * r2c (vol3dr_kernel).  The real volume is read as the packed complex volume z[j0][j1][c] = x[j0][j1][2c] + i x[j0][j1][2c+1],
 * R0 x R1 x H.
 *   stage 1   butterfly g = (volume t, j1, c): DFT of length R0 down axis 0, loaded from global memory (16-byte pairs
 *             at the real row pitch; instruction r reads plane j0 = r)
 *   exchange  layout X (below), real parts then imaginary parts
 *   stage 2   butterfly h = (t, k0, c): DFT of length R1 along axis 1; leaves Z[k0][k1][c], the 2-D DFT of the packed
 *             columns
 *   exchange  layout X again; the item of row (k0, k1) reads its row and the row -k and separates the two real columns
 *             of every packed column while it reads:
 *                 A_2c[k] = (Z[k][c] + conj Z[-k][c]) / 2,      A_2c+1[k] = (Z[k][c] - conj Z[-k][c]) / 2i.
 *             The plane of real parts gives y[2c].x and y[2c+1].y, the plane of imaginary parts y[2c].y and y[2c+1].x,
 *             so one plane at a time is enough.
 *   stage 3   butterfly q = (t, k0, k1) for k0 = 0 ... M0 - 1 and every k1: DFT of length R2 along the row.  Row (k0, k1)
 *             of the result is y[0 ... H]; for 0 < k0 and 2 k0 != R0, row -k is conj y[(R2 - k2) % R2], k2 = 0 ... H
 *             (the planes k0 = 0 and k0 = R0 / 2 hold both (k0, k1) and (k0, -k1) themselves)
 *   transposition through layout O into the order of the run of the half spectra, R0 x R1 x (H + 1) complex, stored as
 *   contiguous 1 KiB pieces per wave instruction.
 *
 * c2r (vol3dc_kernel).  The definition: backward DFTs of length R0 and R1 over the H + 1 columns, then the 1-D c2r of
 * length R2 along every row, which reads the imaginary parts of its entries 0 and H as 0 -- also for half spectra that
 * are not Hermitian.
 *   stage A   butterfly g = (t, k1, c), c = 0 ... H: backward DFT of length R0 down axis 0, loaded from global memory
 *   exchange  layout C
 *   stage B   butterfly h = (t, j0, c): backward DFT of length R1 along axis 1 (stages A and B share one swap at the
 *             load: the value after B is (.y, .x))
 *   exchange  layout C again; butterfly q = (t, pair of rows r = 2q, r' = 2q + 1 of the R0 R1 rows of a volume, in
 *             row-major order over (j0, j1)): W = Y_r + i Y_r', Y the Hermitian expansion of the H + 1 entries of a row
 *             with the two imaginary parts dropped, built while the two planes are read
 *   stage C   one backward DFT of length R2 leaves row r in one component and row r' in the other (an odd R0 R1 leaves
 *             the last row on its own: its partner reads as zeros and is not stored)
 *   transposition through layout R -- the values are real, so one trip -- into the order of the run of the real volumes,
 *   stored as 16-byte pairs (the padding words of padded rows are never written).
 *
 * Layout.  The complex row pitch is always R2 + 2 doubles (dense rows of H + 1 entries); the real row pitch is a kernel
 * argument, R2 (dense) or R2 + 2 (the padded in-place layout).  Planes and volumes are dense at those pitches.  A tile
 * is one contiguous run on both sides that no other workgroup touches, and every global load of a workgroup precedes
 * its first global store (the barriers of the exchanges lie in between), so the transforms work in place on padded rows.
 *
 * LDS.  Four layouts of the form of pass3d.hpp, element (t, a0, a1, a2) at (t R0 + a0) SP + a1 S + a2 doubles with a
 * row of W words: X (r2c exchanges, W = H), O (r2c output, W = H + 1), C (c2r exchanges, W = H + 1), R (c2r output,
 * W = R2).  S = W + ds and SP = R1 S + dp come per kernel from vol3dr_pad.inc, which tools/perf/vol3dr_codeobj.py
 * --search writes: the smallest paddings for which NO wave instruction of any access pattern of the kernel puts more
 * than two distinct words on one bank (32 banks of 64 bits), over every group of 32 consecutive items, ragged ones
 * included, counted by enumeration of the addresses.  No conflict counter of the hardware was read.  The patterns, each
 * one map from items to words because a register index only adds a constant:
 *   r2c  X: stores of stage 1 (items (t, j1, c)), loads and stores of stage 2 (items (t, k0, c)), loads of stage 3 from
 *           the own row and from the row -k (items (t, k0 < M0, k1));  O: stores of stage 3 to the own row and, under
 *           the predicate, to the row -k; loads in the order of the run
 *   c2r  C: stores of stage A, loads and stores of stage B, loads of the rows r and r' of stage C;  R: stores of the rows
 *           r and r' of stage C; loads of the words 2c and 2c + 1 in the order of the run
 * A kernel's plane is the larger of its two layouts and at most FA_IMG2D_LDS_DOUBLES (72 KiB), so two workgroups fit a
 * CU.  A triple for which no padding stays two-way has no entry in vol3dr_pad.inc and a tile of 0.
 *
 * Partial tiles: only the global accesses are predicated (volumes beyond the batch load as zeros and are not stored);
 * an item whose butterfly lies beyond the tile redoes the last valid one, as in pass3d.hpp.  The mirror rows of the r2c
 * stage 3 and the second row of the last pair of an odd c2r stage C are the predicated LDS stores: the predicates depend
 * on the row index alone.
 *
 * Backward transforms use the (re, im) swap identity as register renaming.
 *
 * MEASURED (tools/perf/perf_vol3dr.py, profiles/vol3dr.txt; 1 GiB of real data per batch, one read + one write): r2c
 * 5.3 ... 6.1 TB/s, c2r 4.3 ... 5.9 TB/s over the 69 triples, 4.8 ... 137 x the axis-by-axis plans.  The slowest is
 * 32 x 32 x 4 c2r (4.3 TB/s, T = 1).
 */
#ifndef FA_PASS3DR_HPP
#define FA_PASS3DR_HPP

/* (ds, dp) of layout `lay` (0 X, 1 O, 2 C, 3 R) of the kernels for R0 x R1 x R2 as ds * 64 + dp; -1: none is two-way */
constexpr int fa_vol3dr_pad(int R0, int R1, int R2, int lay) {
    switch (((R0 * 64 + R1) * 64 + R2) * 4 + lay) {
#define P(n0, n1, n2, lay_, ds, dp) case (((n0) * 64 + (n1)) * 64 + (n2)) * 4 + (lay_): return (ds) * 64 + (dp);
#include "vol3dr_pad.inc"
#undef P
    }
    return -1;
}
/* row width of a layout in words */
constexpr int fa_vol3dr_w(int R2, int lay) { return lay == 0 ? R2 / 2 : (lay == 3 ? R2 : R2 / 2 + 1); }
constexpr int fa_vol3dr_s(int R0, int R1, int R2, int lay) { return fa_vol3dr_w(R2, lay) + fa_vol3dr_pad(R0, R1, R2, lay) / 64; }
constexpr int fa_vol3dr_sp(int R0, int R1, int R2, int lay) {
    return R1 * fa_vol3dr_s(R0, R1, R2, lay) + fa_vol3dr_pad(R0, R1, R2, lay) % 64;
}

/* volumes per tile, r2c: the per-item limits of the three stages (fa_img2dr_lim), the run-order registers of the
   complex side, the plane in both of its uses */
constexpr bool fa_vol3dr_fwd_ok(int R0, int R1, int R2, int T) {
    const int H = R2 / 2, M0 = R0 / 2 + 1;
    return fa_img2dr_cdiv(T * R1 * H) * R0 <= fa_img2dr_lim(R0, true) && fa_img2dr_cdiv(T * R0 * H) * R1 <= fa_img2dr_lim(R1, false) &&
           fa_img2dr_cdiv(T * M0 * R1) * R2 <= fa_img2dr_lim(R2, false) && fa_img2dr_cdiv(T * R0 * R1 * (H + 1)) <= FA_IMG2DR_RUN_LIM &&
           T * R0 * fa_vol3dr_sp(R0, R1, R2, 0) <= FA_IMG2D_LDS_DOUBLES && T * R0 * fa_vol3dr_sp(R0, R1, R2, 1) <= FA_IMG2D_LDS_DOUBLES;
}
/* c2r: likewise; the run-order side is the real one, whose plane holds whole real volumes */
constexpr bool fa_vol3dr_bwd_ok(int R0, int R1, int R2, int T) {
    const int H = R2 / 2, P = (R0 * R1 + 1) / 2;
    return fa_img2dr_cdiv(T * R1 * (H + 1)) * R0 <= fa_img2dr_lim(R0, true) && fa_img2dr_cdiv(T * R0 * (H + 1)) * R1 <= fa_img2dr_lim(R1, false) &&
           fa_img2dr_cdiv(T * P) * R2 <= fa_img2dr_lim(R2, false) && fa_img2dr_cdiv(T * R0 * R1 * H) <= FA_IMG2DR_RUN_LIM &&
           T * R0 * fa_vol3dr_sp(R0, R1, R2, 2) <= FA_IMG2D_LDS_DOUBLES && T * R0 * fa_vol3dr_sp(R0, R1, R2, 3) <= FA_IMG2D_LDS_DOUBLES;
}
constexpr int fa_vol3dr_tile(int R0, int R1, int R2, bool fwd) {
    if (R0 < 2 || R1 < 2 || R2 < 2 || R0 > 32 || R1 > 32 || R2 > 32 || (R2 & 1)) return 0;
    if (fa_vol3dr_pad(R0, R1, R2, fwd ? 0 : 2) < 0 || fa_vol3dr_pad(R0, R1, R2, fwd ? 1 : 3) < 0) return 0;
    int T = 16384 / (R0 * R1 * R2);
    while (T > 0 && !(fwd ? fa_vol3dr_fwd_ok(R0, R1, R2, T) : fa_vol3dr_bwd_ok(R0, R1, R2, T))) --T;
    return T;
}

struct Vol3DRArgs {
    const double *src;
    double *dst;
    i64 nvol;                                        /* volumes of this launch */
    int pitch;                                       /* row pitch of the real side in doubles: R2 or R2 + 2 */
    int flags;                                       /* FFTW_AMD_F_NT_IN / NT_OUT */
};

template <int R0, int R1, int R2> struct Vol3DRGeom {
    static constexpr int H = R2 / 2, M0 = R0 / 2 + 1;
    static constexpr int T = fa_vol3dr_tile(R0, R1, R2, true);
    static constexpr int NB1 = T * R1 * H;           /* radix-R0 butterflies per tile (packed columns) */
    static constexpr int NB2 = T * R0 * H;           /* radix-R1 butterflies per tile */
    static constexpr int NB3 = T * M0 * R1;          /* radix-R2 butterflies per tile (rows k0 < M0) */
    static constexpr int Q1 = (NB1 + 255) / 256;
    static constexpr int Q2 = (NB2 + 255) / 256;
    static constexpr int Q3 = (NB3 + 255) / 256;
    static constexpr int VO = R0 * R1 * (H + 1);     /* complex results of a volume */
    static constexpr int E = T * VO;                 /* ... of a tile */
    static constexpr int N = (E + 255) / 256;
    static constexpr int Sx = fa_vol3dr_s(R0, R1, R2, 0), SPx = fa_vol3dr_sp(R0, R1, R2, 0);
    static constexpr int So = fa_vol3dr_s(R0, R1, R2, 1), SPo = fa_vol3dr_sp(R0, R1, R2, 1);
    static constexpr int lds_doubles = T * R0 * (SPx > SPo ? SPx : SPo) + 16;
    static_assert(R2 % 2 == 0 && T >= 1, "vol3dr: even row length, at least one volume");
    static_assert(Q1 * R0 <= fa_img2dr_lim(R0, true), "vol3dr: stage 1 holds too many elements per item");
    static_assert(Q2 * R1 <= fa_img2dr_lim(R1, false), "vol3dr: stage 2 holds too many elements per item");
    static_assert(Q3 * R2 <= fa_img2dr_lim(R2, false), "vol3dr: stage 3 holds too many elements per item");
    static_assert(N <= FA_IMG2DR_RUN_LIM, "vol3dr: too many run-order results per item");
    static_assert(lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16, "vol3dr: the plane does not fit twice on a CU");
};

template <int R0, int R1, int R2>
__global__ void __launch_bounds__(256, 2)
vol3dr_kernel(const Vol3DRArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Vol3DRGeom<R0, R1, R2> G;
    constexpr int H = G::H, M0 = G::M0, T = G::T, NB1 = G::NB1, NB2 = G::NB2, NB3 = G::NB3, Q1 = G::Q1, Q2 = G::Q2, Q3 = G::Q3;
    constexpr int VO = G::VO, E = G::E, N = G::N, Sx = G::Sx, SPx = G::SPx, So = G::So, SPo = G::SPo;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nvol - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid volumes of this tile */
    const int pitch = a.pitch;
    const double *src = a.src + t0 * (i64)(R0 * R1) * pitch;
    double *dst = a.dst + t0 * (i64)(2 * VO);
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;
    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;

    /* ---- load + stage 1: butterfly g = (t, j1, c), (j1, c) fastest across lanes */
    cplx x[Q1][R0];
    int p1[Q1];                                      /* X offset of (t, 0, j1, c) */
#pragma unroll
    for (int u = 0; u < Q1; ++u) {
        int g = u * 256 + tid;
        if (NB1 % 256 != 0 && u == Q1 - 1 && g > NB1 - 1) g = NB1 - 1;
        const int t = g / (R1 * H), m = g - t * (R1 * H);
        const int j1 = m / H, c = m - j1 * H;
        p1[u] = t * (R0 * SPx) + j1 * Sx + c;
        if (t < tcur) {
            ld_run<R0>(x[u], src + ((t * (R0 * R1) + j1) * pitch + 2 * c), (i64)R1 * pitch, nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < R0; ++i) x[u][i] = c_make(0.0, 0.0);
        }
        RB<R0>::run(x[u]);
    }

    /* ---- exchange 1: butterfly h = (t, k0, c), c fastest, owns the column (t, k0, ., c) */
    cplx y[Q2][R1];
    int p2[Q2];                                      /* X offset of (t, k0, 0, c) */
#pragma unroll
    for (int v = 0; v < Q2; ++v) {
        int h = v * 256 + tid;
        if (NB2 % 256 != 0 && v == Q2 - 1 && h > NB2 - 1) h = NB2 - 1;
        const int pl = h / H;                        /* t R0 + k0 */
        p2[v] = pl * SPx + (h - pl * H);
    }
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[p1[u] + k * SPx] = x[u][RB<R0>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].x = plane[p2[v] + c * Sx];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[p1[u] + k * SPx] = x[u][RB<R0>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].y = plane[p2[v] + c * Sx];
    __syncthreads();

    /* ---- stage 2 */
#pragma unroll
    for (int v = 0; v < Q2; ++v) RB<R1>::run(y[v]);

    /* ---- exchange 2: butterfly q = (t, k0 < M0, k1), k1 fastest, reads the rows k and -k and separates */
    cplx z[Q3][R2];
    int p3[Q3], p3m[Q3];                             /* X offsets of the rows k and -k */
    int po[Q3], pm[Q3];                              /* O offsets of the output rows k and -k */
    bool mir[Q3];                                    /* the row has a mirror row that no item computes */
#pragma unroll
    for (int v = 0; v < Q3; ++v) {
        int q = v * 256 + tid;
        if (NB3 % 256 != 0 && v == Q3 - 1 && q > NB3 - 1) q = NB3 - 1;
        const int t = q / (M0 * R1), m = q - t * (M0 * R1);
        const int k0 = m / R1, k1 = m - k0 * R1;
        const int m0 = k0 > 0 ? R0 - k0 : 0, m1 = k1 > 0 ? R1 - k1 : 0;
        p3[v] = (t * R0 + k0) * SPx + k1 * Sx;
        p3m[v] = (t * R0 + m0) * SPx + m1 * Sx;
        po[v] = (t * R0 + k0) * SPo + k1 * So;
        pm[v] = (t * R0 + m0) * SPo + m1 * So;
        mir[v] = k0 > 0 && 2 * k0 != R0;
    }
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[p2[v] + k * Sx] = y[v][RB<R1>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q3; ++v)
#pragma unroll
        for (int c = 0; c < H; ++c) {
            const double zr = plane[p3[v] + c], mr = plane[p3m[v] + c];
            z[v][2 * c].x = 0.5 * (zr + mr);
            z[v][2 * c + 1].y = 0.5 * (mr - zr);
        }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[p2[v] + k * Sx] = y[v][RB<R1>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q3; ++v)
#pragma unroll
        for (int c = 0; c < H; ++c) {
            const double zi = plane[p3[v] + c], mi = plane[p3m[v] + c];
            z[v][2 * c].y = 0.5 * (zi - mi);
            z[v][2 * c + 1].x = 0.5 * (zi + mi);
        }
    __syncthreads();

    /* ---- stage 3 */
#pragma unroll
    for (int v = 0; v < Q3; ++v) RB<R2>::run(z[v]);

    /* ---- rows -> the order of the run: result e = ((t R0 + r0) R1 + r1) (H + 1) + k2 sits at plane e / (R1 (H + 1)),
       row (e / (H + 1)) % R1, position e % (H + 1) */
#define FA_VOL3DR_E(j) ((j) * 256 + tid > E - 1 ? E - 1 : (j) * 256 + tid)
#define FA_VOL3DR_LP(j) (FA_VOL3DR_E(j) + (FA_VOL3DR_E(j) / (H + 1)) * (So - (H + 1)) + (FA_VOL3DR_E(j) / (R1 * (H + 1))) * (SPo - R1 * So))
    cplx w[N];
#pragma unroll
    for (int v = 0; v < Q3; ++v) {
#pragma unroll
        for (int k = 0; k <= H; ++k) plane[po[v] + k] = z[v][RB<R2>::slot(k)].x;
        if (mir[v]) {
#pragma unroll
            for (int k = 0; k <= H; ++k) plane[pm[v] + k] = z[v][RB<R2>::slot((R2 - k) % R2)].x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].x = plane[FA_VOL3DR_LP(j)];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q3; ++v) {
#pragma unroll
        for (int k = 0; k <= H; ++k) plane[po[v] + k] = z[v][RB<R2>::slot(k)].y;
        if (mir[v]) {
#pragma unroll
            for (int k = 0; k <= H; ++k) plane[pm[v] + k] = -z[v][RB<R2>::slot((R2 - k) % R2)].y;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].y = plane[FA_VOL3DR_LP(j)];
#undef FA_VOL3DR_LP
#undef FA_VOL3DR_E

    const int ecur = tcur * VO;                      /* valid results of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        if (e < ecur) st_sel(dst + 2 * e, w[j], nt_out);
    }
}

template <int R0, int R1, int R2> struct Vol3DCGeom {
    static constexpr int H = R2 / 2, NR = R0 * R1, P = (NR + 1) / 2;
    static constexpr int T = fa_vol3dr_tile(R0, R1, R2, false);
    static constexpr int NBA = T * R1 * (H + 1);     /* radix-R0 butterflies per tile (columns 0 ... H) */
    static constexpr int NBB = T * R0 * (H + 1);     /* radix-R1 butterflies per tile */
    static constexpr int NBC = T * P;                /* radix-R2 butterflies per tile (row pairs) */
    static constexpr int QA = (NBA + 255) / 256;
    static constexpr int QB = (NBB + 255) / 256;
    static constexpr int QC = (NBC + 255) / 256;
    static constexpr int VC = NR * (H + 1);          /* complex entries of a volume */
    static constexpr int E = T * NR * H;             /* pairs of reals of a tile */
    static constexpr int N = (E + 255) / 256;
    static constexpr int Sc = fa_vol3dr_s(R0, R1, R2, 2), SPc = fa_vol3dr_sp(R0, R1, R2, 2);
    static constexpr int Sr = fa_vol3dr_s(R0, R1, R2, 3), SPr = fa_vol3dr_sp(R0, R1, R2, 3);
    static constexpr int lds_doubles = T * R0 * (SPc > SPr ? SPc : SPr) + 16;
    static_assert(R2 % 2 == 0 && T >= 1, "vol3dc: even row length, at least one volume");
    static_assert(QA * R0 <= fa_img2dr_lim(R0, true), "vol3dc: stage A holds too many elements per item");
    static_assert(QB * R1 <= fa_img2dr_lim(R1, false), "vol3dc: stage B holds too many elements per item");
    static_assert(QC * R2 <= fa_img2dr_lim(R2, false), "vol3dc: stage C holds too many elements per item");
    static_assert(N <= FA_IMG2DR_RUN_LIM, "vol3dc: too many run-order results per item");
    static_assert(lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16, "vol3dc: the plane does not fit twice on a CU");
};

template <int R0, int R1, int R2>
__global__ void __launch_bounds__(256, 2)
vol3dc_kernel(const Vol3DRArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Vol3DCGeom<R0, R1, R2> G;
    constexpr int H = G::H, NR = G::NR, P = G::P, T = G::T, NBA = G::NBA, NBB = G::NBB, NBC = G::NBC;
    constexpr int QA = G::QA, QB = G::QB, QC = G::QC, VC = G::VC, E = G::E, N = G::N;
    constexpr int Sc = G::Sc, SPc = G::SPc, Sr = G::Sr, SPr = G::SPr;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nvol - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid volumes of this tile */
    const int pitch = a.pitch;
    const double *src = a.src + t0 * (i64)(2 * VC);
    double *dst = a.dst + t0 * (i64)NR * pitch;
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;
    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;

    /* ---- load + stage A: butterfly g = (t, k1, c), c = 0 ... H fastest across lanes; backward by the swap identity */
    cplx x[QA][R0];
    int pa[QA];                                      /* C offset of (t, 0, k1, c) */
#pragma unroll
    for (int u = 0; u < QA; ++u) {
        int g = u * 256 + tid;
        if (NBA % 256 != 0 && u == QA - 1 && g > NBA - 1) g = NBA - 1;
        const int t = g / (R1 * (H + 1)), m = g - t * (R1 * (H + 1));
        const int k1 = m / (H + 1), c = m - k1 * (H + 1);
        pa[u] = t * (R0 * SPc) + k1 * Sc + c;
        if (t < tcur) {
            ld_run<R0>(x[u], src + 2 * (t * VC + m), (i64)(2 * R1 * (H + 1)), nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < R0; ++i) x[u][i] = c_make(0.0, 0.0);
        }
#pragma unroll
        for (int i = 0; i < R0; ++i) { const double s = x[u][i].x; x[u][i].x = x[u][i].y; x[u][i].y = s; }
        RB<R0>::run(x[u]);
    }

    /* ---- exchange 1: butterfly h = (t, j0, c), c fastest, owns the column (t, j0, ., c); the values stay swapped */
    cplx y[QB][R1];
    int pb[QB];                                      /* C offset of (t, j0, 0, c) */
#pragma unroll
    for (int v = 0; v < QB; ++v) {
        int h = v * 256 + tid;
        if (NBB % 256 != 0 && v == QB - 1 && h > NBB - 1) h = NBB - 1;
        const int pl = h / (H + 1);                  /* t R0 + j0 */
        pb[v] = pl * SPc + (h - pl * (H + 1));
    }
#pragma unroll
    for (int u = 0; u < QA; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[pa[u] + k * SPc] = x[u][RB<R0>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QB; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].x = plane[pb[v] + c * Sc];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < QA; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[pa[u] + k * SPc] = x[u][RB<R0>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QB; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].y = plane[pb[v] + c * Sc];
    __syncthreads();

    /* ---- stage B: the result (j0, j1, c) is (y[slot(j1)].y, y[slot(j1)].x) */
#pragma unroll
    for (int v = 0; v < QB; ++v) RB<R1>::run(y[v]);

    /* ---- exchange 2: columns -> pairs of rows; W = Y_r + i Y_r' built while the two planes are read */
    cplx z[QC][R2];
    int pc[QC], pq[QC];                              /* C offsets of the rows r and r' */
    int pw[QC], pv[QC];                              /* R offsets of the output rows r and r' */
    bool two[QC];                                    /* the pair has a second row */
#pragma unroll
    for (int v = 0; v < QC; ++v) {
        int q = v * 256 + tid;
        if (NBC % 256 != 0 && v == QC - 1 && q > NBC - 1) q = NBC - 1;
        const int t = q / P, r = 2 * (q - t * P);
        two[v] = r + 1 < NR;
        const int rr = two[v] ? r + 1 : r;
        const int j0 = r / R1, j1 = r - j0 * R1, i0 = rr / R1, i1 = rr - i0 * R1;
        pc[v] = (t * R0 + j0) * SPc + j1 * Sc;
        pq[v] = (t * R0 + i0) * SPc + i1 * Sc;
        pw[v] = (t * R0 + j0) * SPr + j1 * Sr;
        pv[v] = (t * R0 + i0) * SPr + i1 * Sr;
    }
#pragma unroll
    for (int v = 0; v < QB; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[pb[v] + k * Sc] = y[v][RB<R1>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QC; ++v)
#pragma unroll
        for (int c = 0; c <= H; ++c) {
            const double ar = plane[pc[v] + c], br = two[v] ? plane[pq[v] + c] : 0.0;
            z[v][c] = c_make(ar, br);
            if (c > 0 && c < H) z[v][R2 - c] = c_make(ar, br);
        }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QB; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[pb[v] + k * Sc] = y[v][RB<R1>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QC; ++v)
#pragma unroll
        for (int c = 1; c < H; ++c) {                /* the imaginary parts of the entries 0 and H are dropped */
            const double ai = plane[pc[v] + c], bi = two[v] ? plane[pq[v] + c] : 0.0;
            z[v][c].x -= bi;
            z[v][c].y += ai;
            z[v][R2 - c].x += bi;
            z[v][R2 - c].y -= ai;
        }
    __syncthreads();

    /* ---- stage C, backward by the swap identity: row r leaves in the .y parts, row r' in the .x parts */
#pragma unroll
    for (int v = 0; v < QC; ++v) {
#pragma unroll
        for (int i = 0; i < R2; ++i) { const double s = z[v][i].x; z[v][i].x = z[v][i].y; z[v][i].y = s; }
        RB<R2>::run(z[v]);
    }

    /* ---- rows -> the order of the run: pair e = (t NR + r) H + c sits at plane e / (R1 H), row (e / H) % R1, words
       2c and 2c + 1 */
#pragma unroll
    for (int v = 0; v < QC; ++v) {
#pragma unroll
        for (int k = 0; k < R2; ++k) plane[pw[v] + k] = z[v][RB<R2>::slot(k)].y;
        if (two[v]) {
#pragma unroll
            for (int k = 0; k < R2; ++k) plane[pv[v] + k] = z[v][RB<R2>::slot(k)].x;
        }
    }
    __syncthreads();
    const int ecur = tcur * (NR * H);                /* valid pairs of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        const int ec = e > E - 1 ? E - 1 : e;
        const int row = ec / H, c = ec - row * H;    /* row = t NR + j0 R1 + j1 */
        const int pl = row / R1;                     /* t R0 + j0 */
        const int lp = pl * SPr + (row - pl * R1) * Sr + 2 * c;
        const cplx o = c_make(plane[lp], plane[lp + 1]);
        if (e < ecur) st_sel(dst + ((i64)row * pitch + 2 * c), o, nt_out);
    }
}

#endif /* FA_PASS3DR_HPP */
