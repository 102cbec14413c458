/*
 * pass3d.hpp -- one-trip 3-D transform of small contiguous volumes: T whole volumes of R0 x R1 x R2 points
 * (every extent at most 32, at most 8192 points) per workgroup, all three axes in registers.
 *
 * The structure of pass2d.hpp with one more stage.  The 3-D DFT of a row-major volume x[j0][j1][j2]:
 *
 *   stage 1   butterfly g = (volume t, j1, j2): DFT of length R0 down axis 0, loaded from global memory
 *   exchange  one LDS plane, real parts then imaginary parts
 *   stage 2   butterfly h = (t, k0, j2):        DFT of length R1 along axis 1
 *   exchange  the same plane again
 *   stage 3   butterfly q = (t, k0, k1):        DFT of length R2 along axis 2
 *   transposition through the same plane into the order of the run, stored to global memory
 *
 * No twiddles, no tables: the three stages are plain RB<R> butterflies on separate axes.
 *
 * Global access.  The T volumes of a tile are ONE contiguous run of E = T R0 R1 R2 elements on both sides.
 *   Loads are in the natural order of stage 1: lane (t, j1, j2), (j1, j2) fastest, reads plane j0 = r of its volume
 *   in instruction r, so a wave instruction moves a contiguous piece of a plane (R1 R2 x 16 bytes per volume), and no
 *   LDS round trip stands in front of the first arithmetic.
 *   Stores in the natural order of stage 3 would put consecutive lanes R2 elements apart, so the results go through
 *   the plane once more and leave in the order of the run: item tid stores elements j 256 + tid, every wave
 *   instruction one contiguous 1 KiB piece, whatever the extents are (the reasons of pass2d.hpp).
 *
 * LDS layout.  All three exchanges use one layout: element (t, a0, a1, a2) of the tile sits at
 *   (t R0 + a0) SP + a1 S + a2       S = R2 + ds >= R2 (row stride),  SP = R1 S + dp (plane stride), in doubles.
 * Four lane patterns meet it; the register index of an access only adds a constant, so each pattern is one map from
 * 32 consecutive items to banks (32 banks of 64 bits):
 *   A  items (t, a1, a2), a0 fixed:  the stores of stage 1                      a2 contiguous, a1 S apart
 *   B  items (t, a0, a2), a1 fixed:  the loads and the stores of stage 2        a2 contiguous, a0 SP apart
 *   C  items (t, a0, a1), a2 fixed:  the loads and the stores of stage 3        a1 S apart, a0 SP apart
 *   D  items in the order of the run: the loads of the transposition            contiguous but for the padding
 * A wants rows that follow each other (S near R2), C wants S odd (a row of 32 lanes then walks all banks) or, for
 * R1 < 32, S and SP that interleave the rows of several planes, B wants SP = R2 x odd (mod 32) so that the pieces of
 * 32 / R2 planes tile the banks.  No single (ds, dp) makes all four conflict free for every (R1, R2); fa_vol3d_pad
 * holds, per (R1, R2) of the menu, the smallest padding for which NO wave instruction of any of the four patterns
 * puts more than two distinct words on one bank, over every 32-item group of the tile including the ragged ones
 * (items beyond the tile's butterfly count repeat the last address, which is one word).  Two-way is what a 64-bit LDS
 * access absorbs.  The pairs were found, and are re-counted for every menu entry, by enumeration of the addresses
 * (tools/perf/vol3d_codeobj.py, column `way`); no conflict counter of the hardware was read.  32 x 32 x 8 is the one
 * triple for which no padding inside the plane limit stays two-way (pattern B is four-way at the only padding that
 * fits), so it is not in vol3d_menu.inc.
 * The plane is at most FA_IMG2D_LDS_DOUBLES (72 KiB), so two workgroups fit a CU; where the padding does not fit at
 * 8192 / (R0 R1 R2) volumes the tile has fewer (fa_vol3d_tile).
 *
 * Partial tiles: only the global accesses are predicated (volumes beyond the batch load as zeros and are not stored).
 * Where a stage's butterfly count is no multiple of 256, an item whose butterfly lies beyond the tile redoes the last
 * valid one (same values to the same LDS words): there is no predicate around LDS traffic or butterflies.
 *
 * In place: a tile is entirely in registers before its first store.
 *
 * Backward transforms use the (re, im) swap identity; BWD is a template parameter, so the swaps are register
 * renaming and cost nothing.
 */
#ifndef FA_PASS3D_HPP
#define FA_PASS3D_HPP

/* (ds, dp) of the LDS layout as ds * 64 + dp; any other (R1, R2): the odd row stride of pass2d.hpp */
constexpr int fa_vol3d_pad(int R1, int R2) {
    switch (R1 * 64 + R2) {
    case 4 * 64 + 4: return 1;        case 4 * 64 + 8: return 64;       case 4 * 64 + 16: return 1;      case 4 * 64 + 32: return 64;
    case 8 * 64 + 4: return 2;        case 8 * 64 + 8: return 5;        case 8 * 64 + 16: return 64;     case 8 * 64 + 32: return 64;
    case 16 * 64 + 4: return 2;       case 16 * 64 + 8: return 64;      case 16 * 64 + 16: return 64;    case 16 * 64 + 32: return 64;
    case 32 * 64 + 4: return 64 + 2;  case 32 * 64 + 8: return 64 + 4;  case 32 * 64 + 16: return 64;    case 32 * 64 + 32: return 64;
    case 5 * 64 + 5: return 0;        case 6 * 64 + 6: return 0;        case 10 * 64 + 10: return 1;     case 12 * 64 + 12: return 1;
    case 15 * 64 + 15: return 7;
    case 6 * 64 + 10: return 64 + 4;  case 6 * 64 + 12: return 1;       case 10 * 64 + 6: return 0;      case 10 * 64 + 12: return 1;
    case 12 * 64 + 6: return 0;       case 12 * 64 + 10: return 0;
    }
    return (R2 & 1) ? 0 : 64;
}
constexpr int fa_vol3d_s(int R1, int R2) { return R2 + fa_vol3d_pad(R1, R2) / 64; }
constexpr int fa_vol3d_sp(int R1, int R2) { return R1 * fa_vol3d_s(R1, R2) + fa_vol3d_pad(R1, R2) % 64; }

/* volumes per tile: as many as fit 8192 elements, the per-item limits of the three stages (fa_img2d_lim) and the
   padded plane; 0: not even one */
constexpr int fa_vol3d_tile(int R0, int R1, int R2) {
    int T = 8192 / (R0 * R1 * R2);
    while (T > 0 && (fa_rr_q(R1 * R2, T) * R0 > fa_img2d_lim(R0, true) || fa_rr_q(R0 * R2, T) * R1 > fa_img2d_lim(R1, false) ||
                     fa_rr_q(R0 * R1, T) * R2 > fa_img2d_lim(R2, false) || T * R0 * fa_vol3d_sp(R1, R2) > FA_IMG2D_LDS_DOUBLES)) --T;
    return T;
}

template <int R0, int R1, int R2> struct Vol3DGeom {
    static constexpr int T = fa_vol3d_tile(R0, R1, R2);
    static constexpr int V = R0 * R1 * R2;           /* elements of a volume */
    static constexpr int P = R1 * R2;                /* elements of a plane j0 */
    static constexpr int E = T * V;                  /* elements of a tile */
    static constexpr int NB1 = T * R1 * R2;          /* radix-R0 butterflies per tile */
    static constexpr int NB2 = T * R0 * R2;          /* radix-R1 butterflies per tile */
    static constexpr int NB3 = T * R0 * R1;          /* radix-R2 butterflies per tile */
    static constexpr int Q1 = (NB1 + 255) / 256;
    static constexpr int Q2 = (NB2 + 255) / 256;
    static constexpr int Q3 = (NB3 + 255) / 256;
    static constexpr int N = (E + 255) / 256;        /* elements per item in the order of the run */
    static constexpr int S = fa_vol3d_s(R1, R2);     /* LDS row stride (doubles) */
    static constexpr int SP = fa_vol3d_sp(R1, R2);   /* LDS plane stride (doubles) */
    static constexpr int lds_doubles = T * R0 * SP + 16;
    static_assert(T >= 1, "vol3d: not even one volume fits");
    static_assert(E <= 8192 && lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16, "vol3d: the plane does not fit twice on a CU");
};

struct Vol3DArgs {
    const double *src;
    double *dst;
    i64 nvol;                                        /* volumes of this launch */
    int flags;                                       /* FFTW_AMD_F_NT_IN / NT_OUT (the swap is the BWD parameter) */
};

template <int R0, int R1, int R2, bool BWD>
__global__ void __launch_bounds__(256, 2)
vol3d_kernel(const Vol3DArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Vol3DGeom<R0, R1, R2> G;
    constexpr int T = G::T, V = G::V, P = G::P, E = G::E, NB1 = G::NB1, NB2 = G::NB2, NB3 = G::NB3;
    constexpr int Q1 = G::Q1, Q2 = G::Q2, Q3 = G::Q3, N = G::N, S = G::S, SP = G::SP;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nvol - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid volumes of this tile */
    const double *src = a.src + t0 * (i64)(2 * V);
    double *dst = a.dst + t0 * (i64)(2 * V);
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;
    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;

    /* ---- load + stage 1: butterfly g = (t, j1, j2), (j1, j2) fastest across lanes */
    cplx x[Q1][R0];
    int p1[Q1];                                      /* plane offset of (t, 0, j1, j2) */
#pragma unroll
    for (int u = 0; u < Q1; ++u) {
        int g = u * 256 + tid;
        if (NB1 % 256 != 0 && u == Q1 - 1 && g > NB1 - 1) g = NB1 - 1;
        const int t = g / P, m = g - t * P;
        const int j1 = m / R2, j2 = m - j1 * R2;
        p1[u] = t * (R0 * SP) + j1 * S + j2;
        if (t < tcur) {
            ld_run<R0>(x[u], src + 2 * (t * V + m), (i64)(2 * P), nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < R0; ++i) x[u][i] = c_make(0.0, 0.0);
        }
        if (BWD) {
#pragma unroll
            for (int i = 0; i < R0; ++i) { const double s = x[u][i].x; x[u][i].x = x[u][i].y; x[u][i].y = s; }
        }
        RB<R0>::run(x[u]);
    }

    /* ---- exchange 1: butterfly h = (t, k0, j2), j2 fastest, owns the column (t, k0, ., j2) */
    cplx y[Q2][R1];
    int p2[Q2];                                      /* plane offset of (t, k0, 0, j2) */
#pragma unroll
    for (int v = 0; v < Q2; ++v) {
        int h = v * 256 + tid;
        if (NB2 % 256 != 0 && v == Q2 - 1 && h > NB2 - 1) h = NB2 - 1;
        const int pl = h / R2;                       /* t R0 + k0 */
        p2[v] = pl * SP + (h - pl * R2);
    }
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[p1[u] + k * SP] = x[u][RB<R0>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].x = plane[p2[v] + c * S];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[p1[u] + k * SP] = x[u][RB<R0>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].y = plane[p2[v] + c * S];
    __syncthreads();

    /* ---- stage 2 */
#pragma unroll
    for (int v = 0; v < Q2; ++v) RB<R1>::run(y[v]);

    /* ---- exchange 2: butterfly q = (t, k0, k1), k1 fastest, owns the row (t, k0, k1, .) */
    cplx z[Q3][R2];
    int p3[Q3];                                      /* plane offset of (t, k0, k1, 0) */
#pragma unroll
    for (int v = 0; v < Q3; ++v) {
        int q = v * 256 + tid;
        if (NB3 % 256 != 0 && v == Q3 - 1 && q > NB3 - 1) q = NB3 - 1;
        const int pl = q / R1;                       /* t R0 + k0 */
        p3[v] = pl * SP + (q - pl * R1) * S;
    }
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[p2[v] + k * S] = y[v][RB<R1>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q3; ++v)
#pragma unroll
        for (int c = 0; c < R2; ++c) z[v][c].x = plane[p3[v] + c];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[p2[v] + k * S] = y[v][RB<R1>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q3; ++v)
#pragma unroll
        for (int c = 0; c < R2; ++c) z[v][c].y = plane[p3[v] + c];
    __syncthreads();

    /* ---- stage 3 */
#pragma unroll
    for (int v = 0; v < Q3; ++v) RB<R2>::run(z[v]);

    /* ---- rows -> the order of the run: element e = ((t R0 + k0) R1 + k1) R2 + k2 sits at plane e / P, row
       (e % P) / R2, position e % R2 */
#define FA_VOL3D_E(j) ((j) * 256 + tid > E - 1 ? E - 1 : (j) * 256 + tid)
#define FA_VOL3D_LP(j) (FA_VOL3D_E(j) + (FA_VOL3D_E(j) / R2) * (S - R2) + (FA_VOL3D_E(j) / P) * (SP - R1 * S))
    cplx w[N];
#pragma unroll
    for (int v = 0; v < Q3; ++v)
#pragma unroll
        for (int k = 0; k < R2; ++k) plane[p3[v] + k] = z[v][RB<R2>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].x = plane[FA_VOL3D_LP(j)];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q3; ++v)
#pragma unroll
        for (int k = 0; k < R2; ++k) plane[p3[v] + k] = z[v][RB<R2>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].y = plane[FA_VOL3D_LP(j)];
#undef FA_VOL3D_LP
#undef FA_VOL3D_E

    const int ecur = tcur * V;                       /* valid elements of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        const cplx o = BWD ? c_make(w[j].y, w[j].x) : w[j];
        if (e < ecur) st_sel(dst + 2 * e, o, nt_out);
    }
}

#endif /* FA_PASS3D_HPP */
