/*
 * pass2d.hpp -- one-trip 2-D transform of small contiguous images: T whole images of R0 rows x R1 columns
 * (R0, R1 <= 32) per workgroup, both axes in registers.
 *
 * The 2-D DFT R0 x R1 of a row-major image is the two-stage scheme of passrr.hpp without the inter-stage
 * twiddle and with the output index in row-major order:
 *
 *   stage 1   butterfly g = (image t, column c): DFT of length R0 down the column, loaded from global memory
 *   exchange  one LDS plane, real parts then imaginary parts
 *   stage 2   butterfly h = (image t, row k0):   DFT of length R1 along the row
 *   transposition through the same plane into the order of the run, stored to global memory
 *
 * Global access.  The T images of a tile are ONE contiguous run of E = T R0 R1 elements on both sides.
 *   Loads are in the natural order of stage 1: lane (t, c), c fastest, reads row r of its column in instruction r,
 *   so a wave instruction moves whole image rows, runs of R1 x 16 bytes, and instruction r + 1 of the same lanes
 *   takes the runs right behind them (the lines are touched back to back).
 *   Stores in the natural order of stage 2 would put consecutive lanes R1 elements apart (16-byte segments), so
 *   the results go through the LDS plane once more and leave in the order of the run: item tid stores elements
 *   j 256 + tid, every wave instruction one contiguous 1 KiB piece, whatever R0 and R1 are.
 *   The transposition is on the STORE side because that is where short runs cost: a line written in pieces by
 *   several instructions has to be merged in L2 (and nontemporal stores of partial lines ran at a third of the
 *   rate, rr_dispatch.hpp), while a line read in pieces by consecutive instructions of one wave is served from the
 *   cache it already sits in; and the loads of stage 1 then feed the butterflies without an LDS round trip in front
 *   of the first arithmetic.
 *
 * LDS layout.  Both exchanges use one image of the tile as rows: row rho = t R0 + k0 (the stage-2 butterfly index
 * itself), S = R1 | 1 doubles apart, position c inside.  The odd row stride is the padding against bank conflicts:
 *   - the row-wise accesses of stage 2 (lane h reads / writes position c of row h) are S doubles apart from lane to
 *     lane, and an odd S walks all 32 double-wide banks before it repeats, so the 32 lanes of a group fall on
 *     different banks whatever R0 and T are (with S = R1 even, R1 = 16 or 32 would put every lane on one bank);
 *   - the column-wise stores of stage 1 (lane (t, c) writes row t R0 + k0, position c) are consecutive doubles
 *     inside an image row and t R0 S apart between images: conflict free for R1 >= 16, at most two-way for the
 *     narrower images whose R0 S is a multiple of 8, which a 64-bit LDS store absorbs;
 *   - the run-order reads at the end are consecutive doubles with one skipped per row.
 * The plane is at most 72 KiB (8192 doubles + the padding), so two workgroups fit a CU.
 *
 * Partial tiles: only the global accesses are predicated (images beyond the batch load as zeros and are not
 * stored).  Where a tile's butterfly count is no multiple of 256, an item whose butterfly lies beyond the tile
 * redoes the last valid one (same values to the same LDS words): there is no predicate around LDS traffic.
 *
 * Backward transforms use the (re, im) swap identity; BWD is a template parameter, so the swaps are register
 * renaming and cost nothing.
 */
#ifndef FA_PASS2D_HPP
#define FA_PASS2D_HPP

/* the plane of one workgroup: 72 KiB, two of them fit the 160 KiB of a CU */
#define FA_IMG2D_LDS_DOUBLES 9216

/* elements an item may hold in a stage of radix R: 32 for the powers of two (one butterfly of 32, two of 16 ...),
   the limits of fa_rr_lim for the odd and composite butterflies, which need temporaries */
constexpr int fa_img2d_lim(int R, bool first) {
    return ((R & (R - 1)) == 0) ? 32 : fa_rr_lim(R, first);
}
/* images per tile: as many as fit 8192 elements, the per-item limits of both stages and the plane */
constexpr int fa_img2d_tile(int R0, int R1) {
    int T = 8192 / (R0 * R1);
    while (T > 1 && (fa_rr_q(R1, T) * R0 > fa_img2d_lim(R0, true) || fa_rr_q(R0, T) * R1 > fa_img2d_lim(R1, false) ||
                     T * R0 * (R1 | 1) > FA_IMG2D_LDS_DOUBLES)) --T;
    return T;
}

template <int R0, int R1> struct Img2DGeom {
    static constexpr int T = fa_img2d_tile(R0, R1);
    static constexpr int E = T * R0 * R1;            /* elements of a tile */
    static constexpr int NB1 = R1 * T;               /* radix-R0 butterflies per tile (columns) */
    static constexpr int NB2 = R0 * T;               /* radix-R1 butterflies per tile (rows) */
    static constexpr int Q1 = (NB1 + 255) / 256;
    static constexpr int Q2 = (NB2 + 255) / 256;
    static constexpr int N = (E + 255) / 256;        /* elements per item in the order of the run */
    static constexpr int S = R1 | 1;                 /* LDS row stride (doubles), odd */
    static constexpr int lds_doubles = NB2 * S + 16;
    static_assert(lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16 || T == 1, "img2d: the plane does not fit twice on a CU");
};

struct Img2DArgs {
    const double *src;
    double *dst;
    i64 nimg;                                        /* images of this launch */
    int flags;                                       /* FFTW_AMD_F_NT_IN / NT_OUT (the swap is the BWD parameter) */
};

template <int R0, int R1, bool BWD>
__global__ void __launch_bounds__(256, 2)
img2d_kernel(const Img2DArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DGeom<R0, R1> G;
    constexpr int T = G::T, E = G::E, NB1 = G::NB1, NB2 = G::NB2, Q1 = G::Q1, Q2 = G::Q2, N = G::N, S = G::S;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nimg - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid images of this tile */
    const double *src = a.src + t0 * (i64)(2 * R0 * R1);
    double *dst = a.dst + t0 * (i64)(2 * R0 * R1);
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;
    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;

    /* ---- load + stage 1: butterfly g = (t, c), c fastest across lanes */
    cplx x[Q1][R0];
    int p1[Q1];                                      /* plane offset of (row t R0, position c) */
#pragma unroll
    for (int u = 0; u < Q1; ++u) {
        int g = u * 256 + tid;
        if (NB1 % 256 != 0 && u == Q1 - 1 && g > NB1 - 1) g = NB1 - 1;
        const int t = g / R1, c = g - t * R1;
        p1[u] = t * (R0 * S) + c;
        if (t < tcur) {
            ld_run<R0>(x[u], src + 2 * (t * (R0 * R1) + c), (i64)(2 * R1), nt_in);
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

    /* ---- exchange: columns -> rows, one real plane at a time; butterfly h = (t, k0) owns row h */
    cplx y[Q2][R1];
    int p2[Q2];
#pragma unroll
    for (int v = 0; v < Q2; ++v) {
        int h = v * 256 + tid;
        if (NB2 % 256 != 0 && v == Q2 - 1 && h > NB2 - 1) h = NB2 - 1;
        p2[v] = h * S;
    }
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[p1[u] + k * S] = x[u][RB<R0>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].x = plane[p2[v] + c];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[p1[u] + k * S] = x[u][RB<R0>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].y = plane[p2[v] + c];
    __syncthreads();

    /* ---- stage 2 */
#pragma unroll
    for (int v = 0; v < Q2; ++v) RB<R1>::run(y[v]);

    /* ---- rows -> the order of the run: element e = (t R0 + k0) R1 + k1 sits at row e / R1, position e % R1 */
#define FA_IMG2D_LP(j) (((j) * 256 + tid > E - 1 ? E - 1 : (j) * 256 + tid) + (((j) * 256 + tid > E - 1 ? E - 1 : (j) * 256 + tid) / R1) * (S - R1))
    cplx w[N];
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[p2[v] + k] = y[v][RB<R1>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].x = plane[FA_IMG2D_LP(j)];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[p2[v] + k] = y[v][RB<R1>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].y = plane[FA_IMG2D_LP(j)];
#undef FA_IMG2D_LP

    const int ecur = tcur * (R0 * R1);               /* valid elements of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        const cplx o = BWD ? c_make(w[j].y, w[j].x) : w[j];
        if (e < ecur) st_sel(dst + 2 * e, o, nt_out);
    }
}

#endif /* FA_PASS2D_HPP */
