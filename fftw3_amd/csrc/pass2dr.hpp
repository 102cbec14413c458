/*
 * pass2dr.hpp -- one-trip 2-D r2c and c2r transforms of small real images: T whole images of R0 rows x R1 real
 * columns (R0, R1 <= 32, R1 even) per workgroup, both axes in registers.  The real twins of pass2d.hpp: the same
 * butterflies (RB<R>), the same plane with the odd row stride, the same store in the order of the run; no twiddle
 * appears anywhere, so there is no table.  Below H = R1 / 2 and M = R0 / 2 + 1 (integer division).
 *
 * r2c (img2dr_kernel).  The real image x[r][n] is read as the complex image z[r][c] = x[r][2c] + i x[r][2c+1], R0 x H.
 *   stage 1   butterfly g = (image t, packed column c): Z = DFT of length R0 down the column, loaded from global memory
 *             (16-byte pairs at the real row pitch).  The item holds both Z[k0] and Z[R0 - k0], so it separates the two
 *             real columns itself, in place (slot k0 keeps A_2c[k0], slot R0 - k0 gets A_2c+1[k0]; done on separate values
 *             the compiler kept both planes' worth live beside x and spilled):
 *                                   A_2c[k0] = (Z[k0] + conj Z[(R0-k0) % R0]) / 2,
 *                                   A_2c+1[k0] = (Z[k0] - conj Z[(R0-k0) % R0]) / 2i        for k0 = 0 ... M - 1
 *   exchange  plane rows (t, k0), M per image, S = R1 | 1 doubles apart, R1 values each; real parts, then imaginary parts
 *   stage 2   butterfly h = (t, k0): y = DFT of length R1 along the row.  Row k0 of the output is y[0 ... H]; for
 *             0 < k0 and 2 k0 != R0, row R0 - k0 is conj y[(R1 - k1) % R1], k1 = 0 ... H (the rows 0 and R0 / 2 are
 *             their own mirrors and give only themselves)
 *   transposition through the plane -- rows (t, r), R0 per image, So = (H + 1) | 1 doubles apart -- into the order of
 *   the run of the output images, R0 x (H + 1) complex, stored as contiguous 1 KiB pieces per wave instruction.
 *
 * c2r (img2dc_kernel).  The definition: the backward DFT of length R0 down each of the H + 1 columns, then the 1-D c2r
 * of length R1 along each row, which reads the imaginary parts of its entries 0 and H as 0 -- also for half spectra
 * that are not Hermitian.
 *   stage A   butterfly g = (t, c), c = 0 ... H: backward DFT of length R0 down the column, loaded from global memory
 *   exchange  plane rows (t, r), R0 per image, Sc = (H + 1) | 1 doubles apart; real parts, then imaginary parts
 *   stage B   butterfly h = (t, row pair (r, r') = (2q, 2q + 1)): W = Y_r + i Y_r', Y the Hermitian expansion of the
 *             H + 1 entries of a row with the two imaginary parts dropped; one backward DFT of length R1 leaves row r
 *             in the real parts and row r' in the imaginary parts (an odd R0 leaves the last row on its own: its
 *             partner reads as zeros and is not stored)
 *   transposition through the plane -- rows (t, r) of R1 reals, S = R1 | 1 apart, one trip since the values are real
 *   -- into the order of the run of the real images, stored as 16-byte pairs (the padding of padded rows is not
 *   written).
 *
 * Layout.  The complex row pitch is always R1 + 2 doubles (dense rows of H + 1 entries); the real row pitch is a
 * kernel argument, R1 (dense) or R1 + 2 (the padded in-place layout).  A tile is one contiguous run on both sides
 * that no other workgroup touches, and every global load of a workgroup precedes its first global store (the
 * barriers of the exchanges lie in between), so the transforms work in place on padded rows.
 *
 * Partial tiles: only the global accesses are predicated (images beyond the batch load as zeros and are not stored);
 * an item whose butterfly lies beyond the tile redoes the last valid one, as in pass2d.hpp.  The mirror rows of the
 * r2c stage 2 are the one predicated LDS store: the predicate depends on k0 alone.
 *
 * Backward transforms use the (re, im) swap identity as register renaming.
 *
 * MEASURED (tools/perf/perf_img2dr.py, profiles/img2dr.txt; 1 GiB of real data per batch, one read + one write): r2c
 * 5.3 ... 5.9 TB/s, c2r 4.9 ... 6.0 TB/s over the 130 pairs, 12 ... 122 x the three-trip plans.  The short load runs of
 * n1 = 4 and 6 are not the limiter (5.3 ... 6.0 TB/s), so run-order loads through the plane were not tried.
 */
#ifndef FA_PASS2DR_HPP
#define FA_PASS2DR_HPP

/* run-order values (16 bytes each: a complex result or a pair of reals) an item may hold */
#define FA_IMG2DR_RUN_LIM 32

constexpr int fa_img2dr_cdiv(int a) { return (a + 255) / 256; }
/* elements an item may hold in a stage of radix R: the limit of pass2d.hpp, but always one whole butterfly (the row
   stage of 30 points has a limit of 28: without this a tile would be a single image) */
constexpr int fa_img2dr_lim(int R, bool first) { return fa_img2d_lim(R, first) > R ? fa_img2d_lim(R, first) : R; }
/* images per tile, r2c: the per-item limits of both stages, the run-order registers of the (wider) complex side, the
   plane in both of its uses */
constexpr bool fa_img2dr_fwd_ok(int R0, int R1, int T) {
    const int H = R1 / 2, M = R0 / 2 + 1;
    return fa_img2dr_cdiv(T * H) * R0 <= fa_img2dr_lim(R0, true) && fa_img2dr_cdiv(T * M) * R1 <= fa_img2dr_lim(R1, false) &&
           fa_img2dr_cdiv(T * R0 * (H + 1)) <= FA_IMG2DR_RUN_LIM && T * M * (R1 | 1) <= FA_IMG2D_LDS_DOUBLES &&
           T * R0 * ((H + 1) | 1) <= FA_IMG2D_LDS_DOUBLES;
}
/* c2r: likewise; the run-order side is the real one, whose plane holds whole real images */
constexpr bool fa_img2dr_bwd_ok(int R0, int R1, int T) {
    const int H = R1 / 2, P = (R0 + 1) / 2;
    return fa_img2dr_cdiv(T * (H + 1)) * R0 <= fa_img2dr_lim(R0, true) && fa_img2dr_cdiv(T * P) * R1 <= fa_img2dr_lim(R1, false) &&
           fa_img2dr_cdiv(T * R0 * H) <= FA_IMG2DR_RUN_LIM && T * R0 * (R1 | 1) <= FA_IMG2D_LDS_DOUBLES;
}
constexpr int fa_img2dr_tile(int R0, int R1, bool fwd) {
    if (R0 < 2 || R1 < 2 || R0 > 32 || R1 > 32 || (R1 & 1)) return 0;
    int T = 16384 / (R0 * R1);
    while (T > 1 && !(fwd ? fa_img2dr_fwd_ok(R0, R1, T) : fa_img2dr_bwd_ok(R0, R1, T))) --T;
    return T;
}

struct Img2DRArgs {
    const double *src;
    double *dst;
    i64 nimg;                                        /* images of this launch */
    int pitch;                                       /* row pitch of the real side in doubles: R1 or R1 + 2 */
    int flags;                                       /* FFTW_AMD_F_NT_IN / NT_OUT */
};

template <int R0, int R1> struct Img2DRGeom {
    static constexpr int H = R1 / 2, M = R0 / 2 + 1;
    static constexpr int T = fa_img2dr_tile(R0, R1, true);
    static constexpr int NB1 = H * T;                /* radix-R0 butterflies per tile (packed columns) */
    static constexpr int NB2 = M * T;                /* radix-R1 butterflies per tile (rows k0 < M) */
    static constexpr int Q1 = (NB1 + 255) / 256;
    static constexpr int Q2 = (NB2 + 255) / 256;
    static constexpr int E = T * R0 * (H + 1);       /* complex results of a tile */
    static constexpr int N = (E + 255) / 256;
    static constexpr int S = R1 | 1;                 /* row stride of the exchange (doubles), odd */
    static constexpr int So = (H + 1) | 1;           /* row stride of the output transposition, odd */
    static constexpr int lds_doubles = (NB2 * S > T * R0 * So ? NB2 * S : T * R0 * So) + 16;
    static_assert(R1 % 2 == 0 && T >= 1, "img2dr: even row length");
    static_assert(Q1 * R0 <= fa_img2dr_lim(R0, true) || T == 1, "img2dr: stage 1 holds too many elements per item");
    static_assert(Q2 * R1 <= fa_img2dr_lim(R1, false) || T == 1, "img2dr: stage 2 holds too many elements per item");
    static_assert(N <= FA_IMG2DR_RUN_LIM || T == 1, "img2dr: too many run-order results per item");
    static_assert(lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16, "img2dr: the plane does not fit twice on a CU");
};

template <int R0, int R1>
__global__ void __launch_bounds__(256, 2)
img2dr_kernel(const Img2DRArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DRGeom<R0, R1> G;
    constexpr int H = G::H, M = G::M, T = G::T, NB1 = G::NB1, NB2 = G::NB2, Q1 = G::Q1, Q2 = G::Q2, E = G::E, N = G::N;
    constexpr int S = G::S, So = G::So;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nimg - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid images of this tile */
    const int pitch = a.pitch;
    const double *src = a.src + t0 * (i64)R0 * pitch;
    double *dst = a.dst + t0 * (i64)(2 * R0 * (H + 1));
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;
    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;

    /* ---- load + stage 1: butterfly g = (t, c), c fastest across lanes */
    cplx x[Q1][R0];
    int p1[Q1];                                      /* plane offset of (row t M, position 2c) */
#pragma unroll
    for (int u = 0; u < Q1; ++u) {
        int g = u * 256 + tid;
        if (NB1 % 256 != 0 && u == Q1 - 1 && g > NB1 - 1) g = NB1 - 1;
        const int t = g / H, c = g - t * H;
        p1[u] = t * (M * S) + 2 * c;
        if (t < tcur) {
            ld_run<R0>(x[u], src + (t * R0 * pitch + 2 * c), (i64)pitch, nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < R0; ++i) x[u][i] = c_make(0.0, 0.0);
        }
        RB<R0>::run(x[u]);
    }

    /* ---- exchange: the two real columns of every packed column, separated, into the rows (t, k0) */
    cplx y[Q2][R1];
    int p2[Q2];
    bool mir[Q2];                                    /* the row has a mirror row R0 - k0 */
    int pm[Q2], po[Q2];                              /* plane offsets of the output rows k0 and R0 - k0 */
#pragma unroll
    for (int v = 0; v < Q2; ++v) {
        int h = v * 256 + tid;
        if (NB2 % 256 != 0 && v == Q2 - 1 && h > NB2 - 1) h = NB2 - 1;
        const int t = h / M, k0 = h - t * M;
        p2[v] = h * S;
        mir[v] = k0 > 0 && 2 * k0 != R0;
        po[v] = (t * R0 + k0) * So;
        pm[v] = (t * R0 + (k0 > 0 ? R0 - k0 : 0)) * So;
    }
    /* in place: slot k keeps A_2c[k], slot R0 - k gets A_2c+1[k]; the self-paired slots 0 and R0 / 2 already hold
       (Re A_2c, Re A_2c+1), whose imaginary parts are 0 */
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 1; 2 * k < R0; ++k) {
            const cplx zk = x[u][RB<R0>::slot(k)], zm = x[u][RB<R0>::slot(R0 - k)];
            x[u][RB<R0>::slot(k)] = c_make(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
            x[u][RB<R0>::slot(R0 - k)] = c_make(0.5 * (zk.y + zm.y), 0.5 * (zm.x - zk.x));
        }
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const bool self = k == 0 || 2 * k == R0;
            plane[p1[u] + k * S] = x[u][RB<R0>::slot(k)].x;
            plane[p1[u] + k * S + 1] = self ? x[u][RB<R0>::slot(k)].y : x[u][RB<R0>::slot((R0 - k) % R0)].x;
        }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].x = plane[p2[v] + c];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const bool self = k == 0 || 2 * k == R0;
            plane[p1[u] + k * S] = self ? 0.0 : x[u][RB<R0>::slot(k)].y;
            plane[p1[u] + k * S + 1] = self ? 0.0 : x[u][RB<R0>::slot((R0 - k) % R0)].y;
        }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int c = 0; c < R1; ++c) y[v][c].y = plane[p2[v] + c];
    __syncthreads();

    /* ---- stage 2 */
#pragma unroll
    for (int v = 0; v < Q2; ++v) RB<R1>::run(y[v]);

    /* ---- rows -> the order of the run: result e = (t R0 + r) (H + 1) + k1 sits at row e / (H + 1), position e % (H + 1) */
#define FA_IMG2DR_LP(j) (((j) * 256 + tid > E - 1 ? E - 1 : (j) * 256 + tid) + (((j) * 256 + tid > E - 1 ? E - 1 : (j) * 256 + tid) / (H + 1)) * (So - (H + 1)))
    cplx w[N];
#pragma unroll
    for (int v = 0; v < Q2; ++v) {
#pragma unroll
        for (int k = 0; k <= H; ++k) plane[po[v] + k] = y[v][RB<R1>::slot(k)].x;
        if (mir[v]) {
#pragma unroll
            for (int k = 0; k <= H; ++k) plane[pm[v] + k] = y[v][RB<R1>::slot((R1 - k) % R1)].x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].x = plane[FA_IMG2DR_LP(j)];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v) {
#pragma unroll
        for (int k = 0; k <= H; ++k) plane[po[v] + k] = y[v][RB<R1>::slot(k)].y;
        if (mir[v]) {
#pragma unroll
            for (int k = 0; k <= H; ++k) plane[pm[v] + k] = -y[v][RB<R1>::slot((R1 - k) % R1)].y;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].y = plane[FA_IMG2DR_LP(j)];
#undef FA_IMG2DR_LP

    const int ecur = tcur * (R0 * (H + 1));          /* valid results of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        if (e < ecur) st_sel(dst + 2 * e, w[j], nt_out);
    }
}

template <int R0, int R1> struct Img2DCGeom {
    static constexpr int H = R1 / 2, P = (R0 + 1) / 2;
    static constexpr int T = fa_img2dr_tile(R0, R1, false);
    static constexpr int NBA = (H + 1) * T;          /* radix-R0 butterflies per tile (columns 0 ... H) */
    static constexpr int NBB = P * T;                /* radix-R1 butterflies per tile (row pairs) */
    static constexpr int QA = (NBA + 255) / 256;
    static constexpr int QB = (NBB + 255) / 256;
    static constexpr int E = T * R0 * H;             /* pairs of reals of a tile */
    static constexpr int N = (E + 255) / 256;
    static constexpr int Sc = (H + 1) | 1;           /* row stride of the exchange (doubles), odd */
    static constexpr int S = R1 | 1;                 /* row stride of the output transposition, odd */
    static constexpr int lds_doubles = T * R0 * S + 16;
    static_assert(R1 % 2 == 0 && T >= 1 && Sc <= S, "img2dc: even row length");
    static_assert(QA * R0 <= fa_img2dr_lim(R0, true) || T == 1, "img2dc: stage A holds too many elements per item");
    static_assert(QB * R1 <= fa_img2dr_lim(R1, false) || T == 1, "img2dc: stage B holds too many elements per item");
    static_assert(N <= FA_IMG2DR_RUN_LIM || T == 1, "img2dc: too many run-order results per item");
    static_assert(lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16, "img2dc: the plane does not fit twice on a CU");
};

template <int R0, int R1>
__global__ void __launch_bounds__(256, 2)
img2dc_kernel(const Img2DRArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DCGeom<R0, R1> G;
    constexpr int H = G::H, P = G::P, T = G::T, NBA = G::NBA, NBB = G::NBB, QA = G::QA, QB = G::QB, E = G::E, N = G::N;
    constexpr int S = G::S, Sc = G::Sc;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nimg - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid images of this tile */
    const int pitch = a.pitch;
    const double *src = a.src + t0 * (i64)(2 * R0 * (H + 1));
    double *dst = a.dst + t0 * (i64)R0 * pitch;
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;
    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;

    /* ---- load + stage A: butterfly g = (t, c), c = 0 ... H fastest across lanes; backward by the swap identity */
    cplx x[QA][R0];
    int pa[QA];                                      /* plane offset of (row t R0, position c) */
#pragma unroll
    for (int u = 0; u < QA; ++u) {
        int g = u * 256 + tid;
        if (NBA % 256 != 0 && u == QA - 1 && g > NBA - 1) g = NBA - 1;
        const int t = g / (H + 1), c = g - t * (H + 1);
        pa[u] = t * (R0 * Sc) + c;
        if (t < tcur) {
            ld_run<R0>(x[u], src + 2 * (t * (R0 * (H + 1)) + c), (i64)(2 * (H + 1)), nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < R0; ++i) x[u][i] = c_make(0.0, 0.0);
        }
#pragma unroll
        for (int i = 0; i < R0; ++i) { const double s = x[u][i].x; x[u][i].x = x[u][i].y; x[u][i].y = s; }
        RB<R0>::run(x[u]);                           /* the result r is (x[slot(r)].y, x[slot(r)].x) */
    }

    /* ---- exchange: columns -> pairs of rows; W = Y_r + i Y_r' built while the two planes are read */
    cplx y[QB][R1];
    int pb[QB], pq[QB], pw[QB];                      /* exchange rows r and r', output row r */
    bool two[QB];                                    /* the pair has a second row */
#pragma unroll
    for (int v = 0; v < QB; ++v) {
        int h = v * 256 + tid;
        if (NBB % 256 != 0 && v == QB - 1 && h > NBB - 1) h = NBB - 1;
        const int t = h / P, q = h - t * P;
        two[v] = 2 * q + 1 < R0;
        pb[v] = (t * R0 + 2 * q) * Sc;
        pq[v] = two[v] ? pb[v] + Sc : pb[v];
        pw[v] = (t * R0 + 2 * q) * S;
    }
#pragma unroll
    for (int u = 0; u < QA; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[pa[u] + k * Sc] = x[u][RB<R0>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QB; ++v)
#pragma unroll
        for (int c = 0; c <= H; ++c) {
            const double ar = plane[pb[v] + c], br = two[v] ? plane[pq[v] + c] : 0.0;
            y[v][c] = c_make(ar, br);
            if (c > 0 && c < H) y[v][R1 - c] = c_make(ar, br);
        }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < QA; ++u)
#pragma unroll
        for (int k = 0; k < R0; ++k) plane[pa[u] + k * Sc] = x[u][RB<R0>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QB; ++v)
#pragma unroll
        for (int c = 1; c < H; ++c) {                /* the imaginary parts of the entries 0 and H are dropped */
            const double ai = plane[pb[v] + c], bi = two[v] ? plane[pq[v] + c] : 0.0;
            y[v][c].x -= bi;
            y[v][c].y += ai;
            y[v][R1 - c].x += bi;
            y[v][R1 - c].y -= ai;
        }
    __syncthreads();

    /* ---- stage B, backward by the swap identity: row r leaves in the .y parts, row r' in the .x parts */
#pragma unroll
    for (int v = 0; v < QB; ++v) {
#pragma unroll
        for (int i = 0; i < R1; ++i) { const double s = y[v][i].x; y[v][i].x = y[v][i].y; y[v][i].y = s; }
        RB<R1>::run(y[v]);
    }

    /* ---- rows -> the order of the run: pair e = (t R0 + r) H + c sits at row e / H, positions 2c and 2c + 1 */
#pragma unroll
    for (int v = 0; v < QB; ++v) {
#pragma unroll
        for (int k = 0; k < R1; ++k) plane[pw[v] + k] = y[v][RB<R1>::slot(k)].y;
        if (two[v]) {
#pragma unroll
            for (int k = 0; k < R1; ++k) plane[pw[v] + S + k] = y[v][RB<R1>::slot(k)].x;
        }
    }
    __syncthreads();
    const int ecur = tcur * (R0 * H);                /* valid pairs of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        const int ec = e > E - 1 ? E - 1 : e;
        const int row = ec / H, c = ec - row * H;
        const cplx o = c_make(plane[row * S + 2 * c], plane[row * S + 2 * c + 1]);
        if (e < ecur) st_sel(dst + (row * pitch + 2 * c), o, nt_out);
    }
}

#endif /* FA_PASS2DR_HPP */
