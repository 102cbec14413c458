/*
 * pass2dl.hpp -- one-trip 2-D transform of contiguous images with an extent above 32: T whole images of
 * R0 = A0 B0 rows x R1 = A1 B1 columns per workgroup (extents 16, 32, 40, 48, 64; at least one above 32), both axes
 * in registers.  The companion of pass2d.hpp, whose axes are one register butterfly each; here an axis of 40, 48 or
 * 64 points is two register stages A x B = 8 x 5, 8 x 6, 8 x 8 (the Cooley-Tukey node of passrr.hpp: radix-A
 * butterflies over l = a + B i, conj(w_n^(a d)), radix-B butterflies over a, output k = d + A c), and an axis of at
 * most 32 points is one butterfly (B = 1), so that 64 x 32 and 32 x 64 come out of the same source:
 *
 *   C1  butterfly (image t, residue a0, column c): radix A0 down the column over rows a0 + B0 i, loaded from global
 *       memory; times conj(w_R0^(a0 d))                                                      [B0 > 1]
 *   exchange 1                                                                                [B0 > 1]
 *   C2  butterfly (t, d, c): radix B0 over a0; output row k0 = d + A0 c'                      [B0 > 1]
 *   exchange 2
 *   R1  butterfly (row rho = t R0 + k0, residue a1): radix A1 along the row over positions a1 + B1 i; times
 *       conj(w_R1^(a1 d))                                                                     [B1 > 1]
 *   exchange 3                                                                                [B1 > 1]
 *   R2  butterfly (rho, d): radix B1 over a1; output position k1 = d + A1 c'                  [B1 > 1]
 *   transposition through the same plane into the order of the run, stored to global memory
 *
 * The twiddles w_n^(a d) are entries of the host-generated stage tables of the two axes ((cos, sin)(2 pi m / n),
 * hostmath.c), indexed a d < n: one 16-byte load per element from a table of at most 1 KiB.
 *
 * Global access: that of pass2d.hpp.  The T images of a tile are ONE contiguous run of E = T R0 R1 elements on both
 *   sides.  Loads are in the natural order of C1: lane (t, a0, c), c fastest, reads row a0 + B0 i of its column in
 *   instruction i, so a wave instruction moves whole image rows (runs of R1 x 16 bytes; the rows in between belong
 *   to the neighbouring residues a0, i.e. to the neighbouring waves of the same instruction).  The results pass
 *   through the plane once more and leave in the order of the run: item tid stores elements j 256 + tid, every wave
 *   store one contiguous 1 KiB piece.
 *
 * LDS layout.  One plane of doubles (real parts, then imaginary parts, every exchange), the tile as rows
 * rho = t R0 + r of S = R1 | 1 doubles, position p inside: address rho S + p.  Reads are ds_read_b64 (groups of 32
 * lanes, 32 eight-byte banks), writes ds_write_b64 (groups of 16 lanes, 16 eight-byte banks):
 *   - exchange 1 (C1 writes rows a0 + B0 d, C2 reads rows B0 d + a0, both at position c with c fastest across
 *     lanes): consecutive doubles inside an image row on both sides, conflict free; where R1 is no multiple of the
 *     group (40, 48) a group crosses from one row block into another once, at most two-way;
 *   - exchange 2, write side (C2, or C1 when B0 = 1, writes row d + A0 c' at position c, c fastest): the same;
 *   - exchange 2, read side, and exchange 3, both sides (R1 reads and writes positions a1 + B1 i of its row, R2
 *     reads positions B1 d + a1): the lanes run over the rows, rho fastest (butterfly index a1 NR + rho, NR = T R0
 *     rows), so lane to lane the address moves by S doubles, and an odd S walks all 32 (16) banks before it repeats:
 *     conflict free whatever the position is; a group that crosses from residue a1 to a1 + 1 (NR = 144, 192, 200 are
 *     no multiples of 32) restarts at row 0 one position further, at most two-way.  With the residue fastest
 *     instead (8 residues x 8 rows per wave) S = 65 would put lane (rho, a1) on bank rho + a1 + 8 i: eight-way;
 *   - the last write (R2 writes positions d + A1 c', or R1 the positions of a one-stage row): rho fastest, as above;
 *   - the run-order reads at the end are consecutive doubles with one skipped per row: at most two-way.
 * The plane is at most FA_IMG2D_LDS_DOUBLES (72 KiB), so two workgroups fit a CU.
 *
 * Partial tiles: only the global accesses are predicated (images beyond the batch load as zeros and are not
 * stored).  Where a stage's butterfly count is no multiple of 256, an item whose butterfly lies beyond the tile
 * redoes the last valid one (same values to the same LDS words), which is why every exchange ends with a barrier
 * even where a butterfly writes the positions it has read: there is no predicate around LDS traffic.
 *
 * Backward transforms use the (re, im) swap identity; BWD is a template parameter (register renaming).
 */
#ifndef FA_PASS2DL_HPP
#define FA_PASS2DL_HPP

/* the split of an axis: first-stage radix A, second-stage radix B (1: the axis is one butterfly) */
constexpr int fa_img2dl_a(int n) { return n > 32 ? 8 : n; }
constexpr int fa_img2dl_b(int n) { return n > 32 ? n / 8 : 1; }
constexpr bool fa_img2dl_extent(int n) { return n == 16 || n == 32 || n == 40 || n == 48 || n == 64; }

/* elements an item may hold in a stage of radix R: 32 for the powers of two, FA_IMG2DL_ODD_LIM for the radix-5 and
   radix-6 butterflies.  35 = seven radix-5 butterflies is what 40 x 40 needs for T = 5 (1600 butterflies), and it
   compiles without a spill (profiles/img2dl_codeobj.txt); every other pair stays at 30 or below */
#ifndef FA_IMG2DL_ODD_LIM
#define FA_IMG2DL_ODD_LIM 35
#endif
constexpr int fa_img2dl_lim(int R) { return ((R & (R - 1)) == 0) ? 32 : FA_IMG2DL_ODD_LIM; }
/* does a stage of nb butterflies of radix R stay within the limit? (B = 1: no such stage) */
constexpr bool fa_img2dl_stage_ok(int nb, int R) { return R == 1 || ((nb + 255) / 256) * R <= fa_img2dl_lim(R); }
/* images per tile: as many as fit 8192 elements, the per-item limits of the four stages and the plane */
constexpr int fa_img2dl_tile(int R0, int R1) {
    if (!fa_img2dl_extent(R0) || !fa_img2dl_extent(R1) || (R0 <= 32 && R1 <= 32)) return 0;
    const int A0 = fa_img2dl_a(R0), B0 = fa_img2dl_b(R0), A1 = fa_img2dl_a(R1), B1 = fa_img2dl_b(R1);
    int T = 8192 / (R0 * R1);
    while (T > 1 && !(fa_img2dl_stage_ok(T * B0 * R1, A0) && fa_img2dl_stage_ok(T * A0 * R1, B0) &&
                      fa_img2dl_stage_ok(T * R0 * B1, A1) && fa_img2dl_stage_ok(T * R0 * A1, B1) &&
                      T * R0 * (R1 | 1) <= FA_IMG2D_LDS_DOUBLES)) --T;
    return T;
}

template <int R0_, int R1_> struct Img2DLGeom {
    static constexpr int R0 = R0_, R1 = R1_;
    static constexpr int A0 = fa_img2dl_a(R0), B0 = fa_img2dl_b(R0), A1 = fa_img2dl_a(R1), B1 = fa_img2dl_b(R1);
    static constexpr int T = fa_img2dl_tile(R0, R1);
    static constexpr int E = T * R0 * R1;            /* elements of a tile */
    static constexpr int NR = T * R0;                /* rows of the plane */
    static constexpr int S = R1 | 1;                 /* row stride (doubles), odd */
    static constexpr int NC1 = T * B0 * R1;          /* radix-A0 butterflies per tile */
    static constexpr int NC2 = T * A0 * R1;          /* radix-B0 butterflies */
    static constexpr int NR1 = NR * B1;              /* radix-A1 butterflies */
    static constexpr int NR2 = NR * A1;              /* radix-B1 butterflies */
    static constexpr int QC1 = (NC1 + 255) / 256, QC2 = (NC2 + 255) / 256;
    static constexpr int QR1 = (NR1 + 255) / 256, QR2 = (NR2 + 255) / 256;
    static constexpr int N = (E + 255) / 256;        /* elements per item in the order of the run */
    static constexpr int lds_doubles = NR * S + 16;
    static_assert(T >= 1 && E <= 8192, "img2dl: not a size of this kernel");
    static_assert(NR * S <= FA_IMG2D_LDS_DOUBLES, "img2dl: the plane does not fit twice on a CU");
    static_assert(fa_img2dl_stage_ok(NC1, A0) && fa_img2dl_stage_ok(NC2, B0) && fa_img2dl_stage_ok(NR1, A1) &&
                  fa_img2dl_stage_ok(NR2, B1), "img2dl: a stage holds more elements per item than fa_img2dl_lim allows");
};

struct Img2DLArgs {
    const double *src;
    double *dst;
    const cplx *tw0;                                 /* stage table of the column axis, R0 entries (B0 > 1) */
    const cplx *tw1;                                 /* stage table of the row axis, R1 entries (B1 > 1) */
    i64 nimg;                                        /* images of this launch */
    int flags;                                       /* FFTW_AMD_F_NT_IN / NT_OUT (the swap is the BWD parameter) */
};

/* butterfly u 256 + tid of a stage of NB butterflies, Q per item; beyond the tile: the last valid one */
template <int NB, int Q> FA_DEV int img2dl_bfly(int u, int tid) {
    int g = u * 256 + tid;
    if (NB % 256 != 0 && u == Q - 1 && g > NB - 1) g = NB - 1;
    return g;
}

/* One exchange: output k of butterfly u goes to plane[wb[u] + k WSTEP], input j of butterfly v comes from
   plane[rb[v] + j RSTEP]; real parts, then imaginary parts.  The plane is free again on return. */
template <int WSTEP, int RSTEP, int Q1, int RA, int Q2, int RB_>
FA_DEV void img2dl_xchg(double *plane, const cplx (&x)[Q1][RA], const int (&wb)[Q1], cplx (&y)[Q2][RB_], const int (&rb)[Q2]) {
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < RA; ++k) plane[wb[u] + k * WSTEP] = x[u][RB<RA>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int j = 0; j < RB_; ++j) y[v][j].x = plane[rb[v] + j * RSTEP];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Q1; ++u)
#pragma unroll
        for (int k = 0; k < RA; ++k) plane[wb[u] + k * WSTEP] = x[u][RB<RA>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q2; ++v)
#pragma unroll
        for (int j = 0; j < RB_; ++j) y[v][j].y = plane[rb[v] + j * RSTEP];
    __syncthreads();
}

/* x[slot(d)] *= conj(w^(a d)), d = 1 ... R - 1, from the stage table of the axis */
template <int R> FA_DEV void img2dl_twiddle(cplx *x, const cplx *tw, int a) {
#pragma unroll
    for (int d = 1; d < R; ++d) x[RB<R>::slot(d)] = c_mulc(x[RB<R>::slot(d)], tw[a * d]);
}

/* rows of the plane -> the order of the run -> global memory; output k of butterfly v sits at wb[v] + k WSTEP */
template <class G, bool BWD, int WSTEP, int Q, int R>
FA_DEV void img2dl_store(const Img2DLArgs &a, double *plane, const cplx (&y)[Q][R], const int (&wb)[Q], double *dst,
                         const int tcur, const int tid) {
    constexpr int E = G::E, N = G::N, S = G::S, R1 = G::R1;
    /* element e = rho R1 + k1 sits at row e / R1, position e % R1 */
    int lp[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int e = j * 256 + tid;
        if (E % 256 != 0 && j == N - 1 && e > E - 1) e = E - 1;
        lp[j] = e + (e / R1) * (S - R1);
    }
    cplx w[N];
#pragma unroll
    for (int v = 0; v < Q; ++v)
#pragma unroll
        for (int k = 0; k < R; ++k) plane[wb[v] + k * WSTEP] = y[v][RB<R>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].x = plane[lp[j]];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < Q; ++v)
#pragma unroll
        for (int k = 0; k < R; ++k) plane[wb[v] + k * WSTEP] = y[v][RB<R>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].y = plane[lp[j]];

    const bool nt_out = (a.flags & FFTW_AMD_F_NT_OUT) != 0;
    const int ecur = tcur * (G::R0 * R1);            /* valid elements of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        const cplx o = BWD ? c_make(w[j].y, w[j].x) : w[j];
        if (e < ecur) st_sel(dst + 2 * e, o, nt_out);
    }
}

/* the row axis: the column results (output k of butterfly u at wp[u] + k WSTEP) through exchange 2 into R1, R2 */
template <class G, bool BWD, int WSTEP, int QP, int RP>
FA_DEV void img2dl_rows(const Img2DLArgs &a, double *plane, const cplx (&xp)[QP][RP], const int (&wp)[QP], double *dst,
                        const int tcur, const int tid) {
    constexpr int A1 = G::A1, B1 = G::B1, NR = G::NR, S = G::S, QR1 = G::QR1, QR2 = G::QR2;
    cplx xc[QR1][A1];
    int pc[QR1], ac[QR1];                            /* plane offset of (row rho, position a1), the residue a1 */
#pragma unroll
    for (int u = 0; u < QR1; ++u) {
        const int g = img2dl_bfly<G::NR1, QR1>(u, tid);
        ac[u] = g / NR;
        pc[u] = (g - ac[u] * NR) * S + ac[u];
    }
    img2dl_xchg<WSTEP, B1>(plane, xp, wp, xc, pc);
#pragma unroll
    for (int u = 0; u < QR1; ++u) {
        RB<A1>::run(xc[u]);
        if (B1 > 1) img2dl_twiddle<A1>(xc[u], a.tw1, ac[u]);
    }
    if constexpr (B1 > 1) {
        cplx xd[QR2][B1];
        int rd[QR2], wd[QR2];
#pragma unroll
        for (int v = 0; v < QR2; ++v) {
            const int h = img2dl_bfly<G::NR2, QR2>(v, tid);
            const int d = h / NR, rho = h - d * NR;
            rd[v] = rho * S + B1 * d;
            wd[v] = rho * S + d;
        }
        img2dl_xchg<B1, 1>(plane, xc, pc, xd, rd);
#pragma unroll
        for (int v = 0; v < QR2; ++v) RB<B1>::run(xd[v]);
        img2dl_store<G, BWD, A1>(a, plane, xd, wd, dst, tcur, tid);
    } else {
        img2dl_store<G, BWD, 1>(a, plane, xc, pc, dst, tcur, tid);
    }
}

template <int R0, int R1, bool BWD>
__global__ void __launch_bounds__(256, 2)
img2dl_kernel(const Img2DLArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DLGeom<R0, R1> G;
    constexpr int T = G::T, A0 = G::A0, B0 = G::B0, S = G::S, QC1 = G::QC1, QC2 = G::QC2;
    const int tid = threadIdx.x;

    const i64 tile = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x);
    const i64 t0 = tile * T;
    const i64 left = a.nimg - t0;
    const int tcur = (int)(left < T ? left : T);     /* valid images of this tile */
    const double *src = a.src + t0 * (i64)(2 * R0 * R1);
    double *dst = a.dst + t0 * (i64)(2 * R0 * R1);
    const bool nt_in = (a.flags & FFTW_AMD_F_NT_IN) != 0;

    /* ---- load + C1: butterfly g = (t, a0, c), c fastest across lanes */
    cplx xa[QC1][A0];
    int wa[QC1];                                     /* plane offset of (row t R0 + a0, position c) */
#pragma unroll
    for (int u = 0; u < QC1; ++u) {
        const int g = img2dl_bfly<G::NC1, QC1>(u, tid);
        const int t = g / (B0 * R1), r = g - t * (B0 * R1);
        const int a0 = r / R1, c = r - a0 * R1;
        wa[u] = (t * R0 + a0) * S + c;
        if (t < tcur) {
            ld_run<A0>(xa[u], src + 2 * ((t * R0 + a0) * R1 + c), (i64)(2 * R1 * B0), nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < A0; ++i) xa[u][i] = c_make(0.0, 0.0);
        }
        if (BWD) {
#pragma unroll
            for (int i = 0; i < A0; ++i) { const double s = xa[u][i].x; xa[u][i].x = xa[u][i].y; xa[u][i].y = s; }
        }
        RB<A0>::run(xa[u]);
        if (B0 > 1) img2dl_twiddle<A0>(xa[u], a.tw0, a0);
    }

    if constexpr (B0 > 1) {
        /* ---- exchange 1 + C2: butterfly h = (t, d, c) over the rows B0 d + a0, output rows d + A0 c' */
        cplx xb[QC2][B0];
        int rb[QC2], wb[QC2];
#pragma unroll
        for (int v = 0; v < QC2; ++v) {
            const int h = img2dl_bfly<G::NC2, QC2>(v, tid);
            const int t = h / (A0 * R1), r = h - t * (A0 * R1);
            const int d = r / R1, c = r - d * R1;
            rb[v] = (t * R0 + B0 * d) * S + c;
            wb[v] = (t * R0 + d) * S + c;
        }
        img2dl_xchg<B0 * S, S>(plane, xa, wa, xb, rb);
#pragma unroll
        for (int v = 0; v < QC2; ++v) RB<B0>::run(xb[v]);
        img2dl_rows<G, BWD, A0 * S>(a, plane, xb, wb, dst, tcur, tid);
    } else {
        img2dl_rows<G, BWD, S>(a, plane, xa, wa, dst, tcur, tid);
    }
}

#endif /* FA_PASS2DL_HPP */
