/*
 * pass2dw.hpp -- one-trip 2-D transform of contiguous images with an extent of 128: 128 x 128, 64 x 128 and 128 x 64,
 * a tile of E = 16384 elements (one 128 x 128 image, or T = 2 images of the other pairs) per workgroup of 512
 * work-items, 32 elements per item, one workgroup per CU (the tile's 256 KiB fill half of the CU's register file, as
 * the 16384-point row of pass3w.hpp does; one real plane of 129 KiB goes through the LDS at a time).  The stage
 * structure is that of pass2dl.hpp, whose exchange and whose conventions it takes over: an axis of R = A B points is
 * two register stages (radix-A butterflies over l = a + B i, conj(w_R^(a d)), radix-B butterflies over a, output
 * k = d + A c), 128 = 16 x 8 and 64 = 8 x 8, and no twiddles run between the two axes:
 *
 *   C1  butterfly (image t, residue a0, column c): radix A0 down the column over rows a0 + B0 i, loaded from global
 *       memory; times conj(w_R0^(a0 d))
 *   exchange 1
 *   C2  butterfly (t, d, c): radix B0 over a0; output row k0 = d + A0 c'
 *   exchange 2
 *   R1  butterfly (row rho = t R0 + k0, residue a1): radix A1 along the row over positions a1 + B1 i; times
 *       conj(w_R1^(a1 d))
 *   exchange 3
 *   R2  butterfly (rho, d): radix B1 over a1; output position k1 = d + A1 c'
 *   transposition through the same plane into the order of the run, stored to global memory
 *
 * Every stage has E / radix butterflies, a multiple of 512: 32 / radix butterflies per item, none beyond the tile.
 *
 * The twiddles w_n^(a d), d < A, are products over the bits of d (TwTreeR, passrr.hpp) of the entries a 2^s of the
 * host-generated stage table of the axis ((cos, sin)(2 pi m / n), hostmath.c; a 2^s <= (B - 1) A / 2 < n): three or
 * four 16-byte loads per butterfly from a table of at most 2 KiB.
 *
 * 128 = 16 x 8 and not 8 x 16: both orders compile without a spill (profiles/img2dw_codeobj.txt, which records the
 * register counts of both); FA_IMG2DW_A128 is the first-stage radix.
 *
 * Global access: that of pass2dl.hpp.  The T images of a tile are ONE contiguous run of 16384 elements (256 KiB) on
 *   both sides.  Loads are in the natural order of C1: lane (t, a0, c), c fastest, reads row a0 + B0 i of its column
 *   in instruction i, so a wave instruction moves 64 consecutive elements of one image row (1 KiB).  The results pass
 *   through the plane once more and leave in the order of the run: item tid stores elements j 512 + tid, every wave
 *   store one contiguous 1 KiB piece.
 *
 * LDS layout.  One plane of doubles (real parts, then imaginary parts, every exchange), the tile as rows
 * rho = t R0 + r of S = R1 | 1 doubles, position p inside: address rho S + p; 128 x 129 or 256 x 65 doubles, 129 or
 * 130 KiB.  The bank analysis of pass2dl.hpp carries over with 512 lanes (reads ds_read_b64: groups of 32 lanes, 32
 * eight-byte banks; writes ds_write_b64: groups of 16 lanes, 16 eight-byte banks), and every "at most two-way" of
 * that header becomes conflict free, because the extents here are multiples of the groups:
 *   - exchange 1 (C1 writes rows a0 + B0 d, C2 reads rows B0 d + a0, both at position c with c fastest across
 *     lanes) and exchange 2, write side (C2 writes row d + A0 c' at position c): a group of 32 (16) lanes holds
 *     consecutive c of ONE row (R1 = 64 or 128 is a multiple of 32), consecutive doubles: conflict free;
 *   - exchange 2, read side, and exchange 3, both sides (R1 reads and writes positions a1 + B1 i of its row, R2 reads
 *     positions B1 d + a1): the lanes run over the rows, rho fastest (butterfly index a1 NR + rho, NR = T R0 = 128 or
 *     256 rows), so lane to lane the address moves by S doubles, and an odd S (129, 65) walks all 32 (16) banks
 *     before it repeats; NR is a multiple of 32, so no group crosses from one residue to the next: conflict free
 *     whatever the position is;
 *   - the last write (R2 writes positions d + A1 c'): rho fastest, as above;
 *   - the run-order reads at the end (element e at e + e / R1): a group of 32 lanes holds 32 consecutive elements of
 *     one row, consecutive doubles: conflict free.
 *
 * Partial tiles (T = 2 only): only the global accesses are predicated (an image beyond the batch loads as zeros and
 * is not stored); there is no predicate around LDS traffic.
 *
 * Backward transforms use the (re, im) swap identity; BWD is a template parameter (register renaming), and so is the
 * nontemporal store NT_OUT: as run-time branches around the 32 stores such choices cost pass3w.hpp and pass3q.hpp
 * spilled registers.  FFTW_AMD_F_NT_IN stays a run-time flag (ld_run: one scalar branch per butterfly).
 */
#ifndef FA_PASS2DW_HPP
#define FA_PASS2DW_HPP

#ifndef FA_IMG2DW_A128
#define FA_IMG2DW_A128 16
#endif
#define FA_IMG2DW_ITEMS 512
#define FA_IMG2DW_ELEMS 16384

/* the split of an axis: first-stage radix A, second-stage radix B */
constexpr int fa_img2dw_a(int n) { return n == 128 ? FA_IMG2DW_A128 : 8; }
constexpr int fa_img2dw_b(int n) { return n / fa_img2dw_a(n); }
/* images per tile: 128 x 128 one, 64 x 128 and 128 x 64 two; 0: not a size of this kernel */
constexpr int fa_img2dw_tile(int R0, int R1) {
    return ((R0 == 64 || R0 == 128) && (R1 == 64 || R1 == 128) && (R0 == 128 || R1 == 128)) ? FA_IMG2DW_ELEMS / (R0 * R1) : 0;
}

template <int R0_, int R1_> struct Img2DWGeom {
    static constexpr int R0 = R0_, R1 = R1_, NT = FA_IMG2DW_ITEMS;
    static constexpr int A0 = fa_img2dw_a(R0), B0 = fa_img2dw_b(R0), A1 = fa_img2dw_a(R1), B1 = fa_img2dw_b(R1);
    static constexpr int T = fa_img2dw_tile(R0, R1);
    static constexpr int E = T * R0 * R1;            /* elements of a tile */
    static constexpr int NR = T * R0;                /* rows of the plane */
    static constexpr int S = R1 | 1;                 /* row stride (doubles), odd */
    static constexpr int QC1 = E / A0 / NT, QC2 = E / B0 / NT, QR1 = E / A1 / NT, QR2 = E / B1 / NT;
    static constexpr int N = E / NT;                 /* elements per item in the order of the run */
    static constexpr int lds_doubles = NR * S + 16;
    static_assert(T >= 1 && E == FA_IMG2DW_ELEMS, "img2dw: not a size of this kernel");
    static_assert(A0 * B0 == R0 && A1 * B1 == R1 && QC1 * A0 == N && QC2 * B0 == N && QR1 * A1 == N && QR2 * B1 == N,
                  "img2dw: every stage holds 32 elements per item");
    static_assert(NR % 32 == 0 && R1 % 32 == 0, "img2dw: the bank analysis needs whole groups per row and per residue");
    static_assert(lds_doubles * 8 <= 160 * 1024, "img2dw: the plane does not fit the LDS of a CU");
};

/* x[d] *= conj(w^(a d)), d = 1 ... R - 1 (R a power of two whose butterfly leaves its outputs in order) */
template <int R> FA_DEV void img2dw_twiddle(cplx *x, const cplx *tw, int a) {
    static_assert((R & (R - 1)) == 0 && RB<R>::slot(R - 1) == R - 1, "img2dw: radix 8 or 16");
    cplx pw[RB<R>::bits];
#pragma unroll
    for (int s = 0; s < RB<R>::bits; ++s) pw[s] = tw[a << s];
    TwTreeR<R, RB<R>::bits - 1, 0, false, true>::run(x, pw, c_make(1.0, 0.0));
}

/* the Img2DLArgs of pass2dl.hpp: src, dst, tw0 (column axis), tw1 (row axis), nimg, flags (FFTW_AMD_F_NT_IN only) */
template <int R0, int R1, bool BWD, bool NT_OUT>
__global__ void __launch_bounds__(FA_IMG2DW_ITEMS, 1)
img2dw_kernel(const Img2DLArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DWGeom<R0, R1> G;
    constexpr int T = G::T, NT = G::NT, NR = G::NR, S = G::S, N = G::N;
    constexpr int A0 = G::A0, B0 = G::B0, A1 = G::A1, B1 = G::B1;
    constexpr int QC1 = G::QC1, QC2 = G::QC2, QR1 = G::QR1, QR2 = G::QR2;
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
        const int g = u * NT + tid;
        const int t = g / (B0 * R1), r = g - t * (B0 * R1);
        const int a0 = r / R1, c = r - a0 * R1;
        wa[u] = (t * R0 + a0) * S + c;
        if (T == 1 || t < tcur) {
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
        img2dw_twiddle<A0>(xa[u], a.tw0, a0);
    }

    /* ---- exchange 1 + C2: butterfly h = (t, d, c) over the rows B0 d + a0, output rows d + A0 c' */
    cplx xb[QC2][B0];
    int rb[QC2], wb[QC2];
#pragma unroll
    for (int v = 0; v < QC2; ++v) {
        const int h = v * NT + tid;
        const int t = h / (A0 * R1), r = h - t * (A0 * R1);
        const int d = r / R1, c = r - d * R1;
        rb[v] = (t * R0 + B0 * d) * S + c;
        wb[v] = (t * R0 + d) * S + c;
    }
    img2dl_xchg<B0 * S, S>(plane, xa, wa, xb, rb);
#pragma unroll
    for (int v = 0; v < QC2; ++v) RB<B0>::run(xb[v]);

    /* ---- exchange 2 + R1: butterfly (a1, rho), rho fastest, over the positions a1 + B1 i of row rho */
    cplx xc[QR1][A1];
    int pc[QR1], ac[QR1];                            /* plane offset of (row rho, position a1), the residue a1 */
#pragma unroll
    for (int u = 0; u < QR1; ++u) {
        const int g = u * NT + tid;
        ac[u] = g / NR;
        pc[u] = (g - ac[u] * NR) * S + ac[u];
    }
    img2dl_xchg<A0 * S, B1>(plane, xb, wb, xc, pc);
#pragma unroll
    for (int u = 0; u < QR1; ++u) {
        RB<A1>::run(xc[u]);
        img2dw_twiddle<A1>(xc[u], a.tw1, ac[u]);
    }

    /* ---- exchange 3 + R2: butterfly (d, rho), rho fastest, over the positions B1 d + a1; output d + A1 c' */
    cplx xd[QR2][B1];
    int rd[QR2], wd[QR2];
#pragma unroll
    for (int v = 0; v < QR2; ++v) {
        const int h = v * NT + tid;
        const int d = h / NR, rho = h - d * NR;
        rd[v] = rho * S + B1 * d;
        wd[v] = rho * S + d;
    }
    img2dl_xchg<B1, 1>(plane, xc, pc, xd, rd);
#pragma unroll
    for (int v = 0; v < QR2; ++v) RB<B1>::run(xd[v]);

    /* ---- rows of the plane -> the order of the run -> global memory: element e = j 512 + tid = rho R1 + k1 sits at
       row e / R1, position e % R1, which is lp0 + j (512 + 512 / R1 (S - R1)) */
    const int lp0 = tid + (tid / R1) * (S - R1);
    constexpr int LPJ = NT + (NT / R1) * (S - R1);
    cplx w[N];
#pragma unroll
    for (int v = 0; v < QR2; ++v)
#pragma unroll
        for (int k = 0; k < B1; ++k) plane[wd[v] + k * A1] = xd[v][RB<B1>::slot(k)].x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].x = plane[lp0 + j * LPJ];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < QR2; ++v)
#pragma unroll
        for (int k = 0; k < B1; ++k) plane[wd[v] + k * A1] = xd[v][RB<B1>::slot(k)].y;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) w[j].y = plane[lp0 + j * LPJ];

    const int ecur = tcur * (R0 * R1);               /* valid elements of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * NT + tid;
        const cplx o = BWD ? c_make(w[j].y, w[j].x) : w[j];
        if (T == 1 || e < ecur) st_cplx<NT_OUT>(dst + 2 * e, o);
    }
}

#endif /* FA_PASS2DW_HPP */
