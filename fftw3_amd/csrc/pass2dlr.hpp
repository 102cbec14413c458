/*
 * pass2dlr.hpp -- one-trip 2-D r2c and c2r transforms of real images with an extent above 32: T whole images of R0
 * rows x R1 real columns per workgroup (extents 16, 32, 40, 48, 64; at least one above 32), both axes in registers.
 * The real twins of pass2dl.hpp, with the conventions of pass2dr.hpp.  Below H = R1 / 2 (8, 16, 20, 24 or 32: the
 * real axis is always ONE butterfly RB<H>), R0 = A0 B0 as in pass2dl.hpp (an axis of 40, 48 or 64 points is two
 * register stages 8 x 5, 8 x 6, 8 x 8; an axis of at most 32 points is one butterfly, B0 = 1).
 *
 * Both kernels start with the column node of pass2dl.hpp (img2dlr_cols) on an image of R0 rows x W complex columns:
 *   C1  butterfly (image t, residue a0, column c): radix A0 down the column over rows a0 + B0 i, loaded from global
 *       memory (16-byte pairs, c fastest across lanes); times conj(w_R0^(a0 d))             [B0 > 1]
 *   exchange 1, C2 butterfly (t, d, c): radix B0 over a0; output row k0 = d + A0 c'          [B0 > 1]
 *   exchange 2 to the row items: item rho = t R0 + r reads the W entries of its row
 * The plane of the exchanges has rows rho of SX = W | 1 doubles (real parts, then imaginary parts, as in
 * pass2dl.hpp: c fastest on the column side, rho fastest on the row side, SX odd).
 *
 * r2c (img2dlr_kernel), W = H.  The real image x[r][n] is read as the packed complex image z[r][c] = x[r][2c] +
 *   i x[r][2c+1] at the real row pitch.  Columns, then one RB<H> per row: Z2 = the 2-D DFT of z.  Z2 goes back into
 *   the plane, real parts in its lower half and imaginary parts in its upper half (2 T R0 SX doubles, one barrier),
 *   and the untangle is folded into the transposition to the order of the run: result e = (t R0 + k0) (H + 1) + k1
 *   reads a = Z2[k0][k1 mod H] and b = Z2[(R0 - k0) mod R0][(H - k1) mod H] and is
 *                   E + conj(w_R1^k1) O,   E = (a + conj b) / 2,   O = (a - conj b) / 2i,
 *   w_R1^k1 entry k1 <= H of the stage table of the row axis.  Nothing is held across a barrier in this pass, so its
 *   register cost is the N results of an item; they are stored as contiguous 1 KiB pieces per wave instruction.
 *
 * c2r (img2dlc_kernel), W = H + 1.  The definition of pass2dr.hpp: the backward DFT of length R0 down each of the
 *   H + 1 columns, then the 1-D c2r of length R1 along each row, which reads the imaginary parts of its entries 0 and
 *   H as 0 -- also for half spectra that are not Hermitian.  Columns backward (the swap identity), then the row item
 *   holds Y[r][0 ... H], tangles them in place to the packed spectrum of length H,
 *                   Zp[k] = (Y[k] + conj Y[H-k]) + i w_R1^k (Y[k] - conj Y[H-k]),   w_R1^(H-k) = -conj w_R1^k,
 *   (Zp[0] = (Re Y[0] + Re Y[H]) + i (Re Y[0] - Re Y[H])), one backward RB<H> gives x[r][2c] + i x[r][2c+1], and
 *   the rows pass through the plane -- rows rho of S = R1 | 1 doubles, one trip since the values are real -- into
 *   the order of the run of the real images, stored as 16-byte pairs (the padding of padded rows is not written).
 *
 * Layout: that of pass2dr.hpp.  The complex row pitch is R1 + 2 doubles, the real row pitch a kernel argument, R1 or
 * R1 + 2.  A tile is one contiguous run on both sides that no other workgroup touches, and every global load of a
 * workgroup (the table entries included) precedes its first global store, so the transforms work in place on padded
 * rows.  Partial tiles: only the global accesses are predicated; an item whose butterfly lies beyond the tile redoes
 * the last valid one.  No sincos on the device: every twiddle is an entry of a host stage table.
 *
 * MEASURED (tools/perf/perf_img2dlr.py, profiles/img2dlr.txt; 1 GiB of real data per batch, one read + one write): r2c
 * 4.5 ... 5.3 TB/s, c2r 4.6 ... 5.7 TB/s over the 21 pairs, 5.1 ... 21.7 x the axis-by-axis plans.
 */
#ifndef FA_PASS2DLR_HPP
#define FA_PASS2DLR_HPP

/* run-order results (16 bytes each: a complex result or a pair of reals) an item may hold */
#define FA_IMG2DLR_RUN_LIM 32

constexpr int fa_img2dlr_cdiv(int a) { return (a + 255) / 256; }
/* T images per tile are possible: the per-item element limits of the three stages (fa_img2dl_lim; the c2r row item
   holds one entry more than its butterfly until the tangle), the run-order results, the plane in each of its uses */
constexpr bool fa_img2dlr_ok(int R0, int R1, bool fwd, int T) {
    const int H = R1 / 2, W = fwd ? H : H + 1, SX = W | 1, NR = T * R0;
    const int A0 = fa_img2dl_a(R0), B0 = fa_img2dl_b(R0);
    return fa_img2dl_stage_ok(T * B0 * W, A0) && fa_img2dl_stage_ok(T * A0 * W, B0) && fa_img2dl_stage_ok(NR, H) &&
           fa_img2dlr_cdiv(NR * (fwd ? H + 1 : H)) <= FA_IMG2DLR_RUN_LIM &&
           (fwd ? 2 : 1) * NR * SX <= FA_IMG2D_LDS_DOUBLES && (fwd || NR * (R1 | 1) <= FA_IMG2D_LDS_DOUBLES);
}
constexpr int fa_img2dlr_tile(int R0, int R1, bool fwd) {
    if (!fa_img2dl_extent(R0) || !fa_img2dl_extent(R1) || (R0 <= 32 && R1 <= 32)) return 0;
    int T = 16384 / (R0 * R1);
    while (T > 1 && !fa_img2dlr_ok(R0, R1, fwd, T)) --T;
    return T;
}

struct Img2DLRArgs {
    const double *src;
    double *dst;
    const cplx *tw0;                                 /* stage table of the column axis, R0 entries (B0 > 1) */
    const cplx *tw1;                                 /* stage table of the row axis, R1 entries */
    i64 nimg;                                        /* images of this launch */
    int pitch;                                       /* row pitch of the real side in doubles: R1 or R1 + 2 */
    int flags;                                       /* FFTW_AMD_F_NT_IN / NT_OUT */
};

template <int R0_, int R1_, bool FWD> struct Img2DLRGeom {
    static constexpr int R0 = R0_, R1 = R1_, H = R1 / 2;
    static constexpr int A0 = fa_img2dl_a(R0), B0 = fa_img2dl_b(R0);
    static constexpr int T = fa_img2dlr_tile(R0, R1, FWD);
    static constexpr int W = FWD ? H : H + 1;        /* complex columns of the column node */
    static constexpr int SX = W | 1;                 /* row stride of the exchanges (doubles), odd */
    static constexpr int S = R1 | 1;                 /* row stride of the real plane of the c2r store, odd */
    static constexpr int NR = T * R0;                /* rows of a tile = radix-H butterflies */
    static constexpr int NC1 = T * B0 * W;           /* radix-A0 butterflies per tile */
    static constexpr int NC2 = T * A0 * W;           /* radix-B0 butterflies */
    static constexpr int QC1 = (NC1 + 255) / 256, QC2 = (NC2 + 255) / 256, QR = (NR + 255) / 256;
    static constexpr int E = NR * (FWD ? H + 1 : H); /* complex results / pairs of reals of a tile */
    static constexpr int N = (E + 255) / 256;
    static constexpr int lds_doubles = (FWD ? 2 * NR * SX : NR * S) + 16;
    static_assert(R1 % 2 == 0 && T >= 1 && fa_img2dlr_ok(R0, R1, FWD, T), "img2dlr: not a size of this kernel");
    static_assert(fa_img2dl_stage_ok(NC1, A0) && fa_img2dl_stage_ok(NC2, B0) && fa_img2dl_stage_ok(NR, H),
                  "img2dlr: a stage holds more elements per item than fa_img2dl_lim allows");
    static_assert(N <= FA_IMG2DLR_RUN_LIM, "img2dlr: too many run-order results per item");
    static_assert(NR * SX <= NR * S && lds_doubles <= FA_IMG2D_LDS_DOUBLES + 16, "img2dlr: the plane does not fit twice on a CU");
};

/* The column node: the image rows at `rowpitch` doubles (W 16-byte entries each) -> the row items.  xr[v][j] is entry
   j of the row whose plane offset is pr[v]; BWD: transformed backward, results left (im, re)-swapped.  The plane is
   free again on return. */
template <class G, bool BWD, int QR, int RW>
FA_DEV void img2dlr_cols(double *plane, const cplx *tw0, const double *src, const int rowpitch, const int tcur,
                         const bool nt_in, const int tid, cplx (&xr)[QR][RW], const int (&pr)[QR]) {
    constexpr int R0 = G::R0, A0 = G::A0, B0 = G::B0, W = G::W, SX = G::SX, QC1 = G::QC1, QC2 = G::QC2;
    static_assert(RW == W, "img2dlr: the row item reads whole rows");
    /* ---- load + C1: butterfly g = (t, a0, c), c fastest across lanes */
    cplx xa[QC1][A0];
    int wa[QC1];                                     /* plane offset of (row t R0 + a0, position c) */
#pragma unroll
    for (int u = 0; u < QC1; ++u) {
        const int g = img2dl_bfly<G::NC1, QC1>(u, tid);
        const int t = g / (B0 * W), r = g - t * (B0 * W);
        const int a0 = r / W, c = r - a0 * W;
        wa[u] = (t * R0 + a0) * SX + c;
        if (t < tcur) {
            ld_run<A0>(xa[u], src + ((t * R0 + a0) * rowpitch + 2 * c), (i64)(rowpitch * B0), nt_in);
        } else {
#pragma unroll
            for (int i = 0; i < A0; ++i) xa[u][i] = c_make(0.0, 0.0);
        }
        if (BWD) {
#pragma unroll
            for (int i = 0; i < A0; ++i) { const double s = xa[u][i].x; xa[u][i].x = xa[u][i].y; xa[u][i].y = s; }
        }
        RB<A0>::run(xa[u]);
        if (B0 > 1) img2dl_twiddle<A0>(xa[u], tw0, a0);
    }
    if constexpr (B0 > 1) {
        /* ---- exchange 1 + C2: butterfly h = (t, d, c) over the rows B0 d + a0, output rows d + A0 c' */
        cplx xb[QC2][B0];
        int rb[QC2], wb[QC2];
#pragma unroll
        for (int v = 0; v < QC2; ++v) {
            const int h = img2dl_bfly<G::NC2, QC2>(v, tid);
            const int t = h / (A0 * W), r = h - t * (A0 * W);
            const int d = r / W, c = r - d * W;
            rb[v] = (t * R0 + B0 * d) * SX + c;
            wb[v] = (t * R0 + d) * SX + c;
        }
        img2dl_xchg<B0 * SX, SX>(plane, xa, wa, xb, rb);
#pragma unroll
        for (int v = 0; v < QC2; ++v) RB<B0>::run(xb[v]);
        img2dl_xchg<A0 * SX, 1>(plane, xb, wb, xr, pr);
    } else {
        img2dl_xchg<SX, 1>(plane, xa, wa, xr, pr);
    }
}

template <int R0, int R1>
__global__ void __launch_bounds__(256, 2)
img2dlr_kernel(const Img2DLRArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DLRGeom<R0, R1, true> G;
    constexpr int H = G::H, T = G::T, NR = G::NR, SX = G::SX, QR = G::QR, E = G::E, N = G::N;
    constexpr int P = NR * SX;                       /* the imaginary parts' half of the plane */
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

    /* ---- columns of the packed image, then one butterfly per row: Z2 */
    cplx y[QR][H];
    int pr[QR];                                      /* plane offset of row rho */
#pragma unroll
    for (int v = 0; v < QR; ++v) pr[v] = img2dl_bfly<NR, QR>(v, tid) * SX;
    img2dlr_cols<G, false>(plane, a.tw0, src, pitch, tcur, nt_in, tid, y, pr);
#pragma unroll
    for (int v = 0; v < QR; ++v) RB<H>::run(y[v]);

    /* ---- Z2 into the plane, both parts at once (rho fastest across lanes, SX odd) */
#pragma unroll
    for (int v = 0; v < QR; ++v)
#pragma unroll
        for (int k = 0; k < H; ++k) {
            plane[pr[v] + k] = y[v][RB<H>::slot(k)].x;
            plane[P + pr[v] + k] = y[v][RB<H>::slot(k)].y;
        }
    __syncthreads();

    /* ---- untangle in the order of the run: result e = (t R0 + k0) (H + 1) + k1 */
    cplx o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int e = j * 256 + tid;
        if (E % 256 != 0 && j == N - 1 && e > E - 1) e = E - 1;
        const int rho = e / (H + 1), k1 = e - rho * (H + 1);
        const int k0 = rho % R0;
        const int pa = rho * SX + (k1 == H ? 0 : k1);
        const int pb = (k0 == 0 ? rho : rho + R0 - 2 * k0) * SX + (k1 == 0 ? 0 : H - k1);
        const cplx w = a.tw1[k1];                    /* (cos, sin)(2 pi k1 / R1) */
        const double ar = plane[pa], ai = plane[P + pa], br = plane[pb], bi = plane[P + pb];
        const double ex = 0.5 * (ar + br), ey = 0.5 * (ai - bi);
        const double ox = 0.5 * (ai + bi), oy = 0.5 * (br - ar);
        o[j] = c_make(ex + (w.x * ox + w.y * oy), ey + (w.x * oy - w.y * ox));
    }
    const int ecur = tcur * (R0 * (H + 1));          /* valid results of this tile */
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int e = j * 256 + tid;
        if (e < ecur) st_sel(dst + 2 * e, o[j], nt_out);
    }
}

template <int R0, int R1>
__global__ void __launch_bounds__(256, 2)
img2dlc_kernel(const Img2DLRArgs a) {
    extern __shared__ __attribute__((aligned(16))) double plane[];
    typedef Img2DLRGeom<R0, R1, false> G;
    constexpr int H = G::H, T = G::T, NR = G::NR, SX = G::SX, S = G::S, QR = G::QR, E = G::E, N = G::N;
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

    /* ---- the H + 1 columns backward; the row item gets Y[r][0 ... H], (im, re)-swapped */
    cplx y[QR][H + 1];
    int pr[QR], pw[QR];                              /* offsets of row rho in the exchange plane and the real plane */
#pragma unroll
    for (int v = 0; v < QR; ++v) {
        const int rho = img2dl_bfly<NR, QR>(v, tid);
        pr[v] = rho * SX;
        pw[v] = rho * S;
    }
    img2dlr_cols<G, true>(plane, a.tw0, src, R1 + 2, tcur, nt_in, tid, y, pr);

    /* ---- tangle in place (on the swapped values: .y is the real part), then the backward butterfly by the swap
       identity: its input is Zp swapped, so the tangle writes (Im Zp, Re Zp) */
#pragma unroll
    for (int v = 0; v < QR; ++v) {
        {
            const double x0 = y[v][0].y, xh = y[v][H].y;
            y[v][0] = c_make(x0 - xh, x0 + xh);
        }
#pragma unroll
        for (int k = 1; 2 * k < H; ++k) {
            const cplx w = a.tw1[k];                 /* (cos, sin)(2 pi k / R1) */
            const double Ax = y[v][k].y, Ay = y[v][k].x, Bx = y[v][H - k].y, By = y[v][H - k].x;
            const double sx = Ax + Bx, sy = Ay - By, dx = Ax - Bx, dy = Ay + By;
            const double U = dx * w.x - dy * w.y, V = dx * w.y + dy * w.x;
            y[v][k] = c_make(sy + U, sx - V);
            y[v][H - k] = c_make(U - sy, sx + V);
        }
        {
            const double Ax = y[v][H / 2].y, Ay = y[v][H / 2].x;
            y[v][H / 2] = c_make(-2.0 * Ay, 2.0 * Ax);
        }
        RB<H>::run(y[v]);                            /* sample 2c is y[slot(c)].y, sample 2c + 1 is y[slot(c)].x */
    }

    /* ---- rows -> the order of the run: pair e = (t R0 + r) H + c sits at row e / H, positions 2c and 2c + 1 */
#pragma unroll
    for (int v = 0; v < QR; ++v)
#pragma unroll
        for (int c = 0; c < H; ++c) {
            plane[pw[v] + 2 * c] = y[v][RB<H>::slot(c)].y;
            plane[pw[v] + 2 * c + 1] = y[v][RB<H>::slot(c)].x;
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

#endif /* FA_PASS2DLR_HPP */
