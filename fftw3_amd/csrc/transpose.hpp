/*
 * transpose.hpp -- the transposition kernels of the plan layer (FFTW_AMD_STEP_COPY steps of variant
 * FFTW_AMD_K_TRANSPOSE; planner.c emit_transpose, launcher in kernels_tr.hip).
 *
 * A problem is a batch of n0 x n1 matrices of TUPLES of I contiguous elements,
 *
 *     dst[c ldd + r I + i] = src[r lds + c I + i]        r < n0, c < n1, i < I
 *
 * with an element E of 8 bytes (double: real data, and anything only 8-byte aligned) or 16 bytes (cplx: interleaved
 * complex data and even tuples of reals when bases and strides allow it).  All offsets and strides below count
 * elements of E and are 64-bit.
 *
 * Same structure as slab_transpose_tile_kernel (kernels_slab.hip): a tile is T x T tuples (T = 32 for I = 1, else
 * 16), loaded as T source rows of T I contiguous elements and stored as T destination rows of T I contiguous elements;
 * only edge tiles have inactive lanes.  With I = 1 a wave instruction moves two whole rows of 256 B (E = double: four
 * 128-byte lines) or 512 B (E = cplx) on either side.  The LDS image is [T][(T + 1) I].  The pitch is chosen by the
 * bank rule of the LDS (64 banks of 4 bytes; conflicts inside a 32-lane half for ds_read_b64, inside a 16-lane group
 * for ds_read_b128); this is the design argument, no LDS counter has been read to confirm it:
 *   E = double, I = 1: the row-wise ds_write_b64 is contiguous; the transposed ds_read_b64 of a 32-lane half reads
 *     q * 33 + r for q = 0 .. 31, i.e. 32 different 8-byte slots of the 256-byte bank row: should not conflict.
 *   E = cplx, I = 1: the 16-lane groups of ds_read_b128 read 16-byte slot (q + r) mod 16 for 16 different q mod 16:
 *     should not conflict (the argument of kernels_slab.hip).
 *   I > 1 (an inner tuple loop, uncommon): lanes run along (q, i) inside a destination row; a half that straddles two
 *     rows can meet a 2-way conflict for odd I.
 *
 * In-place square form (n0 == n1, lds == ldd, src == dst): a workgroup owns the tile pair (P, Q) = ((ti, tj), (tj, ti)),
 * ti <= tj, loads both, synchronises and stores each transposed into the other's place (a diagonal tile alone).  A
 * workgroup reads only the two tiles it will write and has every load in registers before its first store, and no
 * other workgroup touches those tiles: no scratch, no ordering between workgroups.  The pairs of one matrix are
 * numbered through a rectangle of nt (nt + 1) / 2 cells (rows a and nt - 1 - a, or nt - a for odd nt, of the upper
 * triangle side by side), so that the decode needs one division and no square root.  Two images of 32 x 33 x 16 B
 * are 33 KiB (the compiler reports 33 792 B of LDS, 76 VGPRs, no spills for E = cplx, I = 1), which leaves room for
 * four workgroups in a CU's 160 KiB; the occupancy a launch really reaches has not been measured.
 */
#ifndef FA_TRANSPOSE_HPP
#define FA_TRANSPOSE_HPP

#include "common.hpp"

#define FA_TR_MAXB (FFTW_AMD_MAX_DIMS - 2)

struct TrArgs {
    const void *src;
    void *dst;
    i64 n0, n1, lds, ldd;
    i64 nt0, nt1;             /* tiles along r and c (in place: nt0 == nt1) */
    i64 per;                  /* work units per matrix */
    i64 cols;                 /* in place: width of the pair rectangle */
    i64 total;                /* work units of the launch */
    int nb;                   /* outer batch loops */
    i64 bn[FA_TR_MAXB], bis[FA_TR_MAXB], bos[FA_TR_MAXB];
};

template <int I> struct TrGeom {
    static constexpr int T = I == 1 ? 32 : 16;
    static constexpr int ROW = T * I;           /* elements per tile row, on either side */
    static constexpr int PITCH = (T + 1) * I;
    static constexpr int PER = T * ROW / 256;   /* elements per work-item and tile */
};

/* matrix index m -> offsets of its first element on the two sides */
FA_DEV void tr_batch_offsets(const TrArgs &a, i64 m, i64 &soff, i64 &doff) {
    soff = 0; doff = 0;
    for (int k = 0; k < a.nb; ++k) {
        const i64 q = m / a.bn[k], idx = m - q * a.bn[k];
        m = q;
        soff += idx * a.bis[k];
        doff += idx * a.bos[k];
    }
}

/* rows r0 .. of a tile at sp (row pitch ld) into registers: rows along r, lanes along (c, i) */
template <class E, int I> FA_DEV void tr_load(E *v, const E *sp, i64 ld, i64 rows, i64 cols) {
    typedef TrGeom<I> G;
#pragma unroll
    for (int j = 0; j < G::PER; ++j) {
        const int e = (int)threadIdx.x + j * 256, r = e / G::ROW, c = e - r * G::ROW;
        v[j] = E();
        if (r < rows && c < cols * I) v[j] = sp[r * ld + c];
    }
}
template <class E, int I> FA_DEV void tr_to_lds(E *tile, const E *v) {
    typedef TrGeom<I> G;
#pragma unroll
    for (int j = 0; j < G::PER; ++j) {
        const int e = (int)threadIdx.x + j * 256, r = e / G::ROW, c = e - r * G::ROW;
        tile[r * G::PITCH + c] = v[j];
    }
}
/* the transposed image to dp (row pitch ld): rows along the source's c, lanes along (source r, i); rows / cols are
   the SOURCE tile's valid extents */
template <class E, int I> FA_DEV void tr_store(E *dp, i64 ld, const E *tile, i64 rows, i64 cols) {
    typedef TrGeom<I> G;
#pragma unroll
    for (int j = 0; j < G::PER; ++j) {
        const int e = (int)threadIdx.x + j * 256, r = e / G::ROW, c = e - r * G::ROW, q = c / I, i = c - q * I;
        const E w = tile[q * G::PITCH + r * I + i];
        if (q < rows && r < cols) dp[r * ld + c] = w;
    }
}

template <class E, int I>
__global__ void __launch_bounds__(256) transpose_tile_kernel(const TrArgs a) {
    typedef TrGeom<I> G;
    __shared__ E tile[G::T * G::PITCH];
    const E *src = (const E *)a.src;
    E *dst = (E *)a.dst;
    for (i64 u = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x); u < a.total; u += gridDim.x) {
        const i64 m = u / a.per, t = u - m * a.per, ta = t / a.nt1, tb = t - ta * a.nt1;
        const i64 r0 = ta * G::T, c0 = tb * G::T;
        i64 soff, doff;
        tr_batch_offsets(a, m, soff, doff);
        E v[G::PER];
        tr_load<E, I>(v, src + soff + r0 * a.lds + c0 * I, a.lds, a.n0 - r0, a.n1 - c0);
        tr_to_lds<E, I>(tile, v);
        __syncthreads();
        tr_store<E, I>(dst + doff + c0 * a.ldd + r0 * I, a.ldd, tile, a.n0 - r0, a.n1 - c0);
        __syncthreads();
    }
}

template <class E, int I>
__global__ void __launch_bounds__(256) transpose_inplace_kernel(const TrArgs a) {
    typedef TrGeom<I> G;
    __shared__ E tp[G::T * G::PITCH], tq[G::T * G::PITCH];
    E *p = (E *)a.dst;
    const i64 n = a.n0, ld = a.lds, nt = a.nt0;
    for (i64 u = fa_xcd_remap((i64)blockIdx.x, (i64)gridDim.x); u < a.total; u += gridDim.x) {
        const i64 m = u / a.per, t = u - m * a.per, ra = t / a.cols, rb = t - ra * a.cols;
        i64 ti, tj;
        if (rb < nt - ra) { ti = ra; tj = ra + rb; }
        else { ti = nt - ra - ((nt & 1) ? 0 : 1); tj = ti + (rb - (nt - ra)); }
        const i64 r0 = ti * G::T, c0 = tj * G::T;
        const bool diag = ti == tj;             /* uniform over the workgroup */
        i64 soff, doff;
        tr_batch_offsets(a, m, soff, doff);     /* in place: both strides of every batch loop are equal */
        E *mp = p + doff;
        E v[G::PER], w[G::PER];
        tr_load<E, I>(v, mp + r0 * ld + c0 * I, ld, n - r0, n - c0);
        if (!diag) tr_load<E, I>(w, mp + c0 * ld + r0 * I, ld, n - c0, n - r0);
        tr_to_lds<E, I>(tp, v);
        if (!diag) tr_to_lds<E, I>(tq, w);
        __syncthreads();
        tr_store<E, I>(mp + c0 * ld + r0 * I, ld, tp, n - r0, n - c0);
        if (!diag) tr_store<E, I>(mp + r0 * ld + c0 * I, ld, tq, n - c0, n - r0);
        __syncthreads();
    }
}

#endif /* FA_TRANSPOSE_HPP */
