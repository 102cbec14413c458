/*
 * split.c -- the measured cost models behind the planner's choice of a multi-pass split.
 *
 * Pure functions of the length: which sub-transform lengths have a register kernel, what a pass of such a length
 * costs by position, and the cheapest two- / three-pass split under those costs.  They read no environment and no
 * plan; whether a model applies (the FFTW_AMD_NO_* test switches, the layout of the axis) is the caller's business
 * (planner.c: axis_split).  The tables are written by tools/perf/fit_split_costs.py.
 */
#include "fa_plan.h"
#include "fa_hip.h"

/* lengths with a register kernel (pass1024 / passrr) */
int fa_has_register_kernel(i64 L) {
    return L == 1024 || (L <= 1024 && (fa_hip_rr_tile((int)L) > 0 || fa_hip_r3t_tile((int)L) > 0));
}

/* Three-pass split of a contiguous power of two (n >= 2^21).  The balanced split is not the
   fastest: per-pass times differ by position (first: long input stride; middle: in place at a
   medium stride; last: contiguous rows in, transposed out) and by tile width -- the 256-point
   kernel (16-wide tiles) is the slow one in the first two positions, short middle passes with
   64 ... 256-wide tiles the fast ones.  Costs: ms per 4 GiB moved, measured on MI355X
   (tests/perf_p512.py); unmeasured positions carry a pessimistic guess. */
void fa_pow2_three_pass_split(i64 n, i64 *lens) {
    /*                              2^4   2^5   2^6   2^7   2^8   2^9   2^10 */
    static const double c_first[] = { 1.00, 1.00, 0.95, 0.80, 1.02, 0.87, 1.30 };
    static const double c_mid[]   = { 0.77, 0.78, 0.75, 0.76, 0.99, 0.90, 1.02 };
    static const double c_last[]  = { 0.95, 0.95, 0.90, 0.80, 0.80, 0.82, 0.84 };
    int e = 0, a, m, c, ba = 0, bm = 0, bc = 0;
    double best = 1e30;
    while (((i64)1 << e) < n) ++e;
    for (a = 4; a <= 10; ++a)
        for (m = 4; m <= 10; ++m) {
            double t;
            c = e - a - m;
            if (c < 4 || c > 10) continue;
            t = c_first[a - 4] + c_mid[m - 4] + c_last[c - 4];
            {   /* near-ties go to the more balanced split */
                int hi = a > m ? (a > c ? a : c) : (m > c ? m : c), lo = a < m ? (a < c ? a : c) : (m < c ? m : c);
                t += 0.01 * (hi - lo);
            }
            if (t < best - 1e-9) { best = t; ba = a; bm = m; bc = c; }
        }
    if (!ba) return;
    lens[0] = (i64)1 << ba;
    lens[1] = (i64)1 << bm;
    lens[2] = (i64)1 << bc;
}

/* Three-pass split of a contiguous length that is not a power of two.  The balanced split the
   factoriser returns is rarely the fastest: the register kernels differ by up to 1.5x from one
   sub-transform length to the next (tile width, ragged tiles, radix mix) and by position (first:
   long input stride; middle: in place; last: rows in, transposed out).  Costs are measured
   medians, ms per GiB of a pass (split_costs.inc); the additive model picks the measured best
   split for 5 of the 8 lengths it was checked on and is within 1-7 % on the others
   (tools/perf/fit_split_costs.py).  Reference counterpart: the planner's choice among
   ct-dit radices by estimated cost (fftw/fftw_api.c:15300-15426). */
typedef struct { int L; double c[3]; } split_cost;
static const split_cost g_split_costs[] = {
#include "split_costs.inc"
};
static double split_cost_of(i64 L, int pos) {
    const int n = (int)(sizeof(g_split_costs) / sizeof(g_split_costs[0]));
    int i;
    for (i = 0; i < n - 1; ++i)
        if (g_split_costs[i].L == L && g_split_costs[i].c[pos] > 0.0) return g_split_costs[i].c[pos];
    return g_split_costs[n - 1].c[pos];
}
/* the measured value only: 0 when the table has no sample for (L, pos) */
double fa_split_cost_measured(i64 L, int pos) {
    const int n = (int)(sizeof(g_split_costs) / sizeof(g_split_costs[0]));
    int i;
    for (i = 0; i < n - 1; ++i)
        if (g_split_costs[i].L == L) return g_split_costs[i].c[pos];
    return 0.0;
}
/* factor on the first (row 0) / last (row 1) pass by min(5, v2(stride)): their strided side moves runs of
   T x 16 bytes that start at multiples of the stride, and runs that do not start on a 128-byte line cost up
   to 1.3x (tools/perf/fit_split_costs.py) */
static const double g_split_align[2][6] = {
#include "split_align.inc"
};
static int v2_capped(i64 x) { int k = 0; while (k < 5 && (x & 1) == 0) { x >>= 1; ++k; } return k; }

/* returns the modelled cost of the split it chose (ms per GiB of a pass, three passes), -1 if none.
   Candidates whose FIRST length is a multiple of 8 come first: with an odd or barely even first length the
   two later passes ran up to 1.3x slower than their lengths' medians in the sweeps (their loops over the first
   pass's output index then start off the 128-byte grid); restricted to L1 % 8 == 0 the model's pick is within
   4.3 % of the measured best on all ten lengths of the sweep, unrestricted it misses by up to 34 %. */
double fa_mixed_three_pass_split(i64 n, i64 *lens) {
    static const int need[4] = { 8, 4, 2, 1 };
    int level;
    for (level = 0; level < 4; ++level) {
        i64 a, c;
        double best = -1.0;
        for (a = 16; a <= 1024; ++a) {
            if (n % a || a % need[level] || !fa_has_register_kernel(a)) continue;
            for (c = 16; c <= 1024; ++c) {
                i64 m, lo, hi;
                double cost;
                if ((n / a) % c || !fa_has_register_kernel(c)) continue;
                m = n / a / c;
                if (m < 16 || m > 1024 || !fa_has_register_kernel(m)) continue;
                lo = a < c ? a : c; if (m < lo) lo = m;
                hi = a > c ? a : c; if (m > hi) hi = m;
                if (hi > 4 * lo) continue;
                cost = split_cost_of(a, 0) * g_split_align[0][v2_capped(m * c)] + split_cost_of(m, 1) +
                       split_cost_of(c, 2) * g_split_align[1][v2_capped(a * m)];
                if (best < 0.0 || cost < best) { best = cost; lens[0] = a; lens[1] = m; lens[2] = c; }
            }
        }
        if (best >= 0.0) return best;
    }
    return -1.0;
}

/* Two-pass split n = L1 x L2 by the measured model of tools/perf/fit_split_costs.py (split2_costs.inc: median cost of
   every menu length as first / last pass over 919 timed plans of 78 lengths; split2_align.inc: the price of strided
   runs that start off the 128-byte grid, which depends on the OTHER length's factors of two and on the tile width T:
   cost = c * (1 + 8 / T * m[v2(other)])).  Against the measured best split: mean +0.8 %, worst +9.8 %; the balanced
   split it replaces: mean +9.6 %, worst +43 % (65 536 = 128 x 512 instead of 256 x 256: 2.67 vs 3.07 ms per 4 GiB). */
static const split_cost g_split2_costs[] = {
#include "split2_costs.inc"
};
static const double g_split2_align[2][6] = {
#include "split2_align.inc"
};
static double split2_cost_of(i64 L, int pos) {
    const int n = (int)(sizeof(g_split2_costs) / sizeof(g_split2_costs[0]));
    int i;
    for (i = 0; i < n - 1; ++i)
        if (g_split2_costs[i].L == L && g_split2_costs[i].c[pos] > 0.0) return g_split2_costs[i].c[pos];
    return g_split2_costs[n - 1].c[pos];
}
static int split_tile_of(i64 L) {
    int t = L == 1024 ? 8 : fa_hip_rr_tile((int)L);
    if (t <= 0) t = fa_hip_r3t_tile((int)L);
    return t > 0 ? t : 8;
}
void fa_mixed_two_pass_split(i64 n, i64 *lens) {
    i64 a;
    double best = -1.0;
    for (a = 16; a <= 1024; ++a) {
        i64 b;
        double cost;
        if (n % a || !fa_has_register_kernel(a)) continue;
        b = n / a;
        if (b < 16 || b > 1024 || !fa_has_register_kernel(b)) continue;
        if (a > 8 * b || b > 8 * a) continue;
        cost = split2_cost_of(a, 0) * (1.0 + 8.0 / split_tile_of(a) * g_split2_align[0][v2_capped(b)]) +
               split2_cost_of(b, 1) * (1.0 + 8.0 / split_tile_of(b) * g_split2_align[1][v2_capped(a)]);
        if (best < 0.0 || cost < best) { best = cost; lens[0] = a; lens[1] = b; }
    }
}

/* cost of a pass of L points on the 512-item strided / transposed three-stage kernels (r3tw_menu.inc), in ms per
   GiB moved like split_costs.inc: last = 0 first pass (columns), 1 last pass (rows in, transposed store, twiddle on
   the input).  Measured with tools/perf/perf_pow2_two_trip.py (profiles/r03_two_trip_wide.txt), taking the two
   2048-point passes as equal; 0: no such kernel */
double fa_wide_pass_cost(i64 L, int last) {
    static const struct { int L; double first, last; } c[] = {
        { 2048, 0.239, 0.239 }, { 2000, 0.247, 0.247 }, { 1920, 0.185, 0.207 }, { 1600, 0.265, 0.265 },
        { 1536, 0.274, 0.290 }, { 1440, 0.339, 0.339 }, { 1280, 0.227, 0.198 }, { 1200, 0.300, 0.300 },
        { 1080, 0.269, 0.298 },
    };
    size_t i;
    if (L <= 1024 || fa_hip_r3t_tile((int)L) < 8) return 0.0;
    for (i = 0; i < sizeof(c) / sizeof(c[0]); ++i)
        if (c[i].L == L) return last ? c[i].last : c[i].first;
    return 0.0;
}
