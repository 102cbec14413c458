/*
 * plan_c2r_decimated.c -- host-only sanitizer check of the two-trip c2r planner path (emit_c2r_decimated) and of the
 * helpers it shares with its forward twin (emit_r2c_decimated, which the r2c problems below reach).
 * Plans c2r problems with FFTW_AMD_REAL_DEC=1 over the admissible and the inadmissible cases (no device is needed to
 * plan) with the C planner sources compiled under -fsanitize=address,undefined; `make san-c2r` builds and runs it.
 * The HIP units come from the ordinary library, only for the host-side tables (tile sizes, menus) the planner asks for.
 */
#include <stdio.h>
#include <stdlib.h>
#include <fftw3.h>
#include <fftw3_amd.h>

static int fails = 0;

/* number of steps, or -1; *dec = 1 when step 0 is the c2r-decimated rows step */
static int look(fftw_plan p, int *dec) {
    fftw_amd_step_desc d;
    int n;
    *dec = 0;
    if (!p) return -1;
    n = fftw_amd_plan_num_steps(p);
    if (n > 0 && fftw_amd_plan_get_step(p, 0, &d) == 0) *dec = (d.flags & FFTW_AMD_F_REAL_DEC_C2R) != 0;
    fftw_destroy_plan(p);
    return n;
}

static void expect(const char *what, int steps, int dec, int want_dec) {
    printf("%-44s steps %d decimated %d\n", what, steps, dec);
    if (steps < 1 || dec != want_dec || (want_dec && steps != 2)) { printf("  UNEXPECTED\n"); ++fails; }
}

static void c2r(const char *what, int rank, const int *n, int hm, unsigned flags, int inplace, int want_dec) {
    size_t nl = (size_t)n[rank - 1], rows = (size_t)hm, i;
    fftw_complex *y;
    double *z;
    int dec, steps;
    for (i = 0; i + 1 < (size_t)rank; ++i) rows *= (size_t)n[i];
    y = (fftw_complex *)fftw_malloc(sizeof(fftw_complex) * rows * (nl / 2 + 1));
    z = inplace ? (double *)y : (double *)fftw_malloc(sizeof(double) * rows * nl);
    if (!y || !z) { printf("out of memory\n"); exit(2); }
    {
        int total = 1, half = 1;
        for (i = 0; i < (size_t)rank; ++i) { total *= n[i]; half *= (i + 1 == (size_t)rank) ? n[i] / 2 + 1 : n[i]; }
        steps = look(fftw_plan_many_dft_c2r(rank, n, hm, y, NULL, 1, half, z, NULL, 1, inplace ? 2 * half : total, flags), &dec);
    }
    expect(what, steps, dec, want_dec);
    if (!inplace) fftw_free(z);
    fftw_free(y);
}

/* the forward twin: the decimated rows step is the LAST of its two steps */
static void r2c(const char *what, int n, int hm, int want_dec) {
    double *x = (double *)fftw_malloc(sizeof(double) * (size_t)hm * (size_t)n);
    fftw_complex *y = (fftw_complex *)fftw_malloc(sizeof(fftw_complex) * (size_t)hm * (size_t)(n / 2 + 1));
    fftw_plan p;
    fftw_amd_step_desc d;
    int steps, dec = 0;
    if (!x || !y) { printf("out of memory\n"); exit(2); }
    p = fftw_plan_many_dft_r2c(1, &n, hm, x, NULL, 1, n, y, NULL, 1, n / 2 + 1, FFTW_ESTIMATE);
    steps = p ? fftw_amd_plan_num_steps(p) : -1;
    if (steps > 0 && fftw_amd_plan_get_step(p, steps - 1, &d) == 0) dec = (d.flags & FFTW_AMD_F_REAL_DEC) != 0;
    if (p) fftw_destroy_plan(p);
    expect(what, steps, dec, want_dec);
    fftw_free(x); fftw_free(y);
}

int main(void) {
    const int n1[1] = { 2048 * 256 }, n2[1] = { 2048 * 1000 }, n3[1] = { 1 << 22 }, bad[1] = { 2000 * 300 }, odd[1] = { 2048 * 255 };
    const int nd[2] = { 4, 2048 * 256 };
    int dec, steps;
    c2r("default (variable unset)", 1, n1, 3, FFTW_ESTIMATE, 0, 0);
    setenv("FFTW_AMD_REAL_DEC", "1", 1);
    c2r("2048 x 256, batch 3", 1, n1, 3, FFTW_ESTIMATE, 0, 1);
    c2r("2048 x 256, batch 3, padded in place", 1, n1, 3, FFTW_ESTIMATE, 1, 1);
    c2r("2048 x 1000, batch 3", 1, n2, 3, FFTW_ESTIMATE, 0, 1);
    c2r("2^22, batch 1", 1, n3, 1, FFTW_ESTIMATE, 0, 1);
    c2r("FFTW_UNALIGNED", 1, n1, 3, FFTW_ESTIMATE | FFTW_UNALIGNED, 0, 0);
    c2r("2000 x 300", 1, bad, 3, FFTW_ESTIMATE, 0, 0);
    c2r("2048 x 255 (odd L1)", 1, odd, 3, FFTW_ESTIMATE, 0, 0);
    r2c("r2c 2048 x 256, batch 3", 2048 * 256, 3, 1);
    r2c("r2c 2048 x 1024, batch 1", 2048 * 1024, 1, 1);
    r2c("r2c 2048 x 2048, batch 1", 2048 * 2048, 1, 1);
    r2c("r2c 2048 x 255 (odd L1)", 2048 * 255, 3, 0);
    {
        /* an r2r problem whose inner transform is a c2r keeps its plan */
        double *h = (double *)fftw_malloc(sizeof(double) * 3 * n1[0]), *z = (double *)fftw_malloc(sizeof(double) * 3 * n1[0]);
        const fftw_r2r_kind k[1] = { FFTW_HC2R };
        fftw_plan p = fftw_plan_many_r2r(1, n1, 3, h, NULL, 1, n1[0], z, NULL, 1, n1[0], k, FFTW_ESTIMATE);
        int i, any = 0, n = p ? fftw_amd_plan_num_steps(p) : -1;
        fftw_amd_step_desc d;
        for (i = 0; i < n; ++i) if (fftw_amd_plan_get_step(p, i, &d) == 0 && (d.flags & FFTW_AMD_F_REAL_DEC_C2R)) any = 1;
        if (p) fftw_destroy_plan(p);
        expect("r2r HC2R of 2048 x 256", n, any, 0);
        fftw_free(h); fftw_free(z);
    }
    {
        /* the 2-D plan: the decimated step follows the leading-axis pass */
        fftw_complex *y = (fftw_complex *)fftw_malloc(sizeof(fftw_complex) * 4 * (nd[1] / 2 + 1));
        double *z = (double *)fftw_malloc(sizeof(double) * 4 * nd[1]);
        fftw_plan p = fftw_plan_dft_c2r_2d(nd[0], nd[1], y, z, FFTW_ESTIMATE);
        fftw_amd_step_desc d;
        int i, n = p ? fftw_amd_plan_num_steps(p) : -1;
        dec = 0;
        for (i = 0; i < n; ++i) if (fftw_amd_plan_get_step(p, i, &d) == 0 && (d.flags & FFTW_AMD_F_REAL_DEC_C2R)) dec = 1;
        if (p) fftw_destroy_plan(p);
        steps = n;
        printf("%-44s steps %d decimated %d\n", "4 x (2048 x 256), any step", steps, dec);
        if (steps != 3 || !dec) { printf("  UNEXPECTED\n"); ++fails; }
        fftw_free(y); fftw_free(z);
    }
    printf(fails ? "FAILED: %d\n" : "ok\n", fails);
    return fails != 0;
}
