/*
 * kernels_sq.hip -- FFTW_AMD_F_LO_DFT steps: the last trip of a two-dimensional transform whose strided axis was
 * split as T x L0 (planner.c emit_rows_lo_dft).  A tile is T whole rows; the kernel transforms the rows and takes the
 * DFT of length T across them in the same registers:
 *     rows of 2048, T = 4   pass3s_kernel<8, 0, true>     256 items, two workgroups per CU
 *     rows of 4096, T = 2   pass3s_kernel<16, 0, true>
 *     rows of 4096, T = 4   pass3q_kernel                 512 items, one workgroup per CU (pass3q.hpp)
 * These steps have no other executor: the planner settles the layout at plan time, and a layout the kernels cannot
 * take is an internal error that fails loudly.
 */
#include "common.hpp"
#include "pass1024.hpp"
#include "passrr.hpp"
#include "pass3s.hpp"
#include "pass3q.hpp"
#include "launch.hpp"

int fa_launch_lo_dft(const fftw_amd_step_desc *d, double *const *bufs, void *const *tables,
                     i64 cs, i64 cn, hipStream_t st) {
    P3SArgs pa = P3SArgs();
    const int T = d->tile_lo_n;
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    fa_copy_dims(pa, g);
    pa.ntiles = pa.dn[0];
    const StepBlocks nb = fa_step_blocks(pa);
    if (!((d->L == 2048 && T == 4) || (d->L == 4096 && (T == 2 || T == 4))) || d->src_im != 1 || d->dst_im != 1 || d->tw_n ||
        d->is_l != 2 || d->os_l != 2 || (d->flags & (FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_CONJ_OUT)) ||
        !g.even_lo() || !g.even_dims() || !g.aligned() || nb.too_large()) {
        fprintf(stderr, "fftw3_amd: internal error: rows step with a DFT across the rows of a tile (L = %d, T = %d) in an unsupported layout\n", d->L, T);
        abort();
    }
    if (nb.empty()) return 0;
    pa.wL = (const cplx *)tables[d->table];
    pa.flags = d->flags;
    pa.srs = d->tile_lo_is;
    pa.drs = d->tile_lo_os;
    const int outf = ((d->flags & FFTW_AMD_F_SWAP_OUT) ? 1 : 0) | ((d->flags & FFTW_AMD_F_NT_OUT) ? 2 : 0);
    const dim3 grid = nb.grid();
    const size_t l8 = P3SGeom<8>::lds_doubles * sizeof(double), l16 = P3SGeom<16>::lds_doubles * sizeof(double);
#define FA_SQ_CASE(F) case F: if (d->L == 2048) fa_launch_lds<pass3s_kernel<8, 0, true, F>>(grid, dim3(256), l8, l8, st, pa); \
                              else fa_launch_lds<pass3s_kernel<16, 0, true, F>>(grid, dim3(256), l16, l16, st, pa); break;
    if (d->L == 2048 || T == 2) {
        switch (outf) { FA_SQ_CASE(0) FA_SQ_CASE(1) FA_SQ_CASE(2) FA_SQ_CASE(3) }
    }
#undef FA_SQ_CASE
    else {
        const size_t lq = P3QGeom::lds_doubles * sizeof(double);
        const bool sw = (d->flags & FFTW_AMD_F_SWAP_OUT) != 0, nt = (d->flags & FFTW_AMD_F_NT_OUT) != 0;
        if (sw && nt) fa_launch_lds<pass3q_kernel<true, true>>(grid, dim3(512), lq, lq, st, pa);
        else if (sw) fa_launch_lds<pass3q_kernel<true, false>>(grid, dim3(512), lq, lq, st, pa);
        else if (nt) fa_launch_lds<pass3q_kernel<false, true>>(grid, dim3(512), lq, lq, st, pa);
        else fa_launch_lds<pass3q_kernel<false, false>>(grid, dim3(512), lq, lq, st, pa);
    }
    return 0;
}
