/*
 * kernels_tr.hip -- launcher of the transposition steps (transpose.hpp): FFTW_AMD_STEP_COPY with variant
 * FFTW_AMD_K_TRANSPOSE.  The step describes the matrix in doubles,
 *     dims[0] = (n0, lds, vl)   dims[1] = (n1, vl, ldd)   dims[2 ...] = outer batch loops
 *     vl = aux_n doubles (FFTW_AMD_F_REAL_IN | _OUT) or 2 aux_n (interleaved complex, src_im = dst_im = 1)
 * and the launcher picks the element size at launch time: 16-byte elements when vl is even and both bases and every
 * stride are multiples of 16 bytes, 8-byte elements otherwise (arrays of reals are only guaranteed 8-byte alignment;
 * a new-array execution may pass a complex array at an 8-byte offset).  FFTW_AMD_F_PAIR_SWAP asks for the in-place
 * square form; it needs src == dst, which a new-array execution on two different arrays does not give -- the
 * out-of-place form computes the same thing then.  There is no other executor: 1 = a step the kernels cannot run.
 */
#include "transpose.hpp"
#include "launch.hpp"

template <class E, int I> static void tr_launch(const TrArgs &a, bool inplace, hipStream_t st) {
    const unsigned grid = (unsigned)(a.total < (1 << 22) ? a.total : (1 << 22));
    if (inplace) hipLaunchKernelGGL((transpose_inplace_kernel<E, I>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((transpose_tile_kernel<E, I>), dim3(grid), dim3(256), 0, st, a);
}

int fa_launch_transpose(const fftw_amd_step_desc *d, double *const *bufs, i64 cs, i64 cn, hipStream_t st) {
    const bool real = (d->flags & FFTW_AMD_F_REAL_IN) != 0;
    const i64 vl = d->aux_n * (real ? 1 : 2);
    const StepGeom g = fa_step_geom(d, bufs, cs, cn);
    TrArgs a = TrArgs();
    if (d->ndims < 2 || d->ndims > FFTW_AMD_MAX_DIMS || vl < 1 || vl > 8 || d->aux_valid != d->aux_n) return 1;
    if (real != ((d->flags & FFTW_AMD_F_REAL_OUT) != 0) || (!real && (d->src_im != 1 || d->dst_im != 1))) return 1;
    if (d->is_l != (real ? 1 : 2) || d->os_l != d->is_l || g.dos[0] != vl || g.dis[1] != vl) return 1;
    if (d->flags & ~(FFTW_AMD_F_REAL_IN | FFTW_AMD_F_REAL_OUT | FFTW_AMD_F_PAIR_SWAP | FFTW_AMD_F_NT_IN | FFTW_AMD_F_NT_OUT)) return 1;
    a.n0 = g.dn[0]; a.n1 = g.dn[1];
    a.lds = g.dis[0]; a.ldd = g.dos[1];
    if (a.n0 < 0 || a.n1 < 0 || a.lds < a.n1 * vl || a.ldd < a.n0 * vl) return 1;
    bool inplace = (d->flags & FFTW_AMD_F_PAIR_SWAP) != 0;
    i64 mats = 1;
    a.nb = d->ndims - 2;
    for (int k = 0; k < a.nb; ++k) {
        a.bn[k] = g.dn[k + 2]; a.bis[k] = g.dis[k + 2]; a.bos[k] = g.dos[k + 2];
        if (a.bn[k] < 0 || a.bis[k] < 0 || a.bos[k] < 0) return 1;
        if (inplace && a.bis[k] != a.bos[k]) return 1;
        mats *= a.bn[k];
    }
    if (inplace && (a.n0 != a.n1 || a.lds != a.ldd)) return 1;
    if (inplace && g.src != g.dst) inplace = false;
    if (a.n0 == 0 || a.n1 == 0 || mats == 0) return 0;
    bool wide = vl % 2 == 0 && g.aligned() && a.lds % 2 == 0 && a.ldd % 2 == 0;
    for (int k = 0; k < a.nb; ++k) wide = wide && a.bis[k] % 2 == 0 && a.bos[k] % 2 == 0;
    const int I = (int)(wide ? vl / 2 : vl), T = I == 1 ? 32 : 16;
    if (wide) {
        a.lds /= 2; a.ldd /= 2;
        for (int k = 0; k < a.nb; ++k) { a.bis[k] /= 2; a.bos[k] /= 2; }
    }
    a.src = g.src;
    a.dst = g.dst;
    a.nt0 = (a.n0 + T - 1) / T;
    a.nt1 = (a.n1 + T - 1) / T;
    if (inplace) {
        const i64 nt = a.nt0;
        a.cols = (nt & 1) ? nt : nt + 1;
        a.per = ((nt & 1) ? (nt + 1) / 2 : nt / 2) * a.cols;
    } else {
        a.cols = 0;
        a.per = a.nt0 * a.nt1;
    }
    if (a.per > 0x7fffffffffffLL / mats) return 1;
    a.total = a.per * mats;
    if (wide) switch (I) {
        case 1: tr_launch<cplx, 1>(a, inplace, st); break;
        case 2: tr_launch<cplx, 2>(a, inplace, st); break;
        case 3: tr_launch<cplx, 3>(a, inplace, st); break;
        default: tr_launch<cplx, 4>(a, inplace, st); break;
    } else switch (I) {
        case 1: tr_launch<double, 1>(a, inplace, st); break;
        case 2: tr_launch<double, 2>(a, inplace, st); break;
        case 3: tr_launch<double, 3>(a, inplace, st); break;
        case 4: tr_launch<double, 4>(a, inplace, st); break;
        case 5: tr_launch<double, 5>(a, inplace, st); break;
        case 6: tr_launch<double, 6>(a, inplace, st); break;
        case 7: tr_launch<double, 7>(a, inplace, st); break;
        default: tr_launch<double, 8>(a, inplace, st); break;
    }
    return 0;
}
