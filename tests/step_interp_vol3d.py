"""Test infrastructure: step_interp.Interp plus the FFTW_AMD_K_VOL3D step (FFTW_AMD_F_VOL3D: whole small volumes in one
trip), interpreted exactly as include/fftw3_amd.h describes it.  Every other step goes to the base interpreter."""
import numpy as np

import fftw3_amd as fa
from step_interp import Interp, _grids, scratch_reals


class InterpVol3D(Interp):
    def step(self, s, bufs, cs, cn):
        if not (s.kind == fa.STEP_PASS and s.variant == fa.K_VOL3D):
            return Interp.step(self, s, bufs, cs, cn)
        n0, n1, n2 = int(s.aux_n), s.tile_lo_n, s.L
        assert (s.flags & fa.F_VOL3D) and (s.flags & fa.F_LO_DFT)
        swap = s.flags & (fa.F_SWAP_IN | fa.F_SWAP_OUT)
        assert swap in (0, fa.F_SWAP_IN | fa.F_SWAP_OUT)
        assert not (s.flags & (fa.F_REAL_IN | fa.F_REAL_OUT | fa.F_CONJ_OUT | fa.F_TW_IN | fa.F_REAL_IMG))
        assert 1 <= n0 <= 32 and 1 <= n1 <= 32 and 1 <= n2 <= 32 and n0 * n1 * n2 <= 8192
        assert s.tw_n == 0 and s.table < 0 and s.table2 < 0 and s.ndims == 1 and s.tile >= 1
        vol = 2 * n0 * n1 * n2
        assert (s.src_im, s.is_l, s.tile_lo_is, s.dim_is[0]) == (1, 2, 2 * n2, vol)
        assert (s.dst_im, s.os_l, s.tile_lo_os, s.dim_os[0]) == (1, 2, 2 * n2, vol)
        nvol, sbase, dbase = s.dim_n[0], s.src_base, s.dst_base
        if s.batch_dim >= 0:
            assert s.batch_dim == 0
            if s.src_buf < 2:
                sbase += cs * s.dim_is[0]
            if s.dst_buf < 2:
                dbase += cs * s.dim_os[0]
            nvol = cn
        src, dst = bufs[s.src_buf], bufs[s.dst_buf]
        b, j0, j1, j2 = _grids([nvol, n0, n1, n2])
        off = b * vol + j0 * (2 * n1 * n2) + j1 * (2 * n2) + 2 * j2
        x = src[sbase + off] + 1j * src[sbase + off + 1]    # every word of the volumes is read before any is written
        if swap:
            x = x.imag + 1j * x.real
        y = np.fft.fftn(x, axes=(1, 2, 3))
        if swap:
            y = y.imag + 1j * y.real
        words = np.concatenate([(dbase + off).ravel(), (dbase + off + 1).ravel()])
        assert np.unique(words).size == words.size, "a word of the volumes is written twice"
        dst[dbase + off] = y.real
        dst[dbase + off + 1] = y.imag


def run_plan_on_host(plan, inarr, outarr):
    """step_interp.run_plan_on_host with the extended interpreter"""
    it = InterpVol3D(plan)
    a = inarr.reshape(-1).view(np.float64)
    b = a if outarr is inarr else outarr.reshape(-1).view(np.float64)
    it.run(a, b, scratch_reals(plan))
