"""Test infrastructure: step_interp.Interp plus the FFTW_AMD_K_VOL3DR step (FFTW_AMD_F_REAL_VOL: whole small real
volumes in one trip, r2c or c2r), interpreted exactly as include/fftw3_amd.h describes it.  Every other step goes to
the base interpreter."""
import numpy as np

import fftw3_amd as fa
from step_interp import Interp, _grids, scratch_reals


class InterpVol3DR(Interp):
    def step(self, s, bufs, cs, cn):
        if not (s.kind == fa.STEP_PASS and s.variant == fa.K_VOL3DR):
            return Interp.step(self, s, bufs, cs, cn)
        n0, n1, n2 = int(s.aux_n), s.tile_lo_n, s.L
        h = n2 // 2 + 1
        real = s.flags & (fa.F_REAL_IN | fa.F_REAL_OUT)
        assert (s.flags & fa.F_REAL_VOL) and real in (fa.F_REAL_IN, fa.F_REAL_OUT) and n2 % 2 == 0
        assert max(n0, n1, n2) <= 32 and min(n0, n1, n2) >= 1
        assert not (s.flags & (fa.F_SWAP_IN | fa.F_SWAP_OUT | fa.F_CONJ_OUT | fa.F_TW_IN | fa.F_LO_DFT | fa.F_REAL_IMG | fa.F_VOL3D))
        assert s.tw_n == 0 and s.table < 0 and s.table2 < 0 and s.ndims == 1 and s.tile >= 1
        fwd = real == fa.F_REAL_IN
        nvol, sbase, dbase = s.dim_n[0], s.src_base, s.dst_base
        if s.batch_dim >= 0:
            assert s.batch_dim == 0
            if s.src_buf < 2:
                sbase += cs * s.dim_is[0]
            if s.dst_buf < 2:
                dbase += cs * s.dim_os[0]
            nvol = cn
        src, dst = bufs[s.src_buf], bufs[s.dst_buf]
        # the real side: elements 1 apart, rows pitch apart, planes n1 pitch, volumes n0 n1 pitch; the complex side:
        # entries 2 apart, rows n2 + 2 apart, planes n1 (n2 + 2), volumes n0 n1 (n2 + 2)
        pitch = s.tile_lo_is if fwd else s.tile_lo_os
        cp = n2 + 2
        assert pitch in (n2, cp)
        rside = (0, 1, pitch, n0 * n1 * pitch)
        cside = (1, 2, cp, n0 * n1 * cp)
        assert (s.src_im, s.is_l, s.tile_lo_is, s.dim_is[0]) == (rside if fwd else cside)
        assert (s.dst_im, s.os_l, s.tile_lo_os, s.dim_os[0]) == (cside if fwd else rside)
        b, j0, j1, jr = _grids([nvol, n0, n1, n2])
        _, _, _, jc = _grids([nvol, n0, n1, h])
        roff = b * (n0 * n1 * pitch) + j0 * (n1 * pitch) + j1 * pitch + jr
        coff = b * (n0 * n1 * cp) + j0 * (n1 * cp) + j1 * cp + 2 * jc
        if fwd:
            x = src[sbase + roff]                           # every word of the volumes is read before any is written
            y = np.fft.fft(np.fft.fft(np.fft.rfft(x, axis=3), axis=2), axis=1)
            words = np.concatenate([(dbase + coff).ravel(), (dbase + coff + 1).ravel()])
            assert np.unique(words).size == words.size, "a word of the half spectra is written twice"
            dst[dbase + coff] = y.real
            dst[dbase + coff + 1] = y.imag
        else:
            y = src[sbase + coff] + 1j * src[sbase + coff + 1]
            z = np.fft.ifft(np.fft.ifft(y, axis=1), axis=2) * (n0 * n1)   # backward over the two leading axes
            z[..., 0] = z[..., 0].real                      # the row c2r reads Im of its entries 0 and n2 / 2 as 0
            z[..., n2 // 2] = z[..., n2 // 2].real
            x = np.fft.irfft(z, n2, axis=3) * n2
            words = (dbase + roff).ravel()
            assert np.unique(words).size == words.size, "a word of the real volumes is written twice"
            dst[dbase + roff] = x


def run_plan_on_host(plan, inarr, outarr):
    """step_interp.run_plan_on_host with the extended interpreter"""
    it = InterpVol3DR(plan)
    a = inarr.reshape(-1).view(np.float64)
    b = a if outarr is inarr else outarr.reshape(-1).view(np.float64)
    it.run(a, b, scratch_reals(plan))
