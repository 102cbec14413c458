"""Test infrastructure: step_interp.Interp plus the FFTW_AMD_K_IMG2DLR step (FFTW_AMD_F_REAL_IMG: whole real images
with extents up to 64, at least one above 32, in one trip, r2c or c2r), interpreted exactly as include/fftw3_amd.h
describes it: the transform of FFTW_AMD_K_IMG2DR (tests/step_interp_img2dr.py), with the stage table of the row axis
always present and that of the column axis exactly when it has two stages.  Every other step goes to the base
interpreter."""
import numpy as np

import fftw3_amd as fa
from step_interp import Interp, _grids, scratch_reals


class InterpImg2DLR(Interp):
    def step(self, s, bufs, cs, cn):
        if not (s.kind == fa.STEP_PASS and s.variant == fa.K_IMG2DLR):
            return Interp.step(self, s, bufs, cs, cn)
        n0, n1 = s.tile_lo_n, s.L
        h = n1 // 2 + 1
        real = s.flags & (fa.F_REAL_IN | fa.F_REAL_OUT)
        assert (s.flags & fa.F_REAL_IMG) and real in (fa.F_REAL_IN, fa.F_REAL_OUT) and n1 % 2 == 0
        assert not (s.flags & (fa.F_SWAP_IN | fa.F_SWAP_OUT | fa.F_CONJ_OUT | fa.F_TW_IN | fa.F_LO_DFT | fa.F_REAL_VOL |
                               fa.F_VOL3D))
        assert n0 in (16, 32, 40, 48, 64) and n1 in (16, 32, 40, 48, 64) and max(n0, n1) > 32
        assert s.tw_n == 0 and s.ndims == 1 and s.tile >= 1
        # the stage tables: the row axis always, the column axis exactly when it has two register stages
        assert s.table >= 0 and (s.table2 >= 0) == (n0 > 32)
        fwd = real == fa.F_REAL_IN
        nimg, sbase, dbase = s.dim_n[0], s.src_base, s.dst_base
        if s.batch_dim >= 0:
            assert s.batch_dim == 0
            if s.src_buf < 2:
                sbase += cs * s.dim_is[0]
            if s.dst_buf < 2:
                dbase += cs * s.dim_os[0]
            nimg = cn
        src, dst = bufs[s.src_buf], bufs[s.dst_buf]
        # the real side: elements 1 apart, rows pitch apart; the complex side: entries 2 apart, rows n1 + 2 apart
        pitch = s.tile_lo_is if fwd else s.tile_lo_os
        assert pitch in (n1, n1 + 2)
        rside = (0, 1, pitch, n0 * pitch)
        cside = (1, 2, n1 + 2, n0 * (n1 + 2))
        assert (s.src_im, s.is_l, s.tile_lo_is, s.dim_is[0]) == (rside if fwd else cside)
        assert (s.dst_im, s.os_l, s.tile_lo_os, s.dim_os[0]) == (cside if fwd else rside)
        b, j0, jr = _grids([nimg, n0, n1])
        _, _, jc = _grids([nimg, n0, h])
        roff = b * (n0 * pitch) + j0 * pitch + jr
        coff = b * (n0 * (n1 + 2)) + j0 * (n1 + 2) + 2 * jc
        if fwd:
            x = src[sbase + roff]                           # every word of the images is read before any is written
            y = np.fft.fft(np.fft.rfft(x, axis=2), axis=1)
            words = np.concatenate([(dbase + coff).ravel(), (dbase + coff + 1).ravel()])
            assert np.unique(words).size == words.size, "a word of the half spectra is written twice"
            dst[dbase + coff] = y.real
            dst[dbase + coff + 1] = y.imag
        else:
            y = src[sbase + coff] + 1j * src[sbase + coff + 1]
            z = np.fft.ifft(y, axis=1) * n0                 # backward, down each of the n1 / 2 + 1 columns
            z[:, :, 0] = z[:, :, 0].real                    # the row c2r reads Im of its entries 0 and n1 / 2 as 0
            z[:, :, n1 // 2] = z[:, :, n1 // 2].real
            x = np.fft.irfft(z, n1, axis=2) * n1
            words = (dbase + roff).ravel()
            assert np.unique(words).size == words.size, "a word of the real images is written twice"
            dst[dbase + roff] = x


def run_plan_on_host(plan, inarr, outarr):
    """step_interp.run_plan_on_host with the extended interpreter"""
    it = InterpImg2DLR(plan)
    a = inarr.reshape(-1).view(np.float64)
    b = a if outarr is inarr else outarr.reshape(-1).view(np.float64)
    it.run(a, b, scratch_reals(plan))
