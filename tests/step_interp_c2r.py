"""Test infrastructure: step_interp.Interp plus the FFTW_AMD_F_REAL_DEC_C2R step (the first trip of the two-trip c2r
plan), interpreted exactly as include/fftw3_amd.h describes it.  Every other step goes to the base interpreter."""
import numpy as np

import fftw3_amd as fa
from step_interp import Interp, _grids, scratch_reals


class InterpC2R(Interp):
    def step(self, s, bufs, cs, cn):
        if not (s.kind == fa.STEP_PASS and (s.flags & fa.F_REAL_DEC_C2R)):
            return Interp.step(self, s, bufs, cs, cn)
        dn, dis, dos, dtw, sbase, dbase = self._dims(s, cs, cn)
        src, dst = bufs[s.src_buf], bufs[s.dst_buf]
        L, nrow = s.L, dn[0]
        L1 = 2 * (nrow - 1)
        assert (s.flags & fa.F_SWAP_IN) and (s.flags & fa.F_SWAP_OUT) and not (s.flags & (fa.F_TW_IN | fa.F_REAL_DEC))
        assert s.tw_n == L1 * L and dtw[0] == 1 and not any(dtw[1:]) and s.src_im == 1 and s.dst_im == 1
        assert s.is_l == L1 * dis[0] and src is not dst
        g = _grids([L] + dn)
        l, idx = g[0], g[1:]
        k1 = idx[0]
        rest_s = np.zeros_like(l[:1])
        rest_d = np.zeros_like(l[:1])
        for i, gi in enumerate(idx):
            if i:
                rest_s = rest_s + gi * dis[i]
                rest_d = rest_d + gi * dos[i]
        # the row: X[k1 + L1 k2] below L / 2, conj X[(L1 - k1) + L1 (L - 1 - k2)] above
        low = l < L // 2
        off = sbase + rest_s + np.where(low, k1 * dis[0] + l * s.is_l, (L1 - k1) * dis[0] + (L - 1 - l) * s.is_l)
        assert off.min() >= 0
        Y = src[off] + 1j * src[off + 1]
        Y = np.where(low, Y, np.conj(Y))
        Y = np.where((k1 == 0) & ((l == 0) | (l == L // 2)), Y.real + 0j, Y)      # Im X[0], Im X[n / 2] read as 0
        A = np.fft.ifft(Y, axis=0) * L * self.tw2(s, l * k1)                      # twiddle on the OUTPUT index j2 = l
        Ae, Ao = A[0::2], A[1::2]
        shape = Ae.shape
        c = _grids([L // 2] + dn)[0]
        k1b = np.broadcast_to(k1, shape)
        edge = (k1b == 0) | (2 * k1b == L1)
        od = np.broadcast_to(dbase + rest_d + c * s.os_l + k1 * dos[0], shape)
        om = np.broadcast_to(dbase + rest_d + c * s.os_l + (L1 - k1) * dos[0], shape)
        Zd = np.where(edge, Ae.real + 1j * Ao.real, Ae + 1j * Ao)
        Zm = np.conj(Ae) + 1j * np.conj(Ao)
        words = np.concatenate([od.ravel(), om[~edge].ravel()])
        assert np.unique(words).size == words.size, "a word of the scratch image is written twice"
        dst[od] = Zd.real
        dst[od + 1] = Zd.imag
        dst[om[~edge]] = Zm.real[~edge]
        dst[om[~edge] + 1] = Zm.imag[~edge]


def run_plan_on_host(plan, inarr, outarr):
    """step_interp.run_plan_on_host with the extended interpreter"""
    it = InterpC2R(plan)
    a = inarr.reshape(-1).view(np.float64)
    b = a if outarr is inarr else outarr.reshape(-1).view(np.float64)
    it.run(a, b, scratch_reals(plan))
