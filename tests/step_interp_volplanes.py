"""Test infrastructure: step_interp.Interp plus the image step as the planes plan and the wide kernel use it, interpreted
exactly as include/fftw3_amd.h describes it: the FFTW_AMD_K_IMG2DW step (128 x 128, 64 x 128, 128 x 64 images, both stage
tables present), and an image step of any of the three families whose loop over the images is no batch dim (the planes
of the volumes of a rank-3 problem: chunk x n0 of them, the plan in one chunk).  Every other step -- the pass over the
first axis among them -- goes to the base interpreter."""
import numpy as np

import fftw3_amd as fa
from step_interp import Interp, _grids, scratch_reals

IMAGE_VARIANTS = (fa.K_IMG2D, fa.K_IMG2DL, fa.K_IMG2DW)


def tile_of(variant, n0, n1):
    """images per workgroup by the tile query of the step's family"""
    if variant == fa.K_IMG2DW:
        return fa.img2dw_tile(n0, n1)
    if variant == fa.K_IMG2DL:
        return fa.img2dl_tile(n0, n1)
    return int(fa.lib.fa_hip_img2d_tile(n0, n1))


def is_planes_step(s):
    return s.kind == fa.STEP_PASS and s.variant in IMAGE_VARIANTS and s.batch_dim < 0


class InterpVolPlanes(Interp):
    def step(self, s, bufs, cs, cn):
        if not (s.kind == fa.STEP_PASS and (s.variant == fa.K_IMG2DW or is_planes_step(s))):
            return Interp.step(self, s, bufs, cs, cn)
        n0, n1 = s.tile_lo_n, s.L
        assert s.flags & fa.F_LO_DFT
        swap = s.flags & (fa.F_SWAP_IN | fa.F_SWAP_OUT)
        assert swap in (0, fa.F_SWAP_IN | fa.F_SWAP_OUT)
        assert not (s.flags & (fa.F_REAL_IN | fa.F_REAL_OUT | fa.F_CONJ_OUT | fa.F_TW_IN | fa.F_REAL_IMG | fa.F_VOL3D))
        assert s.tw_n == 0 and s.ndims == 1 and s.tile == tile_of(s.variant, n0, n1) and s.tile >= 1
        if s.variant == fa.K_IMG2DW:
            assert (n0, n1) in ((128, 128), (64, 128), (128, 64)) and s.tile * n0 * n1 == 16384
        for tid, n in ((s.table, n1), (s.table2, n0)):
            # an axis of two register stages carries its stage table (cos, sin)(2 pi m / n); the others none.  (1e-14:
            # numpy's own argument 2 pi m / n is rounded three times, a few ulps of 2 pi = 9e-16 each)
            if s.variant != fa.K_IMG2D and n > 32:
                t = self.table(tid)
                assert t.shape == (n,) and np.abs(t - np.exp(2j * np.pi * np.arange(n) / n)).max() < 1e-14
            else:
                assert tid < 0
        img = 2 * n0 * n1
        assert (s.src_im, s.is_l, s.tile_lo_is, s.dim_is[0]) == (1, 2, 2 * n1, img)
        assert (s.dst_im, s.os_l, s.tile_lo_os, s.dim_os[0]) == (1, 2, 2 * n1, img)
        nimg, sbase, dbase = s.dim_n[0], s.src_base, s.dst_base
        if s.batch_dim >= 0:
            assert s.batch_dim == 0
            if s.src_buf < 2:
                sbase += cs * s.dim_is[0]
            if s.dst_buf < 2:
                dbase += cs * s.dim_os[0]
            nimg = cn
        else:
            # the planes of whole volumes: the loop is not cut to a chunk, so the plan must run in one
            assert cs == 0 and cn == self.plan.batch == self.plan.chunk
        src, dst = bufs[s.src_buf], bufs[s.dst_buf]
        b, j0, j1 = _grids([nimg, n0, n1])
        off = b * img + j0 * (2 * n1) + 2 * j1
        x = src[sbase + off] + 1j * src[sbase + off + 1]    # every word of the images is read before any is written
        if swap:
            x = x.imag + 1j * x.real
        y = np.fft.fftn(x, axes=(1, 2))
        if swap:
            y = y.imag + 1j * y.real
        dst[dbase + off] = y.real
        dst[dbase + off + 1] = y.imag


def run_plan_on_host(plan, inarr, outarr):
    """step_interp.run_plan_on_host with the extended interpreter"""
    it = InterpVolPlanes(plan)
    a = inarr.reshape(-1).view(np.float64)
    b = a if outarr is inarr else outarr.reshape(-1).view(np.float64)
    it.run(a, b, scratch_reals(plan))
