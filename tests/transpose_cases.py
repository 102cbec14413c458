"""Rank-0 guru transposition problems shared by the CPU tier (tests/test_transpose_plans.py) and the GPU tier
(tests/test_gpu_transpose.py): the loops handed to fftw_plan_guru64_dft / _r2r and, written from the definition of
the layout with numpy index arithmetic, the word offsets every element occupies on the two sides.

A case is a batch of B matrices n0 x n1 of tuples of vl elements (an element: one double for r2r, one interleaved
complex = two words for c2c), source row pitch lds and destination row pitch ldd in tuples:

    out[b][c][r][t] = in[b][r][c][t]      b < B, r < n0, c < n1, t < vl
"""
import numpy as np

import fftw3_amd as fa

NONSQUARE = ((12, 20), (33, 65), (1, 40), (64, 3))
SQUARE_N = (1, 2, 31, 32, 33, 65)
GPU_EXTRA = ((100, 100), (257, 129))


class Case(object):
    def __init__(self, kind, n0, n1, lds=None, ldd=None, batch=1, vl=1, inplace=False):
        assert kind in ("r2r", "c2c")
        self.kind, self.n0, self.n1, self.batch, self.vl, self.inplace = kind, n0, n1, batch, vl, inplace
        self.lds = n1 if lds is None else lds
        self.ldd = n0 if ldd is None else ldd
        self.words = 1 if kind == "r2r" else 2
        self.bs_in = n0 * self.lds * vl             # batch strides, in elements
        self.bs_out = n1 * self.ldd * vl
        if inplace:
            self.bs_in = self.bs_out = max(self.bs_in, self.bs_out)

    def __repr__(self):
        return "%s %dx%d lds=%d ldd=%d batch=%d vl=%d%s" % (self.kind, self.n0, self.n1, self.lds, self.ldd, self.batch,
                                                           self.vl, " in place" if self.inplace else "")

    def loops(self):
        """howmany_dims of the guru call, strides in elements"""
        h = []
        if self.batch > 1:
            h.append((self.batch, self.bs_in, self.bs_out))
        h += [(self.n0, self.lds * self.vl, self.vl), (self.n1, self.vl, self.ldd * self.vl)]
        if self.vl > 1:
            h.append((self.vl, 1, 1))
        return h

    def _offsets(self, out):
        b, r, c, t = np.ix_(np.arange(self.batch), np.arange(self.n0), np.arange(self.n1), np.arange(self.vl))
        if out:
            e = b * self.bs_out + c * self.ldd * self.vl + r * self.vl + t
        else:
            e = b * self.bs_in + r * self.lds * self.vl + c * self.vl + t
        return (e[..., None] * self.words + np.arange(self.words)).astype(np.int64)     # [b][r][c][t][word]

    def in_words(self):
        return self._offsets(False)

    def out_words(self):
        return self._offsets(True)

    def span_in(self):
        """words of the whole input array, the leading-dimension gap of the last row included"""
        return self.batch * self.bs_in * self.words

    def span_out(self):
        return self.batch * self.bs_out * self.words

    def plan(self, i, o, flags=0):
        if self.kind == "r2r":
            return fa.plan_guru64_r2r([], self.loops(), i, o, [], fa.ESTIMATE | flags)
        return fa.plan_guru64_dft([], self.loops(), i, o, fa.FORWARD, fa.ESTIMATE | flags)


def is_transpose_step(s):
    return s.kind == fa.STEP_COPY and s.variant == fa.K_TRANSPOSE
