"""Footprint harness: arenas whose every non-input word is a distinct quiet NaN, the index set
FFTW's definition of a layout says a plan may touch, and the checker for "every word outside it is bit-identical".

An Arena is [guard | payload span | guard] in float64 words.  Before a run every word that is no logical input
element holds 0x7ff8_0000_0000_0000 | word index: a stray write shows as a changed word (also when it copies
another guard word), a used over-read of a gap shows as a NaN in the result, and the input of an out-of-place plan
must come back bit for bit.  footprint() is written from the API definition (fftw3 manual, "Advanced Complex DFTs",
"Advanced Real-data DFTs", "Guru vector and transform sizes") with numpy index arithmetic, never from a plan's
steps: a layout is the guru interface's list of (n, is, os) per dimension plus the howmany dims, and the embed /
stride / dist form of the advanced interface is one constructor of that list (embed_dims).  Nothing here needs a GPU
except Arena.to_device().

Problem describes one plan (transform, both layouts, in place / split / host / flags), builds its arenas, scatters
the logical input, makes the plan on whatever arrays it is given and gathers the logical output; the CPU tier
(tests/test_footprint_cpu.py) runs it through the oracle and the step interpreter, the GPU tier
(tests/test_gpu_footprint.py) on the device.
"""
import numpy as np

NAN_BASE = 0x7FF8000000000000
GUARD_MIN = 8192          # doubles: 64 KiB
GUARD_ROUND = 512         # doubles: 4 KiB, so that the payload keeps the alignment of a bare allocation
KINDS = ("c2c", "r2c", "c2r", "r2r")
SIDES = ("complex", "split", "real", "halfcomplex", "split-halfcomplex", "r2r")


def _round_up(v, m):
    return -(-int(v) // m) * m


class Arena(object):
    """flat float64 buffer [guard | span | guard]; `offset` extra words put the payload off 16-byte alignment"""

    def __init__(self, span_words, dtype=np.float64, guard_words=0, offset=0):
        self.span = int(span_words)
        self.dtype = np.dtype(dtype)
        self.guard = max(GUARD_MIN, _round_up(guard_words, GUARD_ROUND))
        self.lo = self.guard + int(offset)
        self.hi = self.lo + self.span
        self.size = self.hi + self.guard
        self.words = np.empty(self.size, dtype=np.uint64)
        self.fill()

    def fill(self):
        """every word to its distinct quiet NaN"""
        self.words[:] = np.arange(self.size, dtype=np.uint64) | np.uint64(NAN_BASE)

    @property
    def f64(self):
        return self.words.view(np.float64)

    def put(self, idx, values):
        """logical input elements: payload word offsets idx <- values (float64)"""
        self.f64[self.lo + np.asarray(idx, dtype=np.int64)] = values

    def get(self, idx):
        return self.f64[self.lo + np.asarray(idx, dtype=np.int64)]

    def user(self):
        """the array handed to the planner: from the payload's first word to the end of the arena (so that a
        negative index of a numpy executor wraps into the upper guard)"""
        return self.f64[self.lo:]

    def snapshot(self):
        return self.words.copy()

    def abs(self, idx):
        """payload word offsets -> arena word offsets"""
        return np.asarray(idx, dtype=np.int64) + self.lo

    def to_device(self, device="cuda:0"):
        """a device copy of the whole arena as a float64 tensor (the bits survive: it is a memcpy)"""
        import torch
        return torch.from_numpy(self.f64).to(device)


def colocate(arenas):
    """move the arenas into one allocation, in order (a numpy executor that addresses the imaginary plane of split
    data from the real plane's pointer needs both in one buffer); returns the buffer, sets arena.base"""
    buf = np.empty(sum(a.size for a in arenas), dtype=np.uint64)
    pos = 0
    for a in arenas:
        v = buf[pos:pos + a.size]
        v[:] = a.words
        a.words, a.base = v, pos
        pos += a.size
    return buf


def logical_shape(n, side):
    n = tuple(int(v) for v in n)
    if side.endswith("halfcomplex"):
        return n[:-1] + (n[-1] // 2 + 1,)
    return n


def embed_strides(shape, embed, stride):
    """per-dimension strides of a row-major sub-array `shape` of an array `embed` whose elements are `stride` apart:
    element (j0, ..., jr) sits at stride (... (j0 embed1 + j1) embed2 + ...)"""
    shape = tuple(int(v) for v in shape)
    embed = shape if embed is None else tuple(int(v) for v in embed)
    assert len(embed) == len(shape) and all(e >= s for e, s in zip(embed[1:], shape[1:]))
    out, mult = [], int(stride)
    for ax in range(len(shape) - 1, -1, -1):
        out.insert(0, mult)
        mult *= embed[ax]
    return out


def embed_dims(n, howmany, inembed, istride, idist, onembed, ostride, odist, in_side, out_side):
    """the advanced interface's embed / stride / dist as the guru interface's (dims, howmany dims): lists of
    (n, is, os), the strides in elements of each side's type"""
    si = embed_strides(logical_shape(n, in_side), inembed, istride)
    so = embed_strides(logical_shape(n, out_side), onembed, ostride)
    return ([(int(v), a, b) for v, a, b in zip(n, si, so)], [(int(howmany), int(idist), int(odist))])


def elem_offsets(dims, hdims):
    """element offsets of the vector of transforms that the guru lists describe for one side: dims is [(n, stride)]
    per dimension (n in the side's elements), hdims [(n, stride)] per howmany dimension, the first the slowest.
    Shape (product of the howmany extents,) + (n per dimension)"""
    r, h = len(dims), len(hdims)
    off = np.zeros((1,) * (h + r), dtype=np.int64)
    for ax, (n, st) in enumerate(list(hdims) + list(dims)):
        sh = [1] * (h + r)
        sh[ax] = int(n)
        off = off + np.arange(int(n), dtype=np.int64).reshape(sh) * int(st)
    hm = int(np.prod([n for n, _ in hdims], dtype=np.int64)) if h else 1
    return off.reshape((hm,) + tuple(int(n) for n, _ in dims))


def side_dims(dims, hdims, side, which):
    """one side of guru lists of (n, is, os): [(n, stride)] with the last extent halved on a half-complex side"""
    k = 1 if which == "in" else 2
    shape = logical_shape([d[0] for d in dims], side)
    return [(n, d[k]) for n, d in zip(shape, dims)], [(d[0], d[k]) for d in hdims]


def word_offsets(elems, side):
    """element offsets -> word offsets with a trailing axis of the element's words (2 interleaved, else 1)"""
    if side in ("complex", "halfcomplex"):
        return np.stack([2 * elems, 2 * elems + 1], axis=-1)
    return elems[..., None]


def footprint(kind, dims, hdims, side, which):
    """sorted word offsets, from the pointer given to the planner, that the layout's definition says are read
    (which = "in") or written ("out"); dims, hdims: the guru lists of (n, is, os).  side: "complex" (interleaved),
    "split" / "split-halfcomplex" (one plane; both planes have the same set), "real", "halfcomplex" (n_last / 2 + 1
    interleaved elements in the last dimension) or "r2r"."""
    assert kind in KINDS and side in SIDES and which in ("in", "out")
    w = word_offsets(elem_offsets(*side_dims(dims, hdims, side, which)), side)
    w = w.reshape(-1)
    return w if np.all(w[1:] > w[:-1]) else np.unique(w)


class Violations(object):
    def __init__(self, offsets, count=None):
        self.count = int(len(offsets) if count is None else count)
        self.first = [int(v) for v in offsets[:8]]

    def __len__(self):
        return self.count

    def __bool__(self):
        return self.count > 0

    def __repr__(self):
        return "%d words changed outside the footprint, first at %s" % (self.count, self.first)


def _contiguous(written):
    return written is not None and len(written) and int(written[-1]) - int(written[0]) + 1 == len(written)


def check(before, after, written):
    """word offsets outside `written` whose bits differ between the two images of one arena (uint64 / int64 views;
    numpy arrays, or torch tensors, in which case nothing but the offsets leaves the device)"""
    if hasattr(after, "is_cuda"):
        import torch
        diff = after.view(torch.int64) != before.view(torch.int64)
        if _contiguous(written):
            diff[int(written[0]):int(written[-1]) + 1] = False
        elif written is not None and len(written):
            diff[torch.from_numpy(np.asarray(written, dtype=np.int64)).to(after.device)] = False
        count = int(diff.sum())
        return Violations(diff.nonzero().reshape(-1)[:8].cpu().numpy() if count else [], count)
    diff = np.asarray(after).view(np.uint64) != np.asarray(before).view(np.uint64)
    if _contiguous(written):
        diff[int(written[0]):int(written[-1]) + 1] = False
    elif written is not None and len(written):
        diff[np.asarray(written, dtype=np.int64)] = False
    return Violations(np.flatnonzero(diff))


def same_bits(a, b):
    if hasattr(a, "is_cuda"):
        import torch
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------

class Layout(object):
    """one side of a plan_many call: embed (None = the logical shape), stride and dist in the side's elements"""

    def __init__(self, embed=None, stride=1, dist=None):
        self.embed = None if embed is None else tuple(embed)
        self.stride, self.dist = int(stride), dist


class Guru(object):
    """one side of a guru call, where embed / stride / dist cannot say it: the stride of every dimension and the
    howmany dims [(n, stride), ...], the first the slowest, in the side's elements (reals on a split side)"""

    def __init__(self, strides, hdims):
        self.strides = [int(v) for v in strides]
        self.hdims = [(int(n), int(d)) for n, d in hdims]


class Problem(object):
    """kind, shape, howmany, both layouts; inplace: one shared array; split: the complex sides (both of c2c, the
    output of r2c, the input of c2r) are separate real / imaginary planes whose strides count reals; r2r: the
    kinds, one per dimension.  A Problem with a split or a Guru side is planned through the guru interface, every
    other through plan_many_*"""

    def __init__(self, kind, shape, hm, lin, lout, sign=-1, r2r=None, inplace=False, split=False, flags=0, offset=0):
        self.kind, self.shape, self.hm, self.sign = kind, tuple(int(v) for v in shape), int(hm), sign
        self.r2r = None if r2r is None else list(r2r)
        self.inplace, self.split, self.flags, self.offset = inplace, split, flags, offset
        self.in_side = {"c2c": "complex", "r2c": "real", "c2r": "halfcomplex", "r2r": "r2r"}[kind]
        self.out_side = {"c2c": "complex", "r2c": "halfcomplex", "c2r": "real", "r2r": "r2r"}[kind]
        if split:
            assert kind in ("c2c", "r2c", "c2r") and not (inplace and kind != "c2c")
            to_split = {"complex": "split", "halfcomplex": "split-halfcomplex"}
            self.in_side, self.out_side = to_split.get(self.in_side, self.in_side), to_split.get(self.out_side,
                                                                                                 self.out_side)
        self.nin = 2 if self.in_side.startswith("split") else 1
        self.guru = split or isinstance(lin, Guru) or isinstance(lout, Guru)
        if self.guru:
            gi, go = self._guru(lin, self.in_side), self._guru(lout, self.out_side)
            assert [n for n, _ in gi.hdims] == [n for n, _ in go.hdims]
            assert int(np.prod([n for n, _ in gi.hdims], dtype=np.int64)) == self.hm
            self.lin = self.lout = None
            self.dims = [(n, a, b) for n, a, b in zip(self.shape, gi.strides, go.strides)]
            self.hdims = [(n, a, b) for (n, a), (_, b) in zip(gi.hdims, go.hdims)]
        else:
            self.lin, self.lout = self._full(lin, self.in_side), self._full(lout, self.out_side)
            li, lo = self.lin, self.lout
            self.dims, self.hdims = embed_dims(self.shape, hm, li.embed, li.stride, li.dist, lo.embed, lo.stride,
                                               lo.dist, self.in_side, self.out_side)
        self.in_elems = elem_offsets(*side_dims(self.dims, self.hdims, self.in_side, "in"))
        self.out_elems = elem_offsets(*side_dims(self.dims, self.hdims, self.out_side, "out"))
        self.in_fp = footprint(kind, self.dims, self.hdims, self.in_side, "in")
        self.out_fp = footprint(kind, self.dims, self.hdims, self.out_side, "out")

    def _full(self, lay, side):
        lay = lay or Layout()
        ls = logical_shape(self.shape, side)
        embed = ls if lay.embed is None else lay.embed
        dist = int(np.prod(embed)) * lay.stride if lay.dist is None else int(lay.dist)
        return Layout(embed, lay.stride, dist)

    def _guru(self, lay, side):
        if isinstance(lay, Guru):
            return lay
        lay = self._full(lay, side)
        return Guru(embed_strides(logical_shape(self.shape, side), lay.embed, lay.stride), [(self.hm, lay.dist)])

    # -- arenas
    def _one_span(self, side, which):
        """words one transform spans on a side"""
        e = elem_offsets(side_dims(self.dims, [], side, which)[0], [])
        return int(word_offsets(e, side).max()) + 1

    def arenas(self):
        """the arenas, filled with the NaN pattern: [in, out], [shared] in place, and with split planes
        [re_in, im_in, re_out, im_out] (c2c), [in, re_out, im_out] (r2c), [re_in, im_in, out] (c2r) or [re, im]"""
        span_i, span_o = int(self.in_fp.max()) + 1, int(self.out_fp.max()) + 1
        gi, go = self._one_span(self.in_side, "in"), self._one_span(self.out_side, "out")
        if self.inplace:
            A = [Arena(max(span_i, span_o), np.float64, max(gi, go), self.offset)]
            if self.split:
                A.append(Arena(max(span_i, span_o), np.float64, max(gi, go)))
            return A
        A = [Arena(span_i, np.float64, gi, self.offset)]
        if self.in_side.startswith("split"):
            A.append(Arena(span_i, np.float64, gi))
        A.append(Arena(span_o, np.float64, go, self.offset))
        if self.out_side.startswith("split"):
            A.append(Arena(span_o, np.float64, go))
        return A

    def in_arenas(self, A):
        return A[:self.nin]

    def out_arenas(self, A):
        return A if self.inplace else A[self.nin:]

    def scatter(self, A, x):
        """the logical input x, (hm,) + logical input shape, into the input arenas"""
        x = np.asarray(x).reshape(self.in_elems.shape)
        if self.in_side.startswith("split"):
            A[0].put(self.in_elems.reshape(-1), x.real.reshape(-1))
            A[1].put(self.in_elems.reshape(-1), x.imag.reshape(-1))
        elif self.in_side in ("complex", "halfcomplex"):
            w = word_offsets(self.in_elems, self.in_side)
            A[0].put(w[..., 0].reshape(-1), x.real.reshape(-1))
            A[0].put(w[..., 1].reshape(-1), x.imag.reshape(-1))
        else:
            A[0].put(self.in_elems.reshape(-1), x.reshape(-1))

    def gather(self, outs):
        """logical output from the output arrays (payload-based float64 arrays, or anything indexable by an int64
        array that returns numpy), (hm,) + logical output shape"""
        return self._gather(outs, self.out_elems, self.out_side)

    def gather_in(self, ins):
        return self._gather(ins, self.in_elems, self.in_side)

    def _gather(self, arrs, e, side):
        if side.startswith("split"):
            return (arrs[0][e.reshape(-1)] + 1j * arrs[1][e.reshape(-1)]).reshape(e.shape)
        if side in ("complex", "halfcomplex"):
            w = word_offsets(e, side)
            return (arrs[0][w[..., 0].reshape(-1)] + 1j * arrs[0][w[..., 1].reshape(-1)]).reshape(e.shape)
        return np.asarray(arrs[0][e.reshape(-1)]).reshape(e.shape)

    def written(self, A):
        """per arena, the arena word offsets the plan may write: the output footprint on the output arenas, its
        union with the input footprint on the shared arenas of an in-place plan, none on the input arenas of an
        out-of-place plan"""
        if self.inplace:
            return [a.abs(np.union1d(self.in_fp, self.out_fp)) for a in A]
        outs = self.out_arenas(A)
        return [a.abs(self.out_fp) if any(a is o for o in outs) else np.zeros(0, dtype=np.int64) for a in A]

    # -- the plan
    def plan(self, fa, arrays):
        """arrays: what the arenas' payloads became (numpy arrays or device tensors), in the order of arenas()"""
        ins = arrays[:self.nin]
        outs = arrays if self.inplace else arrays[self.nin:]
        fl = fa.ESTIMATE | self.flags
        if self.guru:
            d, h = self.dims, self.hdims
            if self.kind == "c2c" and self.split:
                assert self.sign == -1
                return fa.plan_guru64_split_dft(d, h, ins[0], ins[1], outs[0], outs[1], fl)
            if self.kind == "c2c":
                return fa.plan_guru64_dft(d, h, ins[0], outs[0], self.sign, fl)
            if self.kind == "r2c" and self.split:
                return fa.plan_guru64_split_dft_r2c(d, h, ins[0], outs[0], outs[1], fl)
            if self.kind == "r2c":
                return fa.plan_guru64_dft_r2c(d, h, ins[0], outs[0], fl)
            if self.kind == "c2r" and self.split:
                return fa.plan_guru64_split_dft_c2r(d, h, ins[0], ins[1], outs[0], fl)
            if self.kind == "c2r":
                return fa.plan_guru64_dft_c2r(d, h, ins[0], outs[0], fl)
            return fa.plan_guru64_r2r(d, h, ins[0], outs[0], self.r2r, fl)
        r, n, li, lo = len(self.shape), list(self.shape), self.lin, self.lout
        # NULL where the array is the logical shape itself (in place r2c / c2r NULL would mean the padded layout)
        real_inplace = self.inplace and self.kind in ("r2c", "c2r")
        ie = None if li.embed == logical_shape(n, self.in_side) and not real_inplace else list(li.embed)
        oe = None if lo.embed == logical_shape(n, self.out_side) and not real_inplace else list(lo.embed)
        if self.kind == "c2c":
            return fa.plan_many_dft(r, n, self.hm, ins[0], ie, li.stride, li.dist, outs[0], oe, lo.stride, lo.dist,
                                    self.sign, fl)
        if self.kind == "r2c":
            return fa.plan_many_dft_r2c(r, n, self.hm, ins[0], ie, li.stride, li.dist, outs[0], oe, lo.stride,
                                        lo.dist, fl)
        if self.kind == "c2r":
            return fa.plan_many_dft_c2r(r, n, self.hm, ins[0], ie, li.stride, li.dist, outs[0], oe, lo.stride,
                                        lo.dist, fl)
        return fa.plan_many_r2r(r, n, self.hm, ins[0], ie, li.stride, li.dist, outs[0], oe, lo.stride, lo.dist,
                                self.r2r, fl)

    def oracle(self, A):
        """run the oracle on the (numpy) arenas, from and into the payloads"""
        import util
        assert not self.guru
        li, lo = self.lin, self.lout
        src = A[0].user()                   # contiguous: util.oracle_* pass its memory on as it is
        dst = src if self.inplace else A[1].user()
        kw = dict(inembed=list(li.embed), istride=li.stride, idist=li.dist, onembed=list(lo.embed),
                  ostride=lo.stride, odist=lo.dist)
        if self.kind == "c2c":
            util.oracle_dft(src, self.shape, self.hm, self.sign, out=dst, **kw)
        elif self.kind == "r2c":
            util.oracle_r2c(src, self.shape, self.hm, out=dst, **kw)
        elif self.kind == "c2r":
            util.oracle_c2r(src, self.shape, self.hm, out=dst, **kw)
        else:
            util.oracle_r2r(src, list(self.shape), self.r2r, howmany=self.hm, out=dst, **kw)

