"""Layouts and a numpy model of the slab plans of the C ABI (a helper module like util.py, not a conftest): how the
global arrays are cut over the devices in the normal and the transposed layout (include/fftw3_amd.h), and a replay of
a whole plan on the host -- the local plans' effect from numpy.fft, the exchanges from fftw_amd_slab_exchange_ops."""
import numpy as np

import fftw3_amd as fa

T_IN, T_OUT = fa.SLAB_TRANSPOSED_IN, fa.SLAB_TRANSPOSED_OUT
KIND_FLAGS = {"c2c": (0, T_OUT, T_IN, T_IN | T_OUT), "r2c": (0, T_OUT), "c2r": (0, T_IN)}


class Geo(object):
    """kind 'c2c' | 'r2c' | 'c2r', shape = the logical size, P devices"""

    def __init__(self, kind, shape, P):
        self.kind, self.shape, self.P = kind, tuple(shape), P
        self.real = kind != "c2c"
        self.nc = shape[-1] // 2 + 1
        cdims = list(shape[:-1]) + [self.nc if self.real else shape[-1]]
        self.cdims = cdims
        self.c3 = tuple(cdims) if len(cdims) == 3 else (cdims[0], cdims[1], 1)      # (n0, n1', rest)
        self.cuts = [fa.slab_local_size_transposed(cdims, P, g) for g in range(P)]  # (alloc, ln0, lo0, ln1, lo1)
        self.N = int(np.prod(shape))

    def elems(self, g, flags):
        """complex elements of device g's arrays (at least 1, so that every device has an address)"""
        alloc, ln0 = self.cuts[g][0], self.cuts[g][1]
        return max(1, alloc if flags & (T_IN | T_OUT) else ln0 * self.c3[1] * self.c3[2])

    # complex global array G of shape c3 <-> the parts of the devices
    def cut(self, G, g, transposed):
        _, ln0, lo0, ln1, lo1 = self.cuts[g]
        G = np.asarray(G).reshape(self.c3)
        if transposed:
            return np.ascontiguousarray(G[:, lo1:lo1 + ln1].transpose(1, 0, 2)).reshape(-1)
        return np.ascontiguousarray(G[lo0:lo0 + ln0]).reshape(-1)

    def join(self, parts, transposed):
        n0, n1, rest = self.c3
        G = np.zeros(self.c3, dtype=complex)
        for g, part in enumerate(parts):
            _, ln0, lo0, ln1, lo1 = self.cuts[g]
            if transposed:
                G[:, lo1:lo1 + ln1] = np.asarray(part)[:ln1 * n0 * rest].reshape(ln1, n0, rest).transpose(1, 0, 2)
            else:
                G[lo0:lo0 + ln0] = np.asarray(part)[:ln0 * n1 * rest].reshape(ln0, n1, rest)
        return G.reshape(self.cdims)

    # real global array x of the logical shape <-> padded rows of the devices (as float64)
    def cut_real(self, x, g):
        _, ln0, lo0, _, _ = self.cuts[g]
        rows = np.asarray(x).reshape(self.shape)[lo0:lo0 + ln0]
        pad = np.zeros(rows.shape[:-1] + (2 * self.nc,))
        pad[..., :self.shape[-1]] = rows
        return pad.reshape(-1)

    def join_real(self, parts):
        x = np.zeros(self.shape)
        for g, part in enumerate(parts):
            _, ln0, lo0, _, _ = self.cuts[g]
            k = ln0 * int(np.prod(self.shape[1:-1])) * 2 * self.nc
            x[lo0:lo0 + ln0] = np.asarray(part)[:k].reshape((ln0,) + self.shape[1:-1] + (2 * self.nc,))[..., :self.shape[-1]]
        return x

    def make_plan(self, devs, ins, outs, sign, flags):
        if self.kind == "c2c":
            return fa.SlabPlanC(list(self.shape), devs, ins, outs, sign, fa.ESTIMATE | flags)
        cls = fa.SlabPlanR2cC if self.kind == "r2c" else fa.SlabPlanC2rC
        return cls(list(self.shape), devs, ins, outs, fa.ESTIMATE | flags)

    def expected(self, x, sign):
        """numpy's answer for the global input x (c2r: x is the half spectrum)"""
        if self.kind == "c2c":
            X = np.asarray(x).reshape(self.shape)
            return np.fft.fftn(X) if sign < 0 else np.fft.ifftn(X) * self.N
        if self.kind == "r2c":
            return np.fft.rfftn(np.asarray(x).reshape(self.shape))
        return np.fft.irfftn(np.asarray(x).reshape(self.cdims), s=self.shape, axes=tuple(range(len(self.shape)))) * self.N


def replay(geo, sp, ins, sign, flags):
    """run the plan sp on host copies: ins[g] flat complex arrays (real data viewed as complex).  Returns the out
    arrays.  Asserts that every exchange writes every element of the destination layout exactly once."""
    P = geo.P
    n0, n1, rest = geo.c3
    R = n1 * rest
    tin, tout = bool(flags & T_IN), bool(flags & T_OUT)
    size = [geo.elems(g, flags) for g in range(P)]
    wsize = [max(1, geo.cuts[g][0], n0 * geo.cuts[g][3] * rest) for g in range(P)]
    buf = {0: [np.array(ins[g], dtype=complex) for g in range(P)],
           1: [np.full(size[g], np.nan + 0j) for g in range(P)],
           2: [np.full(wsize[g], np.nan + 0j) for g in range(P)]}
    axes = (1,) if len(geo.shape) == 2 else (1, 2)
    tshape = geo.shape[1:]

    def trailing(sb, db):
        for g in range(P):
            ln0 = geo.cuts[g][1]
            if not ln0:
                continue
            if geo.kind == "c2c":
                a = buf[sb][g][:ln0 * R].reshape((ln0,) + tuple(geo.cdims[1:]))
                y = np.fft.fftn(a, axes=axes) if sign < 0 else np.fft.ifftn(a, axes=axes) * int(np.prod(tshape))
                buf[db][g][:ln0 * R] = y.reshape(-1)
            elif geo.kind == "r2c":
                a = buf[sb][g][:ln0 * R].copy().view(np.float64).reshape((ln0,) + tshape[:-1] + (2 * geo.nc,))[..., :tshape[-1]]
                buf[db][g][:ln0 * R] = np.fft.rfftn(a, axes=axes).reshape(-1)
            else:
                a = buf[sb][g][:ln0 * R].reshape((ln0,) + tuple(geo.cdims[1:]))
                y = np.fft.irfftn(a, s=tshape, axes=axes) * int(np.prod(tshape))
                pad = np.zeros((ln0,) + tshape[:-1] + (2 * geo.nc,))
                pad[..., :tshape[-1]] = y
                buf[db][g][:ln0 * R] = pad.reshape(-1).view(np.complex128)

    def along_n0(sb, db, transposed):
        for g in range(P):
            ln1 = geo.cuts[g][3]
            if not ln1:
                continue
            k = ln1 * n0 * rest
            a = buf[sb][g][:k].reshape((ln1, n0, rest) if transposed else (n0, ln1 * rest))
            ax = 1 if transposed else 0
            y = np.fft.fft(a, axis=ax) if sign < 0 else np.fft.ifft(a, axis=ax) * n0
            buf[db][g][:k] = y.reshape(-1)

    def exchange(which, layout_elems):
        ops = sp.exchange_ops(which)
        assert ops is not None
        count = {}
        staged = []
        for o in ops:
            src = buf[o["sbuf"]][o["sdev"]]
            a, b, i = np.meshgrid(np.arange(o["A"]), np.arange(o["B"]), np.arange(o["I"]), indexing="ij")
            si = (o["soff"] + a * o["ssa"] + b * o["ssb"] + i).reshape(-1)
            di = (o["doff"] + a * o["dsa"] + b * o["dsb"] + i).reshape(-1)
            staged.append((o["dbuf"], o["ddev"], di, src[si].copy()))
            key = (o["dbuf"], o["ddev"])
            count.setdefault(key, np.zeros(len(buf[key[0]][key[1]]), dtype=int))
            np.add.at(count[key], di, 1)
        dbufs = set(k[0] for k in count)
        assert len(dbufs) <= 1
        for db, dd, di, v in staged:
            buf[db][dd][di] = v
        for g in range(P):
            want = layout_elems(g)
            if want == 0:
                assert all(k[1] != g for k in count)
                continue
            c = [v for k, v in count.items() if k[1] == g][0]
            assert (c[:want] == 1).all() and (c[want:] == 0).all(), (which, g)

    normal = lambda g: geo.cuts[g][1] * R                    # noqa: E731
    transp = lambda g: geo.cuts[g][3] * n0 * rest            # noqa: E731
    if not tin and not tout:
        if geo.kind != "c2r":
            trailing(0, 1)
        exchange(0, transp)                                  # W[r] = [n0][w_r] has as many elements
        along_n0(2, 2, False)
        exchange(1, normal)
        if geo.kind == "c2r":
            trailing(1, 1)
        assert sp.exchange_ops(2) is None
    elif tout and not tin:
        trailing(0, 2)
        exchange(0, transp)
        along_n0(1, 1, True)
        assert sp.exchange_ops(1) is None
    elif tin and not tout:
        along_n0(0, 2, True)
        exchange(0, normal)
        trailing(1, 1)
        assert sp.exchange_ops(1) is None
    else:
        along_n0(0, 2, True)
        exchange(0, normal)
        trailing(1, 2)
        exchange(1, transp)
        assert sp.exchange_ops(2) is None
    return buf[1]
