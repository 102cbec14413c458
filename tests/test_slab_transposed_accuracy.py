"""The rms accuracy gate of tests/accuracy.py on the c2c slab plans with TRANSPOSED layouts: the slab result against a
long-double DFT must pass accuracy.passes(e_slab, e_single_device_plan, e_numpy), as for the other GPU transforms."""
import numpy as np
import pytest

import accuracy as A
import fftw3_amd as fa
from slab_layouts import T_IN, T_OUT, Geo
from util import crand

A.require_longdouble()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ndev", [((96, 80), 3), ((7, 5), 4), ((64, 64), 1), ((40, 24, 16), 2), ((1024, 512), 2)])
def test_transposed_slab_plans_pass_the_rms_gate(shape, ndev):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11 + ndev)
    n = int(np.prod(shape))
    geo = Geo("c2c", shape, ndev)
    x = crand(rng, *shape)
    for sign in (-1, 1):
        ref = A.ld_dft(x, shape, 1, sign).reshape(-1)
        xd = torch.from_numpy(x.reshape(-1)).to(dev)
        yd = torch.zeros_like(xd)
        fa.plan_many_dft(len(shape), list(shape), 1, xd, None, 1, n, yd, None, 1, n, sign).execute()
        torch.cuda.synchronize()
        e_single = A.rms_err(yd.cpu().numpy(), ref)
        X = np.fft.fftn(x) if sign < 0 else np.fft.ifftn(x) * n
        e_numpy = A.rms_err(X, ref)
        for flags in (T_OUT, T_IN, T_IN | T_OUT):
            ins = []
            for g in range(ndev):
                part = geo.cut(x, g, bool(flags & T_IN))
                t = np.zeros(geo.elems(g, flags), dtype=complex)
                t[:part.size] = part
                ins.append(torch.from_numpy(t).to(dev))
            outs = [torch.zeros_like(t) for t in ins]
            sp = geo.make_plan([0] * ndev, ins, outs, sign, flags)
            sp.execute()
            sp.sync()
            torch.cuda.synchronize()
            got = geo.join([o.cpu().numpy() for o in outs], bool(flags & T_OUT))
            sp.destroy()
            e = A.rms_err(got, ref)
            print("rms %s P=%d sign=%d flags=%#x: slab %.2f u, single %.2f u, numpy %.2f u"
                  % (shape, ndev, sign, flags, e / A.U, e_single / A.U, e_numpy / A.U))
            assert A.passes(e, e_single, e_numpy), (shape, ndev, sign, hex(flags), e / A.U, e_single / A.U, e_numpy / A.U)
