"""The cases of elem_form_cases.py on the device: every one is executed on device arrays of the same alignment as on
the host, compared with the CPU oracle under the reference's error metric and bound (util.aerror, TOL = 1e-10), and
the form of each of its element-wise steps is compared with tests/golden/elem_forms.txt -- the pinned choice of
kernel, tied to a correct result at the smallest shapes that reach each kernel.  Nothing here is only larger than a
case of tests/test_elem_forms.py."""
import numpy as np
import pytest

import elem_form_cases as E
from util import TOL, aerror, oracle_c2r, oracle_dft, oracle_r2c, oracle_r2r, rrand

pytestmark = pytest.mark.gpu
CASES = E.cases()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import fftw3_amd as fa
    assert fa.device_count() > 0, "no HIP device: the GPU tier cannot run"
    return torch, torch.device("cuda:0")


def want_of(case, x, y):
    """the oracle's answer on the host copies: x the input buffer, y the output buffer's contents before the run
    (what the transform does not write must stay)"""
    fn, a, k = case[2].__name__, case[3], case[4]
    if fn == "r2r_many":
        n, kinds, hm = a
        return oracle_r2r(x, n, kinds, howmany=hm, out=y)
    if fn == "c2c_many":
        n, hm = a
        return oracle_dft(x.view(np.complex128), n, hm, out=y.view(np.complex128)).view(np.float64)
    fwd, n = a[0], a[1]
    hm = a[2] if len(a) > 2 else 1
    total, half = int(np.prod(n)), n[-1] // 2 + 1
    rs, rd, cs, cd = k.get("rstride", 1), k.get("rdist", total), k.get("cstride", 1), k.get("cdist", half)
    if fwd:
        return oracle_r2c(x, n, hm, out=y.view(np.complex128), istride=rs, idist=rd, ostride=cs, odist=cd).view(np.float64)
    return oracle_c2r(x.view(np.complex128), n, hm, out=y, istride=cs, idist=cd, ostride=rs, odist=rd)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_matches_the_oracle_on_the_pinned_forms(torch_dev, case):
    torch, dev = torch_dev
    rng = np.random.default_rng(len(case[0]))
    host = {}

    def doubles(count, off=0):
        """plan_dump.doubles on the device, filled with random values; the host copy is kept"""
        raw = torch.zeros(8 * int(count) + 64 + off, dtype=torch.uint8, device=dev)
        start = (-raw.data_ptr()) % 64 + off
        t = raw[start:start + 8 * int(count)].view(torch.float64)
        h = rrand(rng, int(count))
        t.copy_(torch.from_numpy(h))
        host[t.data_ptr()] = h
        return t

    p = E.make_plan(case, doubles)
    xd, yd = p._keep
    assert E.plan_forms(p) == E.golden()[case[0]]
    want = want_of(case, host[xd.data_ptr()].copy(), host[yd.data_ptr()].copy())
    p.execute()
    torch.cuda.synchronize()
    got = yd.cpu().numpy()
    p.destroy()
    e = aerror(got, want)
    print("%s: error %.3e" % (case[0], e))
    assert e < TOL
