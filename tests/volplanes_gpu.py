"""Test infrastructure shared by tests/test_gpu_img2dw.py and tests/test_gpu_vol_planes.py: one c2c problem on the GPU, its
device arrays inside the NaN-patterned arenas of tests/footprint.py, executed twice, and the gates every case of the two
files must meet."""
import accuracy as A
import accuracy_cases as AC
import fftw3_amd as fa
import footprint as F
from accuracy_cases import knobs
from util import TOL, aerror


def run_in_arenas(dev, env, shape, hm, sign, inplace, check_plan):
    """the plan (planned under the knobs `env`, check_plan(plan) asserts it is the one meant) on device arenas, executed
    twice; returns (case, input, result, bit-identical repeat, violations, input kept)"""
    import torch
    case = AC.Case("volplanes", "c2c", shape, hm, sign, env=env)
    x = AC.make_input(case)
    prob = F.Problem("c2c", shape, hm, F.Layout(), F.Layout(), sign=sign, inplace=inplace)
    AR = prob.arenas()
    prob.scatter(AR, x)
    full = [a.to_device(dev) for a in AR]
    ref = [t.clone() for t in full]
    with knobs(env):
        p = prob.plan(fa, [t[a.lo:] for t, a in zip(full, AR)])
    check_plan(p)
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    first = [t.clone() for t in full]
    viol = [F.check(r, t, w) for r, t, w in zip(ref, full, prob.written(AR))]
    kept = None if inplace else F.same_bits(full[0], ref[0])
    for t, r in zip(full, ref):
        t.copy_(r)
    p.execute()
    p.sync()
    torch.cuda.synchronize()
    repeat = all(F.same_bits(t, f) for t, f in zip(full, first))
    out = first[-1][AR[-1].lo:AR[-1].lo + AR[-1].span].cpu().numpy()
    return case, x, prob.gather([out]).reshape(x.shape), repeat, viol, kept


def gates(case, x, got, what=""):
    """relative L-infinity at most 1e-10 against the oracle, and the rms gate e_gpu <= 3 max(e_oracle, e_numpy, u / 2)
    against the long-double reference, for the batch and for every entry of it"""
    e = aerror(got, AC.ref_oracle(case, x))
    m = AC.measure(case, got, x)
    print("%s%s Linf %.3g gpu %.3f u oracle %.3f u numpy %.3f u" % (case.id, what, e, m["gpu"] / A.U, m["oracle"] / A.U,
                                                                     m["numpy"] / A.U))
    assert e <= TOL, (case.id, what, e)
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, what, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U)
    if "per" in m:
        eg, eo, en = m["per"]
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)


def every_condition(dev, env, shape, hm, sign, inplace, check_plan):
    case, x, got, repeat, viol, kept = run_in_arenas(dev, env, shape, hm, sign, inplace, check_plan)
    assert not any(viol), (case.id, viol)
    assert kept is not False, (case.id, "the input of an out-of-place plan changed")
    assert repeat, (case.id, "the second execution differs from the first")
    gates(case, x, got, " in place" if inplace else "")
