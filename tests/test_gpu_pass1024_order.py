"""The tile order of the register-resident 1024-point pass (pass1024.hpp: p1024_order; FFTW_AMD_P1024_ORDER, read into
the plan's knob snapshot; order 0 marks the plan's steps with F_P1024_EIGHTHS, the default leaves them as they were):
which tile a workgroup gets, and nothing else.

CPU: the order function itself, evaluated on the host through the library's hook (fa.p1024_tile_order), must be a
bijection from the workgroups of a launch onto its (tile, outer index) pairs for every order and grid size.
GPU: every order gives the bits of order 0 (every XCD walks its eighth of the tile list from the start), on the lanes
schedule and on the pair kernel, in one dimension and in two; one case per order goes through the footprint arenas and
the rms gate, where a wrong order shows as an unwritten or a doubly written tile."""
import functools

import numpy as np
import pytest

import accuracy as A
import accuracy_cases as AC
import footprint_cases as FC
import fftw3_amd as fa
from util import crand

ORDERS = list(range(fa.P1024_ORDERS))             # 0 = the XCD-contiguous eighths, walked from their start
NEW_ORDERS = ORDERS[1:]
KNOB = "FFTW_AMD_P1024_ORDER"
DEFAULT = 1                                       # FA_P1024_ORDER_DEFAULT (fa_plan.h): the skewed eighths


# ---- CPU: the map

def _pairs_hit_once(order, nblocks, outer):
    """the kernel's own split of a place into (tile, outer index), every pair exactly once"""
    ntiles = nblocks // outer
    place = fa.p1024_tile_order(order, nblocks)
    if place.min() < 0 or place.max() >= nblocks:
        return False
    hits = np.bincount((place // ntiles) * ntiles + place % ntiles, minlength=nblocks).reshape(outer, ntiles)
    return bool((hits == 1).all())


def test_the_library_has_the_skewed_order():
    assert ORDERS == [0, 1]


@pytest.mark.parametrize("order", ORDERS)
def test_every_grid_hits_every_tile_and_outer_index_once(order):
    """grids of 1 ... 4100 workgroups (every residue mod 8 and mod 64: unequal eighths, rotations longer than a short
    eighth) as one outer index and, where the size allows, as three; and 1 ... 4100 tiles times three outer indices"""
    bad = []
    for g in range(1, 4101):
        if not _pairs_hit_once(order, g, 1):
            bad.append((g, 1))
        if g % 3 == 0 and not _pairs_hit_once(order, g, 3):
            bad.append((g, 3))
        if not _pairs_hit_once(order, 3 * g, 3):
            bad.append((3 * g, 3))
    assert not bad, "order %d: (grid, outer extent) not hit exactly once: %s" % (order, bad[:10])


def test_order_0_is_the_xcd_contiguous_eighths():
    """what the pair kernel and every other kernel family keep: identity unless the grid is a multiple of 8"""
    for n in (1, 7, 8, 127, 128, 1024, 1152):
        b = np.arange(n, dtype=np.int64)
        want = b if n % 8 else (b % 8) * (n // 8) + b // 8
        assert np.array_equal(fa.p1024_tile_order(0, n), want)


def test_order_1_rotates_the_eighth_of_xcd_x_by_an_odd_step():
    """the benchmark's column-pass launch, 8 transforms of 128 tiles: XCD x stays inside transform x and starts 17 x
    tiles into it, so no two XCDs work on the same column band at the same place of their walk"""
    place = fa.p1024_tile_order(1, 1024)
    for x in range(8):
        mine = place[x::8]
        assert np.array_equal(mine // 128, np.full(128, x))
        assert np.array_equal(mine % 128, (np.arange(128) + 17 * x) % 128)
    with pytest.raises(ValueError):
        fa.p1024_tile_order(len(ORDERS), 1024)


def _step_orders(plan):
    """tile order of every step of the 1024-point pass: 0 when the step carries F_P1024_EIGHTHS, else 1"""
    return [0 if s.flags & fa.F_P1024_EIGHTHS else 1 for s in plan.steps() if s.variant == fa.K_P1024]


def test_the_knob_reaches_the_step_per_plan(monkeypatch):
    """read in the planner's knob snapshot at every build; only order 0 leaves a mark, and only on steps of the
    1024-point pass, so that a plan built without the knob is the plan it always was"""
    n = 1 << 20
    x = np.zeros((2, n), dtype=complex)
    y = np.zeros_like(x)
    for v in ORDERS:
        monkeypatch.setenv(KNOB, str(v))
        p = fa.plan_many_dft(1, [n], 2, x, None, 1, n, y, None, 1, n, fa.FORWARD)
        assert _step_orders(p) == [v, v], p.sprint()
        p.destroy()
    monkeypatch.delenv(KNOB)
    p = fa.plan_many_dft(1, [n], 2, x, None, 1, n, y, None, 1, n, fa.FORWARD)
    assert _step_orders(p) == [DEFAULT] * 2
    p.destroy()
    monkeypatch.setenv(KNOB, "0")
    x = np.zeros((4, 512), dtype=complex)
    p = fa.plan_many_dft(1, [512], 4, x, None, 1, 512, x.copy(), None, 1, 512, fa.FORWARD)
    assert [s.flags & fa.F_P1024_EIGHTHS for s in p.steps()] == [0]
    p.destroy()


# ---- GPU

@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert fa.device_count() > 0, "no HIP device: the GPU tier cannot run"
    return torch, torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _input(shape):
    x = crand(np.random.default_rng(sum(shape)), *shape)
    x.setflags(write=False)
    return x


def _bits(torch, dev, shape, order, plan_of):
    """the raw doubles that a plan built under FFTW_AMD_P1024_ORDER=order writes into a zeroed output"""
    xd = torch.from_numpy(_input(shape).copy()).to(dev)
    yd = torch.zeros_like(xd)
    with AC.knobs({KNOB: str(order)}):
        p = plan_of(xd, yd)
    orders = _step_orders(p)
    assert orders and set(orders) == {order}, p.sprint()
    p.execute()
    torch.cuda.synchronize()
    out = yd.cpu().numpy().view(np.float64)
    p.destroy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 1])
@pytest.mark.parametrize("howmany", [1, 3, 8, 9])
def test_2_20_every_order_gives_the_bits_of_order_0(torch_dev, monkeypatch, howmany, lanes):
    """column-pass grids of 128, 384, 1024 and 1152 tiles (9 = a chunk of 8 and a ragged one of 1): one XCD per
    transform, fewer transforms than XCDs, more than one chunk; on two lanes and on the pair kernel (FFTW_AMD_LANES=1,
    which keeps order 0 whatever the knob says)"""
    torch, dev = torch_dev
    n = 1 << 20
    if lanes == 1:
        monkeypatch.setenv("FFTW_AMD_LANES", "1")
    plan_of = lambda xd, yd: fa.plan_many_dft(1, [n], howmany, xd, None, 1, n, yd, None, 1, n, fa.FORWARD)
    want = _bits(torch, dev, (howmany, n), 0, plan_of)
    assert np.abs(want).max() > 1.0
    for order in NEW_ORDERS:
        got = _bits(torch, dev, (howmany, n), order, plan_of)
        assert np.array_equal(got, want), "order %d differs from order 0 in %d doubles" % (order, int((got != want).sum()))


@pytest.mark.gpu
def test_2d_4096_x_4096_every_order_gives_the_bits_of_order_0(torch_dev):
    """the column form of the pass with an outer dim and a twiddle per row class: `rest / dn[d]` of
    p1024_block_origin under the new order"""
    torch, dev = torch_dev
    plan_of = lambda xd, yd: fa.plan_dft_2d(4096, 4096, xd, yd, fa.FORWARD)
    want = _bits(torch, dev, (4096, 4096), 0, plan_of)
    assert np.abs(want).max() > 1.0
    for order in NEW_ORDERS:
        got = _bits(torch, dev, (4096, 4096), order, plan_of)
        assert np.array_equal(got, want), "order %d differs from order 0 in %d doubles" % (order, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("order", NEW_ORDERS)
def test_every_order_passes_the_footprint_arenas_and_the_rms_gate(order):
    """n = 2^20 x 2 in a gapped layout on arenas of distinct NaNs: no word outside the footprint changes, the values
    inside pass the rms gate against the long-double reference (an unwritten tile is NaN), a second execution repeats
    the bits"""
    A.require_longdouble()
    case = FC.FCase("pass1024", "c2c", (1 << 20,), 2, "gapped", env={KNOB: str(order)})
    x = FC.make_input(case)
    r = FC.run(case, x)
    assert "pass-1024/reg32x32 tile=8 buf0" in r.sprint and "pass-1024/reg32x32 tile=8 tw=1048576" in r.sprint, r.sprint
    assert not any(r.violations), (case.id, r.violations, r.sprint)
    m = FC.measure(case, r.got, x)
    print("order %d: gpu %.3f u oracle %.3f u numpy %.3f u" % (order, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U))
    assert A.passes(m["gpu"], m["oracle"], m["numpy"]), (case.id, m["gpu"] / A.U, m["oracle"] / A.U, m["numpy"] / A.U)
    if "per" in m:
        eg, eo, en = m["per"]
        for b in range(case.hm):
            assert A.passes(eg[b], eo[b], en[b]), (case.id, "entry %d" % b, eg[b] / A.U, eo[b] / A.U, en[b] / A.U)
    assert r.repeat and r.preserved is not False, (case.id, r.sprint)
