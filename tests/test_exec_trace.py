"""CPU tier: the executor (fftw3_amd/csrc/exec.c) run against a recording fake of the runtime calls.

tools/trace/exec_trace.c is compiled with the C sources of the library (the HIP units' host-side tables come from
the built library) and prints, per case, one line per runtime call: which copy, wait, record and launch goes onto
which stream, in which order.  Every trace must equal tests/golden/exec_trace/<case>.txt byte for byte; those files
were recorded from the executor as it was before it became a unit of its own.  So that a wrongly recorded file
cannot hide a dead branch, each case is also checked for the feature it is named for."""
import os
import re
import subprocess

import pytest

from util import ROOT

CSRC = os.path.join(ROOT, "fftw3_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "exec_trace")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("exec_trace") / "exec_trace")
    libdir = os.path.join(ROOT, "fftw3_amd", "lib")
    src = [os.path.join(CSRC, f) for f in ("api.c", "planner.c", "exec.c", "sharded.c", "slab.c", "slab1d.c", "hostmath.c")]
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tools", "trace", "exec_trace.c")] + src +
                   ["-o", out, "-L", libdir, "-lfftw3_amd", "-Wl,-rpath," + libdir, "-lm", "-lpthread", "-ldl"], check=True)
    return out


def _trace(exe, case):
    r = subprocess.run([exe, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _executions(trace):
    """the lines of every execution, without planning and destruction"""
    parts = re.split(r"^# execute \d+\n", trace.split("# destroy\n")[0], flags=re.M)[1:]
    assert parts
    return [p.splitlines() for p in parts]


def _field(line, name):
    return int(re.search(r"\b%s=(-?\d+)" % name, line).group(1))


def _launches(lines):
    """(line index, stream, step, chunk start) of every ordinary launch"""
    return [(i, l.split()[1], _field(l, "step"), _field(l, "cs")) for i, l in enumerate(lines) if l.startswith("launch ")]


def test_the_program_lists_exactly_the_recorded_cases(exe):
    names = subprocess.run([exe, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert sorted(names) == CASES and len(CASES) >= 25


@pytest.mark.parametrize("case", CASES)
def test_trace_equals_the_recorded_one(exe, case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        want = f.read()
    assert _trace(exe, case) == want


@pytest.mark.parametrize("case", ["pair_forward", "pair_backward", "pair_profiled", "hpipe_pair"])
def test_pair_cases_launch_pairs(exe, case):
    for lines in _executions(_trace(exe, case)):
        pairs = [l for l in lines if l.startswith("pair ")]
        assert not _launches(lines)
        assert any(all(int(cn) > 0 for cn in re.findall(r"\bcn=(\d+)", l)) for l in pairs), "no launch with two non-empty halves"
        # every chunk passes through both halves once: 2 + 2 + 1 transforms
        assert sum(int(re.findall(r"\bcn=(\d+)", l)[0]) for l in pairs) == 5
        assert sum(int(re.findall(r"\bcn=(\d+)", l)[1]) for l in pairs) == 5


@pytest.mark.parametrize("case,lanes", [("lanes2", 2), ("lanes3", 3), ("lanes_inplace_new_array", 2), ("lanes_profiled", 2),
                                        ("hpipe_lanes", 2)])
def test_lanes_cases_run_on_side_streams_that_join_the_callers(exe, case, lanes):
    for lines in _executions(_trace(exe, case)):
        la = _launches(lines)
        side = sorted({s for _, s, _, _ in la})
        assert len(side) == lanes and "s0" not in side
        for s in side:
            last = max(i for i, st, _, _ in la if st == s)
            rec = [i for i, l in enumerate(lines) if i > last and l.startswith("record %s " % s)]
            assert rec, "no record on %s after its last launch" % s
            assert "wait s0 " + lines[rec[-1]].split()[2] in lines[rec[-1]:], "s0 does not wait for %s" % s


def test_pipeline_overlaps_stage_a_of_the_next_chunk_with_stage_b(exe):
    (lines,) = _executions(_trace(exe, "pipeline"))
    la = _launches(lines)
    a = {cs: (i, s) for i, s, step, cs in la if step == 0}
    b = {cs: (i, s) for i, s, step, cs in la if step == 1}
    assert sorted(a) == sorted(b) == list(range(9))
    for c in range(8):
        (ia, sa), (ib, sb) = a[c + 1], b[c]
        assert sa != sb and "s0" not in (sa, sb)
        done = lines[ib + 1].split()            # the event that says stage B of chunk c is complete
        assert done[:2] == ["record", sb]
        # stage A of chunk c+1 is queued without waiting for it
        assert "wait %s %s" % (sa, done[2]) not in lines[:ia]
    # ... but a scratch slot (3 of them) is reused only after its previous user's stage B
    for c in range(3, 9):
        done = lines[b[c - 3][0] + 1].split()[2]
        assert "wait %s %s" % (a[c][1], done) in lines[:a[c][0]]


@pytest.mark.parametrize("case,chunks,step", [("hpipe_lanes", 3, 2), ("hpipe_serial", 6, 2), ("hpipe_pair", 3, 2)])
def test_host_pipeline_stages_chunk_by_chunk_on_copy_streams(exe, case, chunks, step):
    for lines in _executions(_trace(exe, case)):
        h2d = [(i, l.split()[1]) for i, l in enumerate(lines) if l.startswith("h2d ")]
        d2h = [(i, l.split()[1]) for i, l in enumerate(lines) if l.startswith("d2h ")]
        work = [(i, l.split()[1], _field(l, "cs")) for i, l in enumerate(lines) if l.startswith(("launch ", "pair "))]
        assert len(h2d) == chunks and len(d2h) == chunks
        up, down = {s for _, s in h2d}, {s for _, s in d2h}
        assert len(up) == 1 and len(down) == 1 and up != down
        assert not (up | down) & ({"s0"} | {s for _, s, _ in work})
        for c, (i, s) in enumerate(h2d):
            arrived = lines[i + 1].split()
            assert arrived[:2] == ["record", s]
            # the first launch that touches chunk c (a pair launch names chunk c in its second half first: cs of pass 1)
            if case == "hpipe_pair":
                first = min(j for j, l in enumerate(lines) if l.startswith("pair ") and
                            int(re.findall(r"\bcs=(-?\d+)", l)[1]) == c * step)
                st = "s0"
            else:
                first, st = min((j, s2) for j, s2, cs in work if cs == c * step)
            assert "wait %s %s" % (st, arrived[2]) in lines[:first]


@pytest.mark.parametrize("case", ["pair_refused", "hpipe_pair_refused"])
def test_a_refused_first_pair_launch_falls_back_to_ordinary_launches(exe, case):
    trace = _trace(exe, case)
    assert "paired 1" in trace.split("# execute")[0]
    runs = _executions(trace)
    assert len(runs) == 2
    assert [l.split()[0] for l in runs[0]].count("pair-refused") == 1 and "pair-refused s0" not in runs[1]
    for lines in runs:
        assert not [l for l in lines if l.startswith("pair ")]
        assert [(step, cs) for _, s, step, cs in _launches(lines) if s == "s0"] == [(st, cs) for cs in (0, 2, 4) for st in (0, 1)]


def test_switches_and_exclusions_take_the_other_path(exe):
    (lines,) = _executions(_trace(exe, "pair_off"))
    assert not [l for l in lines if l.startswith("pair")] and len(_launches(lines)) == 6
    for case in ("hpipe_off", "hpipe_under_pipeline"):
        (lines,) = _executions(_trace(exe, case))
        assert [l.split()[1] for l in lines if l.startswith(("h2d ", "d2h "))] == ["s0", "s0"]
    (lines,) = _executions(_trace(exe, "howmany_zero"))
    assert lines == []
