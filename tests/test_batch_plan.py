"""The batch grid (csrc/batch_plan.hpp: plan_batch, plan_segment_only, meter_segment_wgs, decode_block) on
the CPU: tests/abi/batch_plan_dump.cpp, a stand-alone host program, evaluates the header on a table of
shapes, and every BatchPlan field and the grid must equal tools/model/batch_plan_model.py's. For every plan the
invariants the kernel relies on are checked as well: the segments, the small resolutions' ranges and the
meter segment partition [0, grid); each small resolution owns ceil(n / frames per workgroup) workgroups;
every role of a channel-frame sits at a blockIdx congruent to the frame's index modulo 8, once. The same
program runs decode_block, the composition of the pieces the kernel decodes a block with, over every block
of every planned grid, and what it returns must be the model's work for that block."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from host_program import compile_host_program

sys.path.insert(0, os.path.join(REPO, "tools", "model"))
import batch_plan_model as M  # noqa: E402

SRC = os.path.join(REPO, "tests", "abi", "batch_plan_dump.cpp")

N_CF = (1, 7, 8, 9, 511, 512, 513)
ROLES = ((1, 0), (0, 1), (1, 1))  # (do_kw, do_tp); with mr >= 0 the 16384-point resolution joins segment 0
MR = (-1, 0, 2)
RES = (
    ((16384, 0), (4096, 0), (2048, 0), (1024, 0)),   # none wanted
    ((16384, 1), (4096, 1), (2048, 1), (1024, 1)),
    ((8192, 1), (512, 1)),
    ((4096, 1), (2048, 0), (1024, 1)),               # an unwanted one in the middle
)
Q_N = (0, 1, 64)
BIG = ((8192, 1),) * 4  # two frames per workgroup each: 2 n workgroups
# (n_cf, do_kw, do_tp, mr, res, q_n, q_before_multi) -> code
REFUSED = (
    ((2 ** 31 - 1, 1, 0, -1, (), 0, 0), M.SEGMENT_TOO_LARGE),    # segment 0 alone: 8 ceil(n / 8) = 2^31
    ((2 ** 31 - 1, 1, 1, 0, RES[1], 64, 0), M.SEGMENT_TOO_LARGE),
    ((2 ** 30 - 8, 1, 1, 0, (), 0, 0), M.SEGMENT_TOO_LARGE),     # segment 0 fits (2^31 - 16), segment 1's end not
    ((2 ** 30 - 8, 1, 1, -1, (), 64, 1), M.GRID_TOO_LARGE),      # both fit (2^31 - 16), the meter segment not
    ((2 ** 30, 0, 0, -1, BIG, 0, 0), M.GRID_TOO_LARGE),          # no segment: the small resolutions alone
    ((2 ** 31 - 8, 0, 1, -1, BIG, 0, 1), M.GRID_TOO_LARGE),      # the true peaks fit, the resolutions do not
    ((2 ** 32 - 2, 0, 0, -1, ((8192, 1),), 1, 0), M.GRID_TOO_LARGE),  # the meter segment's one workgroup
)
LARGEST = (2 ** 32 - 2, 0, 0, -1, ((8192, 1),), 0, 0)  # a grid of exactly INT32_MAX workgroups is planned


def _cases():
    return [(n, kw, tp, mr, res, q, first) for n, (kw, tp), mr, res, q, first
            in itertools.product(N_CF, ROLES, MR, RES, Q_N, (0, 1))]


def _line(case):
    n, kw, tp, mr, res, q, first = case
    return " ".join(map(str, ["P", n, kw, tp, mr, q, first, len(res)] + [v for r in res for v in r]))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """The program, compiled once: the host compiler against the ROCm headers, or hipcc (a .cpp file is host
    code to it) where g++ is missing or cannot digest them."""
    exe = compile_host_program(SRC, str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_dump"))

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        out = []
        for ln in r.stdout.splitlines():
            kv = dict(t.split("=") for t in ln.split())
            out.append({k: [int(x) for x in v.split(",")] if "," in v else int(v) for k, v in kv.items()})
        assert len(out) == len(lines)
        return out

    def decode(lines):
        """decode_block of every block of each line's plan: [(code, grid, [grid, 3] kind / which / index)]"""
        r = subprocess.run([exe], input="".join("D " + ln + "\n" for ln in lines), capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        v = np.fromstring(r.stdout, dtype=np.int64, sep=" ")
        out, at = [], 0
        for _ in lines:
            code, grid = int(v[at]), int(v[at + 1])
            n = 3 * grid if code == 0 else 0
            out.append((code, grid, v[at + 2:at + 2 + n].reshape(-1, 3)))
            at += 2 + n
        assert at == len(v)
        return out
    run.decode = decode
    return run


def _assert_equal(got, want, grid, what):
    assert got["code"] == 0, what
    assert got["grid"] == grid, (what, got["grid"], grid)
    assert set(got) == set(want) | {"code", "grid"}
    for k, v in want.items():
        assert got[k] == v, (what, k, got[k], v)


def _assert_invariants(f, grid, case):
    n, kw, tp, mr, res, q, first = case
    # the ranges partition [0, grid): in order, each begins where the one before ended
    rs = sorted(M.ranges(f, grid))
    pos = 0
    for a, b, what in rs:
        assert a == pos, (case, rs)
        pos = b
    assert pos == grid, (case, rs)
    owned = {what[1]: b - a for a, b, what in rs if what[0] == "res"}
    want = {r: M.ceil_div(n, M.frames_per_wg(res[r][0])) for r in range(len(res)) if res[r][1] and r != mr}
    assert owned == want, (case, owned, want)
    assert sum(b - a for a, b, what in rs if what[0] == "meter") == q
    if q:
        at = [a for a, b, what in rs if what[0] == "meter"][0]
        assert at == (f["multi_start"] if first else grid - q), case
    # every role of a segment runs each channel-frame once (the workgroups past n_cf of the last group of 8
    # return at once), at a blockIdx congruent to the frame's index mod 8
    roles_seen = []
    for sg in range(2):
        role, cf = M.segment_work(f, sg)
        b = f["seg_start"][sg] + np.arange(len(cf))
        assert np.all(b % 8 == cf % 8), case
        for ro in np.unique(role):
            live = np.sort(cf[(role == ro) & (cf < n)])
            assert np.array_equal(live, np.arange(n)), (case, sg, ro)
            roles_seen.append(int(ro))
    assert sorted(roles_seen) == sorted([0] * kw + [1] * tp + [2] * (mr >= 0)), (case, roles_seen)


def test_plan_matches_model_and_partitions_the_grid(dump):
    cases = _cases() + [LARGEST]
    assert len(cases) == 7 * 3 * 3 * 4 * 3 * 2 + 1
    for case, got in zip(cases, dump([_line(c) for c in cases])):
        n, kw, tp, mr, res, q, first = case
        code, f, grid = M.plan(n, res, mr, bool(kw), bool(tp), q, bool(first))
        assert code == 0
        _assert_equal(got, f, grid, case)
        if case is not LARGEST:
            _assert_invariants(f, grid, case)
    assert got["grid"] == M.INT32_MAX


def test_segment_only_plan(dump):
    for nq, got in zip((1, 64), dump(["S 1", "S 64"])):
        f, grid = M.segment_only(nq)
        _assert_equal(got, f, grid, nq)
        assert M.ranges(f, grid) == [(0, nq, ("meter",))]


NOTHING, METER, ROLE, SMALL_RES = range(4)  # BatchWorkKind


def _model_decode(f, grid):
    """[grid, 3] kind / which / index of every block from the model's ranges and segment_work, and how many
    of the ranges claim each block"""
    want = np.full((grid, 3), -1, dtype=np.int64)
    claims = np.zeros(grid, dtype=np.int64)
    for a, b, what in M.ranges(f, grid):
        claims[a:b] += 1
        if what[0] == "meter":    # q counts 0..q_n-1 in order
            want[a:b] = np.stack([np.full(b - a, METER), np.zeros(b - a, np.int64), np.arange(b - a)], axis=1)
        elif what[0] == "seg":
            role, cf = M.segment_work(f, what[1])
            want[a:b] = np.stack([np.full(b - a, ROLE), role, cf], axis=1)
        else:                     # a resolution's workgroups count 0..count-1 in grid order
            want[a:b] = np.stack([np.full(b - a, SMALL_RES), np.full(b - a, what[1]), np.arange(b - a)], axis=1)
    return want, claims


def _assert_decode(got, f, grid, what):
    code, got_grid, work = got
    assert (code, got_grid) == (0, grid), what
    want, claims = _model_decode(f, grid)
    assert np.all(claims == 1), (what, np.flatnonzero(claims != 1)[:8])
    assert not np.any(work[:, 0] == NOTHING), (what, np.flatnonzero(work[:, 0] == NOTHING)[:8])
    bad = np.flatnonzero(np.any(work != want, axis=1))
    assert bad.size == 0, (what, bad[:8], work[bad[:8]], want[bad[:8]])
    assert len(np.unique(work, axis=0)) == grid, what  # no work claimed by two blocks


def test_decode_block_inverts_the_plan(dump):
    """The kernel's blockIdx -> work map (decode_block: batch_body runs the pieces it is composed of, in its
    order), block by block over every planned grid: the meter blocks count q = 0..q_n-1, the role blocks have the model's role and
    channel-frame, each small resolution's blocks count its workgroups in grid order -- with the meter
    segment before them, after them and absent -- and no block decodes to nothing or to another's work."""
    cases = _cases()
    assert len(cases) == 1512 and {(q > 0, first) for *_, q, first in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for case, got in zip(cases, dump.decode([_line(c) for c in cases])):
        n, kw, tp, mr, res, q, first = case
        _, f, grid = M.plan(n, res, mr, bool(kw), bool(tp), q, bool(first))
        _assert_decode(got, f, grid, case)
    for nq, got in zip((1, 64), dump.decode(["S 1", "S 64"])):
        _assert_decode(got, *M.segment_only(nq), nq)


def test_meter_segment_workgroups(dump):
    ns = N_CF + (504, 505, 2 ** 31 - 1)
    got = dump([f"M {n}" for n in ns])
    assert [g["wgs"] for g in got] == [M.meter_segment_wgs(n) for n in ns]
    assert [g["wgs"] for g in got] == [1, 1, 1, 2, 64, 64, 64, 63, 64, 64]


def test_plans_past_int32_are_refused(dump):
    got = dump([_line(c) for c, _ in REFUSED])
    for (case, code), g in zip(REFUSED, got):
        n, kw, tp, mr, res, q, first = case
        assert M.plan(n, res, mr, bool(kw), bool(tp), q, bool(first))[0] == code, case
        assert g["code"] == code, (case, g)
