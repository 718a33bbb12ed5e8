"""The meter pipeline's ledger (csrc/meter_sync.hpp: the step functions behind every counter target of the
batch launch path) on the CPU: tests/abi/meter_sync_dump.cpp, a stand-alone host program, takes scripts of
steps and prints each step's targets and the whole ledger, and both must equal
tools/model/meter_sync_model.py's after every step -- step tables from the zero ledger and from one about
to wrap, then long seeded sequences that mix every path with failed batch launches. On both traces the
orders the kernels rely on are checked in the device's own wrap-aware comparison: nothing waits for work
that was never launched, a failed pipelined launch or flush changes nothing, a failed direct or chunked
launch publishes the K-weighting count the prep waits for, the mirror parities alternate, the pending
segment keeps its size, and a flush leaves no segment target ahead of the segment count."""
import os
import random
import subprocess
import sys

import pytest

from conftest import REPO
from host_program import compile_host_program

sys.path.insert(0, os.path.join(REPO, "tools", "model"))
import meter_sync_model as M  # noqa: E402

SRC = os.path.join(REPO, "tests", "abi", "meter_sync_dump.cpp")

N_CF = (1, 7, 8, 9, 511, 512, 513)
CH = (1, 2)
FRAMES = ((1,), (2048,), (2048, 1))
NEAR_WRAP = 2 ** 32 - 3
LISTS = ("frames", "par", "seg_pre", "seg_post", "seg_par")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = compile_host_program(SRC, str(tmp_path_factory.mktemp("meter_sync") / "meter_sync_dump"))

    def run(lines):
        """[(targets, ledger)] of every line, in the model's form"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        out = []
        for ln in r.stdout.splitlines():
            kv = dict(t.split("=") for t in ln.split())
            d = {k: ([] if v == "-" else [int(x) for x in v.split(",")]) if k in LISTS else int(v)
                 for k, v in kv.items()}
            ledger = {k: d.pop(k) for k in M.zero()}
            out.append((d, ledger))
        assert len(out) == len(lines)
        return out
    return run


def _model(lines):
    m, out = M.zero(), []
    for ln in lines:
        t, m = M.step(m, ln)
        out.append((t, M.copy(m)))
    return out


def _fr(frames):
    return f"{len(frames)} " + " ".join(map(str, frames))


def _assert_same(lines, got, want):
    for i, (ln, g, w) in enumerate(zip(lines, got, want)):
        assert g[0] == w[0], (i, ln, "targets", g[0], w[0], lines[max(0, i - 5):i])
        assert g[1] == w[1], (i, ln, "ledger", g[1], w[1], lines[max(0, i - 5):i])


# ---- the invariants, on a trace [(line, targets, ledger before, ledger after)] ----

def _reached(issued, target):
    return M.sdiff(issued, target) >= 0


def _assert_invariants(trace):
    last_par = None   # mirror parity of the last successful pipelined step of this context
    pend_n_cf = None  # n_cf of the step that set the pending segment
    for i, (ln, t, before, after) in enumerate(trace):
        w = ln.split()
        kind, good, what = w[0], w[-1] == "ok", (i, ln)
        if kind == "Z":
            last_par = pend_n_cf = None
        # nothing waits for work that was never launched: every target against its counter's issued count,
        # once the step that enqueues the awaited workgroups has committed
        if kind in ("K", "D"):          # (the prep is enqueued and waits even when the batch launch fails)
            assert _reached(after["kw"], t["wait"]), what
            if not good:                # the host publishes kw: it must be the target just handed out
                assert after["kw"] == t["wait"], what
        if kind == "K":
            assert _reached(after["query"], t["join"]), what
        if kind == "L" and good:
            assert _reached(after["lufs_tp"], t["wait"]), what
        if kind == "D" and good:
            assert _reached(after["tp"], t["join"]) and _reached(after["prep"], t["start"]), what
        if kind == "P" and good:
            assert _reached(after["prep"], t["start"]), what
            if int(w[3]):
                assert _reached(after["tail"], t["tail_target"]), what
        if good or kind == "K":
            for pre, post in zip(t["seg_pre"], t["seg_post"]):
                assert _reached(after["seg"], pre) and _reached(after["seg"], post), what
        # a failed pipelined launch or flush: bit-equal
        if kind in ("P", "F") and not good:
            assert after == before, what
        if kind == "P" and good:
            assert t["gen"] != 0 and after["mirror_gen"] == t["gen"], what
            assert last_par is None or (t["gen"] & 1) != last_par, what
            last_par = t["gen"] & 1
            pend_n_cf = int(w[1])
        if after["pend"]:
            assert after["pend_nq"] == M.meter_segment_wgs(pend_n_cf), what
        if kind == "F" and good:
            assert not after["pend"], what
            for p in (0, 1):
                assert M.sdiff(after["seg_par"][p], after["seg"]) <= 0, what


def _trace(lines, steps):
    before = [M.zero()] + [m for _, m in steps[:-1]]
    return [(ln, t, b, a) for ln, (t, a), b in zip(lines, steps, before)]


# ---- step tables ----

def _table():
    """every step kind and outcome, from the zero ledger and from every count at 2^32 - 3 (each target and
    count wraps inside the step), with nothing pending and -- pipelined, flush -- behind a pipelined step"""
    lines = []
    for start in (["Z"], ["Z", f"S {NEAR_WRAP}"]):
        for n in N_CF:
            for C in CH:
                for res in ("ok", "fail"):
                    lines += start + [f"D {n} {C} {res}"]
                    lines += start + [f"L {n} {res}"]
                    for fr in FRAMES:
                        lines += start + [f"K {n} {C} {_fr(fr)} {res}"]
                for tail in (0, 1):
                    for res in ("ok", "fail", "launched", "waited"):
                        lines += start + [f"P {n} {C} {tail} {res}"]
                        lines += start + [f"P 9 {C} {tail} ok", f"P {n} {C} {tail} {res}"]
                for res in ("ok", "fail"):
                    lines += start + [f"P {n} {C} 1 ok", f"F {res}"]
        for fr in FRAMES:
            lines += start + [f"B {_fr(fr)} ok"]
            lines += start + ["P 512 2 1 ok", "F ok", f"B {_fr(fr)} ok", f"B {_fr(fr)} ok"]
        lines += start + ["F ok"] + start + ["F fail"]
        lines += start + ["P 9 2 1 ok"] * 4 + ["F ok"]   # (from 2^32 - 3: the generation crosses 0xFFFFFFFF -> 2)
    return lines


def test_step_tables_match_the_model(dump):
    lines = _table()
    got, want = dump(lines), _model(lines)
    _assert_same(lines, got, want)
    # from 2^32 - 3 a step that adds 3 or more to a count takes it, and its target, past the wrap
    for i, ln in enumerate(lines):
        if ln.startswith("S ") and lines[i + 1].split()[0] in "DK" and int(lines[i + 1].split()[1]) >= 7:
            t, m = got[i + 1]
            assert t["wait"] == m["kw"] == int(lines[i + 1].split()[1]) - 3, (lines[i + 1], t, m)


def test_steps_by_hand(dump):
    """a few rows worked out from the rules by hand, so the header and the model cannot agree on a wrong rule"""
    got = dump(["Z", "D 8 2 ok", "P 9 1 1 ok", "P 512 2 1 ok", "F ok", "K 8192 2 2 2048 1 fail",
                f"S {2 ** 32 - 1}", "P 8 2 0 ok", "L 3 ok"])
    t, m = got[1]   # direct, 8 channel-frames of 2 channels: one meter workgroup
    assert (t["wait"], t["start"], t["join"], t["q_n"], t["par"], t["seg_pre"], t["seg_post"]) == (8, 2, 8, 1, [0], [0], [0])
    assert (m["kw"], m["tp"], m["prep"], m["seg"], m["seg_par"], m["cur"]) == (8, 8, 2, 1, [1, 0], 1)
    t, m = got[2]   # pipelined, nothing pending: no segment in the grid, 9 channel-frames leave 2 workgroups pending
    assert (t["q_n"], t["start"], t["tail_target"], t["gen"], t["par"], t["seg_pre"], t["seg_post"]) == (0, 3, 1, 1, [1], [0], [1])
    assert (m["prep"], m["seg"], m["tail"], m["pend"], m["pend_nq"], m["pend_par"], m["cur"]) == (3, 1, 1, 1, 2, 1, 0)
    t, m = got[3]   # pipelined, runs the 2 pending workgroups (parity 1): seg_par[1] = 1 + 2 before the targets
    assert (t["q_n"], t["start"], t["tail_target"], t["gen"], t["par"], t["seg_pre"], t["seg_post"]) == (2, 5, 2, 2, [0], [1], [3])
    assert (m["seg"], m["seg_par"], m["pend_nq"], m["pend_par"], m["kw"], m["tp"]) == (3, [1, 3], 64, 0, 8, 8)
    t, m = got[4]   # flush: the 64 pending workgroups of parity 0
    assert (t["q_n"], m["seg"], m["seg_par"], m["pend"]) == (64, 67, [67, 3], 0)
    t, m = got[5]   # chunks, failed launch: kept as advanced; queries ceil(2048 / 4) * 2 + ceil(1 / 4) * 2
    assert (t["wait"], t["join"], t["par"], t["seg_pre"], t["seg_post"]) == (8 + 8192, 1026, [1, 0], [3, 67], [67, 3])
    assert (m["kw"], m["query"], m["cur"]) == (8200, 1026, 1)
    t, m = got[7]   # the generation after 0xFFFFFFFF is 2; prep 2^32 - 1 + 2 wraps to 1
    assert (t["gen"], t["start"], m["prep"], m["tail"]) == (2, 1, 1, 2 ** 32 - 1)
    t, m = got[8]
    assert (t["wait"], m["lufs_tp"]) == (2, 2)


# ---- sequences ----

def _sequence(rng, near_wrap):
    """200 steps of one context as the entry points drive it: a pending segment is flushed before any
    step but a pipelined one (a failed flush ends the call: the step is not taken); each batch launch and
    each flush fails with probability 0.1"""
    lines = ["Z"]
    if near_wrap:   # (within 40: the counts that grow by one or two per step -- generation, tail, prep -- wrap too)
        lines.append(f"S {2 ** 32 - rng.randint(1, rng.choice((40, 3000)))}")
    tail = rng.randint(0, 1)
    pend = False
    while len(lines) < 200:
        res = "fail" if rng.random() < 0.1 else "ok"
        C = rng.choice(CH)
        n = C * rng.choice((1, 3, 4, 5, 256, 511, 512, 2048))
        kind = rng.choices("PDFKBLZ", (35, 20, 10, 10, 10, 10, 2))[0]
        if kind == "L":     # the counted true peaks go first, then the flush, then the chunks of meters_enqueue
            lines.append(f"L {n} {res}")
            if res == "fail":
                continue
        if kind != "P" and kind != "Z" and pend:
            fres = "fail" if rng.random() < 0.1 else "ok"
            lines.append(f"F {fres}")
            if fres == "fail":
                continue
            pend = False
        if kind == "P":
            lines.append(f"P {n} {C} {tail} {res}")
            pend = pend or res == "ok"
        elif kind == "D":
            lines.append(f"D {n} {C} {res}")
        elif kind == "K":
            k = rng.randint(2, 4)
            fr = [2048] * (k - 1) + [rng.randint(1, 2048)]
            lines.append(f"K {sum(fr) * C} {C} {_fr(fr)} {res}")
        elif kind in "BL":
            fr = [2048] * rng.randint(0, 2) + [rng.randint(1, 2048)]
            lines.append(f"B {_fr(fr)} ok")
        elif kind == "Z":
            lines.append("Z")
            pend = False
    return lines[:200]


def test_sequences_match_the_model_and_keep_the_orders(dump):
    rng = random.Random(20240607)
    seqs = [_sequence(rng, near_wrap=bool(s & 1)) for s in range(300)]
    lines = [ln for sq in seqs for ln in sq]
    kinds = {ln.split()[0] + ln.split()[-1] for ln in lines}
    assert {"Pok", "Pfail", "Dok", "Dfail", "Fok", "Ffail", "Kok", "Kfail", "Bok", "Lok"} <= kinds
    got, want = dump(lines), _model(lines)   # (every sequence starts with Z: one run serves them all)
    _assert_same(lines, got, want)
    wraps = sum(1 for ln, (_, m), (_, b) in zip(lines[1:], got[1:], got) if ln != "Z" and m["kw"] < b["kw"])
    assert wraps > 50, "the sequences started near the wrap never crossed it"
    gen_wraps = sum(1 for (t, m), (_, b) in zip(got[1:], got) if b["mirror_gen"] == 2 ** 32 - 1 and m["mirror_gen"] == 2)
    assert gen_wraps > 5, "no sequence took the mirror generation across 0xFFFFFFFF -> 2"
    _assert_invariants(_trace(lines, want))
    _assert_invariants(_trace(lines, got))
