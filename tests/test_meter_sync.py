"""The meter pipeline's ledger (csrc/meter_sync.hpp: the step functions behind every counter target of the
batch launch path) on the CPU: tests/abi/meter_sync_dump.cpp, a stand-alone host program, takes scripts of
steps and prints each step's targets and the whole ledger, and both must equal
tools/model/meter_sync_model.py's after every step -- step tables from the zero ledger and from one about
to wrap, then long seeded sequences that mix every path with failed batch launches. On both traces the
orders the kernels rely on are checked in the device's own wrap-aware comparison: nothing waits for work
that was never launched, a failed pipelined launch or flush changes nothing, a failed direct or chunked
launch publishes the K-weighting count the prep waits for, the mirror parities alternate, the pending
segment keeps its size, and a flush leaves no segment target ahead of the segment count. The side flag
(MeterSync::side: a meter kernel is on the side stream, unjoined) follows the same traces: only a step that
enqueues there sets it, only the join step clears it, a counted omega_calculate_lufs is told to join exactly
when such a step came since the last join, and a call that ends before its join leaves it set."""
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


def _on_side(w):
    """the line's step enqueued (or may have enqueued) a meter prep or LUFS query on the side stream: chunked
    with chunks and direct whatever the batch launch did, the back-to-back layout, pipelined unless its
    launch failed"""
    return (w[0] == "K" and int(w[3]) > 0) or w[0] in ("D", "E") or (w[0] == "P" and w[-1] != "fail")


def _assert_invariants(trace):
    last_par = None   # mirror parity of the last pipelined launch of this context
    pend_n_cf = None  # n_cf of the step that set the pending segment
    dirty = False     # a step enqueued on the side stream since the last join step
    for i, (ln, t, before, after) in enumerate(trace):
        w = ln.split()
        kind, good, what = w[0], w[-1] == "ok", (i, ln)
        if kind == "Z":
            last_par = pend_n_cf = None
            dirty = False
        # the side flag: set only by a step that enqueues on the side stream -- in every outcome of it, the
        # failed, launched and waited ones included -- and cleared only by the join step
        if _on_side(w):
            dirty = True
            assert after["side"] == 1, what
        elif kind == "J" and good:
            dirty = False
            assert after["side"] == 0, what
        elif kind not in "ZS":
            assert after["side"] == before["side"], what
        assert after["side"] == int(dirty), what
        # a counted omega_calculate_lufs skips its join only when nothing went to the side stream since the last
        if kind == "L":
            assert t["join_side"] == int(bool(int(w[2])) and dirty), what
            if int(w[2]) and not t["join_side"]:
                assert not dirty, what
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
        # a failed pipelined launch or flush: bit-equal, the side flag included
        if kind in ("P", "F") and w[-1] == "fail":
            assert after == before and after["side"] == before["side"], what
        if kind == "P" and w[-1] != "fail":   # (launched, waited: the batch ran with this generation too)
            assert t["gen"] != 0 and after["mirror_gen"] == t["gen"], what
            assert last_par is None or (t["gen"] & 1) != last_par, what
            last_par = t["gen"] & 1
        if kind == "P" and good:
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
                    for counted in (0, 1):
                        lines += start + [f"L {n} {counted} {res}"]
                        lines += start + [f"D {n} {C} ok", f"L {n} {counted} {res}", f"J {res}", f"L {n} {counted} {res}"]
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
            lines += start + [f"E {_fr(fr)} ok", "J fail", f"B {_fr(fr)} ok", "J ok", f"E {_fr(fr)} ok"]
            lines += start + ["P 512 2 1 ok", "F ok", f"B {_fr(fr)} ok", f"B {_fr(fr)} ok"]
        lines += start + ["F ok"] + start + ["F fail"]
        lines += start + ["P 9 2 1 ok"] * 4 + ["F ok"]   # (from 2^32 - 3: the generation crosses 0xFFFFFFFF -> 2)
    return lines


def test_step_tables_match_the_model(dump):
    lines = _table()
    got, want = dump(lines), _model(lines)
    _assert_same(lines, got, want)
    _assert_invariants(_trace(lines, got))   # (every outcome of every step: the side flag's rules above all)
    # from 2^32 - 3 a step that adds 3 or more to a count takes it, and its target, past the wrap
    for i, ln in enumerate(lines):
        if ln.startswith("S ") and lines[i + 1].split()[0] in "DK" and int(lines[i + 1].split()[1]) >= 7:
            t, m = got[i + 1]
            assert t["wait"] == m["kw"] == int(lines[i + 1].split()[1]) - 3, (lines[i + 1], t, m)


def test_steps_by_hand(dump):
    """a few rows worked out from the rules by hand, so the header and the model cannot agree on a wrong rule"""
    got = dump(["Z", "D 8 2 ok", "P 9 1 1 ok", "P 512 2 1 ok", "F ok", "K 8192 2 2 2048 1 fail",
                f"S {2 ** 32 - 1}", "P 8 2 0 ok", "L 3 1 ok", "L 3 0 ok", "J ok", "L 3 1 ok", "E 1 5 ok"])
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
    assert [m["side"] for _, m in got[:9]] == [0, 1, 1, 1, 1, 1, 1, 1, 1]   # (a flush is no join; S keeps it)
    t, m = got[8]   # counted true peaks behind batches: they count in, and the call is told to join first
    assert (t["wait"], t["join_side"], m["lufs_tp"], m["side"]) == (2, 1, 2, 1)
    t, m = got[9]   # not counted: no counter moves, no join before (it joins behind its true peak)
    assert (t["join_side"], m["lufs_tp"], m["side"]) == (0, 2, 1)
    t, m = got[11]  # after the join: nothing to join
    assert (got[10][1]["side"], t["wait"], t["join_side"], m["lufs_tp"], m["side"]) == (0, 5, 0, 5, 0)
    t, m = got[12]  # the back-to-back layout: no counter, one chunk, the side stream used again
    assert (t["par"], m["cur"], m["side"], m["lufs_tp"]) == ([0], 1, 1, 5)


def test_a_call_that_ends_before_its_join_keeps_the_side_flag(dump):
    """omega_calculate_lufs behind a batch whose prep went to the side stream: a call that ends early -- refused,
    or a failed launch -- takes no join step, so the flag stays and the next counted call still joins first"""
    lines = ["Z", "D 32 2 ok",
             "L 4 0 ok",            # frames of another length: the true peak went out, the weighting failed: no join
             "L 4 1 fail",          # counted: the join's event record failed (no J), or the true-peak launch
             "L 4 1 fail", "J ok", "L 4 1 ok", "B 1 2 ok",   # a whole counted call: told to join, joins, counts in
             "L 4 1 ok", "B 1 2 ok",                         # the steady state: nothing to join
             "P 32 2 1 fail", "L 4 1 ok", "F ok", "B 1 2 ok",   # a failed pipelined launch put nothing there
             "P 32 2 1 launched", "L 4 1 fail"]              # one that failed after its launch may have
    got, want = dump(lines), _model(lines)
    _assert_same(lines, got, want)
    _assert_invariants(_trace(lines, got))
    side = [m["side"] for _, m in got]
    join = [t["join_side"] for t, _ in got]
    assert side == [0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert [join[i] for i in (2, 3, 4, 6, 8, 11, 15)] == [0, 1, 1, 0, 0, 0, 1]


# ---- sequences ----

def _sequence(rng, near_wrap):
    """200 steps of one context as the entry points drive it: a pending segment is flushed before any
    step but a pipelined one (a failed flush ends the call: the step is not taken); each batch launch and
    each flush fails with probability 0.1. omega_calculate_lufs (L), counted or not: the join step first where
    the model's step says so, the true peaks, the join of the uncounted path, the flush, the chunks of
    meters_enqueue -- and with probability 0.1 each the call ends before its join or at its true-peak launch.
    E: the back-to-back layout, its chunks on the side stream."""
    lines = ["Z"]
    led = [M.zero()]   # the model's ledger after the lines so far: what the entry point reads its join from

    def emit(ln):
        lines.append(ln)
        led[0] = M.step(led[0], ln)[1]

    if near_wrap:   # (within 40: the counts that grow by one or two per step -- generation, tail, prep -- wrap too)
        emit(f"S {2 ** 32 - rng.randint(1, rng.choice((40, 3000)))}")
    tail = rng.randint(0, 1)
    pend = False
    while len(lines) < 200:
        res = "fail" if rng.random() < 0.1 else "ok"
        C = rng.choice(CH)
        n = C * rng.choice((1, 3, 4, 5, 256, 511, 512, 2048))
        kind = rng.choices("PDFKBLZE", (35, 20, 10, 10, 10, 10, 2, 5))[0]
        if kind == "L":     # the true peaks go first, then the flush, then the chunks of meters_enqueue
            counted = rng.randint(0, 1)
            if M.lufs_tp(led[0], n, counted)[0]["join_side"]:
                if rng.random() < 0.1:   # (the join's event record or wait failed: the call ends, no step taken)
                    continue
                emit("J ok")
            emit(f"L {n} {counted} {res}")
            if res == "fail":
                continue
            if not counted:
                if rng.random() < 0.1:   # (the weighting refused or failed: no join)
                    continue
                emit("J ok")
        if kind != "P" and kind != "Z" and pend:
            fres = "fail" if rng.random() < 0.1 else "ok"
            emit(f"F {fres}")
            if fres == "fail":
                continue
            pend = False
        if kind == "P":
            if res == "ok" and rng.random() < 0.1:   # (the tail wait or the prep launch failed)
                res = rng.choice(("launched", "waited"))
            emit(f"P {n} {C} {tail} {res}")
            pend = pend or res == "ok"
        elif kind == "D":
            emit(f"D {n} {C} {res}")
        elif kind == "K":
            k = rng.randint(2, 4)
            fr = [2048] * (k - 1) + [rng.randint(1, 2048)]
            emit(f"K {sum(fr) * C} {C} {_fr(fr)} {res}")
        elif kind in "BLE":
            fr = [2048] * rng.randint(0, 2) + [rng.randint(1, 2048)]
            emit(f"{'E' if kind == 'E' else 'B'} {_fr(fr)} ok")
        elif kind == "Z":
            emit("Z")
            pend = False
    return lines[:200]


def test_sequences_match_the_model_and_keep_the_orders(dump):
    rng = random.Random(20240607)
    seqs = [_sequence(rng, near_wrap=bool(s & 1)) for s in range(300)]
    lines = [ln for sq in seqs for ln in sq]
    kinds = {ln.split()[0] + ln.split()[-1] for ln in lines}
    assert {"Pok", "Pfail", "Plaunched", "Pwaited", "Dok", "Dfail", "Fok", "Ffail", "Kok", "Kfail", "Bok", "Eok",
            "Lok", "Lfail", "Jok"} <= kinds
    for counted in (0, 1):   # both values of counted, and counted calls with and without a join before them
        assert any(ln.startswith("L ") and int(ln.split()[2]) == counted for ln in lines)
    assert any(a == "J ok" and b.split()[0] == "L" and b.split()[2] == "1" for a, b in zip(lines, lines[1:]))
    got, want = dump(lines), _model(lines)   # (every sequence starts with Z: one run serves them all)
    _assert_same(lines, got, want)
    wraps = sum(1 for ln, (_, m), (_, b) in zip(lines[1:], got[1:], got) if ln != "Z" and m["kw"] < b["kw"])
    assert wraps > 50, "the sequences started near the wrap never crossed it"
    gen_wraps = sum(1 for (t, m), (_, b) in zip(got[1:], got) if b["mirror_gen"] == 2 ** 32 - 1 and m["mirror_gen"] == 2)
    assert gen_wraps > 5, "no sequence took the mirror generation across 0xFFFFFFFF -> 2"
    _assert_invariants(_trace(lines, want))
    _assert_invariants(_trace(lines, got))
