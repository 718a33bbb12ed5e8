"""Beat detection and band tracking: tests/rhythm_ref.py against tests/golden/rhythm.npz (recorded from the
reference's own BeatDetectionPanel and FrequencyBandTrackerPanel by tests/golden/gen_rhythm.py), both facades' host
logic against the recorded attribute sequences, and omega_rhythm_features on the device against the golden rows.

Bars on the device. Exact: the flags. 1e-12 relative: columns 1-12, sums of non-negative float64 terms of exactly
representable inputs (float32 bins, float32 differences, products of a float64 frequency and a float32 bin rounded
once) -- any summation order of n <= 16384 such terms is within about log2(n) 2^-53 = 1.6e-15 of the recorded
math.fsum. 1e-9 relative, the project's float64 bar: column 13, sum (f - c)^2 s, whose c comes from a total rounded
to float32; d/dc of the sum vanishes at the centroid, so the 26 2^-24 difference in c enters at second order.

Bars on the facades, with u = 2^-24. The reference's np.sum over the float32 spectrum is numpy's float32 pairwise
sum, within 25 u relative of exact for K <= 8193 non-negative terms (tests/test_voice.py counts the adds); the
facade rounds the device's float64 sum to float32 once, within u: 26 u per sum, 52 u for a quotient of two, under
F32_BAR = 64 u = 3.8e-6. Held to it: onset strength, beat strength, band energies, RMS, peaks, balance, tilt,
centroid, total_energy_db, the dB and normalised values, the reference level, syncopation and groove strength
(ratios and weighted sums of such values). Held to 1e-9: BPM, confidence, regularity, complexity, phase, spread.
Equal: is_beat, the beat count, last_beat_time, dominant_band, the history lengths, the hold times, the flash
counter. The two recorded sequences draw their spectra from a pool on the 2^-10 grid, where every float32 sum is
exact in any order (tests/golden/gen_rhythm.py says why: complexity and spread descend from float32 totals and
could not meet 1e-9 otherwise); the other groups carry unquantised spectra and pin the rows.

The observed worst deviation per column is printed (run with -s).
Observed on an MI355X over all golden groups, float32 and float64 frames, host and device memory, strided and
overlapping rows, with and without frames (worst per column, relative to math.fsum): sumsq 2.05e-16, spec_sum
2.04e-16, flux 0, kick 0, band0-3 0, band4 2.03e-16, band5 2.12e-16, band6 2.02e-16, spec_fsum 2.02e-16 (bar 1e-12);
spread_sum 2.08e-16 (bar 1e-9); flags equal on every frame; chained calls, two-part calls and a call with state_in
and state_out in one buffer bit-equal to one call; the state unchanged through an all-gated call; both 300-step
sequences through both panels' update() matched step by step. On the recorded rows the host logic's worst float
attribute deviation is spectral_spread's 1.3e-16; every other attribute is equal (the pool's sums are exact).
Time per frame, F = 4096 frames of K = 513 bins in device memory without audio, device events, the best of five
calls: 55.7 us per call, 13.6 ns per frame. A frame moves 2 K 4 + 14 * 8 = 4216 bytes (its row, the predecessor's
row, its output row): 310 GB/s, some 4 % of the HBM rate, and the 8.4 MB of spectra stay in the cache between the
calls. At this size the call is two dependent launches of 16 workgroups per CU each; their launch and drain time,
not the bytes, sets the figure.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rhythm_ref as RR
from conftest import REPO, load_golden
from host_program import compile_host_program

F32_BAR = 64 * 2.0 ** -24
GROUPS = ("app", "k2", "k8193", "lin", "fs8", "zero", "nonfinite", "gated", "allgated")
SEQS = ("seq_kick", "seq_irreg")
EXACT = ("n_", "is_beat", "last_beat_time", "info_last_beat_time", "has_prev", "beat_flash_time", "dominant_band",
         "info_dominant_band", "hold_time_")
F64 = ("current_bpm", "bpm_confidence", "beat_phase", "rhythmic_complexity", "beat_regularity", "info_current_bpm",
       "info_bpm_confidence", "info_beat_phase", "pattern_regularity", "pattern_complexity", "spectral_spread",
       "info_spectral_spread")
WORST = {}


@pytest.fixture(scope="module")
def G():
    return load_golden("rhythm")


class Clock:
    T0 = 1000.0

    def __init__(self, step):
        self.t, self.step = self.T0, step

    def at(self, i):
        self.t = self.T0 + i * self.step

    def __call__(self):
        return self.t


def inputs(G, g):
    return G[f"{g}/spec"], G[f"{g}/frame"].astype(np.float64), G[f"{g}/freqs"]


def seq_inputs(G, seq):
    return (G[f"{seq}/pool"][G[f"{seq}/idx"]], G[f"{seq}/audio_pool"][G[f"{seq}/audio_idx"]].astype(np.float64),
            G[f"{seq}/freqs"])


def check_rows(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg=f"{what}: flags")
    for c in range(1, len(RR.COLUMNS)):
        d = np.abs(got[:, c] - want[:, c]) / np.where(want[:, c] != 0, np.abs(want[:, c]), 1.0)
        w = float(np.max(d)) if len(d) else 0.0
        WORST[RR.COLUMNS[c]] = max(WORST.get(RR.COLUMNS[c], 0.0), w)
    print(f"{what}: worst so far " + ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))
    for c in range(1, len(RR.COLUMNS)):
        d = np.abs(got[:, c] - want[:, c])
        bar = 1e-9 if c == 13 else 1e-12
        assert np.all(d <= bar * np.abs(want[:, c])), (what, RR.COLUMNS[c], float(d.max()))


def bar_of(name):
    if any(name == e or (e.endswith("_") and name.startswith(e)) for e in EXACT):
        return 0.0
    return 1e-9 if name in F64 else F32_BAR


def check_attrs(names, got, want, what):
    for n, w in zip(names, want):
        g, bar = float(got[n]), bar_of(n)
        d = abs(g - w) / abs(w) if w != 0 else abs(g)
        if bar:
            WORST["attr " + n] = max(WORST.get("attr " + n, 0.0), d)
        ok = (g == w or (np.isnan(g) and np.isnan(w))) if bar == 0.0 else (abs(g - w) <= bar * abs(w) or (np.isnan(g) and np.isnan(w)))
        assert ok, (what, n, g, w)


def gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rhythm", os.path.join(REPO, "tests", "golden", "gen_rhythm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- CPU ----

@pytest.mark.parametrize("g", GROUPS + SEQS)
def test_ref_equals_golden(G, g):
    spec, frames, freqs = seq_inputs(G, g) if g in SEQS else inputs(G, g)
    rows, _ = RR.rows(spec, frames, freqs)
    check_rows(rows, G[f"{g}/row"], f"ref {g}")


def test_golden_covers_the_cases(G):
    assert G["k2/spec"].shape[1] == 2 and G["k2/frame"].shape[1] == 1
    assert G["app/spec"].shape[1] == 513 and G["app/frame"].shape[1] == 2048
    assert G["k8193/spec"].shape[1] == 8193 and G["k8193/frame"].shape[1] == 16384
    assert not np.any(G["k2/row"][:, 4:12])  # lo >= hi: every band is empty
    assert np.array_equal(G["lin/freqs"], np.linspace(0, 20000, 512))
    e = RR.edges(G["fs8/freqs"])
    assert e[8] == 0 and e[9] == 513  # 8000 and 20000 Hz beyond the spectrum
    assert np.array_equal(G["fs8/row"][:, 11], G["fs8/row"][:, 2])
    assert not np.any(G["zero/spec"][1]) and not np.any(G["zero/row"][1, 2:])
    assert list(G["nonfinite/row"][:, 0].astype(int)) == [4, 1, 0, 1, 0]
    assert np.isnan(G["nonfinite/frame"][1]).any() and np.isinf(G["nonfinite/spec"][3]).any()
    assert list(G["gated/row"][:, 0].astype(int)) == [6, 4, 2, 2, 0, 0, 2]
    assert list(G["allgated/row"][:, 0].astype(int)) == [6, 6, 6]
    bn = [str(n) for n in G["beat_names"]]
    b = G["seq_kick/beat"]
    assert b[-1, bn.index("n_beats")] >= 8 and b[-1, bn.index("current_bpm")] != 120.0
    assert abs(float(G["seq_kick/clock_step"]) - 1 / 60) < 1e-15 and abs(float(G["seq_irreg/clock_step"]) - 1 / 30) < 1e-15
    b = G["seq_irreg/beat"]
    full = (b[:, bn.index("n_beats")] >= 8) & (b[:, bn.index("n_patterns")] == 4)
    reg, sync = b[:, bn.index("pattern_regularity")], b[:, bn.index("pattern_syncopation")]
    assert np.any(full & (reg == 0)) and np.any(full & (reg > 0))
    assert np.any(full & (sync == 1)) and np.any(full & (sync > 0) & (sync < 1)) and np.any(full & (sync == 0))
    assert np.any(b[:, bn.index("n_patterns")] == 0)  # gated steps
    assert len(G["seq_kick/idx"]) == 300 and len(G["seq_irreg/idx"]) == 300


def host_panels(fs, clock):
    from omega_gpu.beat_detection import BeatDetectionPanel
    from omega_gpu.frequency_band_tracker import FrequencyBandTrackerPanel
    bp = BeatDetectionPanel.__new__(BeatDetectionPanel)
    bp._host_init(fs, clock)
    tp = FrequencyBandTrackerPanel.__new__(FrequencyBandTrackerPanel)
    tp._host_init(fs)
    return bp, tp


@pytest.mark.parametrize("seq", SEQS)
def test_host_logic_reproduces_sequence(G, seq):
    """Both facades' host logic on the recorded rows gives the reference's attributes after every step."""
    from omega_gpu import _rhythm as R
    M = gen()
    clock = Clock(float(G[f"{seq}/clock_step"]))
    bp, tp = host_panels(48000, clock)
    spec, _, freqs = seq_inputs(G, seq)
    empty = R.empty_bands(freqs)
    bn, tn = [str(n) for n in G["beat_names"]], [str(n) for n in G["track_names"]]
    state = None
    for i, (row, wb, wt) in enumerate(zip(G[f"{seq}/row"], G[f"{seq}/beat"], G[f"{seq}/track"])):
        clock.at(i)
        assert bp._apply_row(row)
        if not int(row[0]) & RR.FLAG_GATED:  # (has_prev: the state the device would hand back)
            state = np.concatenate([[1.0, 513.0], spec[i].astype(np.float64)])
        bp.detector._state = state
        trow = row.copy()
        trow[0] = 0  # the tracker's call has no gate; its columns are the same sums
        assert tp._apply_row(trow, empty)
        check_attrs(bn, M.beat_attrs(bp), wb, (seq, i))
        check_attrs(tn, M.track_attrs(tp), wt, (seq, i))
    print({k: v for k, v in WORST.items() if k.startswith("attr") and v > 0})


def test_host_logic_leaves_state_on_nonfinite():
    bp, tp = host_panels(48000, Clock(1.0))
    row = np.zeros(len(RR.COLUMNS))
    row[0] = RR.FLAG_NONFINITE
    assert not bp._apply_row(row) and not tp._apply_row(row)
    assert len(bp.detector.onset_strength_history) == 0 and len(tp.tracker.band_history["bass"]) == 0
    assert not hasattr(tp.tracker, "total_energy_history")
    from omega_gpu import UnsupportedError
    with pytest.raises(UnsupportedError):
        tp.tracker.add_custom_band("x", "X", 1, 2, (0, 0, 0))
    with pytest.raises(UnsupportedError):
        tp.tracker.remove_band("bass")


def test_configure_checks_its_arguments_without_a_device(tmp_path):
    """tests/abi/rhythm_args.cpp: omega_rhythm_configure's refusals and omega_rhythm_state_size, on the CPU."""
    lib = os.path.join(REPO, "audio-analyzer-omega_amd", "lib")
    exe = compile_host_program(os.path.join(REPO, "tests", "abi", "rhythm_args.cpp"), str(tmp_path / "rhythm_args"))
    env = dict(os.environ, LD_LIBRARY_PATH=lib + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, os.path.join(lib, "libomega.so")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout


# ---- GPU ----

@pytest.fixture(scope="module")
def det():
    from omega_gpu.beat_detection import BeatDetector
    return BeatDetector(48000)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_device_rows(G, det, g):
    """Host memory, float64 and float32 frames, and frames == NULL, against the golden rows and the state."""
    spec, frames, freqs = inputs(G, g)
    rows, state = det.analyze_frames(spec, frames, freqs)
    check_rows(rows, G[f"{g}/row"], f"device {g}")
    _, want = RR.rows(spec, frames, freqs)
    np.testing.assert_array_equal(state, want)
    r32, s32 = det.analyze_frames(spec, G[f"{g}/frame"], freqs)
    np.testing.assert_array_equal(r32, rows)
    np.testing.assert_array_equal(s32, state)
    finite = np.all(np.isfinite(spec), axis=1)
    want, wstate = RR.rows(spec, None, freqs)
    got, gstate = det.analyze_frames(spec, None, freqs)
    check_rows(got, want, f"device {g} without frames")
    np.testing.assert_array_equal(gstate, wstate)
    assert not np.any(got[:, 1]) and not np.any(got[finite, 0].astype(int) & RR.FLAG_GATED)


@pytest.mark.gpu
def test_device_variants(G, det):
    """Device memory, strided and overlapping rows give the host call's rows bit for bit."""
    import torch
    spec, frames, freqs = inputs(G, "gated")
    base, bstate = det.analyze_frames(spec, frames, freqs)
    K, m = spec.shape[1], frames.shape[1]
    dspec = torch.zeros((len(spec), K + 87), dtype=torch.float32, device="cuda:0")
    dspec[:, :K] = torch.from_numpy(spec)
    dfr = torch.zeros((len(frames), m + 5), dtype=torch.float64, device="cuda:0")
    dfr[:, :m] = torch.from_numpy(frames)
    rd, sd = det.analyze_frames(dspec[:, :K], dfr[:, :m], freqs)  # strided views, device memory
    np.testing.assert_array_equal(rd.cpu().numpy(), base)
    np.testing.assert_array_equal(sd.cpu().numpy(), bstate)
    rd32, _ = det.analyze_frames(dspec[:, :K], dfr[:, :m].float(), torch.from_numpy(freqs))
    np.testing.assert_array_equal(rd32.cpu().numpy(), base)
    rn, _ = det.analyze_frames(dspec[:, :K], None, freqs)
    check_rows(rn.cpu().numpy(), RR.rows(spec, None, freqs)[0], "device memory without frames")
    # overlapping rows: unfold views of one stream of samples and one of bins against their contiguous copies
    stream = torch.from_numpy(np.concatenate(frames)).to("cuda:0")
    view = stream.unfold(0, m, 16)[:9]
    bins = torch.from_numpy(np.concatenate(spec[:2])).to("cuda:0")
    sv = bins.unfold(0, K, 57)[:9]
    ro, so = det.analyze_frames(sv, view, freqs)
    rc, sc = det.analyze_frames(sv.contiguous(), view.contiguous(), freqs)
    np.testing.assert_array_equal(ro.cpu().numpy(), rc.cpu().numpy())
    np.testing.assert_array_equal(so.cpu().numpy(), sc.cpu().numpy())
    check_rows(ro.cpu().numpy(), RR.rows(sv.cpu().numpy(), view.cpu().numpy(), freqs)[0], "device overlapping")
    # state_in and state_out in one buffer, through the C entry point
    from omega_gpu import _lib as L
    a, sa = det.analyze_frames(spec[:3], frames[:3], freqs)
    buf = sa.copy()
    out = np.empty((len(spec) - 3, len(RR.COLUMNS)))
    s2, f2 = np.ascontiguousarray(spec[3:]), np.ascontiguousarray(frames[3:])
    det._dev._eng._check(L.lib().omega_rhythm_features(
        det._dev._eng._ctx, s2.ctypes.data, K, f2.ctypes.data, 1, len(s2), m, buf.ctypes.data, buf.ctypes.data,
        out.ctypes.data, L.MEM_HOST))
    np.testing.assert_array_equal(np.concatenate([a, out]), base)
    np.testing.assert_array_equal(buf, bstate)


@pytest.mark.gpu
@pytest.mark.parametrize("g", ("app", "nonfinite", "gated", "k2"))
def test_chaining_is_bit_equal(G, det, g):
    """F frames in one call against F one-frame calls chained through the blob, and against two parts."""
    spec, frames, freqs = inputs(G, g)
    rows, state = det.analyze_frames(spec, frames, freqs)
    st, got = None, []
    for i in range(len(spec)):
        r, st = det.analyze_frames(spec[i:i + 1], frames[i:i + 1], freqs, st)
        got.append(r[0])
    np.testing.assert_array_equal(np.array(got), rows)
    np.testing.assert_array_equal(st, state)
    a, sa = det.analyze_frames(spec[:2], frames[:2], freqs)
    b, sb = det.analyze_frames(spec[2:], frames[2:], freqs, sa)
    np.testing.assert_array_equal(np.concatenate([a, b]), rows)
    np.testing.assert_array_equal(sb, state)


@pytest.mark.gpu
def test_multi_launch_chain_is_bit_equal(det):
    """A call of more than 65536 frames takes several launches that hand the state on through the context's two
    blobs. 65537 frames of K = 2 bins without audio, the smallest such call: non-finite rows lie on both sides of
    the launch boundary (65535, 65536) and before it, so the last launch finds its predecessor, and the call its
    outgoing state, in the launch before. One call equals the chained calls 65536 + 1 and 1 + 65536, and the same
    call through the C entry point with state_in and state_out in one buffer, bit for bit."""
    from omega_gpu import _lib as L
    F, K = 65537, 2
    spec = np.random.default_rng(11).random((F, K), dtype=np.float32)
    bad = {3: np.nan, 40000: np.inf, 65534: -np.inf, 65535: np.nan, 65536: np.inf}
    for i, v in bad.items():
        spec[i, i & 1] = v
    freqs = np.array([0.0, 100.0])
    rows, state = det.analyze_frames(spec, None, freqs)
    flags = rows[:, 0].astype(int) & RR.FLAG_NONFINITE
    assert sorted(np.flatnonzero(flags)) == sorted(bad)
    np.testing.assert_array_equal(state, np.concatenate([[1.0, K], spec[65533].astype(np.float64)]))
    for cut in (65536, 1):
        a, sa = det.analyze_frames(spec[:cut], None, freqs)
        b, sb = det.analyze_frames(spec[cut:], None, freqs, sa)
        np.testing.assert_array_equal(np.concatenate([a, b]), rows)
        np.testing.assert_array_equal(sb, state)
    buf = np.zeros(len(state))  # (a blob that is not valid: a stream's first call)
    out = np.empty_like(rows)
    det._dev._eng._check(L.lib().omega_rhythm_features(
        det._dev._eng._ctx, spec.ctypes.data, K, None, 0, F, 0, buf.ctypes.data, buf.ctypes.data, out.ctypes.data,
        L.MEM_HOST))
    np.testing.assert_array_equal(out, rows)
    np.testing.assert_array_equal(buf, state)


@pytest.mark.gpu
def test_all_gated_call_passes_the_state_through(G, det):
    spec, frames, freqs = inputs(G, "app")
    _, state = det.analyze_frames(spec, frames, freqs)
    gs, gf, _ = inputs(G, "allgated")
    pad = np.zeros((len(gf), frames.shape[1]))
    pad[:, :gf.shape[1]] = gf
    rows, after = det.analyze_frames(gs, pad, freqs, state)
    assert list(rows[:, 0].astype(int)) == [2, 2, 2] and np.all(rows[:, 3] > 0)
    np.testing.assert_array_equal(after, state)
    want, _ = RR.rows(gs, pad, freqs, state)
    check_rows(rows, want, "all gated behind a state")
    rows, none = det.analyze_frames(gs, pad, freqs)  # and without one: no live frame yet
    assert list(rows[:, 0].astype(int)) == [6, 6, 6] and none[0] == 0 and none[1] == 513 and not np.any(none[2:])


@pytest.mark.gpu
@pytest.mark.parametrize("seq", SEQS)
def test_update_sequence_on_device(G, seq):
    """Both panels' update() against the reference's attributes after every step."""
    from omega_gpu import BeatDetectionPanel, FrequencyBandTrackerPanel
    M = gen()
    clock = Clock(float(G[f"{seq}/clock_step"]))
    bp, tp = BeatDetectionPanel(48000, clock=clock), FrequencyBandTrackerPanel(48000)
    spec, frames, freqs = seq_inputs(G, seq)
    bn, tn = [str(n) for n in G["beat_names"]], [str(n) for n in G["track_names"]]
    for i, (wb, wt) in enumerate(zip(G[f"{seq}/beat"], G[f"{seq}/track"])):
        clock.at(i)
        bp.update(spec[i], frames[i], freqs)
        tp.update(spec[i], freqs)
        check_attrs(bn, M.beat_attrs(bp), wb, (seq, i))
        check_attrs(tn, M.track_attrs(tp), wt, (seq, i))
    assert bp.get_results()["current_bpm"] == bp.detector.current_bpm
    assert set(tp.get_results()["bands"]) == set(tp.tracker.frequency_bands)
    bp.detector.reset()
    assert bp.detector._state is None and len(bp.detector.beat_times) == 0


@pytest.mark.gpu
def test_nonfinite_update_leaves_state(G):
    from omega_gpu import BeatDetectionPanel, FrequencyBandTrackerPanel
    M = gen()
    spec, frames, freqs = inputs(G, "nonfinite")
    bp, tp = BeatDetectionPanel(48000, clock=Clock(1.0)), FrequencyBandTrackerPanel(48000)
    bp.update(spec[0], frames[0], freqs)
    tp.update(spec[0], freqs)
    before = (M.beat_attrs(bp), M.track_attrs(tp), bp.detector._state.copy())
    bp.update(spec[1], frames[1], freqs)  # a NaN sample
    bp.update(spec[3], frames[3], freqs)  # an infinite bin
    tp.update(spec[3], freqs)
    assert M.beat_attrs(bp) == before[0] and M.track_attrs(tp) == before[1]
    np.testing.assert_array_equal(bp.detector._state, before[2])


@pytest.mark.gpu
def test_unsupported_shapes_leave_the_configured_one(G, det):
    import omega_gpu
    from omega_gpu import _lib as L
    from omega_gpu import _rhythm as R
    spec, frames, freqs = inputs(G, "app")
    base, _ = det.analyze_frames(spec, frames, freqs)
    for K, m in ((1, 2048), (8194, 2048), (513, 16385), (513, 0), (0, 2048)):
        if K >= 1 and m >= 1:
            with pytest.raises(omega_gpu.UnsupportedError):
                det.analyze_frames(np.zeros((1, K), np.float32), np.zeros((1, m)), np.arange(K, dtype=np.float64))
        cfg = L.RhythmConfig(K, m)
        f = np.arange(max(K, 1), dtype=np.float64)
        e = np.zeros(10, np.int32)
        assert L.lib().omega_rhythm_configure(det._dev._eng._ctx, C.byref(cfg), f.ctypes.data, e.ctypes.data) == L.EUNSUP
    assert det._dev._configured[:2] == (513, 2048)
    again, _ = det.analyze_frames(spec, frames, freqs)
    np.testing.assert_array_equal(again, base)
    assert R.state_len(513) == L.lib().omega_rhythm_state_size(513)


@pytest.mark.gpu
def test_time_per_frame(G, det):
    """F = 4096 frames of K = 513 bins in device memory, timed with device events (the figure is in the module's
    docstring; no bar is set on it)."""
    import torch
    F, K = 4096, 513
    rng = np.random.default_rng(3)
    spec = torch.from_numpy(rng.random((F, K), dtype=np.float32)).to("cuda:0")
    freqs = np.fft.rfftfreq(1024, 1 / 48000)
    det.analyze_frames(spec, None, freqs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(5):
        t0.record()
        det.analyze_frames(spec, None, freqs)
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    per = best * 1e3 / F
    moved = 2 * K * 4 + len(RR.COLUMNS) * 8
    print(f"rhythm: {best * 1e3:.1f} us for {F} frames, {per * 1e3:.1f} ns per frame, {moved} bytes per frame, "
          f"{moved / per / 1e3:.1f} GB/s")
    assert np.isfinite(per) and per > 0
