"""Transient detection: tests/tdetect_ref.py against tests/golden/tdetect.npz (recorded from the reference's own
TransientDetectionPanel by tests/golden/gen_tdetect.py), the facade's host logic against the two recorded
update() sequences, and omega_tdetect_features on the device against the golden rows.

Bars on the device. Exact: flags, max |x| (one of the inputs), sum |diff(sign x)|, the peak, start and end
indices, the rolloff index, the guard bits. The generator asserts the margins that make them decidable: the prefix
sums 1e-6 relative away from 0.85 of the total, every |x_i| 1e-9 peak away from a tenth of the peak, the best two
|x| distinct or exactly equal. 1e-12 relative: the spectrum's sums (spec_sum, spec_fsum, the band sums) and sum
x^2 -- any summation order of n <= 8193 non-negative float64 terms is within about log2(n) 2^-53 = 1.4e-15 of the
recorded math.fsum, and the float32 inputs are exact in float64. 1e-9, the project's float64 bar for transform-
and filter-derived values: the envelope mean, the flux spectrum's sum and the flux relative to their own value
(atol 1e-15), mag_sum likewise, hf_energy relative to sum x^2, novelty relative to pi mag_sum (each bin
contributes at most pi times its magnitude; the generator keeps every bin that counts 1e-6 rad away from the
+-pi cut, so no phase flips by 2 pi).

The facade's last_centroid and band_energies against the reference's, F32_BAR = 64 * 2^-24 = 3.8e-6, with u =
2^-24: the reference's np.sum over the float32 spectrum is numpy's float32 pairwise sum, within 25 u relative of
exact for K <= 8193 non-negative terms (tests/test_voice.py counts the adds); the facade rounds the device's
float64 sum to float32 once, within u. The centroid divides a float64 sum by that float32 sum: the two routes
differ by at most 26 u relative. A band energy is one such sum over the total of four: 26 u in the numerator,
26 u in the denominator, 52 u relative of a value <= 1. Every other float attribute: 1e-9 relative. Discrete
attributes (detected, type, history lengths, event count, event time, update counter): equal.

The observed worst deviation per column is printed (run with -s).
Observed on an MI355X over all golden groups, float32 and float64 frames, host and device memory, strided and
overlapping rows (worst per column): spec_sum 0, spec_fsum 1.92e-16, the band sums 0, sum x^2 2.19e-16 (bar
1e-12); envelope 2.12e-15, flux_sum 5.51e-16, flux 2.81e-13 of its own value (a sum of differences of nearly
equal spectra), mag_sum 7.26e-16, hf_energy 2.28e-15 of sum x^2, novelty 1.87e-14 of pi mag_sum (bar 1e-9); every
exact column equal on every frame; chained calls bit-equal to one call; both 300-step sequences through update()
matched step by step.
"""
import numpy as np
import pytest

import tdetect_ref as TR
from conftest import load_golden

F32_BAR = 64 * 2.0 ** -24
GROUPS = ("m256", "m512", "m1024", "app", "m8192", "fs44", "fs16", "k2", "k8193", "zero", "nonfinite", "edge")
SEQS = ("seq_fast", "seq_slow")
SUMS = (3, 13, 14, 16, 17, 18, 19)
WORST = {}


@pytest.fixture(scope="module")
def G():
    return load_golden("tdetect")


class Clock:
    T0 = 1000.0

    def __init__(self, step):
        self.t, self.step = self.T0, step

    def at(self, i):
        self.t = self.T0 + i * self.step

    def __call__(self):
        return self.t


def inputs(G, g):
    return int(G[f"{g}/fs"]), G[f"{g}/spec"], G[f"{g}/frame"].astype(np.float64)


def host_panel(fs, clock):
    from omega_gpu.transient_detection import TransientDetectionPanel
    p = TransientDetectionPanel.__new__(TransientDetectionPanel)
    p._host_init(fs, clock)
    return p


def check_rows(got, want, what, sum_rtol=1e-12, tol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what

    def dev(c, den, atol=0.0):
        d = np.abs(got[:, c] - want[:, c])
        d = np.where(d <= atol, 0.0, d) / np.where(den != 0, np.abs(den), 1.0)
        w = float(np.max(d)) if len(d) else 0.0
        WORST[TR.COLUMNS[c]] = max(WORST.get(TR.COLUMNS[c], 0.0), w)
        return w

    worst = {c: dev(c, want[:, c]) for c in SUMS}
    worst.update({c: dev(c, want[:, c], 1e-15) for c in (1, 4, 5, 7)})
    worst[8] = dev(8, want[:, 3])
    worst[6] = dev(6, np.pi * want[:, 7])
    print(f"{what}: worst so far " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    for c in TR.EXACT:
        np.testing.assert_array_equal(got[:, c], want[:, c], err_msg=f"{what}: {TR.COLUMNS[c]}")
    for c, w in worst.items():
        assert w <= (sum_rtol if c in SUMS else tol), (what, TR.COLUMNS[c], w)


def check_attrs(G, panel, want, what):
    names = [str(n) for n in G["attr_names"]]
    types = [str(t) for t in G["types"]]
    got = {"detected": float(panel.transient_detected), "strength": panel.transient_strength,
           "type": float(types.index(panel.transient_type)), "attack_time": panel.attack_time,
           "decay_time": panel.decay_time, "peak_level": panel.peak_level, "rms_level": panel.rms_level,
           "crest_factor": panel.crest_factor, "envelope": panel.envelope, "sensitivity": panel.sensitivity,
           "centroid": panel.last_centroid, "zcr": panel.last_zcr, "rolloff": panel.last_rolloff,
           "n_transient_history": len(panel.transient_history), "n_envelope_history": len(panel.envelope_history),
           "n_events": len(panel.transient_events), "n_flux_history": len(panel._flux_sums),
           "n_novelty_history": len(panel.novelty_history), "update_counter": panel.update_counter,
           "last_event_time": panel.transient_events[-1]["time"] if panel.transient_events else 0.0,
           "prev_envelope": panel.prev_envelope}
    for b in range(4):
        got[f"band{b}"] = panel.band_energies[b]
    for n, w in zip(names, want):
        g = float(got[n])
        if n in ("detected", "type", "update_counter", "last_event_time") or n.startswith("n_"):
            assert g == w, (what, n, g, w)
        elif n.startswith("band"):
            assert abs(g - w) <= F32_BAR, (what, n, g, w)
        else:
            assert abs(g - w) <= (F32_BAR if n == "centroid" else 1e-9) * abs(w), (what, n, g, w)


# ---- CPU ----

@pytest.mark.parametrize("g", GROUPS)
def test_ref_equals_golden(G, g):
    fs, spec, frames = inputs(G, g)
    rows, _ = TR.rows(spec, frames, fs)
    check_rows(rows, G[f"{g}/row"], f"ref {g}")


def test_golden_covers_the_cases(G):
    assert int(G["m256/row"][0, 0]) & TR.FLAG_NO_HF and int(G["m256/row"][0, 0]) & TR.FLAG_NO_NOVELTY_SHAPE
    assert not int(G["m512/row"][0, 0]) & TR.FLAG_NO_HF and int(G["m512/row"][0, 0]) & TR.FLAG_NO_NOVELTY_SHAPE
    r = G["app/row"]
    assert int(r[0, 0]) == TR.FLAG_NO_FLUX | TR.FLAG_NO_NOVELTY and int(r[1, 0]) == 0 and r[1, 6] > 0
    assert list(G["nonfinite/row"][:, 0].astype(int) & 1) == [0, 1, 0, 1, 0]
    assert G["edge/row"][0, 10] == 0 and G["edge/row"][1, 10] == 2047
    assert G["edge/row"][2, 11] == 0 and G["edge/row"][2, 12] == 2047
    s = G["seq_fast/attrs"][:, list(G["attr_names"]).index("sensitivity")]
    assert s[-1] > 1.5
    s = G["seq_slow/attrs"][:, list(G["attr_names"]).index("sensitivity")]
    assert s[-1] < 1.5


@pytest.mark.parametrize("seq", SEQS)
def test_host_logic_reproduces_sequence(G, seq):
    """The facade's host logic on the recorded rows gives the reference's attributes after every step."""
    clock = Clock(float(G[f"{seq}/clock_step"]))
    p = host_panel(48000, clock)
    for i, (row, frozen, want) in enumerate(zip(G[f"{seq}/row"], G[f"{seq}/frozen"], G[f"{seq}/attrs"])):
        clock.at(i)
        if not frozen:
            assert p._apply_row(row, 513, 2048)
        check_attrs(G, p, want, (seq, i))


def test_host_logic_leaves_state_on_nonfinite():
    p = host_panel(48000, Clock(1.0))
    row = np.zeros(len(TR.COLUMNS))
    row[0] = TR.FLAG_NONFINITE
    assert not p._apply_row(row, 513, 2048)
    assert p.update_counter == 0 and len(p.envelope_history) == 0 and len(p._flux_sums) == 0


# ---- GPU ----

@pytest.fixture(scope="module")
def panels():
    from omega_gpu.transient_detection import TransientDetectionPanel
    cache = {}

    def get(fs):
        if fs not in cache:
            cache[fs] = TransientDetectionPanel(fs)
        return cache[fs]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_device_rows(G, panels, g):
    fs, spec, frames = inputs(G, g)
    rows, state = panels(fs).analyze_frames(spec, frames)
    check_rows(rows, G[f"{g}/row"], f"device {g}")
    _, want = TR.rows(spec, frames, fs)
    assert state[0] == want[0] and state[1] == want[1]
    np.testing.assert_allclose(state[4:4 + TR.FLUX_BINS], want[4:4 + TR.FLUX_BINS], rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_device_variants(G, panels):
    """float32 copies of the (float32-representable) frames, device memory, strided and overlapping rows, and
    shapes alternating on one context give the same rows."""
    import torch
    fs, spec, frames = inputs(G, "app")
    p = panels(fs)
    base, bstate = p.analyze_frames(spec, frames)
    r32, s32 = p.analyze_frames(spec, G["app/frame"])
    np.testing.assert_array_equal(r32, base)
    np.testing.assert_array_equal(s32, bstate)
    fs2, spec2, frames2 = inputs(G, "m512")
    other, _ = p.analyze_frames(spec2, frames2)  # another shape in between
    check_rows(other, G["m512/row"], "device m512 alternating")
    dspec = torch.zeros((len(spec), 600), dtype=torch.float32, device="cuda:0")
    dspec[:, :513] = torch.from_numpy(spec)
    dfr = torch.zeros((len(frames), 2048 + 64), dtype=torch.float64, device="cuda:0")
    dfr[:, :2048] = torch.from_numpy(frames)
    rd, sd = p.analyze_frames(dspec[:, :513], dfr[:, :2048])  # strided views, device memory
    np.testing.assert_array_equal(rd.cpu().numpy(), base)
    np.testing.assert_array_equal(sd.cpu().numpy(), bstate)
    rd32, _ = p.analyze_frames(dspec[:, :513], dfr[:, :2048].float())
    np.testing.assert_array_equal(rd32.cpu().numpy(), base)
    # overlapping rows: an unfold view of one stream against its contiguous copy
    stream = torch.from_numpy(np.concatenate(frames[:3])).to("cuda:0")
    view = stream.unfold(0, 2048, 512)
    sv = dspec[torch.arange(view.shape[0]) % len(spec)][:, :513]
    ro, so = p.analyze_frames(sv, view)
    rc, sc = p.analyze_frames(sv.contiguous(), view.contiguous())
    np.testing.assert_array_equal(ro.cpu().numpy(), rc.cpu().numpy())
    np.testing.assert_array_equal(so.cpu().numpy(), sc.cpu().numpy())
    want, _ = TR.rows(sv.cpu().numpy(), view.cpu().numpy(), fs)
    check_rows(ro.cpu().numpy(), want, "device overlapping")


@pytest.mark.gpu
@pytest.mark.parametrize("g", ("app", "nonfinite", "m512"))
def test_chaining_is_bit_equal(G, panels, g):
    """F frames in one call against F one-frame calls chained through the blob, and against two halves."""
    fs, spec, frames = inputs(G, g)
    p = panels(fs)
    rows, state = p.analyze_frames(spec, frames)
    st, got = None, []
    for i in range(len(spec)):
        r, st = p.analyze_frames(spec[i:i + 1], frames[i:i + 1], st)
        got.append(r[0])
    np.testing.assert_array_equal(np.array(got), rows)
    np.testing.assert_array_equal(st, state)
    a, sa = p.analyze_frames(spec[:2], frames[:2])
    b, sb = p.analyze_frames(spec[2:], frames[2:], sa)
    np.testing.assert_array_equal(np.concatenate([a, b]), rows)
    np.testing.assert_array_equal(sb, state)


@pytest.mark.gpu
@pytest.mark.parametrize("seq", SEQS)
def test_update_sequence_on_device(G, seq):
    from omega_gpu.transient_detection import TransientDetectionPanel
    clock = Clock(float(G[f"{seq}/clock_step"]))
    p = TransientDetectionPanel(48000, clock=clock)
    _, spec, frames = inputs(G, "app")
    for i, (k, frozen, want) in enumerate(zip(G[f"{seq}/idx"], G[f"{seq}/frozen"], G[f"{seq}/attrs"])):
        clock.at(i)
        p.is_frozen = bool(frozen)
        p.update(frames[k], spec[k])
        check_attrs(G, p, want, (seq, i))
    assert len(p.spectral_flux_history) == 10 and p.prev_phase is not None
    p.reset()
    assert p.update_counter == 0 and p._state is None and p.transient_type == "None"


@pytest.mark.gpu
def test_nonfinite_update_leaves_state(G, panels):
    _, spec, frames = inputs(G, "nonfinite")
    from omega_gpu.transient_detection import TransientDetectionPanel
    p = TransientDetectionPanel(48000, clock=Clock(1.0))
    p.update(frames[0], spec[0])
    before = (p.update_counter, p.envelope, len(p.envelope_history), p._state.copy())
    p.update(frames[1], spec[1])
    assert (p.update_counter, p.envelope, len(p.envelope_history)) == before[:3]
    np.testing.assert_array_equal(p._state, before[3])


@pytest.mark.gpu
def test_unsupported_shapes_leave_the_configured_one(G, panels):
    import omega_gpu
    from omega_gpu import _lib as L
    import ctypes as C
    fs, spec, frames = inputs(G, "app")
    p = panels(fs)
    base, _ = p.analyze_frames(spec, frames)
    for K, m in ((513, 128), (513, 16384), (513, 1000), (1, 2048), (8194, 2048)):
        with pytest.raises(omega_gpu.UnsupportedError):
            p.analyze_frames(np.zeros((1, K), np.float32), np.zeros((1, m)))
        cfg = L.TdetectConfig(float(fs), K, m)
        assert L.lib().omega_tdetect_configure(p._eng._ctx, C.byref(cfg)) == L.EUNSUP
    assert p._configured == (513, 2048)
    again, _ = p.analyze_frames(spec, frames)
    np.testing.assert_array_equal(again, base)
