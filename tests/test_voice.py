"""Voice detection: tests/voice_ref.py against tests/golden/voice.npz (recorded from the
reference's own VoiceDetectionPanel by tests/golden/gen_voice.py), the facade's host logic against the recorded
sequence, and omega_voice_features on the device against the golden rows.

Bars on the device. Exact: flags, voice_start / voice_end, formant_count, the formant bins, peak_lag. The
generator asserts the margins that make them decidable: every prominence 1e-3 relative away from its threshold,
every smoothed value a peak decision compares 64 float32 ulps of the frame's maximum away from the peak's height
(the device's smoothed values are a float64 dot product rounded to float32 once: within 1 ulp of scipy's), the
best two lags 1e-6 of corr0 apart. Bit-equal: the formant frequencies, one IEEE product k * (1.0 / (m * (1 /
fs))) with contraction off. voice_energy and total_energy: 1e-12 relative -- any summation order of K <= 8193
non-negative float64 terms is within about log2(K) 2^-53 = 1.4e-15 of exact, and the float32 inputs are exact in
float64. corr0 and corr_peak: 1e-9 of corr0, the project's float64 bar (a sum of m <= 8192 products in any order
is within m 2^-53 sum|x x'| <= 9.1e-13 corr0 of exact, by Cauchy-Schwarz).

The facade's confidence against the reference's, CONF_BAR = 5800 * 2^-24 = 3.46e-4 absolute, with u = 2^-24:
numpy's float32 pairwise sum of K <= 8193 non-negative terms passes each term through at most 15 adds in a leaf's
accumulator, 3 in the leaf's tree and 7 levels of halves, so each of the reference's two sums is within 25 u
relative of exact; the facade's float64 sums rounded to float32 are within u. The ratio of the two differs
between the two routes by at most (25 + 25 + 1 + 1) u plus one rounding each: 54 u relative, and ratio <= 1.
confidence = (ratio * 200 + score * 100) / 2 carries that as 54 u * 100, and its three float32 operations at
magnitudes up to 200 add at most 2 * 200 u on either route: (5400 + 400) u.

The observed worst deviation per column is printed (run with -s).
Observed on an MI355X over all golden frames (worst per column): voice_energy 0, total_energy 0 (bar 1e-12);
corr0 5.13e-16, corr_peak 1.39e-15 of corr0 (bar 1e-9); flags, ranges, formant count, formant bins, peak lag and
the bit-equal formant frequencies equal on every frame, for float32 and float64 audio, host and device memory,
strided views and alternating shapes; the 300 recorded steps through update() matched step by step.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import voice_ref as VR
from conftest import load_golden

CONF_BAR = 5800 * 2.0 ** -24
SUM_RTOL, CORR_TOL = 1e-12, 1e-9
GROUPS = ("app", "k10", "k10b", "k11", "k12", "k20", "m64", "m1024", "m8192", "fs44", "fs16", "fs8", "plateau",
          "zero", "nonfinite", "weak")
EXACT = (0, 1, 2, 5, 6, 7, 8, 9, 15)
WORST = {}


@pytest.fixture(scope="module")
def G():
    return load_golden("voice")


def inputs(G, g):
    """(fs, spectra float32 [F, K], audio float64 [F, m]) as the reference saw them."""
    fs = int(G[f"{g}/fs"])
    fr = G[f"{g}/frame"].astype(np.float64)
    sha = str(G[f"{g}/audio_sha"])
    for audio in (fr * np.hanning(fr.shape[1]), fr):  # (`plateau` is not windowed)
        audio = np.ascontiguousarray(audio)
        if hashlib.sha256(audio.tobytes()).hexdigest() == sha:
            return fs, G[f"{g}/spec"], audio
    raise AssertionError(f"{g}: the audio frames do not hash to the recorded sha256")


def host_panel(fs):
    from omega_gpu.voice_detection import VoiceDetectionPanel
    p = VoiceDetectionPanel.__new__(VoiceDetectionPanel)
    p._host_init(fs)
    return p


def check_rows(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    for c in EXACT:
        np.testing.assert_array_equal(got[:, c], want[:, c], err_msg=f"{what}: {VR.COLUMNS[c]}")
    np.testing.assert_array_equal(got[:, 10:14], want[:, 10:14], err_msg=f"{what}: formant frequencies")
    for c in (3, 4):
        den = np.where(want[:, c] != 0, np.abs(want[:, c]), 1.0)
        d = float(np.max(np.abs(got[:, c] - want[:, c]) / den))
        WORST[VR.COLUMNS[c]] = max(WORST.get(VR.COLUMNS[c], 0.0), d)
        assert d <= SUM_RTOL, (what, VR.COLUMNS[c], d)
    for c in (14, 16):
        den = np.where(want[:, 14] != 0, want[:, 14], 1.0)
        d = float(np.max(np.abs(got[:, c] - want[:, c]) / den))
        WORST[VR.COLUMNS[c]] = max(WORST.get(VR.COLUMNS[c], 0.0), d)
        assert d <= CORR_TOL, (what, VR.COLUMNS[c], d)
    print(f"{what}: worst so far " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


# ---- CPU ----

@pytest.mark.parametrize("g", GROUPS)
def test_ref_equals_golden(G, g):
    fs, spec, audio = inputs(G, g)
    for i in range(len(spec)):
        np.testing.assert_array_equal(VR.row(spec[i], audio[i], fs), G[f"{g}/row"][i])
        if not int(G[f"{g}/row"][i][0]) & VR.FLAG_NONFINITE and spec.shape[1] > 10:
            sm, peaks, prom, _ = VR.smoothed_peaks(spec[i])
            np.testing.assert_array_equal(sm, G[f"{g}/smoothed"][i])
            np.testing.assert_array_equal(peaks, G[f"{g}/peaks"][i][:len(peaks)])
            np.testing.assert_array_equal(prom, G[f"{g}/prom"][i][:len(peaks)])
            assert np.all(G[f"{g}/peaks"][i][len(peaks):] == -1)
    assert tuple(G[f"{g}/range"]) == VR.bin_range(fs, audio.shape[1])
    fb = np.fft.rfftfreq(audio.shape[1], 1 / fs)
    assert hashlib.sha256(fb.tobytes()).hexdigest() == str(G[f"{g}/rfftfreq_sha"])


@pytest.mark.parametrize("g", GROUPS)
def test_host_result_matches_reference(G, g):
    """result_from_row on the golden rows gives the reference's own results."""
    fs, spec, _ = inputs(G, g)
    p = host_panel(fs)
    for i, row in enumerate(G[f"{g}/row"]):
        res = p.result_from_row(row, spec.shape[1])
        if not res["valid"]:
            assert g == "nonfinite"
            continue
        if res["range_ok"]:
            assert bool(res["active"]) == bool(G[f"{g}/ref_active"][i])
            assert abs(float(res["confidence"]) - G[f"{g}/ref_conf"][i]) <= CONF_BAR
            want = G[f"{g}/ref_formants"][i]
            want = want[~np.isnan(want)]
            got = res["formants"] if res["formants"] is not None else []
            np.testing.assert_array_equal(np.array(got, np.float64), want)
        want = G[f"{g}/ref_pitch"][i]
        assert (res["pitch"] is None and want == 0.0) or res["pitch"] == want


def seq_pool(G):
    pool = []
    for g, i in zip(G["seq/pool_group"], G["seq/pool_frame"]):
        fs, spec, audio = inputs(G, str(g))
        pool.append((spec[i], audio[i]))
    return pool


def run_seq(G, panel, pool):
    types = [str(t) for t in G["voice_types"]]
    for s, (k, frozen) in enumerate(zip(G["seq/idx"], G["seq/frozen"])):
        panel.is_frozen = bool(frozen)
        spec, audio = pool[k]
        panel.update(audio, spec)
        st = panel.get_status()
        assert list(st) == ["active", "confidence", "pitch", "voice_type", "formants"]
        assert bool(st["active"]) == bool(G["seq/active"][s]), s
        assert abs(float(st["confidence"]) - G["seq/confidence"][s]) <= CONF_BAR, s
        # the reference's types: np.float32 from the expression, int where min() picks 100, float before any update
        assert isinstance(st["confidence"], int) == bool(G["seq/confidence_is_int"][s]), s
        assert float(st["pitch"]) == G["seq/pitch"][s], s
        assert st["voice_type"] == types[G["seq/voice_type"][s]], s
        assert len(st["formants"]) == G["seq/n_formants"][s], s
        np.testing.assert_array_equal(np.array(st["formants"], np.float64), G["seq/formants"][s][:len(st["formants"])])
        lens = [len(panel.voice_history), len(panel.formant_history), len(panel.pitch_history)]
        assert lens == list(G["seq/lens"][s]), s
    assert panel.vocal_quality == 0.0
    active = [c for c in panel.voice_history if c > 30]
    assert active and all(isinstance(c, np.float32) for c in active)
    assert isinstance(panel.voice_pitch, np.float64)


def test_host_logic_reproduces_seq(G):
    """The facade's host logic over tests/voice_ref.py's rows, step by step: the interval gate, the frozen
    steps, the stale state after a failed range check, the carried pitch, the three deques wrapping."""
    pool = seq_pool(G)
    rows = {id(a): VR.row(s, a, 48000) for s, a in pool}
    panel = host_panel(48000)
    panel._row = lambda audio, spec: rows[id(audio)]
    run_seq(G, panel, pool)
    assert list(G["seq/lens"][-1]) == [120, 60, 120]
    panel.reset()
    assert panel.get_status() == {"active": False, "confidence": 0.0, "pitch": 0.0, "voice_type": "Unknown",
                                  "formants": []}
    assert panel.update_counter == 0 and not panel.voice_history


def test_bin_range_matches_numpy(G):
    from omega_gpu.voice_detection import voice_bin_range
    for g in GROUPS:
        fs, m = int(G[f"{g}/fs"]), int(G[f"{g}/m"])
        assert voice_bin_range(fs, m) == tuple(G[f"{g}/range"]), g
    for fs in (8000, 11025, 22050, 44100, 48000, 88200, 96000, 192000):
        for m in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
            assert voice_bin_range(fs, m) == VR.bin_range(fs, m), (fs, m)
    with pytest.raises(Exception):
        voice_bin_range(0, 2048)


def test_unsupported_shapes_are_refused_on_the_host():
    from omega_gpu import UnsupportedError
    p = host_panel(48000)
    p._configured = (1025, 2048)
    for K, m in ((8194, 2048), (0, 2048), (1025, 1000), (1025, 32), (1025, 16384)):
        with pytest.raises(UnsupportedError):
            p._configure(K, m)
        assert p._configured == (1025, 2048)
    with pytest.raises(UnsupportedError):
        host_panel(4000)._configure(1025, 2048)


def test_status_keys_and_surface():
    p = host_panel(48000)
    assert list(p.get_status()) == ["active", "confidence", "pitch", "voice_type", "formants"]
    assert p.update_interval == 2 and p.is_frozen is False
    for pitch, name in ((100, "Bass"), (110, "Baritone"), (164.9, "Baritone"), (165, "Tenor"), (262, "Alto"),
                        (330, "Soprano")):
        p.voice_pitch = pitch
        p.analyze_voice_type()
        assert p.voice_type == name
    from omega_gpu import _lib as L
    from omega_gpu.voice_detection import COLUMNS
    assert COLUMNS == VR.COLUMNS and len(COLUMNS) == 17
    assert C.sizeof(L.VoiceConfig) == 16


# ---- GPU ----

@pytest.fixture(scope="module")
def panels():
    from omega_gpu import VoiceDetectionPanel
    cache = {}

    def get(fs):
        if fs not in cache:
            cache[fs] = VoiceDetectionPanel(fs)
        return cache[fs]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("mem", ("host", "device"))
@pytest.mark.parametrize("g", GROUPS)
def test_device_rows_match_golden(G, panels, g, mem):
    fs, spec, audio = inputs(G, g)
    assert len(spec) <= 16
    p = panels(fs)
    if mem == "host":
        got = p.analyze_frames(spec, audio)
        assert isinstance(got, np.ndarray)
    else:
        import torch
        got = p.analyze_frames(torch.from_numpy(spec).cuda(), torch.from_numpy(audio).cuda())
        assert got.is_cuda
        got = got.cpu().numpy()
    check_rows(got, G[f"{g}/row"], f"{g}/{mem}")
    # and through the host part: the reference's own decisions
    for i, row in enumerate(got):
        res = p.result_from_row(row, spec.shape[1])
        if res["valid"] and res["range_ok"]:
            assert bool(res["active"]) == bool(G[f"{g}/ref_active"][i])
            assert abs(float(res["confidence"]) - G[f"{g}/ref_conf"][i]) <= CONF_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("g", ("app", "m8192", "fs16"))
def test_device_float32_audio(G, panels, g):
    """Float32 samples are widened on load: the rows of the frames before the window, as float32."""
    fs, spec, _ = inputs(G, g)
    fr = G[f"{g}/frame"]
    want = np.stack([VR.row(s, a.astype(np.float64), fs) for s, a in zip(spec, fr)])
    check_rows(panels(fs).analyze_frames(spec, fr), want, f"{g}/float32")


@pytest.mark.gpu
def test_device_strided_views(G, panels):
    """An unfold view of one sample stream (overlapping frames) and a strided view of wider spectra."""
    import torch
    fs, spec, audio = inputs(G, "app")
    m, hop, F = 2048, 512, 5
    stream = np.concatenate([audio[0], audio[2], audio[3]])[:m + (F - 1) * hop].copy()
    wide = np.zeros((F, 1025 + 7), np.float32)
    wide[:, 3:1028] = spec[:F]
    ds, dw = torch.from_numpy(stream).cuda(), torch.from_numpy(wide).cuda()
    frames, view = ds.unfold(0, m, hop), dw[:, 3:1028]
    assert frames.stride(0) == hop and view.stride(0) == 1032
    want = np.stack([VR.row(spec[i], stream[i * hop:i * hop + m], fs) for i in range(F)])
    check_rows(panels(fs).analyze_frames(view, frames).cpu().numpy(), want, "strided")


@pytest.mark.gpu
def test_device_alternating_configurations(G, panels):
    p = panels(48000)
    for _ in range(2):
        for g in ("app", "k12", "m8192", "m64"):
            fs, spec, audio = inputs(G, g)
            check_rows(p.analyze_frames(spec, audio), G[f"{g}/row"], f"alternating/{g}")


@pytest.mark.gpu
def test_device_unsupported_leaves_the_configuration_usable(G, panels):
    from omega_gpu import UnsupportedError
    from omega_gpu import _lib as L
    fs, spec, audio = inputs(G, "app")
    p = panels(fs)
    p.analyze_frames(spec[:1], audio[:1])
    lib = L.lib()
    for cfg in (L.VoiceConfig(48000.0, 8194, 2048), L.VoiceConfig(48000.0, 1025, 1000),
                L.VoiceConfig(4000.0, 1025, 2048), L.VoiceConfig(48000.0, 1025, 16384)):
        assert lib.omega_voice_configure(p._eng._ctx, C.byref(cfg)) == L.EUNSUP
        assert b"voice" in lib.omega_last_error(p._eng._ctx)
    with pytest.raises(UnsupportedError):
        p.analyze_frames(np.zeros((1, 9000), np.float32), audio[:1])
    # the configured shape is still the app's: a direct call without reconfiguring
    out = np.empty((1, 17), np.float64)
    a = np.ascontiguousarray(audio[:1])
    p._eng._check(lib.omega_voice_features(p._eng._ctx, spec[:1].ctypes.data, 1025, a.ctypes.data, 1, 2048, 2048, 1,
                                           out.ctypes.data, L.MEM_HOST))
    check_rows(out, G["app/row"][:1], "after-unsupported")


@pytest.mark.gpu
def test_device_seq_through_update(G):
    """The recorded 300 steps end to end: update() on the device."""
    from omega_gpu import VoiceDetectionPanel
    run_seq(G, VoiceDetectionPanel(48000), seq_pool(G))


@pytest.mark.gpu
def test_device_detect_voice_and_pitch(G, panels):
    fs, spec, audio = inputs(G, "app")
    from omega_gpu import VoiceDetectionPanel
    p = VoiceDetectionPanel(fs)
    active, conf = p.detect_voice(audio[1], spec[1])
    assert active and abs(float(conf) - G["app/ref_conf"][1]) <= CONF_BAR
    p.detect_pitch(audio[1])
    assert p.voice_pitch == G["app/ref_pitch"][1] and len(p.pitch_history) == 1
    p.detect_pitch(audio[1][:1024])
    assert len(p.pitch_history) == 1
    # update(audio, None): the host computes the spectrum; float64 bins are rounded to float32 for the device
    p.reset()
    p.update(audio[1])
    p.update(audio[1])
    assert p.voice_active and p.voice_type == "Baritone"
