"""§8(f) row 5: CepstralAnalyzer.detect_pitch_advanced on the device (omega_pitch_detect through
omega_gpu.pitch_detection) against the reference's own outputs (tests/golden/pitch.npz, recorded by
tests/golden/gen_pitch.py under the conditions listed there) and the restatement tests/pitch_ref.py,
which is pinned to the golden on the CPU.

Tolerances. Integer decisions (cepstral period, autocorrelation period, YIN tau), the cepstral pitch,
note, octave and cents are exact; the float64 cepstral confidence matches to 1e-9 relative (another
FFT and summation order than pocketfft's and numpy's pairwise sums). The float32-path values
(autocorrelation confidence, YIN pitch, YIN confidence) must lie within 4 x the reference's own recorded
deviation from the float64 evaluation of the same formulas (golden `dev`; the factor covers another
summation order than numpy's pairwise sum and BLAS sdot). The combined pitch and confidence follow:
with e = 4 max(dev) the weights move by at most 1.1 e, the weighted mean of pitches within [min, max] by
at most 4 dev_yin_pitch + 2 * 1.1 e / total_weight relative (total_weight >= 0.12, the smallest
accepted weight), the confidence by at most 1.2 * 1.1 e.
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import pitch_ref as PR
from conftest import load_golden

GROUPS = ("tones", "t2048", "t8192", "edges", "dist", "fs44", "music", "lowlat", "noise", "seq")


@functools.lru_cache(maxsize=None)
def G():
    return load_golden("pitch")


def params(name):
    c = dict(zip([str(k) for k in G()["cfg_fields"]], G()[f"{name}/cfg"][:-2]))
    P = PR.Params(int(c["sample_rate"]), c["min_pitch"], c["max_pitch"], c["yin_threshold"], int(c["yin_window_size"]),
                  bool(c["enable_preprocessing"]), c["highpass_frequency"], int(c["highpass_order"]),
                  bool(c["enable_compression"]), c["compression_threshold"], c["compression_ratio"])
    assert [P.min_period, P.max_period] == list(G()[f"{name}/cfg"][-2:])
    return P


def frames(name):
    x = G()[f"{name}/x"]
    return np.stack([x[f * 512:f * 512 + 4096] for f in range(30)]) if name == "seq" else x


@functools.lru_cache(maxsize=None)
def f64_eval(name):
    """The float64 evaluation of the group's frames (computed once, shared by the tests)."""
    P = params(name)
    return [PR.analyze(x, P, f64=True) for x in frames(name)]


def tolerances():
    dev = G()["dev"]
    e = 4 * float(max(dev[0], dev[2]))
    return dict(ac_conf=4 * dev[0], yin_pitch=4 * dev[1], yin_conf=4 * dev[2],
                pitch=4 * dev[1] + 2 * 1.1 * e / 0.12 + 1e-9, conf=1.2 * 1.1 * e + 1e-9)


def check_rows(name, rows, notes=None):
    """rows [F, >= 8] (pitch, confidence, three (pitch, confidence) pairs) against the group's golden."""
    g, P, T = G(), params(name), tolerances()
    dec, ref, out = g[f"{name}/dec"], g[f"{name}/methods"], g[f"{name}/out"]
    ev = f64_eval(name)
    fs = P.sample_rate
    for f, r in enumerate(rows):
        per = [int(round(fs / r[2])) if r[2] > 0 else 0, int(round(fs / r[4])) if r[4] > 0 else 0,
               int(round(fs / r[6])) if r[6] > 0 else 0]
        assert per == list(dec[f]), (name, f, per, dec[f])
        assert r[2] == ref[f, 0] and r[4] == ref[f, 2], (name, f)  # fs / period
        np.testing.assert_allclose(r[3], ref[f, 1], rtol=1e-9, err_msg=f"{name} {f} cepstral confidence")
        d = (abs(r[5] - ev[f]["autocorr"][1]), abs(r[6] - ev[f]["yin"][0]) / max(ev[f]["yin"][0], 1e-300),
             abs(r[7] - ev[f]["yin"][1]))
        print(f"{name}[{f}] deviation from the float64 evaluation: ac conf {d[0]:.2e} yin pitch {d[1]:.2e} yin conf {d[2]:.2e}")
        assert d[0] <= T["ac_conf"] and d[1] <= T["yin_pitch"] and d[2] <= T["yin_conf"], (name, f, d, T)
        np.testing.assert_allclose(r[0], out[f, 0], rtol=T["pitch"], err_msg=f"{name} {f} pitch")
        np.testing.assert_allclose(r[1], out[f, 1], rtol=0, atol=T["conf"], err_msg=f"{name} {f} confidence")
        if notes is not None:
            assert notes[f] == (str(g[f"{name}/note"][f]), int(out[f, 2]), int(out[f, 3])), (name, f, notes[f])


# ---- CPU ----

@pytest.mark.parametrize("name", GROUPS)
def test_pitch_ref_matches_reference_golden(name):
    """tests/pitch_ref.py against the reference: integers exact, float64 quantities to 1e-12, the
    float32-path quantities within the recorded deviation of the float64 evaluation (x 4 for this machine's
    BLAS), the combined values within the margins derived above."""
    g, P = G(), params(name)
    dev = g["dev"]
    an = PR.Analyzer(P)
    rows, notes, stab = [], [], []
    for f, x in enumerate(frames(name)):
        r = an.detect(x) if name == "seq" else PR.Analyzer(P).detect(x)
        assert [r["cep_period"], r["ac_period"], r["yin_tau"]] == list(g[f"{name}/dec"][f])
        np.testing.assert_allclose(r["cepstral"], g[f"{name}/methods"][f, :2], rtol=1e-12)
        rows.append([r["pitch"], r["confidence"], *r["cepstral"], *r["autocorr"], *r["yin"]])
        notes.append((r["note"], r["octave"], r["cents_offset"]))
        stab.append(r["stability"])
        e = f64_eval(name)[f]  # the recorded deviations really are the reference's
        m = g[f"{name}/methods"][f]
        assert abs(m[3] - e["autocorr"][1]) <= dev[0] * (1 + 1e-9)
        assert abs(m[5] - e["yin"][1]) <= dev[2] * (1 + 1e-9)
        if e["yin_tau"]:
            assert abs(m[4] - e["yin"][0]) / e["yin"][0] <= dev[1] * (1 + 1e-9)
    check_rows(name, np.array(rows, np.float64), notes)
    np.testing.assert_allclose(stab, g[f"{name}/out"][:, 4], rtol=0, atol=1e-4)
    if name == "seq":
        np.testing.assert_allclose(list(an.pitch_history), g["seq/pitch_history"], rtol=tolerances()["pitch"])
    if name == "dist":  # the distance rule decided: peaks[0] is not the first raw local maximum >= 0.3
        r = PR.analyze(frames(name)[0], P)
        assert r["ac_first_raw"] == int(g["dist/first_raw"]) != r["ac_period"]


def test_pitch_config_mirror_matches_reference():
    from omega_gpu.pitch_detection import PitchDetectionConfig, get_preset_config, list_presets
    cfgs = json.loads(str(G()["configs"]))
    derived = ("min_period", "max_period")
    for sr in (44100, 48000, 96000):
        ref = cfgs[f"default_{sr}"]
        c = PitchDetectionConfig(sample_rate=sr)
        assert c.to_dict() == {k: v for k, v in ref.items() if k not in derived}, sr
        assert (int(sr / c.max_pitch), int(sr / c.min_pitch)) == (ref["min_period"], ref["max_period"])
    assert list_presets() == [str(p) for p in G()["presets"]]
    for name in list_presets():
        ref = cfgs[f"preset_{name}"]
        assert get_preset_config(name).to_dict() == {k: v for k, v in ref.items() if k not in derived}, name
    c = PitchDetectionConfig()
    assert (int(48000 / c.max_pitch), int(48000 / c.min_pitch), c.yin_window_size) == (24, 960, 1920)
    with pytest.raises(ValueError):
        get_preset_config("nope")
    with pytest.raises(AssertionError):
        PitchDetectionConfig(min_pitch=100.0, max_pitch=50.0)


# ---- GPU ----

def analyzer(name):
    from omega_gpu.pitch_detection import CepstralAnalyzer, PitchDetectionConfig, get_preset_config
    cfg = {"fs44": lambda: PitchDetectionConfig(sample_rate=44100), "music": lambda: get_preset_config("music_optimized"),
           "lowlat": lambda: get_preset_config("low_latency")}.get(name, lambda: get_preset_config("balanced"))()
    an = CepstralAnalyzer(cfg.sample_rate, cfg)
    P = params(name)
    assert (an.min_period, an.max_period, an.yin_window_size) == (P.min_period, P.max_period, P.yin_window_size)
    return an


def run_group(name):
    """Every frame of the group through detect_pitch_advanced_safe (each on fresh histories, as recorded)."""
    an = analyzer(name)
    rows, notes = [], []
    for x in frames(name):
        an.pitch_history.clear()
        an.confidence_history.clear()
        r = an.detect_pitch_advanced_safe(x)
        assert r.get("error") is None and set(r) == {"pitch", "confidence", "note", "octave", "cents_offset",
                                                     "stability", "methods"}, r
        m = r["methods"]
        assert set(m) == {"cepstral", "autocorr", "yin"}
        assert r["stability"] == 0.0
        rows.append([r["pitch"], r["confidence"], *m["cepstral"], *m["autocorr"], *m["yin"]])
        notes.append((r["note"], r["octave"], r["cents_offset"]))
    rows = np.array(rows, np.float64)
    check_rows(name, rows, notes)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tones", "t2048", "t8192", "noise"])
def test_pitch_golden_parity(name):
    """Golden parity through the facade, float32-path values included. The device's deviation from the
    float64 evaluation is printed per frame (run with -s); the recorded reference deviations (the
    yardstick, x 4) are 1.3e-7 (autocorrelation confidence), 1.8e-7 relative (YIN pitch) and 1.0e-7
    (YIN confidence). The device sums the float32 differences in float64 and runs the autocorrelation's
    transforms in float64, so its own deviation is expected at the final float32 cast's rounding
    (<= 6e-8 on the autocorrelation confidence); no MI355X figure has been recorded here yet."""
    rows = run_group(name)
    if name == "tones":
        had = {tuple(int(v > 0) for v in r[[2, 4, 6]]) for r in rows}
        assert (1, 1, 0) in had and (1, 1, 1) in had  # YIN without an estimate; all three methods
    if name == "noise":
        assert rows[0, 4] == 0 and rows[0, 6] == 0  # autocorrelation and YIN give nothing


@pytest.mark.gpu
def test_pitch_switch_edge_and_distance_rule_frames():
    """YIN minima either side of the tau = 100 switch between the two difference-function definitions,
    periods at min_period (24) and near max_period (941), and the frame whose first raw autocorrelation
    maximum >= 0.3 the distance rule removes: exact on the integers."""
    g = G()
    rows = run_group("edges")
    taus = [int(round(48000 / r[6])) if r[6] > 0 else 0 for r in rows]
    assert taus[0] > 100 > taus[2] and taus[3] == 24 and round(48000 / rows[4, 4]) >= 930
    rows = run_group("dist")
    assert round(48000 / rows[0, 4]) == g["dist/dec"][0, 1] != int(g["dist/first_raw"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fs44", "music", "lowlat"])
def test_pitch_other_settings(name):
    """A 44.1 kHz analyzer (window 1764), music_optimized (periods 12..1200, window 2400, 30 Hz
    high-pass) and low_latency (no pre-processing)."""
    run_group(name)


@pytest.mark.gpu
def test_pitch_sequence_history_and_batch():
    """One analyzer over the 30-frame stream: single calls reproduce the recorded stability and
    histories; detect_batch over the same frames equals the single calls bitwise."""
    g, T = G(), tolerances()
    an = analyzer("seq")
    x = frames("seq")
    rows, notes, stab = [], [], []
    for fr in x:
        r = an.detect_pitch_advanced_safe(fr)
        m = r["methods"]
        rows.append([r["pitch"], r["confidence"], *m["cepstral"], *m["autocorr"], *m["yin"]])
        notes.append((r["note"], r["octave"], r["cents_offset"]))
        stab.append(r["stability"])
    rows = np.array(rows, np.float64)
    check_rows("seq", rows, notes)
    # stability = 1 - 10 std / mean over pitches that each moved by at most T["pitch"] relative
    np.testing.assert_allclose(stab, g["seq/out"][:, 4], rtol=0, atol=20 * T["pitch"] + 1e-12)
    assert (np.array(stab[:9]) == 0).all() and min(stab[9:]) > 0
    np.testing.assert_allclose(list(an.pitch_history), g["seq/pitch_history"], rtol=T["pitch"])
    np.testing.assert_allclose(list(an.confidence_history), g["seq/confidence_history"], rtol=0, atol=T["conf"])
    bn = analyzer("seq")
    got = bn.detect_batch(x)
    np.testing.assert_array_equal(got[:, :8], rows)
    assert list(bn.pitch_history) == list(an.pitch_history)
    assert list(bn.confidence_history) == list(an.confidence_history)
    assert bn.calculate_pitch_stability() == stab[-1]


@pytest.mark.gpu
def test_pitch_invalid_frames():
    """Silent, NaN and short frames give the reference's dicts and error strings; in a batch they give
    zero rows and leave the valid rows bitwise unchanged; an unsupported length is reported, not computed."""
    from omega_gpu import _lib as L
    g = G()
    an = analyzer("tones")
    for name in ("silent", "nan", "short"):
        r = an.detect_pitch_advanced_safe(g[f"bad/{name}/x"])
        assert sorted(r) == [str(k) for k in g[f"bad/{name}/keys"]], (name, r)
        assert (r.get("error") or "") == str(g[f"bad/{name}/error"]), (name, r)
        assert (r["pitch"], r["confidence"], r["note"], r["octave"], r["cents_offset"], r["stability"]) == (0.0, 0.0, "", 0, 0, 0.0)
    assert len(an.pitch_history) == 0
    # the device's own validation (the batch path has no host check)
    tones = g["tones/x"][[4, 9, 12, 17]]
    clean = analyzer("tones").detect_batch(tones)
    mixed = np.stack([tones[0], g["bad/silent/x"], tones[1], g["bad/nan/x"], g["noise/x"][0], tones[2], tones[3]])
    bn = analyzer("tones")
    got = bn.detect_batch(mixed)
    np.testing.assert_array_equal(got[[0, 2, 5, 6]], clean)
    assert (got[1, :8] == 0).all() and got[1, 9] == 2 and (got[3, :9] == 0).all() and got[3, 9] == 1
    assert got[4, 9] == 0 and got[4, 2] > 0 and len(bn.pitch_history) == 5
    np.testing.assert_allclose(got[0, 8], np.sqrt(np.mean(tones[0].astype(np.float64) ** 2)), rtol=1e-12)
    # a float64 frame is cast on load (:587-588)
    np.testing.assert_array_equal(analyzer("tones").detect_batch(tones.astype(np.float64)), clean)
    # a length the library does not build: no CPU fallback, the default dict with the error
    r = an.detect_pitch_advanced_safe(g["bad/n3000/x"])
    assert r["error"] and "3000" in r["error"] and r["methods"] == {} and r["pitch"] == 0.0
    out = np.empty((1, 10))
    x = np.ascontiguousarray(g["bad/n3000/x"])
    lib = L.lib()
    assert lib.omega_pitch_detect(an._eng._ctx, x.ctypes.data, 0, 1, 3000, 3000, out.ctypes.data, L.MEM_HOST) == L.EUNSUP
    assert b"3000" in lib.omega_last_error(an._eng._ctx)
    # below yin_window_size: the all-zero result (:487-495); no frames: a no-op
    x = np.ascontiguousarray(g["bad/short/x"])
    out[:] = 7
    assert lib.omega_pitch_detect(an._eng._ctx, x.ctypes.data, 0, 1, 1000, 1000, out.ctypes.data, L.MEM_HOST) == L.OK
    assert (out == 0).all()
    assert lib.omega_pitch_detect(an._eng._ctx, x.ctypes.data, 0, 0, 4096, 4096, out.ctypes.data, L.MEM_HOST) == L.OK
    cfg = L.PitchConfig()
    lib.omega_pitch_config_default(C.byref(cfg))
    assert (cfg.sample_rate, cfg.yin_window_size, cfg.highpass_order) == (48000, 1920, 4)
    cfg.highpass_order = 2
    assert lib.omega_pitch_configure(an._eng._ctx, C.byref(cfg)) == L.EUNSUP


@pytest.mark.gpu
def test_pitch_device_memory_and_stream_view():
    """Device-memory input -- a materialised tensor and an overlapping view of the stream at
    frame_stride = 512 -- equals the host-memory result bitwise; two runs are bitwise equal."""
    import torch
    x = frames("seq")
    host = analyzer("seq").detect_batch(x)
    xd = torch.from_numpy(x).cuda()
    a = analyzer("seq").detect_batch(xd)
    assert a.is_cuda and a.dtype == torch.float64
    np.testing.assert_array_equal(a.cpu().numpy(), host)
    s = torch.from_numpy(G()["seq/x"]).cuda()
    view = s.unfold(0, 4096, 512)
    assert view.shape == (30, 4096) and view.stride(0) == 512
    an = analyzer("seq")
    b = an.detect_batch(view).cpu().numpy()
    np.testing.assert_array_equal(b, host)
    np.testing.assert_array_equal(an.detect_batch(view).cpu().numpy(), b)
    assert len(an.pitch_history) == 60


@pytest.mark.gpu
def test_pitch_broadcast_device_batch_is_copied():
    """A device batch built by ``expand`` of one frame (row stride 0) takes the common row rule: it is
    copied and analysed, bit-equal to its ``.contiguous()`` copy. F = 3 frames of n = 2048 samples. (Before
    the facades shared their marshalling this facade tested stride(1) alone and the library refused the
    batch as a bad layout.)"""
    import torch
    x = G()["t2048/x"][0]
    assert x.shape == (2048,) and analyzer("t2048").yin_window_size <= 2048
    batch = torch.from_numpy(x).cuda()[None, :].expand(3, 2048)
    assert batch.stride(0) == 0
    got = analyzer("t2048").detect_batch(batch)
    want = analyzer("t2048").detect_batch(batch.contiguous())
    assert got.is_cuda and tuple(got.shape) == (3, 10)
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    rows = got.cpu().numpy()
    assert (rows[:, 9] == 0).all() and (rows[:, 0] > 0).all()  # (every row is an estimate, not the zero row)
    np.testing.assert_array_equal(rows[1:], rows[:1].repeat(2, axis=0))


@pytest.mark.gpu
def test_pitch_integer_device_samples_become_float64():
    """Device samples that are neither float32 nor float64 are converted to float64, as the host path always
    did (the device path used to hand their bytes to the library as float32): an int16 batch is bit-equal
    to its float64 copy."""
    import torch
    x = G()["t2048/x"][:1]
    pcm = torch.from_numpy(np.round(x * 32767 / np.abs(x).max()).astype(np.int16)).cuda()
    got = analyzer("t2048").detect_batch(pcm)
    want = analyzer("t2048").detect_batch(pcm.double())
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), analyzer("t2048").detect_batch(pcm.cpu().numpy()))
    assert got[0, 9] == 0 and 210 < float(got[0, 0]) < 230  # (the 220 Hz tone, not reinterpreted bytes)
