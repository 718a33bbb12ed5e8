"""§8(f) row 8: HipHopDetector.analyze on the device (omega_hiphop_features through
omega_gpu.hip_hop_detector) against the reference's own outputs (tests/golden/hiphop.npz, recorded by
tests/golden/gen_hiphop.py with the group assertions and decision margins listed there) and the restatement
tests/hiphop_ref.py, which is pinned to the golden on the CPU.

Tolerances. The integer decisions (both peak counts, the kick peak positions, the zero-crossing count, the
flags, the branches) and every float32-path value (the nine power sums, spectral_tilt, vocal_presence, the
float32 rms) are exact. The float64 columns that pass through the filters (the two filtered RMS values, the
envelope threshold, sub_bass_presence, hihat_density, kick_pattern_factor) are held to 1e-9 relative against
the golden: a CPU emulation of a 256-chunk float64 scan of these filters deviates from a long-double
evaluation by at most 4.3e-11 normwise at m 8192 (scipy's sequential filter: 2.0e-12; recorded here as
golden `dev`: 1.3e-12), the filtered RMS by 3.8e-11; 1e-9 leaves about 25 x for another chunk length and
carry order and sits six orders below any threshold the features feed. The observed deviation is printed
per column (run with -s).
Observed on an MI355X over all golden frames (worst per column): sub_bass_rms 1.72e-10, envelope_threshold
1.72e-10, sub_bass_presence 1.03e-10, hihat_rms 2.06e-15, hihat_density 2.08e-15, kick_pattern_factor 0
(bit-equal); every exact column equal on every frame.
The library's designed sections differ from the recorded scipy sections by at most 1.8e-15 relative per
coefficient (48000, 44100 and 16000 Hz); filtering the golden inputs with them sequentially on the CPU
moves the filtered RMS by at most 2e-12.
"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import hiphop_ref as HR
from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "tools", "model"))
import peaks_model as M  # noqa: E402

GROUPS = ("app", "app1025", "m64", "m512", "m8192", "fs44", "fs16", "twopeak", "onepeak", "nopeak", "k16a", "k16b",
          "k16c", "edges", "vocal", "hann", "silent", "lowratio")
COL = {k: i for i, k in enumerate(HR.COLUMNS)}
RTOL = 1e-9
KEYS = ["sub_bass_presence", "kick_pattern_score", "hihat_density", "spectral_tilt", "vocal_presence", "tempo_match"]
DRUM = {"kick": {"kick_detected": True, "magnitude": 0.9}}
RESULT_KEYS = ["confidence", "features", "subgenre", "is_hip_hop", "sub_bass_detected", "strong_beat"]


@functools.lru_cache(maxsize=None)
def G():
    return load_golden("hiphop")


def group(name):
    g = G()
    n = int(g[f"{name}/n"])
    return int(g[f"{name}/fs"]), g[f"{name}/freqs"], [(g[f"{name}/{i}/spec"], g[f"{name}/{i}/audio"]) for i in range(n)]


def golden_sos(fs):
    return dict(zip(HR.BANDS, G()[f"sos/{fs}"]))


@functools.lru_cache(maxsize=None)
def evals(name):
    """The restatement of the group's frames with the recorded scipy sections (computed once)."""
    fs, freqs, frames = group(name)
    return [HR.features(spec, freqs, audio, fs, golden_sos(fs) if f"sos/{fs}" in G() else None) for spec, audio in frames]


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def check_frame(name, i, row, peaks, worst=None):
    """One device (or restatement) row with its kick peaks against frame i of the group's golden."""
    g, p = G(), f"{name}/{i}/"
    ref = g[p + "row"]
    for k in HR.EXACT:
        assert row[COL[k]] == ref[COL[k]], (name, i, k, row[COL[k]], ref[COL[k]])
    np.testing.assert_array_equal(peaks, g[p + "kick_peaks"], err_msg=f"{name} {i} kick peaks")
    d = {k: rel(row[COL[k]], ref[COL[k]]) for k in HR.FILTERED}
    print(f"{name}[{i}] deviation from the golden:", {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
        assert v <= RTOL, (name, i, k, v)


def typed(d):
    return [[k, float(v), type(v).__name__] for k, v in d.items()]


def detector_host(fs=48000):
    from omega_gpu.hip_hop_detector import HipHopDetector
    det = HipHopDetector.__new__(HipHopDetector)  # (the constructor opens the device)
    det._host_init(fs)
    return det


# ---- CPU ----

@pytest.mark.parametrize("name", GROUPS)
def test_hiphop_ref_matches_reference_golden(name):
    """tests/hiphop_ref.py against the reference: every recorded value, peak and feature exactly."""
    g = G()
    for i, e in enumerate(evals(name)):
        p = f"{name}/{i}/"
        np.testing.assert_array_equal(HR.row(e), g[p + "row"])
        np.testing.assert_array_equal(HR.peaks_row(e), g[p + "kick_peaks"])
        check_frame(name, i, HR.row(e), HR.peaks_row(e))
        want = json.loads(str(g[p + "features"]))
        if e["flags"]:
            assert want == []
            continue
        assert [k for k, _, _ in want] == KEYS
        assert typed(HR.reference_features(e, DRUM)) == want


def test_hiphop_closed_form_design_is_scipys():
    """The restatement's step-by-step butter design gives scipy's recorded sections bit for bit."""
    for fs in (48000, 44100, 16000):
        for k, ref in golden_sos(fs).items():
            np.testing.assert_array_equal(HR.butter4_bandpass_sos(*HR.band_edges(fs)[k], fs), ref)
            np.testing.assert_array_equal(HR.scipy_sos(fs)[k], ref)


def test_hiphop_golden_group_assertions():
    """Each group does on the committed golden what it was made for."""
    g = G()
    E = {n: evals(n) for n in GROUPS}
    rows = {n: [g[f"{n}/{i}/row"] for i in range(int(g[f"{n}/n"]))] for n in GROUPS}
    assert [len(f[1]) for f in group("app")[2]] == [2048] * 3 and group("app")[1].shape == (512,)
    assert group("app1025")[1].shape == (1025,)
    for n, m in (("m64", 64), ("m512", 512), ("m8192", 8192), ("fs16", 8192), ("twopeak", 8192)):
        assert all(len(a) == m for _, a in group(n)[2])
    assert group("fs44")[0] == 44100 and group("fs16")[0] == 16000
    e = E["fs16"]
    sp = np.diff(e[0]["kick_peaks"])
    assert e[0]["kick_peak_count"] >= 3 and len(set(sp)) > 1 and e[0]["syncopation"] > 0
    from scipy import signal as ss
    raw = ss.find_peaks(e[1]["envelope"], height=e[1]["envelope_threshold"])[0]
    assert any(any(0 < q - k < 1600 for k in e[1]["kick_peaks"]) for q in raw if q not in e[1]["kick_peaks"])
    assert E["twopeak"][0]["kick_peak_count"] == 2 and rows["twopeak"][0][COL["kick_pattern_factor"]] != 0.5
    assert E["onepeak"][0]["kick_peak_count"] == 1 and E["nopeak"][0]["kick_peak_count"] == 0
    assert rows["onepeak"][0][COL["kick_pattern_factor"]] == rows["nopeak"][0][COL["kick_pattern_factor"]] == 0.5
    # 16-bin tables: ranges without bins, the reference's early returns
    ra, rb, rc = (HR.band_ranges(g[f"k16{c}/freqs"], 48000) for c in "abc")
    assert ra[0][1] == 0 and ra[3][1] == 0 and 0 < ra[6][1] <= 10 and rb[4][1] == 0 and rb[6][1] == 10 and rc[6][1] == 0
    for c in "abc":
        assert rows[f"k16{c}"][0][COL["tilt_branch"]] == 0 and rows[f"k16{c}"][0][COL["vocal_branch"]] == 0
    assert E["k16b"][0]["freq_domain_ratio"] > 0 and E["k16c"][0]["freq_domain_ratio"] == 0.0
    fe = g["edges/freqs"]
    assert all(v in fe for v in (60.0, 500.0, 2000.0))
    rr = HR.band_ranges(fe, 48000)
    assert rr[0][0] + rr[0][1] - 1 == rr[1][0] and rr[3][0] + rr[3][1] - 1 == rr[4][0] and rr[4][0] + rr[4][1] - 1 == rr[5][0]
    v = E["vocal"][0]
    assert 32 in v["vocal_distance_peaks"] and 32 not in v["vocal_peaks"] and 18 not in v["vocal_distance_peaks"]
    assert 54 in v["vocal_peaks"] and 8 in v["vocal_peaks"] and v["vocal_peak_count"] == 2
    s = g["vocal/0/spec"][HR.band_ranges(g["vocal/freqs"], 48000)[6][0]:]
    assert s[53] == s[54] == s[55]
    for i, e in enumerate(E["hann"]):
        assert g[f"hann/{i}/audio"][0] == 0 and e["hihat"][0] == 0 and e["hihat"][1] != 0
    assert rows["silent"][0][COL["flags"]] == 1 and 0.00099 < rows["silent"][0][COL["rms"]] < 0.001
    assert not rows["silent"][0][1:9].any() and not rows["silent"][0][10:].any()
    assert rows["silent"][1][COL["flags"]] == 0 and 0.001 <= rows["silent"][1][COL["rms"]] < 0.00101
    lr = E["lowratio"]
    assert lr[0]["low_ratio"] > 0.5 > lr[1]["low_ratio"] and lr[0]["sub_to_bass_ratio"] > 1 > lr[1]["sub_to_bass_ratio"] > 0
    assert {int(r[COL["tilt_branch"]]) for n in GROUPS for r in rows[n]} >= {0, 1, 2, 3}
    assert {int(r[COL["vocal_branch"]]) for n in GROUPS for r in rows[n]} >= {0, 1, 2}
    for i in range(2):
        assert int(g[f"nonfinite/{i}/flags"]) == 2
        assert not (np.isfinite(g[f"nonfinite/{i}/spec"]).all() and np.isfinite(g[f"nonfinite/{i}/audio"]).all())
    # the decision margins
    for n in GROUPS:
        for e in E[n]:
            if e["flags"]:
                continue
            env, thr = e["envelope"], e["envelope_threshold"]
            loc = np.nonzero((env[1:-1] >= env[:-2]) & (env[1:-1] >= env[2:]))[0] + 1
            assert np.all(np.abs(env[loc] - thr) >= 1e-6 * thr)
            assert all(env[q] - max(env[q - 1], env[q + 1]) >= 1e-9 * env[q] for q in e["kick_peaks"])
            hat = e["hihat"]
            assert np.abs(hat[hat != 0]).min() >= 1e-9 * np.abs(hat).max()
    dev = json.loads(str(g["dev"]))
    assert 0 < dev["sub_bass_normwise"] < 1e-10 and 0 < dev["kick_rms"] < 1e-10


def test_hiphop_facade_host_logic():
    """The facade's host-side parts against the recorded sequences: the result dict built from a recorded row
    equals the reference's (keys, order, values, value types), confidence scaling on both sides of 0.3 and
    0.7, the sub-genre, smoothing with the boost, silent frames leaving the histories untouched,
    get_debug_info and reset. No device is touched."""
    from omega_gpu.hip_hop_detector import COLUMNS
    assert tuple(COLUMNS) == tuple(HR.COLUMNS)
    g = G()
    det = detector_host()
    assert det.feature_weights == json.loads(str(g["feature_weights"]))
    prof = json.loads(str(g["subgenre_profiles"]))
    assert {k: {a: (list(b) if isinstance(b, tuple) else b) for a, b in v.items()} for k, v in det.subgenre_profiles.items()} == prof
    assert [len(h) for h in (det.sub_bass_history, det.kick_pattern_history, det.hihat_density_history,
                             det.spectral_tilt_history, det.confidence_history)] == [0] * 5
    assert det.confidence_history.maxlen == 30
    for name in ("seq", "seq_w"):
        rec = json.loads(str(g[name]))
        det = detector_host()
        if rec["weights"]:
            det.feature_weights = dict(rec["weights"])
        raw, n_silent = [], 0
        for st in rec["steps"]:
            before = list(det.confidence_history)
            r = det.result_from_row(g[f"{st['frame'][0]}/{st['frame'][1]}/row"], st["drum"])
            assert list(r) == RESULT_KEYS
            assert typed(r["features"]) == st["features"], (name, st["frame"])
            assert r["subgenre"] == st["subgenre"] and r["is_hip_hop"] == st["is_hip_hop"]
            assert r["sub_bass_detected"] == st["sub_bass_detected"] and r["strong_beat"] == st["strong_beat"]
            assert abs(r["confidence"] - st["confidence"]) <= 1e-15
            assert [float(c) for c in det.confidence_history] == st["history"]
            if not st["features"]:
                n_silent += 1
                assert list(det.confidence_history) == before and r["confidence"] == 0.0 and r["subgenre"] == "unknown"
            else:
                raw.append(st["history"][-1])
        assert n_silent >= 3 and len(raw) > 30 and len(det.confidence_history) == 30
        dbg = det.get_debug_info()
        assert list(dbg) == list(rec["debug"])
        for k, v in rec["debug"].items():
            np.testing.assert_allclose(np.asarray(dbg[k], float), np.asarray(v, float), rtol=1e-15, atol=0)
        if rec["weights"]:
            assert any(c > 0.7 for c in raw) and any(s["subgenre"] != "unknown" for s in rec["steps"])
            assert any(sum(1 for c in s["history"][-10:] if c > 0.6) >= 7 for s in rec["steps"])
        else:
            assert any(c < 0.3 for c in raw) and any(c >= 0.3 for c in raw)
        det.reset()
        assert not det.confidence_history and det.get_debug_info()["current_confidence"] == 0
    # a frame the device flags as non-finite: the fixed dict, like a silent one
    row = np.zeros(len(HR.COLUMNS))
    row[COL["flags"]] = 2
    assert detector_host().result_from_row(row, DRUM)["features"] == {}
    from omega_gpu import HipHopDetector
    with pytest.raises(ValueError):
        HipHopDetector(0)


def test_hiphop_abi_argument_checks():
    """The entry points' argument checks that run before any device call, and the documented defaults."""
    from omega_gpu import _lib as L
    lib = L.lib()
    cfg = L.HipHopConfig()
    lib.omega_hiphop_config_default(C.byref(cfg))
    assert (cfg.sample_rate, cfg.n_bins) == (48000, 512)
    fr = np.linspace(0, 24000, 512)
    out, kp = np.empty((1, 24)), np.empty((1, 16), np.int32)
    spec, audio = np.zeros(512, np.float32), np.zeros(2048, np.float32)
    assert lib.omega_hiphop_configure(None, C.byref(cfg), fr.ctypes.data) == L.EINVAL
    assert lib.omega_hiphop_features(None, spec.ctypes.data, 512, audio.ctypes.data, 0, 2048, 2048, 1, out.ctypes.data,
                                     kp.ctypes.data, L.MEM_HOST) == L.EINVAL
    assert lib.omega_hiphop_get_sos(None, 0, out.ctypes.data) == L.EINVAL
    sos = np.empty((4, 6))
    assert lib.omega_hiphop_design_sos(48000, 3, sos.ctypes.data) == L.EINVAL
    assert lib.omega_hiphop_design_sos(4000, 0, sos.ctypes.data) == L.EINVAL
    assert lib.omega_hiphop_design_sos(48000, 0, None) == L.EINVAL
    assert b"ABI 5" in lib.omega_version()  # (the entry points are additive)
    assert len(HR.COLUMNS) == 24 and HR.N_PEAKS == 16 >= (8192 - 3) // int(0.1 * HR.MIN_RATE) + 1


def test_hiphop_designed_sections():
    """The library's butter design (omega_hiphop_design_sos, what omega_hiphop_configure stores) against the
    recorded scipy sections at the three rates: the section order and numerators are scipy's, and filtering
    the golden inputs with the library's coefficients (the restatement's sequential filter, on the CPU)
    keeps the filtered RMS within 1e-9. Largest relative coefficient difference: 1.8e-15."""
    from omega_gpu import _lib as L
    lib = L.lib()
    worst = 0.0
    mine = {}
    for fs in (48000, 44100, 16000):
        ref = golden_sos(fs)
        for w, k in enumerate(HR.BANDS):
            sos = np.empty((4, 6))
            assert lib.omega_hiphop_design_sos(fs, w, sos.ctypes.data) == 0
            np.testing.assert_array_equal(sos[1:, :3], ref[k][1:, :3])  # (1, +-2, 1) as scipy pairs them
            np.testing.assert_array_equal(sos[:, 3], 1.0)
            assert list(np.argsort(sos[:, 5])) == [0, 1, 2, 3]          # ascending pole radius
            worst = max(worst, float(np.max(np.abs(sos - ref[k]) / np.abs(np.where(ref[k] == 0, 1, ref[k])))))
            mine[fs, k] = sos
    print(f"largest relative coefficient difference from scipy's sections: {worst:.2e}")
    assert worst <= 1e-13
    assert golden_sos(16000)["hihat"][3, 1] == 2.0 and golden_sos(48000)["hihat"][3, 1] == -2.0  # (the pairing depends on the band)
    dev = 0.0
    for name, i in (("app", 0), ("fs44", 0), ("fs16", 0), ("m64", 1)):
        fs, _, frames = group(name)
        x = frames[i][1][:2048]
        for k in HR.BANDS:
            a, b = HR.sosfilt_seq(mine[fs, k], x), HR.sosfilt_seq(golden_sos(fs)[k], x)
            ra, rb = np.sqrt(np.mean(a ** 2)), np.sqrt(np.mean(b ** 2))
            dev = max(dev, rel(ra, rb))
            if k != "kick":
                want = g_row(name, i)[COL[k + "_rms"]] if len(frames[i][1]) <= 2048 else None
                if want is not None:
                    assert rel(ra, want) <= RTOL, (name, k)
    print(f"filtered RMS with the library's sections against scipy's: {dev:.2e}")
    assert dev <= RTOL


def g_row(name, i):
    return G()[f"{name}/{i}/row"]


# ---- GPU ----

def detector(name):
    from omega_gpu import HipHopDetector
    return HipHopDetector(group(name)[0])


WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUPS)
def test_hiphop_golden_parity(name):
    """Every frame of the group through analyze_frames and through analyze: the golden values, the
    reference's dict."""
    g = G()
    _, freqs, frames = group(name)
    det = detector(name)
    for i, (spec, audio) in enumerate(frames):
        out, kp = det.analyze_frames(spec[None], freqs, audio[None])
        check_frame(name, i, out[0], kp[0], WORST)
        det.reset()
        r = det.analyze(audio, spec, freqs, DRUM)
        want = json.loads(str(g[f"{name}/{i}/features"]))
        assert list(r) == RESULT_KEYS
        got = typed(r["features"])
        assert [(k, t) for k, _, t in got] == [(k, t) for k, _, t in want]
        for (k, a, _), (_, b, _) in zip(got, want):
            assert rel(a, b) <= (RTOL if k in ("sub_bass_presence", "kick_pattern_score", "hihat_density") else 0), (name, i, k)
        if want:
            sub, hip, sb, beat, conf = json.loads(str(g[f"{name}/{i}/result"]))
            assert (r["subgenre"], r["is_hip_hop"], r["sub_bass_detected"], r["strong_beat"]) == (sub, hip, sb, beat)
            assert rel(r["confidence"], conf) <= RTOL
        else:
            assert r["confidence"] == 0.0 and not det.confidence_history
    print("worst so far:", {k: f"{v:.2e}" for k, v in WORST.items()})


@pytest.mark.gpu
def test_hiphop_batch_independence():
    """33 frames of mixed content in one call, a silent and a non-finite frame in the middle, equal the same
    frames one by one; the flagged rows are zero and their neighbours untouched."""
    g = G()
    _, freqs, frames = group("app")
    rng = np.random.default_rng(3)
    pool = frames + group("hann")[2] + group("lowratio")[2] + group("vocal")[2]
    spec = np.stack([pool[i % len(pool)][0] * np.float32(0.5 + rng.random()) for i in range(33)]).astype(np.float32)
    audio = np.stack([np.roll(pool[(i * 3) % len(pool)][1], 37 * i) for i in range(33)])
    audio[15] = g["silent/0/audio"]
    audio[16, 100] = np.nan
    spec[20, 7] = np.inf
    det = detector("app")
    one = det.analyze_frames(spec, freqs, audio)
    for i in range(33):
        r = det.analyze_frames(spec[i:i + 1], freqs, audio[i:i + 1])
        np.testing.assert_array_equal(r[0][0], one[0][i], err_msg=f"frame {i}")
        np.testing.assert_array_equal(r[1][0], one[1][i], err_msg=f"frame {i}")
    fl = one[0][:, COL["flags"]]
    assert fl[15] == 1 and fl[16] == 2 and fl[20] == 2 and not np.delete(fl, [15, 16, 20]).any()
    assert not one[0][16, :9].any() and not one[0][20, :9].any() and (one[1][[15, 16, 20]] == -1).all()
    assert one[0][15, COL["rms"]] == g["silent/0/row"][COL["rms"]] and not one[0][15, 1:9].any()
    e = HR.features(spec[32], freqs, audio[32], 48000)
    for k in HR.EXACT:
        assert one[0][32, COL[k]] == float(e[k]), k
    for k in HR.FILTERED:
        assert rel(one[0][32, COL[k]], float(e[k])) <= RTOL, k


@pytest.mark.gpu
def test_hiphop_input_forms():
    """Device tensors give the host rows bitwise: contiguous, an overlapping unfold view of a stream as
    frames, a strided view of wider spectra; float64 audio follows numpy's float64 rms and energies."""
    import torch
    fs, freqs, frames = group("app1025")
    x = np.concatenate([frames[0][1], frames[1][1]])
    rows = np.stack([x[i * 512:i * 512 + 2048] for i in range(5)])
    spec = np.stack([frames[i % 2][0] * np.float32(1 + 0.1 * i) for i in range(5)]).astype(np.float32)
    want = detector("app1025").analyze_frames(spec, freqs, rows)
    dev = detector("app1025").analyze_frames(torch.from_numpy(spec).cuda(), freqs, torch.from_numpy(rows).cuda())
    assert dev[0].is_cuda and dev[1].dtype == torch.int32
    view = torch.from_numpy(x).cuda().unfold(0, 2048, 512)[:5]
    wide = torch.zeros(5, 1100, device="cuda")
    wide[:, :1025] = torch.from_numpy(spec).cuda()
    got = detector("app1025").analyze_frames(wide[:, :1025], freqs, view)
    for k in range(2):
        np.testing.assert_array_equal(dev[k].cpu().numpy(), want[k])
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k])
    x64 = rows[0].astype(np.float64) * 1.000000123
    out, kp = detector("app1025").analyze_frames(spec[:1], freqs, x64[None])
    e = HR.features(spec[0], freqs, x64, fs)
    for k in HR.EXACT:
        if k != "rms":
            assert out[0, COL[k]] == float(e[k]), k
    assert rel(out[0, COL["rms"]], float(e["rms"])) <= 1e-14
    for k in HR.FILTERED:
        assert rel(out[0, COL[k]], float(e[k])) <= RTOL, k
    np.testing.assert_array_equal(kp[0], HR.peaks_row(e))


@pytest.mark.gpu
def test_hiphop_unsupported_shapes_leave_table():
    """m = 32, 100 and 16384, K = 15 and 8194 raise UnsupportedError naming the number (no CPU fallback); the
    configured table still works afterwards. The library's own checks give the same codes."""
    from omega_gpu import UnsupportedError
    from omega_gpu import _lib as L
    _, freqs, frames = group("app")
    spec, audio = frames[0][0][None], frames[0][1][None]
    det = detector("app")
    want = det.analyze_frames(spec, freqs, audio)
    for K, m in ((512, 32), (512, 100), (512, 16384), (15, 2048), (8194, 2048)):
        with pytest.raises(UnsupportedError, match=str(K if K != 512 else m)):
            det.analyze_frames(np.ones((1, K), np.float32), np.arange(float(K)) if K != 512 else freqs,
                               np.ones((1, m), np.float32))
    lib, ctx = L.lib(), det._eng._ctx
    out, kp, one = np.empty((1, 24)), np.empty((1, 16), np.int32), np.ones(20000, np.float32)
    for K in (15, 8194):
        cfg = L.HipHopConfig(48000, K)
        assert lib.omega_hiphop_configure(ctx, C.byref(cfg), np.arange(float(K)).ctypes.data) == L.EUNSUP
        assert str(K).encode() in lib.omega_last_error(ctx)
    cfg = L.HipHopConfig(4000, 512)
    assert lib.omega_hiphop_configure(ctx, C.byref(cfg), freqs.ctypes.data) == L.EUNSUP
    cfg = L.HipHopConfig(48000, 512)
    assert lib.omega_hiphop_configure(ctx, C.byref(cfg), freqs[::-1].copy().ctypes.data) == L.EINVAL
    for m in (32, 100, 16384):
        assert lib.omega_hiphop_features(ctx, spec.ctypes.data, 512, one.ctypes.data, 0, m, m, 1, out.ctypes.data,
                                         kp.ctypes.data, L.MEM_HOST) == L.EUNSUP
        assert str(m).encode() in lib.omega_last_error(ctx)
    # kick_peaks may be NULL
    assert lib.omega_hiphop_features(ctx, spec.ctypes.data, 512, audio.ctypes.data, 0, 2048, 2048, 1, out.ctypes.data,
                                     None, L.MEM_HOST) == 0
    np.testing.assert_array_equal(out, want[0])
    got = det.analyze_frames(spec, freqs, audio)
    for k in range(2):
        np.testing.assert_array_equal(got[k], want[k])


@pytest.mark.gpu
def test_hiphop_reconfigure_rate():
    """One context from 48000 to 16000 Hz: the sections become the 16 kHz ones and the peak distance 1600, so
    the fs16 frame gives its recorded peaks; at 48000 Hz the same samples give others."""
    from omega_gpu import _lib as L
    g = G()
    _, freqs, frames = group("fs16")
    spec, audio = frames[0]
    det = detector("app")  # 48000 Hz
    a = det.analyze_frames(spec[None], freqs, audio[None])
    s48 = det.filter_sections("kick")
    cfg = L.HipHopConfig(16000, len(freqs))
    det._eng._check(L.lib().omega_hiphop_configure(det._eng._ctx, C.byref(cfg), freqs.ctypes.data))
    s16 = det.filter_sections("kick")
    np.testing.assert_allclose(s16, golden_sos(16000)["kick"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(s48, golden_sos(48000)["kick"], rtol=1e-13, atol=0)
    b = det.analyze_frames(spec[None], freqs, audio[None])  # (same table: the facade does not configure again)
    check_frame("fs16", 0, b[0][0], b[1][0])
    assert int(b[0][0, COL["kick_peak_count"]]) >= 3
    assert not np.array_equal(a[1][0], b[1][0]) and a[0][0, COL["sub_bass_rms"]] != b[0][0, COL["sub_bass_rms"]]
    assert np.diff(b[1][0][b[1][0] >= 0]).min() >= 1600 > int(0.1 * 16000) - 1


def vocal_tie_spectra():
    """Three 1025-bin spectra whose vocal range (bins 9..128 of the 48 kHz table, 120 bins) holds designed
    spikes on a zero floor, positions relative to the range's first bin:
      0  two equal peaks 19 bins apart (10, 29) and a lower one at 45, 16 above the second: the later of the
         equal pair is kept and removes both others, the earlier one would leave the third standing
      1  six peaks 19 apart with increasing heights: one is kept and its lower neighbour removed per round
      2  flat tops of width 2 (30, 31) and 3 (69..71) with lower peaks exactly 20 past their middles (50, 90),
         which stay only while the middles are 30 and 70"""
    freqs = np.linspace(0.0, 24000.0, 1025)
    lo, n = HR.band_ranges(freqs, 48000)[6]
    assert (lo, n) == (9, 120)
    spec = np.zeros((3, 1025), np.float32)
    v = spec[:, lo:lo + n]
    v[0, [10, 29, 45]] = 1.0, 1.0, 0.8
    v[1, 5 + 19 * np.arange(6)] = 0.5 + 0.1 * np.arange(6)
    v[2, [30, 31]], v[2, 50], v[2, 69:72], v[2, 90] = 1.0, 0.6, 0.9, 0.5
    return freqs, spec


@pytest.mark.gpu
def test_hiphop_vocal_peaks_equal_heights_staircase_and_plateaus():
    """The vocal peak count (column 7) on designed spectra with equal heights, several rounds of the distance
    rule and flat tops, at 1025 bins and 64 samples. The expected counts are the restatement's with the kept
    peaks from tools/model/peaks_model.py ("the later index wins"; scipy has no rule for equal heights), and
    they are not the counts the opposite tie rule gives."""
    freqs, spec = vocal_tie_spectra()
    rounds = []

    def later(x, cand, d):
        kept, r = M.select_by_distance(x, cand, d)
        rounds.append(r)
        return kept

    def earlier(x, cand, d):
        return M.select_by_distance(x, cand, d, later_wins=False)[0]
    want = [HR.spectrum_side(s, freqs, 48000, later)["vocal_peak_count"] for s in spec]
    other = [HR.spectrum_side(s, freqs, 48000, earlier)["vocal_peak_count"] for s in spec]
    print("expected counts:", want, "with the earlier index winning:", other, "rounds:", rounds)
    assert want == [1, 3, 4] and other == [2, 3, 4] and rounds[1] == 3  # (non-zero, and the tie rule shows)
    audio = np.sin(0.3 * np.arange(64), dtype=np.float32)[None].repeat(3, axis=0)
    out, _ = detector("app").analyze_frames(spec, freqs, audio)
    assert not out[:, COL["flags"]].any()
    assert list(out[:, COL["vocal_peak_count"]]) == want
