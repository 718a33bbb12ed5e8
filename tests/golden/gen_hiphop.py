"""Makes tests/golden/hiphop.npz by calling the reference's HipHopDetector
(omega4/panels/hip_hop_detector.py:16-486) itself (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_hiphop.py <reference checkout>

The reference module is loaded by path (the omega4.panels package import needs pygame; the module does
not). Only float32 inputs, the reference's outputs, its three *_sos arrays at 48000, 44100 and 16000 Hz and
its weights and profiles (settings and names, as JSON) are written. Per frame: the reference's feature dict
for a kick that is detected (JSON with the value types, in its insertion order), the row of
tests/hiphop_ref.py's COLUMNS -- every feature asserted equal to the reference's own -- and the kept
envelope peaks. The groups, each asserted here for what it is for:

  app        m 2048, K 512 and 1025, at 48 kHz
  m64, m512, m8192   the frame-length ends and a middle size
  fs44       44100 Hz
  fs16       m 8192 at 16 kHz: at least 3 kept envelope peaks with unequal spacings (np.std, np.median and a
             nonzero syncopation); one frame where the distance rule removes a higher-index peak
  twopeak    exactly two kept peaks at 48 kHz, m 8192
  onepeak, nopeak    the 0.5 branch
  k16        16-bin tables on which the sub-bass, a tilt band or the vocal range is empty; <= 10 vocal bins
  edges      table entries at exactly 60, 500 and 2000 Hz
  vocal      a peak that passes the distance rule and fails the prominence threshold, one that passes both,
             a plateau
  hann       frames beginning with exact zeros
  silent     rms just below and just above 0.001
  nonfinite  flags only
  lowratio   both sides of low_ratio > 0.5, and sub_to_bass_ratio above and below 1

Decision margins asserted on every frame: every local maximum of the kick envelope is at least 1e-6
(relative) from the height threshold, every kept peak exceeds its neighbours by at least 1e-9 relative, every
nonzero hi-hat sample has a magnitude of at least 1e-9 of the signal's maximum.
`dev`: the reference's (scipy's sequential sosfilt's) largest deviation from a long-double sequential
evaluation of the same filters over the app and m8192 frames: normwise per filtered signal and relative
per filtered RMS. For the record; it is not the bar.
`seq`: 36 frames through one detector with silent frames in between (the 30-deep histories wrap);
`seq_w`: the same through a detector whose feature_weights attribute names the features as they are called,
so that confidences above 0.7 and 0.6, a sub-genre and the recent_high >= 7 boost occur.
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hiphop_ref as HR  # noqa: E402

KEYS = ["sub_bass_presence", "kick_pattern_score", "hihat_density", "spectral_tilt", "vocal_presence", "tempo_match"]
DRUM = {"kick": {"kick_detected": True, "magnitude": 0.9}}


def import_reference(path):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_hip_hop_detector",
                                                  os.path.join(path, "omega4", "panels", "hip_hop_detector.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HipHopDetector


def typed(d):
    return [[k, float(v), type(v).__name__] for k, v in d.items()]


def track(fs, n, seed, kicks=(), sub=0.3, hats=0.1, voice=0.2, noise=0.003, tau=0.012):
    """A synthetic bar: a 50 Hz sub-bass tone, decaying 70 Hz kick bursts at the given sample offsets
    (offset, amplitude), gated high-passed noise as hi-hats, a few vocal-range partials and a noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = sub * np.sin(2 * np.pi * 50.0 * t + 0.3)
    for at, amp in kicks:
        d = np.maximum(t - at / fs, 0)
        x += amp * (t >= at / fs) * np.exp(-d / tau) * np.sin(2 * np.pi * 70.0 * d)
    h = rng.standard_normal(n)
    h = np.diff(h, prepend=0.0) * (np.sin(2 * np.pi * 8.0 * t) > 0)
    x += hats * h
    for k, f0 in enumerate((330.0, 660.0, 1240.0, 2100.0)):
        x += voice / (k + 1) * np.sin(2 * np.pi * f0 * t + k)
    return x + noise * rng.standard_normal(n)


def spectrum(x, n_fft):
    s = np.abs(np.fft.rfft(x[:n_fft] * np.hanning(n_fft)))
    return (s / s.max()).astype(np.float32)


def bumps(K, at, seed, floor=0.01):
    rng = np.random.default_rng(seed)
    s = floor * (0.5 + rng.random(K))
    for b, h in at:
        s[b] = h
        for d in (1, 2):
            for q in (b - d, b + d):
                if 0 <= q < K:
                    s[q] = max(s[q], h * (1 - 0.4 * d))
    return s.astype(np.float32)


class Recorder:
    def __init__(self, Ref):
        self.Ref, self.d, self.count = Ref, {}, 0

    def frame(self, name, i, fs, spec, freqs, audio):
        spec, audio, freqs = np.asarray(spec, np.float32), np.asarray(audio, np.float32), np.asarray(freqs, np.float64)
        tag = f"{name}[{i}]"
        det = self.Ref(fs)
        r = det.analyze(audio, spec, freqs, DRUM)
        e = HR.features(spec, freqs, audio, fs)
        p = f"{name}/{i}/"
        d = self.d
        d[p + "spec"], d[p + "audio"] = spec, audio
        d[p + "row"], d[p + "kick_peaks"] = HR.row(e), HR.peaks_row(e)
        if e["flags"]:
            assert r["features"] == {} and r["confidence"] == 0.0 and not det.confidence_history, tag
            d[p + "features"] = np.array(json.dumps([]))
            print(f"{tag:12s} silent rms {float(e['rms']):.6f}")
            return r, e
        # the restatement gives the reference's values, bit for bit, and its types
        want = HR.reference_features(e, DRUM)
        assert list(r["features"]) == KEYS == list(want), tag
        for k in KEYS:
            assert r["features"][k] == want[k] and type(r["features"][k]) is type(want[k]), (tag, k, r["features"][k], want[k])
        sos = {"sub_bass": det.sub_bass_sos, "kick": det.kick_sos, "hihat": det.hihat_sos}
        for k in HR.BANDS:
            assert np.array_equal(sos[k], HR.scipy_sos(fs)[k]), tag
        # decision margins
        env, thr = e["envelope"], e["envelope_threshold"]
        loc = np.nonzero((env[1:-1] >= env[:-2]) & (env[1:-1] >= env[2:]))[0] + 1
        assert np.all(np.abs(env[loc] - thr) >= 1e-6 * thr), (tag, "envelope maximum at the threshold")
        for q in e["kick_peaks"]:
            assert env[q] - max(env[q - 1], env[q + 1]) >= 1e-9 * env[q], (tag, q)
        cand = [q for q in loc if env[q] >= thr]
        hts = sorted(env[q] for q in cand)
        assert all(b - a > 1e-9 * b for a, b in zip(hts, hts[1:])), (tag, "equal envelope peaks")
        hat = e["hihat"]
        nz = np.abs(hat[hat != 0])
        assert nz.min() >= 1e-9 * np.abs(hat).max(), (tag, nz.min() / np.abs(hat).max())
        vm = np.abs(spec[(freqs >= 200) & (freqs <= 3000)]).astype(np.float64)
        if len(vm) > 10:
            import scipy.signal as ss
            pk = ss.find_peaks(vm)[0]
            for a in pk:
                for b in pk:
                    assert a == b or abs(a - b) >= 20 or vm[a] != vm[b], (tag, "equal vocal peaks within the distance")
            prom = ss.peak_prominences(vm, e["vocal_distance_peaks"])[0]
            assert np.all(np.abs(prom - e["vocal_pmin"]) > 0), tag
        d[p + "features"] = np.array(json.dumps(typed(r["features"])))
        d[p + "result"] = np.array(json.dumps([r["subgenre"], bool(r["is_hip_hop"]), bool(r["sub_bass_detected"]),
                                               bool(r["strong_beat"]), float(r["confidence"])]))
        self.count += 1
        print(f"{tag:12s} sub {float(e['sub_bass_presence']):.4f} kick {e['kick_peak_count']} {list(e['kick_peaks'])} "
              f"f {float(e['kick_pattern_factor']):.4f} zc {e['hihat_zero_crossings']:4d} hat {float(e['hihat_density']):.4f} "
              f"tilt {float(e['spectral_tilt']):.4f}/{e['tilt_branch']} vocal {float(e['vocal_presence']):.4f}/{e['vocal_branch']} "
              f"pk {e['vocal_peak_count']}")
        return r, e

    def group(self, name, fs, freqs, frames):
        self.d[f"{name}/freqs"] = np.asarray(freqs, np.float64)
        self.d[f"{name}/fs"] = np.array(fs)
        self.d[f"{name}/n"] = np.array(len(frames))
        return [self.frame(name, i, fs, spec, freqs, audio)[1] for i, (spec, audio) in enumerate(frames)]


def main():
    Ref = import_reference(sys.argv[1])
    R = Recorder(Ref)
    d = R.d
    d["versions"] = np.array([np.__version__])
    for fs in (48000, 44100, 16000):
        det = Ref(fs)
        d[f"sos/{fs}"] = np.stack([det.sub_bass_sos, det.kick_sos, det.hihat_sos])
    det = Ref(48000)
    d["feature_weights"] = np.array(json.dumps(det.feature_weights))
    d["subgenre_profiles"] = np.array(json.dumps(det.subgenre_profiles))

    fs = 48000
    f512, f1025 = np.fft.rfftfreq(1022, 1 / fs), np.fft.rfftfreq(2048, 1 / fs)
    f4097 = np.fft.rfftfreq(8192, 1 / fs)
    kicks48 = [(300, 0.9), (5600, 0.7)]

    def plain(x, m):
        return x[:m].astype(np.float32)

    # the app's shapes
    xs = [track(fs, 8192, s, kicks48, sub=a, hats=h) for s, a, h in ((1, 0.3, 0.1), (2, 0.05, 0.3), (3, 0.6, 0.02))]
    app = R.group("app", fs, f512, [(spectrum(x, 1022), plain(x, 2048)) for x in xs])
    app2 = R.group("app1025", fs, f1025, [(spectrum(x, 2048), plain(x[1000:], 2048)) for x in xs[:2]])
    assert len({e["tilt_branch"] for e in app + app2}) >= 1
    R.group("m64", fs, f512, [(spectrum(xs[0], 1022), plain(xs[0][500:], 64)), (spectrum(xs[1], 1022), plain(xs[1], 64))])
    R.group("m512", fs, f512, [(spectrum(xs[1], 1022), plain(xs[1][100:], 512))])
    m8192 = R.group("m8192", fs, f4097, [(spectrum(x, 8192), plain(x, 8192)) for x in xs[:2]])
    x44 = track(44100, 4096, 4, [(200, 0.8)])
    R.group("fs44", 44100, np.fft.rfftfreq(2048, 1 / 44100), [(spectrum(x44, 2048), plain(x44, 2048))])

    # 16 kHz, m 8192: three or more kept peaks with unequal spacings; a higher-index peak the distance rule removes
    f16 = np.fft.rfftfreq(2048, 1 / 16000)
    xa = track(16000, 8192, 5, [(500, 1.0), (2400, 0.9), (4300, 0.95), (7000, 0.85)], sub=0.02, tau=0.01)
    xb = track(16000, 8192, 6, [(1000, 1.0), (2000, 0.8), (5000, 0.9)], sub=0.02, tau=0.008)
    g = R.group("fs16", 16000, f16, [(spectrum(xa, 2048), plain(xa, 8192)), (spectrum(xb, 2048), plain(xb, 8192))])
    sp = np.diff(g[0]["kick_peaks"])
    assert g[0]["kick_peak_count"] >= 3 and len(set(sp)) > 1 and g[0]["syncopation"] > 0 and np.std(sp) > 0, g[0]["kick_peaks"]
    import scipy.signal as ss
    raw = ss.find_peaks(g[1]["envelope"], height=g[1]["envelope_threshold"])[0]
    gone = [q for q in raw if q not in g[1]["kick_peaks"]]
    assert any(any(0 < q - k < 1600 for k in g[1]["kick_peaks"]) for q in gone), (raw, g[1]["kick_peaks"])

    xt = track(fs, 8192, 7, [(800, 1.0), (6200, 0.9)], sub=0.02, tau=0.006)
    g = R.group("twopeak", fs, f512, [(spectrum(xt, 1022), plain(xt, 8192))])
    assert g[0]["kick_peak_count"] == 2 and g[0]["kick_pattern_factor"] != 0.5
    xo = track(fs, 8192, 8, [(3000, 1.0)], sub=0.02, tau=0.006)
    g = R.group("onepeak", fs, f512, [(spectrum(xo, 1022), plain(xo, 8192))])
    assert g[0]["kick_peak_count"] == 1 and g[0]["kick_pattern_factor"] == 0.5
    found = None
    for off in range(0, 6000, 500):  # a short frame on which the kick band only swells: no local maximum above the height
        xn = xs[2][off:off + 2048]
        if HR.audio_side(xn.astype(np.float32), HR.scipy_sos(fs), fs)["kick_peak_count"] == 0:
            found = xn
            break
    assert found is not None
    g = R.group("nopeak", fs, f512, [(spectrum(found, 1022), plain(found, 2048))])
    assert g[0]["kick_peak_count"] == 0 and g[0]["kick_pattern_factor"] == 0.5

    # 16-bin tables
    rng = np.random.default_rng(9)
    s16 = [(0.1 + rng.random(16)).astype(np.float32) for _ in range(3)]
    tabs = [np.linspace(0, 24000, 16), 20.0 + 30.0 * np.arange(16), 5000.0 + 1000.0 * np.arange(16)]
    ka, kb, kc = (R.group(f"k16{c}", fs, tab, [(s, plain(xs[0], 256))])[0] for c, tab, s in zip("abc", tabs, s16))
    ra, rb, rc = (dict(enumerate(HR.band_ranges(tab, fs))) for tab in tabs)
    assert ra[0][1] == 0 and ra[3][1] == 0 and ka["tilt_branch"] == 0 and 0 < ra[6][1] <= 10 and ka["vocal_branch"] == 0
    assert rb[0][1] > 0 and rb[4][1] == 0 and kb["tilt_branch"] == 0 and rb[6][1] == 10 and kb["vocal_branch"] == 0
    assert kb["freq_domain_ratio"] > 0
    assert rc[6][1] == 0 and rc[0][1] == 0 and kc["vocal_presence"] == 0.0 and kc["freq_domain_ratio"] == 0.0

    # table entries at exactly 60, 500 and 2000 Hz: the bins belong to two bands
    fe = 20.0 * np.arange(1025)
    assert all(v in fe for v in (60.0, 500.0, 2000.0))
    se = bumps(1025, [(3, 0.9), (25, 0.8), (100, 0.7), (60, 0.4)], 10)
    ge = R.group("edges", fs, fe, [(se, plain(xs[0], 2048))])[0]
    rr = HR.band_ranges(fe, fs)
    assert rr[0][0] + rr[0][1] - 1 == rr[1][0] == 3 and rr[3][0] + rr[3][1] - 1 == rr[4][0] == 25 and rr[4][0] + rr[4][1] - 1 == rr[5][0] == 100
    assert ge["tilt_branch"] > 0

    # vocal peaks over the 512-bin table (vocal range: bins 5..63)
    lo = HR.band_ranges(f512, fs)[6][0]
    sv = [bumps(512, [(lo + 8, 1.0), (lo + 18, 0.5), (lo + 32, 0.25), (lo + 54, 0.8)], 11),
          bumps(512, [(lo + 10, 0.6), (lo + 35, 1.0), (lo + 52, 0.2)], 12)]
    sv[0][lo + 53:lo + 56] = np.float32(0.8)  # a plateau: scipy takes its middle
    gv = R.group("vocal", fs, f512, [(s, plain(xs[0], 2048)) for s in sv])
    assert 54 in gv[0]["vocal_peaks"] and sv[0][lo + 53] == sv[0][lo + 54] == sv[0][lo + 55]
    assert 32 in gv[0]["vocal_distance_peaks"] and 32 not in gv[0]["vocal_peaks"]  # passes the distance rule, fails prominence
    assert 18 not in gv[0]["vocal_distance_peaks"] and 8 in gv[0]["vocal_peaks"]  # removed by the distance rule
    assert gv[0]["vocal_peak_count"] == 2 and gv[1]["vocal_peak_count"] >= 1

    # Hann-windowed frames begin with an exact zero
    gh = R.group("hann", fs, f512, [(spectrum(x, 1022), (x[:2048] * np.hanning(2048)).astype(np.float32)) for x in xs[:2]])
    for i, e in enumerate(gh):
        assert d[f"hann/{i}/audio"][0] == 0 and e["hihat"][0] == 0 and e["hihat"][1] != 0

    # the silence gate
    base = xs[0][:2048] / np.sqrt(np.mean(xs[0][:2048] ** 2))
    gs = R.group("silent", fs, f512, [(spectrum(xs[0], 1022), (base * 0.000999).astype(np.float32)),
                                      (spectrum(xs[0], 1022), (base * 0.001001).astype(np.float32))])
    assert gs[0]["flags"] == 1 and 0.00099 < gs[0]["rms"] < 0.001 and gs[1]["flags"] == 0 and 0.001 <= gs[1]["rms"] < 0.00101

    # non-finite frames: flags only
    bad_spec = spectrum(xs[0], 1022)
    bad_spec[77] = np.nan
    bad_audio = plain(xs[0], 2048).copy()
    bad_audio[5] = np.inf
    d["nonfinite/freqs"], d["nonfinite/fs"], d["nonfinite/n"] = f512, np.array(fs), np.array(2)
    for i, (s, a) in enumerate(((bad_spec, plain(xs[0], 2048)), (spectrum(xs[0], 1022), bad_audio))):
        e = HR.features(s, f512, a, fs)
        assert e["flags"] == 2 and not HR.row(e)[:9].any()
        d[f"nonfinite/{i}/spec"], d[f"nonfinite/{i}/audio"], d[f"nonfinite/{i}/flags"] = s, a, np.array(2)

    # low_ratio on both sides of 0.5, sub_to_bass_ratio above and below 1
    sl = [bumps(512, [(1, 1.0), (4, 0.3), (30, 0.5), (100, 0.4)], 13), bumps(512, [(1, 0.2), (4, 0.9), (30, 1.0), (100, 0.9)], 14)]
    gl = R.group("lowratio", fs, f512, [(s, plain(xs[0], 2048)) for s in sl])
    assert gl[0]["low_ratio"] > 0.5 > gl[1]["low_ratio"] and gl[0]["tilt_branch"] in (2, 3) and gl[1]["tilt_branch"] == 1
    assert gl[0]["sub_to_bass_ratio"] > 1 > gl[1]["sub_to_bass_ratio"] > 0

    # the reference's deviation from a long-double evaluation of the same filters
    dev = {}
    for name, es in (("app", app), ("m8192", m8192)):
        for i, e in enumerate(es):
            x = d[f"{name}/{i}/audio"]
            for k in HR.BANDS:
                yl = HR.sosfilt_seq(HR.scipy_sos(fs)[k], x, np.longdouble)
                import scipy.signal as ss2
                y = ss2.sosfilt(HR.scipy_sos(fs)[k], x)
                nw = float(np.max(np.abs(y - yl)) / np.max(np.abs(yl)))
                rl = np.sqrt(np.mean(yl ** 2))
                rr_ = float(abs(np.sqrt(np.mean(y ** 2)) - rl) / rl)
                dev[k + "_normwise"] = max(dev.get(k + "_normwise", 0.0), nw)
                dev[k + "_rms"] = max(dev.get(k + "_rms", 0.0), rr_)
    d["dev"] = np.array(json.dumps(dev))
    print("reference deviation from the long-double evaluation:", dev)

    # recorded analyze sequences: rows from a pool of frames, drum_info varying, silent frames in between
    pool = [("app", 0), ("k16a", 0), ("app", 2), ("lowratio", 0), ("vocal", 0), ("twopeak", 0), ("silent", 0), ("hann", 1)]
    good = {"sub_bass_presence": 0.25, "kick_pattern_score": 0.20, "hihat_density": 0.15, "spectral_tilt": 0.15,
            "vocal_presence": 0.15, "tempo_match": 0.10}
    for seq_name, weights in (("seq", None), ("seq_w", good)):
        det = Ref(fs)
        if weights:
            det.feature_weights = dict(weights)
        steps = []
        for i in range(36):
            name, k = pool[6] if i in (4, 17, 18, 33) else pool[(i * 5 + i // 7) % 6 if i % 9 else 7]
            drum = {"kick": {"kick_detected": i % 4 != 3, "magnitude": [0.95, 0.6, 1.3, 0.2][i % 4]}} if i % 11 != 10 else {}
            if weights and 8 <= i < 30:  # a stretch of confident frames
                name, k = ("lowratio", 0) if i not in (17, 18) else pool[6]
                drum = {"kick": {"kick_detected": True, "magnitude": 1.5}}
            r = det.analyze(d[f"{name}/{k}/audio"], d[f"{name}/{k}/spec"], d[f"{name}/freqs"], drum)
            steps.append({"frame": [name, k], "drum": drum, "features": typed(r["features"]), "confidence": float(r["confidence"]),
                          "subgenre": r["subgenre"], "is_hip_hop": bool(r["is_hip_hop"]),
                          "sub_bass_detected": bool(r["sub_bass_detected"]), "strong_beat": bool(r["strong_beat"]),
                          "history": [float(c) for c in det.confidence_history]})
        dbg = det.get_debug_info()
        d[seq_name] = np.array(json.dumps({"weights": weights, "steps": steps,
                                           "debug": {k: ([float(x) for x in v] if isinstance(v, list) else float(v)) for k, v in dbg.items()}}))
        hist = [s["history"][-1] for s in steps if s["features"]]
        assert len(hist) > 30 and any(not s["features"] for s in steps)
        if weights:
            assert any(c > 0.7 for c in hist) and any(s["subgenre"] != "unknown" for s in steps)
            assert any(sum(1 for c in s["history"][-10:] if c > 0.6) >= 7 for s in steps)
        else:
            assert any(c < 0.3 for c in hist) and any(0.3 <= c for c in hist) and max(hist) < 0.6
    out = os.path.join(HERE, "hiphop.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes;", R.count, "frames recorded")


if __name__ == "__main__":
    main()
