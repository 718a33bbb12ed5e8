"""Makes tests/golden/genre.npz by calling the reference's GenreClassifier
(omega4/panels/genre_classification.py:16-795) itself (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_genre.py <reference checkout>

The reference is imported with ``pygame`` stubbed (the panel module imports it at the top; no drawing
code runs). Only inputs (float32), the reference's outputs and its genre_patterns table (settings and
names, as JSON) are written. Per frame: the reference's feature dict (JSON, in its insertion order), the
row of tests/genre_ref.py's COLUMNS -- every value asserted equal to the reference's own -- and the
intermediate decisions (rolloff index, crossing count, percentile ranks and order statistics, the five
peak bins and the qualifying count, the mid_frequency_dominance branch). The spectra and audio of the
groups app, k1025, k4097, m1024, m4096, fs44 and offset are those of tests/golden/harmonic.npz (its
tables too); the other groups are made here and each asserts what it is for:

  k16a/b/c   16-bin tables on which bands are empty: the reference's "no bins" branches are taken
  seq        five consecutive frames through one classifier (the flux state)
  distort    a qualifying count strictly between 0 and 5; a top-5 peak below bin 5; peak * n >= K cutting
             the harmonics; two equal magnitudes among the five largest peaks
  rolloff    the float64 cumsum picks another bin than the float32 one (seeds are searched)
  zeros      audio with exact zeros and runs of equal values (np.sign, ties in the order statistics)
  silent     the all-zero frame
  mid        both mid_frequency_dominance branches
  nonfinite  non-finite frames, recorded only as flags
  and on every frame mid_energy is at least MID (1e-4, relative) from 1.2 low and 1.5 high.

`dev`: per float32-path column (genre_ref.F32_PATH) the reference's largest deviation from the float64
evaluation of the same formulas (relative; absolute where that evaluation is 0) over all frames.
`classify`: a sequence of recorded feature dicts through one classifier's classify(), with the
probabilities in their order; `classify_hh`: the same with a hip-hop confidence supplied to it.
"""
import json
import os
import sys
import time
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import genre_ref as GR  # noqa: E402

MID = 1e-4
REF_KEYS = {"spectral_centroid": "spectral_centroid", "spectral_rolloff": "spectral_rolloff",
            "spectral_bandwidth": "spectral_bandwidth", "dynamic_range": "dynamic_range", "bass_emphasis": "bass_emphasis",
            "vocal_presence": "vocal_presence", "high_freq_energy": "high_freq_energy", "spectral_flux": "spectral_flux",
            "mid_frequency_dominance": "mid_frequency_dominance"}


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = types.ModuleType("pygame")
    pg.font = SimpleNamespace(Font=object)
    pg.Surface = object
    sys.modules.setdefault("pygame", pg)
    sys.path.insert(0, path)
    from omega4.panels.genre_classification import GenreClassifier
    return GenreClassifier


def stack(fs, f0, n, seed, partials, noise=0.002):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = sum(a * np.sin(2 * np.pi * f0 * (k + 1) * t + 0.4 * k) for k, a in enumerate(partials))
    return x / np.max(np.abs(x)) + noise * rng.standard_normal(n)


def audio_frame(x, m):
    return (x[:m] * np.hanning(m)).astype(np.float32)


def rfft_spec(x, n):
    s = np.abs(np.fft.rfft(x[:n] * np.hanning(n)))
    return (s / s.max()).astype(np.float32)


def bumps(K, at, seed, floor=0.01):
    rng = np.random.default_rng(seed)
    s = floor * (0.5 + rng.random(K))
    for b, h in at:
        for d in range(-2, 3):
            if 0 <= b + d < K:
                s[b + d] = max(s[b + d], h * (1 - 0.4 * abs(d)))
    return s.astype(np.float32)


def host_inputs(i):
    """Drum, harmonic, chroma and history inputs that vary from frame to frame (deterministic)."""
    rng = np.random.default_rng(1000 + i)
    drum = {"kick": {"magnitude": float(rng.random()), "kick_detected": bool(i % 2)},
            "snare": {"magnitude": float(rng.random())}}
    if i % 5 == 4:
        drum = {}
    if i % 3 == 0:
        harm = {"harmonic_series": [{"strength": float(rng.random())} for _ in range(1 + i % 7)]}
    elif i % 3 == 1:
        harm = {"harmonic_series": []}
    else:
        harm = {}
    if i % 4 == 0:
        chroma = None
    elif i % 4 == 1:
        chroma = [0.0] * 12
    else:
        chroma = rng.random(12)
        if i % 4 == 3:  # a power chord: root and fifth, weak thirds
            chroma = np.full(12, 0.01)
            chroma[(i // 4) % 12], chroma[((i // 4) % 12 + 7) % 12] = 1.0, 0.5
        chroma = [float(v) for v in chroma]
    names = ["C", "G", "Am", "F"]
    chords = None if i % 3 == 0 else [names[int(k)] for k in rng.integers(0, 4, 2 + i % 6)]
    keys = None if i % 3 == 1 else [names[int(k)] for k in rng.integers(0, 2, 2 + i % 5)]
    return drum, harm, chroma, chords, keys


class Recorder:
    def __init__(self, Ref):
        self.Ref = Ref
        self.d = {}
        self.dev = dict.fromkeys(GR.F32_PATH, 0.0)
        self.count = 0
        self.feats = []

    def frame(self, name, i, clf, spec, freqs, audio, prev):
        spec, audio, freqs = np.asarray(spec, np.float32), np.asarray(audio, np.float32), np.asarray(freqs, np.float64)
        tag = f"{name}[{i}]"
        drum, harm, chroma, chords, keys = host_inputs(self.count)
        r = clf.extract_features(spec, audio, freqs, drum, harm, None if chroma is None else np.array(chroma), chords, keys)
        e = GR.features(spec, freqs, audio, prev)
        e64 = GR.features(spec, freqs, audio, prev, f64=True)
        # the restatement gives the reference's values, bit for bit
        for rk, ek in REF_KEYS.items():
            assert float(r[rk]) == e[ek], (tag, rk, r[rk], e[ek])
        assert float(r["zero_crossing_rate"]) == e["zero_crossings"] / len(audio), tag
        mag = np.abs(spec)
        assert float(clf.compute_spectral_complexity(mag, freqs)) == e["spectral_complexity"], tag
        if not harm.get("harmonic_series"):
            assert float(r["harmonic_complexity"]) == e["spectral_complexity"], tag
        score = 0.0
        for _ in range(e["distortion_count"]):
            score += 0.2
        assert float(r["harmonic_distortion"]) == min(score, 1.0), (tag, r["harmonic_distortion"], e["distortion_count"])
        a = np.abs(audio)
        assert float(np.percentile(a, 95)) == e["loud"] and float(np.percentile(a, 20)) == e["quiet"], tag
        s = np.sort(a)
        assert (float(s[e["ranks"][0]]), float(s[e["ranks"][0] + 1]), float(s[e["ranks"][1]]), float(s[e["ranks"][1] + 1])) == e["order_stats"]
        assert float(np.sqrt(np.mean(audio ** 2))) == e["rms"], tag
        cs = np.cumsum(mag)
        if cs[-1] > 0:
            assert e["rolloff_index"] == np.where(cs >= 0.85 * cs[-1])[0][0] and r["spectral_rolloff"] == freqs[e["rolloff_index"]], tag
        assert e["mid_branch"] == 0 or e["mid_margin"] >= MID, (tag, e["mid_margin"])
        assert e64["mid_branch"] == e["mid_branch"], tag
        for k in GR.F32_PATH:
            dv = abs(e[k] - e64[k]) / abs(e64[k]) if e64[k] != 0 else abs(e[k])
            self.dev[k] = max(self.dev[k], dv)
        d, p = self.d, f"{name}/{i}/"
        d[p + "spec"], d[p + "audio"] = spec, audio
        d[p + "row"] = GR.row(e)
        d[p + "peak_bins"] = e["peak_bins"]
        d[p + "ranks"] = np.array(e["ranks"])
        d[p + "order_stats"] = np.array(e["order_stats"], np.float64)
        d[p + "mid_branch"] = np.array(e["mid_branch"])
        d[p + "rolloff_index64"] = np.array(e64["rolloff_index"])
        d[p + "features"] = np.array(json.dumps([[k, float(v)] for k, v in r.items()]))
        d[p + "host"] = np.array(json.dumps({"drum": drum, "harmonic": harm, "chroma": chroma, "chords": chords, "keys": keys}))
        self.count += 1
        self.feats.append({k: float(v) for k, v in r.items()})
        print(f"{tag:12s} roll {e['rolloff_index']:5d}/{e64['rolloff_index']:5d} zc {e['zero_crossings']:4d} dr {e['dynamic_range']:.4f} "
              f"bass {e['bass_emphasis']:.4f} vocal {e['vocal_presence']:.4f} high {e['high_freq_energy']:.4f} flux {e['spectral_flux']:.4f} "
              f"dist {e['distortion_count']} {list(e['peak_bins'])} mid {e['mid_frequency_dominance']:.4f}/{e['mid_branch']} cx {e['spectral_complexity']:.4f}")
        return r, e, e64

    def group(self, name, fs, freqs, frames, sequence=False):
        self.d[f"{name}/freqs"] = np.asarray(freqs, np.float64)
        self.d[f"{name}/fs"] = np.array(fs)
        self.d[f"{name}/n"] = np.array(len(frames))
        out, clf, prev = [], self.Ref(fs), None
        for i, (spec, audio) in enumerate(frames):
            if not sequence:
                clf, prev = self.Ref(fs), None
            out.append(self.frame(name, i, clf, spec, freqs, audio, prev))
            prev = np.abs(np.asarray(spec, np.float32))
        return out


def main():
    Ref = import_reference(sys.argv[1])
    R = Recorder(Ref)
    d = R.d
    d["versions"] = np.array([np.__version__])
    H = np.load(os.path.join(HERE, "harmonic.npz"), allow_pickle=False)
    for name, take in (("app", 3), ("k1025", 2), ("k4097", 2), ("m1024", 1), ("m4096", 1), ("fs44", 1), ("offset", 1)):
        # (the offset table's 3 kHz rate is below what the reference's constructor accepts -- its hip-hop
        # filter bank -- and extract_features never reads the rate: that group is recorded at 48 kHz)
        R.group(name, max(int(H[f"{name}/fs"]), 44100), H[f"{name}/freqs"],
                [(H[f"{name}/{i}/spec"], H[f"{name}/{i}/audio"]) for i in range(take)])
    fs = 48000
    fa = np.linspace(0, 24000, 512)
    fp = np.fft.rfftfreq(2048, 1 / fs)
    saw = [1.0 / k for k in range(1, 20)]
    rng = np.random.default_rng(5)

    # 16-bin tables with empty bands
    x = stack(fs, 300.0, 256, 21, saw[:6], 0.01)
    s16 = [(0.1 + rng.random(16)).astype(np.float32) for _ in range(3)]
    ga = R.group("k16a", fs, np.linspace(0, 24000, 16), [(s16[0], audio_frame(x, 15))])[0]
    gb = R.group("k16b", fs, 5000.0 + 1000.0 * np.arange(16), [(s16[1], audio_frame(x, 100))])[0]
    gc = R.group("k16c", fs, np.linspace(0, 300, 16), [(s16[2], audio_frame(x, 33))])[0]
    assert ga[0]["bass_emphasis"] == 0.0 and ga[1]["mid_branch"] != 0 and ga[0]["vocal_presence"] > 0 and ga[0]["high_freq_energy"] > 0
    assert gb[0]["vocal_presence"] == 0.0 and gb[1]["mid_branch"] == 0 and gb[0]["high_freq_energy"] > 0 and gb[1]["spectral_complexity"] == 0.3
    assert gc[0]["bass_emphasis"] > 0 and gc[0]["high_freq_energy"] == 0.0 and gc[1]["mid_branch"] == 0 and gc[0]["vocal_presence"] > 0
    for g, tab in ((ga, np.linspace(0, 24000, 16)), (gb, 5000.0 + 1000.0 * np.arange(16)), (gc, np.linspace(0, 300, 16))):
        assert any(n == 0 for _, n in GR.band_ranges(tab))

    # the sequence: five frames at hop 512 through one classifier
    s = stack(fs, 200.0, 2048 + 4 * 512, 14, saw[:10], 0.003)
    s = s * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * np.arange(len(s)) / fs))
    got = R.group("seq", fs, fp, [(rfft_spec(s[f * 512:], 2048), audio_frame(s[f * 512:], 2048)) for f in range(5)], sequence=True)
    flux = [e["spectral_flux"] for _, e, _ in got]
    assert flux[0] == 0 and min(flux[1:]) > 0, flux

    # distortion
    au = audio_frame(stack(fs, 440.0, 1024, 22, saw[:5]), 1024)
    dsp = [bumps(512, [(20, 1.0), (40, 0.5), (60, 0.4), (33, 0.9), (150, 0.8), (200, 0.7), (251, 0.6)], 31),   # some qualify
           bumps(512, [(3, 1.0), (30, 0.8), (60, 0.5), (90, 0.4), (120, 0.3), (150, 0.2)], 32),                   # a peak below bin 5
           bumps(512, [(300, 1.0), (110, 0.9), (220, 0.5), (330, 0.4), (440, 0.3), (50, 0.2)], 33),               # peak * n >= K
           bumps(512, [(25, 0.75), (50, 0.75), (75, 0.5), (100, 0.25), (125, 0.125), (400, 1.0)], 34)]            # equal magnitudes
    got = R.group("distort", fs, fa, [(sp, au) for sp in dsp])
    e = [g[1] for g in got]
    assert any(0 < x["distortion_count"] < 5 for x in e), [x["distortion_count"] for x in e]
    assert any(0 <= b < 5 for b in e[1]["peak_bins"]), e[1]["peak_bins"]
    assert any(b >= 5 and b * 2 < 512 <= b * 5 for b in e[2]["peak_bins"]) and any(b * 2 >= 512 for b in e[2]["peak_bins"])
    top = [dsp[3][b] for b in e[3]["peak_bins"] if b >= 0]
    assert len(top) == 5 and len(set(top)) < 5 and list(e[3]["peak_bins"]).index(25) < list(e[3]["peak_bins"]).index(50), (top, e[3]["peak_bins"])

    # rolloff: a spectrum on which the float64 running sum picks another bin
    fk = np.fft.rfftfreq(8192, 1 / fs)
    found = []
    for seed in range(200):
        # (strong bins, a long stretch of weak ones that holds the 85 % point, strong bins again: the weak
        # bins' steps are of the size of the float32 running sum's error)
        sp = np.random.default_rng(seed).random(4097)
        sp[1000:3000] *= 0.002
        sp[3000:] *= ((sp[:1000].sum() + 0.5 * sp[1000:3000].sum()) / 0.85 - sp[:3000].sum()) / sp[3000:].sum()
        sp = sp.astype(np.float32)
        c32, c64 = np.cumsum(sp), np.cumsum(sp.astype(np.float64))
        i32, i64 = np.where(c32 >= 0.85 * c32[-1])[0][0], np.where(c64 >= 0.85 * c64[-1])[0][0]
        if i32 != i64:
            found.append(sp)
            if len(found) == 2:
                break
    assert len(found) == 2
    got = R.group("rolloff", fs, fk, [(sp, au) for sp in found])
    assert all(e["rolloff_index"] != e64["rolloff_index"] for _, e, e64 in got)

    # zeros and runs of equal values in the audio
    z = np.round(stack(fs, 700.0, 1000, 23, saw[:4], 0.0) * 8) / 8
    z[100:140] = 0.0
    z[500:520] = 0.25
    z2 = np.round(stack(fs, 1500.0, 999, 24, saw[:3], 0.0) * 4) / 4
    z2[::7] = 0.0
    got = R.group("zeros", fs, fa, [(dsp[0], z.astype(np.float32)), (dsp[1], z2.astype(np.float32))])
    for (_, e, _), x in zip(got, (z, z2)):
        assert (x == 0).sum() > 20 and e["zero_crossings"] > 0 and len(np.unique(np.abs(x))) < 12
    assert any(e["order_stats"][0] == e["order_stats"][1] for _, e, _ in got)
    R.group("silent", fs, fa, [(np.zeros(512, np.float32), np.zeros(2048, np.float32))])

    # both mid_frequency_dominance branches
    mids = [bumps(512, [(21, 1.0), (30, 0.9), (5, 0.2), (100, 0.3)], 41), bumps(512, [(5, 1.0), (21, 0.4), (100, 0.9)], 42)]
    got = R.group("mid", fs, fa, [(sp, au) for sp in mids])
    assert sorted(e["mid_branch"] for _, e, _ in got) == [1, 2], [e["mid_branch"] for _, e, _ in got]

    # non-finite frames: flags only
    bad_spec = dsp[0].copy()
    bad_spec[77] = np.nan
    bad_audio = au.copy()
    bad_audio[5] = np.inf
    d["nonfinite/freqs"], d["nonfinite/fs"], d["nonfinite/n"] = fa, np.array(fs), np.array(2)
    for i, (sp, a) in enumerate(((bad_spec, au), (dsp[0], bad_audio))):
        e = GR.features(sp, fa, a)
        assert e["flags"] == 2 and not GR.row(e)[:16].any()
        d[f"nonfinite/{i}/spec"], d[f"nonfinite/{i}/audio"], d[f"nonfinite/{i}/flags"] = sp, a, np.array(2)

    assert all(v > 0 for v in R.dev.values()), R.dev
    d["dev"] = np.array([R.dev[k] for k in GR.F32_PATH], np.float64)
    d["dev_names"] = np.array(GR.F32_PATH)
    print("reference deviation from the float64 evaluation:", R.dev)

    clf = Ref(fs)
    pat = {g: {k: (list(v) if isinstance(v, tuple) else v) for k, v in row.items()} for g, row in clf.genre_patterns.items()}
    d["genre_patterns"] = np.array(json.dumps(pat))
    d["genres"] = np.array(json.dumps(clf.genres))
    seq = R.feats[:3] + R.feats[10:18]
    rec = []
    for ft in seq:
        pr = clf.classify(dict(ft))
        rec.append([[k, float(v)] for k, v in pr.items()])
    d["classify"] = np.array(json.dumps({"features": [list(map(list, ft.items())) for ft in seq], "probabilities": rec,
                                         "top3": [[g, float(v)] for g, v in clf.get_top_genres(pr, 3)]}))
    clf = Ref(fs)
    clf.hip_hop_detector.analyze = lambda *a, **k: {"confidence": 0.77}
    rec = []
    for ft in seq[:5]:
        pr = clf.classify(dict(ft), np.zeros(8), np.zeros(8), np.zeros(8), {})
        rec.append([[k, float(v)] for k, v in pr.items()])
    d["classify_hh"] = np.array(json.dumps({"confidence": 0.77, "probabilities": rec}))
    assert clf.classify({}) != {} and Ref(fs).classify({}) == {"Unknown": 1.0}

    # the reference's time per call on one core (DESIGN: beside tools/kernel_bench.py genre)
    spec, audio = H["app/0/spec"], H["app/0/audio"]
    drum, harm, chroma, chords, keys = host_inputs(2)
    clf = Ref(fs)
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        clf.extract_features(spec, audio, fa, drum, harm, np.array(chroma), chords, keys)
        ts.append(time.perf_counter() - t0)
    d["ref_ms_per_call"] = np.array(float(np.median(ts)) * 1e3)
    print(f"reference: {np.median(ts) * 1e3:.2f} ms per call (median of 20); {R.count} frames recorded")
    out = os.path.join(HERE, "genre.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
