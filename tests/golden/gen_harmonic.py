"""Makes tests/golden/harmonic.npz by calling the reference's HarmonicAnalyzer
(omega4/panels/harmonic_analysis.py:15-431, with omega4/analyzers/harmonic_metrics.py) itself (build
container only; TEST INFRASTRUCTURE ONLY). Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_harmonic.py <reference checkout>

The reference is imported with ``pygame`` stubbed (the panel module imports it at the top; no drawing
code runs). Only inputs (float32), the reference's outputs and its instrument_profiles table (settings
and names, as JSON) are written. Every frame is recorded only when the conditions of
tests/test_harmonic.py hold for it (asserted here, on the CPU), so no device test leaves a frame out.
The margins, chosen against the recorded deviations (float32 paths ~1e-7 relative, root finding
~1e-12), with several orders of magnitude to spare:

  STRENGTH   every candidate strength at least 0.01 from 0.3; kept strengths differ by at least 1e-4
  TOL        every |freqs[idx] - n f0| against 0.05 f0 / 0.1 f0 at least 1e-6 f0 from equality
  ARGMIN     the two smallest |freqs - target| differ by at least 1e-6 bin widths, or not at all: an exact
             tie (a target half-way between two bins, e.g. 0.95 f0 for f0 on an even bin) is intended --
             numpy and the kernel compare the same float64 differences and both keep the first minimum;
             the frames with one are listed in `argmin_ties`
  ARGMAX     the two largest values of an inharmonicity search range differ by at least 1e-5 relative
  ROLLOFF    the cumulative magnitude either side of the decision at least 1e-5 of the total from 85 %
             (the device's float64 running sum differs from the float64 evaluation's by ~1e-15)
  FUNDPOWER  fund_power at least 10 % from 1e-10
  ROOT       every non-real root has |imag| >= 1e-4 (the kernel's real-root rule: 1e-8 max(1, |z|)); every
             accepted formant at least 1 Hz from 50 Hz and from Nyquist; no other root's frequency within
             1 Hz of either bound
  and the float64 evaluation (tests/harmonic_ref.py, f64=True) takes the same integer decisions.

`dev`: the reference's largest deviation from the float64 evaluation over all frames -- strengths, thd,
thd_plus_noise and flux relative, hnr_db absolute -- and `dev_formant`, the largest relative deviation
of a formant from the extended-precision evaluation.
"""
import json
import os
import sys
import time
import types
from types import SimpleNamespace

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import harmonic_ref as HR  # noqa: E402

STRENGTH, STRENGTH_TIE, TOL, ARGMIN, ARGMAX, ROLLOFF, FUNDPOWER, ROOT_IMAG, FORMANT_EDGE = (
    0.01, 1e-4, 1e-6, 1e-6, 1e-5, 1e-5, 0.1, 1e-4, 1.0)
KEYS = ("thd", "thd_plus_noise", "spectral_centroid", "spectral_spread", "spectral_flux", "spectral_rolloff",
        "inharmonicity", "hnr_db")
DEV = ("strength", "thd", "thd_plus_noise", "spectral_flux", "hnr_db")


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = types.ModuleType("pygame")
    pg.font = SimpleNamespace(Font=object)
    pg.Surface = object
    sys.modules.setdefault("pygame", pg)
    sys.path.insert(0, path)
    from omega4.panels.harmonic_analysis import HarmonicAnalyzer
    return HarmonicAnalyzer


def stack(fs, f0, n, seed, partials, noise=0.002, start=0):
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + start) / fs
    x = sum(a * np.sin(2 * np.pi * f0 * (k + 1) * t + 0.4 * k) for k, a in enumerate(partials))
    return x / np.max(np.abs(x)) + noise * rng.standard_normal(n)


SAW = [1.0 / k for k in range(1, 20)]


def audio_frame(x, m):
    """The app's frame: Hann-windowed float64 whose values are float32 numbers (the fixture stores float32)."""
    return (x[:m] * np.hanning(m)).astype(np.float32).astype(np.float64)


def rfft_spec(x, n):
    s = np.abs(np.fft.rfft(x[:n] * np.hanning(n)))
    return (s / s.max()).astype(np.float32)


def app_spec(x):
    """A 512-bin spectrum like the app's combined one: normalised, compressed and clamped at 1."""
    s = np.abs(np.fft.rfft(x[:1022] * np.hanning(1022)))
    return np.minimum(1.6 * (s / s.max()) ** 0.7, 1.0).astype(np.float32)


def bumps(K, at, seed, floor=0.01):
    """A synthetic spectrum: noise floor plus triangular bumps (bin, height, flat-top width)."""
    rng = np.random.default_rng(seed)
    s = floor * (0.5 + rng.random(K))
    for b, h, flat in at:
        for d in range(-3, 4 + flat - 1):
            k = b + d
            e = 0 if 0 <= d < flat else (-d if d < 0 else d - flat + 1)
            s[k] = max(s[k], h * (1 - 0.27 * e))
    return s.astype(np.float32)


class Recorder:
    def __init__(self, Ref):
        self.Ref = Ref
        self.d = {}
        self.dev = dict.fromkeys(DEV, 0.0)
        self.dev_formant = 0.0
        self.count = 0
        self.ties = set()

    def frame(self, name, i, an, spec, freqs, audio, fs, prev, want_series=True):
        """One reference call on analyzer `an`, checked against the restatement and the conditions, recorded."""
        spec = np.asarray(spec, np.float32)
        freqs = np.asarray(freqs, np.float64)
        r = an.detect_harmonic_series(spec, freqs, audio)
        HR.CHECKS = []
        e = HR.analyze(spec, freqs, audio, fs, prev)
        checks, HR.CHECKS = HR.CHECKS, None
        e64 = HR.analyze(spec, freqs, audio, fs, prev, f64=True)
        tag = f"{name}[{i}]"
        # the restatement takes the reference's decisions and values
        hs = r["harmonic_series"]
        assert len(hs) == e["series_count"] == e64["series_count"], tag
        assert bool(hs) == want_series, (tag, len(hs))
        for s, pk, bins, st in zip(hs, e["series_peak"], e["series_bins"], e["series_strength"]):
            assert s["fundamental"] == freqs[pk] and [h["number"] for h in s["harmonics"]] == [n + 1 for n in range(16) if bins[n] >= 0], tag
            assert [h["actual_freq"] for h in s["harmonics"]] == [freqs[b] for b in bins if b >= 0], tag
            assert float(s["strength"]) == st, (tag, s["strength"], st)
        for k in KEYS:
            assert float(r[k]) == e[k], (tag, k, r[k], e[k])
        assert [float(v) for v in r["formants"]] == list(e["formants"]), (tag, r["formants"], e["formants"])
        assert (e64["peaks"] == e["peaks"]).all() and (e64["series_peak"] == e["series_peak"]).all(), tag
        assert (e64["series_bins"] == e["series_bins"]).all() and e64["rolloff_idx"] == e["rolloff_idx"], tag
        # the conditions
        for pk, s in e["candidates"]:
            assert abs(float(s) - 0.3) >= STRENGTH, (tag, pk, s)
        st = np.sort(e["series_strength"])
        assert len(st) < 2 or np.min(np.diff(st)) >= STRENGTH_TIE, (tag, st)
        for kind, margin in checks:
            lim = {"argmin": ARGMIN, "tol5": TOL, "tol10": TOL, "argmax": ARGMAX, "fund_power": FUNDPOWER}[kind]
            if kind == "argmin" and margin == 0.0:
                self.ties.add(tag)
                continue
            assert margin >= lim, (tag, kind, margin)
        hp = e["peaks"]  # equal heights among the peaks the distance rule weighs against each other
        for a, b in zip(hp[:-1], hp[1:]):
            assert b - a >= 10, tag
        if hs:
            assert HR.rolloff_margin(spec) >= ROLLOFF, (tag, HR.rolloff_margin(spec))
        ext = []
        if e["roots"] is not None:
            ext, _ = HR.formants_ext(audio, fs)
            assert len(ext) == len(e["formants"]), (tag, ext, e["formants"])
            for z in e["roots"]:
                assert z.imag == 0 or abs(z.imag) >= ROOT_IMAG, (tag, z)
                if z.imag > 0:
                    fq = np.angle(z) * fs / (2 * np.pi)
                    assert abs(fq - 50) >= FORMANT_EDGE and abs(fq - fs / 2) >= FORMANT_EDGE, (tag, fq)
            for a, b in zip(e["formants"], ext):
                self.dev_formant = max(self.dev_formant, abs(a - b) / b)
        # the reference's deviation from the float64 evaluation
        for a, b in zip(e["series_strength"], e64["series_strength"]):
            self.dev["strength"] = max(self.dev["strength"], abs(a - b) / abs(b))
        for k in ("thd", "thd_plus_noise", "spectral_flux"):
            if e64[k] != 0:
                self.dev[k] = max(self.dev[k], abs(e[k] - e64[k]) / abs(e64[k]))
        self.dev["hnr_db"] = max(self.dev["hnr_db"], abs(e["hnr_db"] - e64["hnr_db"]))
        d, p = self.d, f"{name}/{i}/"
        d[p + "spec"] = spec
        if audio is not None:
            assert (audio.astype(np.float32) == audio).all()
            d[p + "audio"] = audio.astype(np.float32)
        d[p + "row"] = HR.row(e)
        d[p + "peaks"] = e["peaks"]
        d[p + "series_peak"] = e["series_peak"]
        d[p + "series_bins"] = e["series_bins"]
        d[p + "series_strength"] = e["series_strength"]
        d[p + "rolloff_idx"] = np.array(e["rolloff_idx"])
        d[p + "matches"] = np.array(json.dumps([[m["instrument"], float(m["confidence"]), m["match_count"]]
                                                for m in r["instrument_matches"]]))
        if e["roots"] is not None:
            d[p + "lags"] = e["lags"]
            d[p + "roots"] = e["roots"]
            d[p + "formants_ext"] = np.array(ext, np.float64)
        self.count += 1
        print(f"{tag:14s} series {len(hs)} f0 {e['dominant_fundamental']:8.2f} thd {e['thd']:7.3f} thd+n {e['thd_plus_noise']:7.3f} "
              f"hnr {e['hnr_db']:6.3f} flux {e['spectral_flux']:8.4f} formants {[round(v, 1) for v in e['formants']]}")
        return r, e

    def group(self, name, fs, freqs, frames, want_series=True):
        """frames: [(spec, audio or None)], each through a fresh analyzer (no previous spectrum)."""
        self.d[f"{name}/freqs"] = np.asarray(freqs, np.float64)
        self.d[f"{name}/fs"] = np.array(fs)
        self.d[f"{name}/n"] = np.array(len(frames))
        out = []
        for i, (spec, audio) in enumerate(frames):
            out.append(self.frame(name, i, self.Ref(fs), spec, freqs, audio, fs, None, want_series))
        return out


def main():
    Ref = import_reference(sys.argv[1])
    R = Recorder(Ref)
    d = R.d
    d["versions"] = np.array([np.__version__, scipy.__version__])
    fs = 48000
    fa = np.linspace(0, 24000, 512)
    df = fa[1]
    # (fundamentals on bins k where 0.95 k, 1.05 k and (n +- 0.1) k are no half-integers: no argmin tie)
    sigs = [stack(fs, fa[12], 8192, 1, SAW), stack(fs, fa[11], 8192, 2, SAW[:12]),
            stack(fs, fa[7], 8192, 3, [1, 0.8, 0.9, 0.5, 0.6, 0.3, 0.2, 0.1])]
    R.group("app", fs, fa, [(app_spec(x), audio_frame(x, 2048)) for x in sigs])
    tones = [stack(fs, 220.0, 8192, 4, SAW, 0.002), stack(fs, 110.0, 8192, 5, SAW, 0.002),
             stack(fs, 140.0, 8192, 6, [1, 0.7, 0.5, 0.6, 0.3, 0.2], 0.002)]
    R.group("k1025", fs, np.fft.rfftfreq(2048, 1 / fs), [(rfft_spec(x, 2048), audio_frame(x, 2048)) for x in tones])
    R.group("k4097", fs, np.fft.rfftfreq(8192, 1 / fs), [(rfft_spec(x, 8192), audio_frame(x, 2048)) for x in tones[:2]])
    R.group("m1024", fs, fa, [(app_spec(sigs[0]), audio_frame(sigs[0], 1024))])
    R.group("m4096", fs, fa, [(app_spec(sigs[2]), audio_frame(sigs[2], 4096))])
    x44 = stack(44100, 220.0, 4096, 7, SAW)
    R.group("fs44", 44100, np.fft.rfftfreq(2048, 1 / 44100), [(rfft_spec(x44, 2048), audio_frame(x44, 2048))])
    # a low-distortion tone on a bin centre: THD+N and HNR off their caps
    fp = np.fft.rfftfreq(2048, 1 / fs)
    pure = [stack(fs, fp[40], 4096, 8, [1, 0.02, 0.01], 0.0005), stack(fs, fp[24], 4096, 9, [1, 0.05, 0.02, 0.01], 0.001)]
    got = R.group("pure", fs, fp, [(rfft_spec(x, 2048), audio_frame(x, 2048)) for x in pure])
    assert any(e["thd_plus_noise"] < 100 and 0 < e["hnr_db"] < 60 for _, e in got), [(e["thd_plus_noise"], e["hnr_db"]) for _, e in got]
    # flat tops: two and three equal bins at the maximum and at an in-range peak
    plat = [bumps(512, [(12, 1.0, 2), (24, 0.7, 1), (36, 0.5, 3), (60, 0.3, 1), (200, 0.2, 1)], 10),
            bumps(512, [(20, 1.0, 3), (8, 0.6, 2), (40, 0.62, 1), (60, 0.4, 2)], 11)]
    got = R.group("plateau", fs, fa, [(s, audio_frame(sigs[0], 2048)) for s in plat])
    assert 12 in got[0][1]["peaks"] and 37 in got[0][1]["peaks"] and 21 in got[1][1]["peaks"] and 8 in got[1][1]["peaks"]
    # the distance rule: the in-range peak at bin 15 is removed by the higher one 6 bins on
    dist = bumps(512, [(15, 0.6, 1), (21, 1.0, 1), (42, 0.5, 1), (63, 0.4, 1)], 12)
    got = R.group("distance", fs, fa, [(dist, audio_frame(sigs[1], 2048))])
    assert 15 not in got[0][1]["peaks"] and 21 in got[0][1]["peaks"]
    # nothing in 20..2000 Hz reaches a tenth of the maximum: no series, every metric 0. (The recipe "noise
    # where no strength exceeds 0.3" cannot be met on a uniform table that starts at 0: every harmonic of a
    # bin frequency is a bin frequency, so it is accepted, and with two accepted harmonics the fundamental's
    # own term alone gives 1 / H_8 = 0.368. The strength filter is exercised by the `offset` group instead.)
    rng = np.random.default_rng(13)
    low = (0.02 * rng.random(512)).astype(np.float32)
    low[100:110] = np.float32(0.5) + 0.05 * np.arange(10, dtype=np.float32)
    got = R.group("noseries", fs, fa, [(low, audio_frame(sigs[0], 2048))], want_series=False)
    assert not HR.row(got[0][1]).any() and not got[0][1]["candidates"]
    # a table that is not a multiple grid (bin centres (i + 0.37) df up to a 1500 Hz Nyquist), where the
    # 5 % acceptance and the strength filter decide: bin 7 (21.6 Hz) has harmonics rejected between
    # accepted ones and more than eight accepted; bin 340 (997 Hz) has one harmonic below Nyquist, so fewer
    # than two accepted, strength 0, rejected, while the others are kept; frame 1 has in-range peaks only
    # above 750 Hz: candidates, but no series
    fo = (np.arange(512) + 0.37) * (1500.0 / 512)
    x3k = stack(3000, 120.0, 4096, 15, SAW[:8], 0.002)
    off = [bumps(512, [(7, 1.0, 1), (30, 0.8, 1), (340, 0.9, 1), (53, 0.5, 1), (120, 0.6, 1)], 16, floor=0.05),
           bumps(512, [(300, 1.0, 1), (400, 0.7, 1)], 17, floor=0.02)]
    got = R.group("offset", 3000, fo, [(off[0], audio_frame(x3k, 2048))])
    e = got[0][1]
    cand = dict(e["candidates"])
    assert cand[340] == 0.0 and 340 not in e["series_peak"] and len(e["series_peak"]) >= 2, (cand, e["series_peak"])
    b7 = e["series_bins"][list(e["series_peak"]).index(7)]
    acc = [n + 1 for n in range(16) if b7[n] >= 0]
    assert len(acc) > 8 and acc[:8] != list(range(1, 9)) and any(b7[n] < 0 for n in range(acc[-1])), acc
    d[f"offset/n"] = np.array(2)
    _, e = R.frame("offset", 1, Ref(3000), off[1], fo, audio_frame(x3k, 2048), 3000, None, want_series=False)
    assert len(e["candidates"]) == 2 and all(s == 0.0 for _, s in e["candidates"]) and not HR.row(e).any()
    R.group("silent", fs, fa, [(np.zeros(512, np.float32), np.zeros(2048))], want_series=False)
    # a negative real root of the LPC polynomial (the 220 Hz sawtooth frame)
    t = np.arange(2048) / fs
    saw = 2 * ((t * 220.0) % 1) - 1 + 0.002 * np.random.default_rng(2).standard_normal(2048)
    got = R.group("realroot", fs, np.fft.rfftfreq(2048, 1 / fs), [(rfft_spec(saw, 2048), audio_frame(saw, 2048))])
    roots = got[0][1]["roots"]
    assert any(z.imag == 0 and z.real < 0 for z in roots), roots
    # the sequence: 12 frames at hop 512 through one analyzer (frames 4 and 5 without a series)
    s = stack(fs, 200.0, 2048 + 11 * 512, 14, SAW[:10], 0.003)
    s = s * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * np.arange(len(s)) / fs))
    an, prev = Ref(fs), None
    d["seq/freqs"], d["seq/fs"], d["seq/n"] = fp, np.array(fs), np.array(12)
    flux = []
    for f in range(12):
        x = s[f * 512:f * 512 + 2048]
        spec = low[:1025].copy() if f in (4, 5) else rfft_spec(x, 2048)
        if f in (4, 5):
            spec = np.concatenate([low, low, low[:1]])[:1025] * np.float32(1 + 0.1 * f)
        _, e = R.frame("seq", f, an, spec, fp, audio_frame(x, 2048), fs, prev, want_series=f not in (4, 5))
        prev = spec
        flux.append(e["spectral_flux"])
    assert flux[0] == 0 and flux[4] == 0 and min(flux[1:4] + flux[6:]) > 0, flux
    d["seq/centroid_history"] = np.array(list(an.spectral_centroid_history), np.float64)
    d["seq/thd_history"] = np.array([float(v) for v in an.thd_history], np.float64)

    assert all(v > 0 for v in R.dev.values()) and R.dev_formant > 0, (R.dev, R.dev_formant)
    d["dev"] = np.array([R.dev[k] for k in DEV], np.float64)
    d["dev_names"] = np.array(DEV)
    d["argmin_ties"] = np.array(sorted(R.ties))
    print("frames with an exact argmin tie:", sorted(R.ties))
    d["dev_formant"] = np.array(R.dev_formant)
    print("reference deviation from the float64 evaluation:", R.dev, "formants from extended precision:", R.dev_formant)

    an = Ref(fs)
    prof = {k: {kk: (list(vv) if isinstance(vv, (tuple, list)) else vv) for kk, vv in v.items()}
            for k, v in an.instrument_profiles.items()}
    d["instrument_profiles"] = np.array(json.dumps(prof))
    v = an.metrics.detect_vowel_from_formants([700.0, 1100.0, 2500.0])
    d["vowel"] = np.array(json.dumps([[700.0, 1100.0, 2500.0], v[0], float(v[1])]))
    d["tables"] = np.array(json.dumps({"formant_ranges": {k: {kk: list(vv) for kk, vv in t.items()} for k, t in an.metrics.formant_ranges.items()},
                                       "vowel_formants": an.metrics.vowel_formants}))

    # the reference's time per call on one core (DESIGN: beside tools/kernel_bench.py harmonic)
    spec, audio = app_spec(sigs[0]), audio_frame(sigs[0], 2048)
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        an.detect_harmonic_series(spec, fa, audio)
        ts.append(time.perf_counter() - t0)
    d["ref_ms_per_call"] = np.array(float(np.median(ts)) * 1e3)
    print(f"reference: {np.median(ts) * 1e3:.2f} ms per call (median of 20); {R.count} frames recorded")
    out = os.path.join(HERE, "harmonic.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
