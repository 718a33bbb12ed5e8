"""Makes tests/golden/pitch.npz by calling the reference's CepstralAnalyzer
(omega4/panels/pitch_detection.py:21-611) itself (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_pitch.py <reference checkout>

The reference is imported with ``pygame`` stubbed (the panel module imports it at the top; no drawing
code runs). Only inputs and the reference's outputs are written. Every frame is accepted only when the
conditions of tests/test_pitch.py hold for it (asserted here, on the CPU); a frame that misses one is
redrawn with the next noise seed, so no frame is ever dropped from a comparison:

  * every integer decision (cepstral period, autocorrelation period, YIN tau) is unchanged under four
    perturbations of the frame at float32 rounding size (relative 3e-7), and equals the float64
    evaluation's (tests/pitch_ref.py, f64=True);
  * the cents value is at least 0.05 away from an integer (int() truncation cannot flip);
  * the std/mean consistency ratio is at least 10 % away from 0.02 and 0.05;
  * each method confidence is at least 0.01 away from its acceptance threshold (0.15 / 0.2 / 0.25).

Recorded per frame: the three integers, the (pitch, confidence) pairs, pitch, confidence, octave,
cents, stability and the note; per group the configuration with its derived periods; `dev`: the
reference's largest deviation from the float64 evaluation of the float32 paths (autocorrelation
confidence and YIN confidence absolute, YIN pitch relative) over all frames.
"""
import json
import os
import sys
import time
import types
from types import SimpleNamespace

import numpy as np
import scipy
from scipy import signal as sps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pitch_ref as PR  # noqa: E402

CFG_FIELDS = ("sample_rate", "min_pitch", "max_pitch", "yin_threshold", "yin_window_size", "enable_preprocessing",
              "highpass_frequency", "highpass_order", "enable_compression", "compression_threshold",
              "compression_ratio")
THRESHOLDS = (0.15, 0.2, 0.25)
TONES = (55.0, 82.41, 110.0, 146.83, 220.0, 329.63, 440.0, 659.25, 880.0, 1318.5, 1900.0)


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = types.ModuleType("pygame")
    pg.font = SimpleNamespace(Font=object)
    pg.Surface = object
    sys.modules.setdefault("pygame", pg)
    sys.path.insert(0, path)
    from omega4.panels.pitch_detection import CepstralAnalyzer
    from omega4.panels.pitch_detection_config import PitchDetectionConfig, get_preset_config, list_presets
    return SimpleNamespace(**locals())


def tone(fs, f0, n, seed, win, nh=6, noise=0.01, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = sum((0.7 ** k) * np.sin(2 * np.pi * f0 * (k + 1) * t + 0.3 * k) for k in range(nh))
    x = amp * x / np.max(np.abs(x)) + noise * rng.standard_normal(n)
    if win:
        x = x * np.hanning(n)
    return x.astype(np.float32)


def ripple(fs, n, seed):
    """The distance-rule frame: a 1 kHz tone whose autocorrelation rises from lag 24 to its peak at lag
    48, with an 8 kHz component that puts lower local maxima (>= 0.3) on the way up."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = 0.3 * np.sin(2 * np.pi * 1000.0 * t) + 0.12 * np.sin(2 * np.pi * 8000.0 * t + 0.4)
    return (x + 0.005 * rng.standard_normal(n)).astype(np.float32)


def glide(fs, n, seed):
    """The sequence's stream: a harmonic tone gliding 215 -> 232 Hz."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    f = 215.0 + 17.0 * t / t[-1]
    ph = 2 * np.pi * np.cumsum(f) / fs
    x = sum((0.6 ** k) * np.sin((k + 1) * ph + 0.2 * k) for k in range(5))
    return (0.3 * x / np.max(np.abs(x)) + 0.01 * rng.standard_normal(n)).astype(np.float32)


def ref_call(an, x):
    """One detect_pitch_advanced_safe call -> (dict, [cepstral period, autocorrelation period, YIN tau])."""
    seen = []
    orig = type(an)._parabolic_interpolation

    def spy(y1, y2, y3, t):
        seen.append(int(t))
        return orig(an, y1, y2, y3, t)
    an._parabolic_interpolation = spy
    try:
        r = an.detect_pitch_advanced_safe(x)
    finally:
        del an._parabolic_interpolation
    m = r.get("methods") or {}
    dec = [0, 0, 0]
    if m:
        for i, k in enumerate(("cepstral", "autocorr")):
            if m[k][0] > 0:
                dec[i] = int(round(an.sample_rate / m[k][0]))
                assert an.sample_rate / dec[i] == m[k][0]
        if m["yin"][0] > 0:
            dec[2] = seen[-1]
    return r, dec


def conditions(R, cfg, x, r, dec):
    """None when the frame meets every condition, else the reason."""
    fs = cfg.sample_rate
    P = PR.Params.from_config(cfg)
    m = r["methods"]
    for s in range(4):
        xp = (x.astype(np.float64) * (1 + 3e-7 * np.random.default_rng(1000 + s).standard_normal(len(x)))).astype(np.float32)
        _, dp = ref_call(R.CepstralAnalyzer(fs, cfg), xp)
        if dp != dec:
            return f"decision moves under perturbation {dec} -> {dp}"
    e = PR.analyze(x, P, f64=True)
    if [e["cep_period"], e["ac_period"], e["yin_tau"]] != dec:
        return "float64 evaluation decides differently"
    for k, thr in zip(("cepstral", "autocorr", "yin"), THRESHOLDS):
        if abs(float(m[k][1]) - thr) < 0.01:
            return f"{k} confidence {m[k][1]} near {thr}"
    _, _, ratio = PR.combine((m["cepstral"], m["autocorr"], m["yin"]), P)
    if np.isfinite(ratio) and (abs(ratio - 0.02) < 0.002 or abs(ratio - 0.05) < 0.005):
        return f"consistency ratio {ratio}"
    if r["pitch"] > 0:
        c = PR.pitch_to_note(r["pitch"])[3]
        if abs(c - round(c)) < 0.05:
            return f"cents {c}"
    return None


class Group:
    def __init__(self, R, cfg):
        self.R, self.cfg = R, cfg
        self.x, self.dec, self.methods, self.out, self.note = [], [], [], [], []
        self.dev = np.zeros(3)

    def record(self, x, r, dec):
        m = r["methods"]
        self.x.append(x)
        self.dec.append(dec)
        self.methods.append([float(v) for k in ("cepstral", "autocorr", "yin") for v in m[k]])
        self.out.append([r["pitch"], r["confidence"], r["octave"], r["cents_offset"], r["stability"]])
        self.note.append(r["note"])
        e = PR.analyze(x, PR.Params.from_config(self.cfg), f64=True)
        if dec[1]:
            self.dev[0] = max(self.dev[0], abs(float(m["autocorr"][1]) - e["autocorr"][1]))
        if dec[2]:
            self.dev[1] = max(self.dev[1], abs(m["yin"][0] - e["yin"][0]) / e["yin"][0])
            self.dev[2] = max(self.dev[2], abs(m["yin"][1] - e["yin"][1]))

    def add(self, make, what):
        """make(seed) -> frame; the first seed whose frame meets the conditions is recorded."""
        for seed in range(64):
            x = make(seed)
            r, dec = ref_call(self.R.CepstralAnalyzer(self.cfg.sample_rate, self.cfg), x)
            assert r.get("error") is None and r["methods"], (what, r)
            why = conditions(self.R, self.cfg, x, r, dec)
            if why is None:
                self.record(x, r, dec)
                print(f"{what:28s} seed {seed} dec {dec} pitch {r['pitch']:.3f} conf {r['confidence']:.3f} {r['note']}{r['octave']}")
                return x, r, dec
            print(f"{what:28s} seed {seed} redrawn: {why}")
        raise AssertionError(f"no admissible frame for {what}")

    def save(self, d, name):
        an = self.R.CepstralAnalyzer(self.cfg.sample_rate, self.cfg)
        d[f"{name}/x"] = np.stack(self.x)
        d[f"{name}/dec"] = np.array(self.dec, np.int32)
        d[f"{name}/methods"] = np.array(self.methods, np.float64)
        d[f"{name}/out"] = np.array(self.out, np.float64)
        d[f"{name}/note"] = np.array(self.note)
        d[f"{name}/cfg"] = np.array([float(getattr(self.cfg, k)) for k in CFG_FIELDS] + [an.min_period, an.max_period],
                                    np.float64)


def main():
    R = import_reference(sys.argv[1])
    d = {"versions": np.array([np.__version__, scipy.__version__]), "cfg_fields": np.array(CFG_FIELDS)}
    bal = R.get_preset_config("balanced")
    groups = {}

    g = groups["tones"] = Group(R, bal)
    for f0 in TONES:
        for win in (True, False):
            g.add(lambda s, f0=f0, win=win: tone(48000, f0, 4096, s, win), f"tone {f0} win={win}")
    cases = {tuple(int(v > 0) for v in dd) for dd in g.dec}
    assert (1, 1, 0) in cases and (1, 1, 1) in cases, cases  # YIN without an estimate / all three
    g = groups["t2048"] = Group(R, bal)
    g.add(lambda s: tone(48000, 220.0, 2048, s, True), "220 Hz n=2048")
    g = groups["t8192"] = Group(R, bal)
    g.add(lambda s: tone(48000, 220.0, 8192, s, True), "220 Hz n=8192")

    g = groups["edges"] = Group(R, bal)
    taus, lags = [], []
    for f0 in (470.0, 480.5, 490.0, 1990.0, 51.0):
        _, _, dec = g.add(lambda s, f0=f0: tone(48000, f0, 4096, s, False), f"edge {f0}")
        taus.append(dec[2])
        lags.append(dec[1])
    assert taus[0] > 100 and taus[2] < 100 and 99 <= taus[1] <= 101, taus  # either side of the tau = 100 switch
    # period 24 = min_period: YIN's first admissible tau, and a lag the autocorrelation's find_peaks cannot
    # return (the slice's first element); period 941 near max_period (YIN has no estimate there)
    assert taus[3] == 24 and lags[3] == 48 and lags[4] >= 930, (taus, lags)

    g = groups["dist"] = Group(R, bal)
    x, r, dec = g.add(lambda s: ripple(48000, 4096, s), "distance rule")
    an = R.CepstralAnalyzer(48000, bal)
    v = an.compute_autocorrelation(x)[an.min_period:min(an.max_period, len(x) - 1)]
    raw, _ = sps.find_peaks(v, height=0.3)
    assert int(raw[0]) + an.min_period != dec[1], (raw[:4], dec)  # peaks[0] is not the first raw maximum
    d["dist/first_raw"] = np.array(int(raw[0]) + an.min_period)

    g = groups["fs44"] = Group(R, R.PitchDetectionConfig(sample_rate=44100))
    g.add(lambda s: tone(44100, 220.0, 4096, s, True), "44.1 kHz 220 Hz")
    g.add(lambda s: tone(44100, 659.25, 4096, s, False), "44.1 kHz 659.25 Hz")
    g = groups["music"] = Group(R, R.get_preset_config("music_optimized"))
    g.add(lambda s: tone(48000, 146.83, 4096, s, True), "music_optimized 146.83 Hz")
    g.add(lambda s: tone(48000, 3000.0, 4096, s, False, nh=2), "music_optimized 3000 Hz")
    g = groups["lowlat"] = Group(R, R.get_preset_config("low_latency"))
    g.add(lambda s: tone(48000, 329.63, 4096, s, True), "low_latency 329.63 Hz")
    g.add(lambda s: tone(48000, 110.0, 4096, s, False, amp=0.004, noise=0.0001), "low_latency quiet 110 Hz")

    # the noise frame: a valid frame on which autocorrelation and YIN give nothing
    g = groups["noise"] = Group(R, bal)
    _, r, dec = g.add(lambda s: (0.1 * np.random.default_rng(s).standard_normal(4096)).astype(np.float32), "white noise")
    assert dec[1] == 0 and dec[2] == 0, dec

    # invalid frames: the reference's dicts and error strings
    rng = np.random.default_rng(7)
    bad = {"silent": np.zeros(4096, np.float32), "nan": tone(48000, 220.0, 4096, 0, True),
           "short": tone(48000, 220.0, 1000, 0, False), "n3000": tone(48000, 220.0, 3000, 0, False)}
    bad["nan"][rng.integers(0, 4096)] = np.nan
    for name, x in bad.items():
        r = R.CepstralAnalyzer(48000, bal).detect_pitch_advanced_safe(x)
        d[f"bad/{name}/x"] = x
        if name == "n3000":  # (the reference analyses it; the device build reports the length as unsupported)
            continue
        assert r["pitch"] == 0.0 and r["confidence"] == 0.0 and r["note"] == "" and r["stability"] == 0.0
        d[f"bad/{name}/keys"] = np.array(sorted(r.keys()))
        d[f"bad/{name}/error"] = np.array(r.get("error") or "")

    # the sequence: one analyzer over 30 frames of a stream at hop 512
    for seed in range(64):
        s = glide(48000, 4096 + 29 * 512, seed)
        g = Group(R, bal)
        an = R.CepstralAnalyzer(48000, bal)
        why = None
        for f in range(30):
            x = s[f * 512:f * 512 + 4096]
            r, dec = ref_call(an, x)
            why = conditions(R, bal, x, r, dec)
            if why:
                break
            g.record(x, r, dec)
        if why is None:
            break
        print(f"sequence seed {seed} redrawn at frame {f}: {why}")
    assert why is None
    assert len({tuple(o[:1]) for o in g.out}) > 5 and any(o[4] > 0 for o in g.out)
    groups["seq"] = g
    g.save(d, "seq")
    d["seq/x"] = s  # the stream itself: frame f = s[f * 512 : f * 512 + 4096]
    d["seq/pitch_history"] = np.array(list(an.pitch_history), np.float64)
    d["seq/confidence_history"] = np.array(list(an.confidence_history), np.float64)
    print("sequence stability", [round(o[4], 4) for o in g.out])

    dev = np.zeros(3)
    for name, g in groups.items():
        if name != "seq":
            g.save(d, name)
        dev = np.maximum(dev, g.dev)
    assert (dev > 0).all()
    d["dev"] = dev
    print("reference deviation from the float64 evaluation (ac conf abs, yin pitch rel, yin conf abs):", dev)

    # configurations: the default at three sample rates and the five presets
    cfgs = {f"default_{sr}": R.PitchDetectionConfig(sample_rate=sr).to_dict() for sr in (44100, 48000, 96000)}
    for sr in (44100, 48000, 96000):
        a = R.CepstralAnalyzer(sr, R.PitchDetectionConfig(sample_rate=sr))
        cfgs[f"default_{sr}"].update(min_period=a.min_period, max_period=a.max_period)
    for name in R.list_presets():
        c = R.get_preset_config(name)
        a = R.CepstralAnalyzer(c.sample_rate, c)
        cfgs[f"preset_{name}"] = dict(c.to_dict(), min_period=a.min_period, max_period=a.max_period)
    d["configs"] = np.array(json.dumps(cfgs, sort_keys=True))
    d["presets"] = np.array(R.list_presets())

    # the reference's time per call on one core (DESIGN: beside tools/kernel_bench.py pitch)
    an = R.CepstralAnalyzer(48000, bal)
    x = groups["tones"].x[8]
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        an.detect_pitch_advanced_safe(x)
        ts.append(time.perf_counter() - t0)
    d["ref_ms_per_call"] = np.array(float(np.median(ts)) * 1e3)
    print(f"reference: {np.median(ts) * 1e3:.2f} ms per call (median of 20)")

    out = os.path.join(HERE, "pitch.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
