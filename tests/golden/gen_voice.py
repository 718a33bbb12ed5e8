"""Makes tests/golden/voice.npz by calling the reference's VoiceDetectionPanel
(omega4/panels/voice_detection.py:11-192, :299-307) itself (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_voice.py <reference checkout>

The reference module is loaded by path with ``pygame`` stubbed (the module imports it at the top; nothing is
drawn). Its own detect_voice, detect_pitch and update are called with what the app passes: a float32 spectrum
and a float64 frame (a float32 frame times np.hanning). Written per group: fs, m, the float32 spectra and the
float32 frames before the window (`<g>/audio_sha`: sha256 of the float64 frames the reference saw), the rows in
tests/voice_ref.py's COLUMNS order, scipy's smoothed arrays, the kept peaks with their prominences (padded
with -1 / nan), the reference's results (active, confidence, formants, pitch), voice_start / voice_end, the
rfftfreq sha256 and `<g>/dev`; and the numpy and scipy versions. tests/voice_ref.py's row is asserted equal to
what the reference returns on every frame: the range decision, the formant list and the pitch bit for bit, the
confidence through the facade's host expression within CONF_BAR.

  app        48 kHz, m 2048, K 1025: synthetic vowels at f0 100, 140, 220, 300, 350 Hz (one per voice type),
             white noise, a pure 1 kHz tone
  k10        K 10, m 2048: at 48 kHz voice_end is 11, so the range check fails there as at K 11; a second frame
             at 96 kHz (voice_end 6) passes it and reaches the unsmoothed branch (count 0)
  k11        K 11: the failed range check (voice_end == 11)
  k12, k20   K 12 (window 7) and K 20 (the first window 11)
  m64        m 64, K 1025: 33 frequency bins, peaks at bin >= 33 are ignored; voice_start == voice_end; no pitch
  m1024      m 1024, K 513: no pitch
  m8192      m 8192, K 4097
  fs44, fs16, fs8   44100, 16000 (lags 40..200) and 8000 Hz (F4's range lies above Nyquist), m 2048
  plateau    exactly representable values: a flat-topped peak, peaks on the first and last interior bin; an audio
             frame whose autocorrelation has two equal maxima (the first wins)
  zero       an all-zero spectrum (with a vowel's audio); all-zero audio (with a vowel's spectrum)
  nonfinite  flags only: a NaN bin, an infinite sample
  weak       a vowel's spectrum over white-noise audio: active, but corr_peak < 0.3 corr0 keeps the old pitch
  seq        300 update() steps of ONE reference object over a pool of these 2048-sample frames (`seq/idx`),
             frozen over `seq/frozen`: the interval gate, all three deques wrapping, the stale state after a
             failed range check, the pitch carried across a weak frame. After every step: get_status() and the
             three history lengths

Margins, asserted here on every non-degenerate frame (conditions on the inputs, not measurements):
|confidence - 30| >= 1; every local maximum's prominence is at least 1e-3 relative away from the threshold;
for every local maximum whose prominence reaches half the threshold, every smoothed value outside its plateau
that its prominence walk compares with its height (up to the walk's stop on either side) differs from it by at
least 64 float32 ulps of the frame's maximum (its neighbours decide the maximum, the others where the walk
stops), `plateau` exempt; the best two lags differ by at least 1e-6 of
corr0 (`plateau` exempt: its tie is exact); |corr_peak - 0.3 corr0| >= 1e-3 corr0.
`<g>/dev`: the largest relative deviation of the reference's float32 sums from a float64 evaluation, as
[voice_energy, total_energy]. For the record; it is not the bar.
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import scipy
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "audio-analyzer-omega_amd"))
import voice_ref as VR  # noqa: E402

CONF_BAR = 5800 * 2.0 ** -24  # tests/test_voice.py derives it
VOICE_TYPES = ["Unknown", "Bass", "Baritone", "Tenor", "Alto", "Soprano"]


def import_reference(path):
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    spec = importlib.util.spec_from_file_location("ref_voice_detection",
                                                  os.path.join(path, "omega4", "panels", "voice_detection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VoiceDetectionPanel


def host_panel(fs):
    from omega_gpu.voice_detection import VoiceDetectionPanel
    p = VoiceDetectionPanel.__new__(VoiceDetectionPanel)
    p._host_init(fs)
    return p


def vowel(fs, m, f0, seed, centres=(650.0, 1500.0, 2700.0, 3700.0), width=130.0):
    """Harmonics of f0 under four equally strong formant bumps, a little noise: a float32 frame."""
    rng = np.random.default_rng(seed)
    t = np.arange(m) / fs
    x = np.zeros(m)
    top = min(5000.0, 0.45 * fs)
    for k in range(1, int(top / f0) + 1):
        f = k * f0
        a = 0.04 + sum(np.exp(-0.5 * ((f - c) / width) ** 2) for c in centres if c < 0.45 * fs)
        x += a * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    x = 0.1 * x / np.max(np.abs(x)) + 1e-4 * rng.standard_normal(m)
    return x.astype(np.float32)


def noise(m, seed, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(m)).astype(np.float32)


def tone(fs, m, f):
    return (0.2 * np.sin(2 * np.pi * f * np.arange(m) / fs)).astype(np.float32)


def windowed(frame):
    return frame.astype(np.float64) * np.hanning(len(frame))  # the app's audio_windowed


def spectrum_of(frame, K=None):
    s = np.abs(np.fft.rfft(windowed(frame))).astype(np.float32)
    return s if K is None else s[:K]


def check_margins(group, i, spec, audio, fs, row, conf):
    K, m = len(spec), len(audio)
    flags = int(row[0])
    if flags & (VR.FLAG_NONFINITE | VR.FLAG_RANGE):
        return
    exempt = group == "plateau"
    if not flags & VR.FLAG_NO_ENERGY:
        assert abs(float(conf) - 30) >= 1, (group, i, conf)
        sp = VR.smoothed_peaks(spec)
        if sp is not None:
            sm, _, _, thr = sp
            allp, _ = signal.find_peaks(sm)
            prom = signal.peak_prominences(sm, allp)[0]
            thr = float(thr)
            if thr > 0:
                assert np.all(np.abs(prom - thr) >= 1e-3 * thr), (group, i, prom, thr)
            if not exempt:
                gap = 64 * np.spacing(np.float32(np.max(sm)))
                for p, pr in zip(allp, prom):
                    if pr < thr / 2:
                        continue
                    d = np.abs(sm.astype(np.float64) - float(sm[p]))
                    lo = hi = p
                    while lo > 0 and sm[lo - 1] == sm[p]:
                        lo -= 1
                    while hi < K - 1 and sm[hi + 1] == sm[p]:
                        hi += 1
                    d[lo:hi + 1] = np.inf
                    # the values the prominence walk compares with the height: up to its stop on either side
                    a, b = lo, hi
                    while a > 0 and sm[a] <= sm[p]:
                        a -= 1
                    while b < K - 1 and sm[b] <= sm[p]:
                        b += 1
                    assert d[a:b + 1].min() >= gap, (group, i, int(p), d[a:b + 1].min(), gap)
    if not flags & VR.FLAG_NO_PITCH and row[14] > 0:
        x = np.asarray(audio, np.float64)
        c = np.correlate(x, x, "full")[m - 1:]
        sl = np.sort(c[int(fs / 400):int(fs / 80)])
        if not exempt:
            assert sl[-1] - sl[-2] >= 1e-6 * c[0], (group, i, (sl[-1] - sl[-2]) / c[0])
        assert abs(row[16] - 0.3 * row[14]) >= 1e-3 * row[14], (group, i)


def record(Ref, out, group, fs, frames, spectra, audio=None):
    """frames: float32 [F, m] before the window (audio: the float64 frames, by default frames * hanning)."""
    frames = np.asarray(frames, np.float32)
    spectra = np.asarray(spectra, np.float32)
    F, m = frames.shape
    K = spectra.shape[1]
    if audio is None:
        audio = np.stack([windowed(f) for f in frames])
    rows = np.zeros((F, len(VR.COLUMNS)))
    smoothed = np.zeros((F, K), np.float32)
    kept = [VR.smoothed_peaks(s_) if np.all(np.isfinite(s_)) else None for s_ in spectra]
    P = max([1] + [len(k_[1]) for k_ in kept if k_ is not None])
    peaks = np.full((F, P), -1, np.int32)
    proms = np.full((F, P), np.nan)
    r_active = np.zeros(F, np.int8)
    r_conf = np.zeros(F)
    r_form = np.full((F, 4), np.nan)
    r_pitch = np.zeros(F)
    dev = np.zeros(2)
    fb = np.fft.rfftfreq(m, 1 / fs)
    host = host_panel(fs)
    for i in range(F):
        spec, x = spectra[i], audio[i]
        finite = bool(np.all(np.isfinite(spec)) and np.all(np.isfinite(x)))
        rows[i] = row = VR.row(spec, x, fs)
        sp = VR.smoothed_peaks(spec) if finite else None
        if sp is not None:
            smoothed[i] = sp[0]
            peaks[i, :len(sp[1])] = sp[1]
            proms[i, :len(sp[1])] = sp[2]
        if not finite:
            assert int(row[0]) == VR.FLAG_NONFINITE
            continue
        ref = Ref(fs)
        with np.errstate(all="ignore"):
            active, conf = ref.detect_voice(x, spec)
        ref2 = Ref(fs)
        ref2.detect_pitch(x)
        r_active[i], r_conf[i], r_pitch[i] = bool(active), float(conf), float(ref2.voice_pitch)
        r_form[i, :len(ref.formants)] = ref.formants
        # the row against the reference
        res = host.result_from_row(row, K)
        vs, ve = VR.bin_range(fs, m)
        assert res["range_ok"] == (vs < K and ve < K)
        if res["range_ok"]:
            assert bool(res["active"]) == bool(active), (group, i)
            assert abs(float(res["confidence"]) - float(conf)) <= CONF_BAR, (group, i, res["confidence"], conf)
            assert type(res["confidence"]) is type(conf), (group, i, type(res["confidence"]), type(conf))
            got = res["formants"] if res["formants"] is not None else []
            assert len(got) == len(ref.formants) and all(a == b for a, b in zip(got, ref.formants)), (group, i)
            if row[4] > 0:
                e = [float(np.sum(spec[vs:ve])), float(np.sum(spec))]
                for j in range(2):
                    if row[3 + j] > 0:
                        dev[j] = max(dev[j], abs(e[j] - row[3 + j]) / row[3 + j])
        else:
            assert not active and conf == 0.0
        if res["pitch"] is None:
            assert ref2.voice_pitch == 0.0, (group, i)
        else:
            assert res["pitch"] == ref2.voice_pitch and type(res["pitch"]) is type(ref2.voice_pitch), (group, i)
        check_margins(group, i, spec, x, fs, row, conf)
    out[f"{group}/fs"] = np.int64(fs)
    out[f"{group}/m"] = np.int64(m)
    out[f"{group}/spec"] = spectra
    out[f"{group}/frame"] = frames
    out[f"{group}/audio_sha"] = np.array(hashlib.sha256(np.ascontiguousarray(audio).tobytes()).hexdigest())
    out[f"{group}/row"] = rows
    out[f"{group}/smoothed"] = smoothed
    out[f"{group}/peaks"] = peaks
    out[f"{group}/prom"] = proms
    out[f"{group}/ref_active"] = r_active
    out[f"{group}/ref_conf"] = r_conf
    out[f"{group}/ref_formants"] = r_form
    out[f"{group}/ref_pitch"] = r_pitch
    out[f"{group}/range"] = np.array(VR.bin_range(fs, m), np.int32)
    out[f"{group}/rfftfreq_sha"] = np.array(hashlib.sha256(fb.tobytes()).hexdigest())
    out[f"{group}/dev"] = dev
    return rows, r_active, r_conf, r_pitch


def small_spectrum(K, bumps):
    """A K-bin spectrum of Gaussian bumps (centre, height, width) on a sloping floor."""
    k = np.arange(K, dtype=np.float64)
    s = 0.2 + 0.01 * k
    for c, h, w in bumps:
        s = s + h * np.exp(-0.5 * ((k - c) / w) ** 2)
    return s.astype(np.float32)


def main(ref_path):
    Ref = import_reference(ref_path)
    out = {}
    fs = 48000
    f0s = (100.0, 140.0, 220.0, 300.0, 350.0)
    vow = [vowel(fs, 2048, f0, 10 + i) for i, f0 in enumerate(f0s)]
    app = vow + [noise(2048, 3), tone(fs, 2048, 1000.0)]
    rows, act, conf, pit = record(Ref, out, "app", fs, app, [spectrum_of(f) for f in app])
    types_ = []
    for i in range(5):
        ref = Ref(fs)
        ref.voice_pitch = pit[i]
        ref.analyze_voice_type()
        types_.append(ref.voice_type)
    assert types_ == VOICE_TYPES[1:], types_
    assert all(act[:5]) and not act[6], (act, conf)  # (white noise shows four 'formants' too)
    print("app confidences", conf, "pitch", pit)

    v = vow[2]
    record(Ref, out, "k10", fs, [v], [spectrum_of(v, 10)])
    record(Ref, out, "k10b", 96000, [v], [small_spectrum(10, [(4, 1.0, 1.0)])])
    r = record(Ref, out, "k11", fs, [v], [small_spectrum(11, [(5, 1.0, 1.0)])])[0]
    assert int(r[0, 0]) & VR.FLAG_RANGE and r[0, 2] == 11
    assert int(out["k10/row"][0, 0]) & VR.FLAG_RANGE and not int(out["k10b/row"][0, 0]) & VR.FLAG_RANGE
    r = record(Ref, out, "k12", fs, [v, v], [small_spectrum(12, [(9, 1.0, 0.9)]), small_spectrum(12, [(3, 1.0, 1.2), (10, 0.8, 0.6)])])[0]
    assert r[0, 5] == 1 and r[0, 6] == 9, r[:, :7]
    r = record(Ref, out, "k20", fs, [v, v], [small_spectrum(20, [(10, 1.0, 1.5)]), small_spectrum(20, [(4, 1.0, 1.0), (15, 0.9, 1.4)])])[0]
    assert r[0, 5] == 1 and r[1, 5] == 1, r[:, :7]

    # m 64: 33 frequency bins of 750 Hz; a spectrum of 1025 bins with peaks below and above bin 33
    k = np.arange(1025, dtype=np.float64)
    s64 = (0.05 + np.exp(-0.5 * ((k - 4) / 2.5) ** 2) + 0.9 * np.exp(-0.5 * ((k - 40) / 3.0) ** 2)
           + 0.8 * np.exp(-0.5 * ((k - 500) / 3.0) ** 2)).astype(np.float32)
    r = record(Ref, out, "m64", fs, [vowel(fs, 64, 750.0, 5)], [s64])[0]
    assert r[0, 1] == r[0, 2] == 1 and r[0, 3] == 0 and int(r[0, 0]) & VR.FLAG_NO_PITCH and r[0, 5] >= 1, r
    assert np.any(out["m64/peaks"][0] >= 33), out["m64/peaks"]
    print("m64 row", r[0, 5:14])
    f = vowel(fs, 1024, 220.0, 6)
    r = record(Ref, out, "m1024", fs, [f], [spectrum_of(f)])[0]
    assert int(r[0, 0]) & VR.FLAG_NO_PITCH
    for seed in range(7, 40):  # the first seed whose frame keeps the margins
        f = vowel(fs, 8192, 140.0, seed)
        try:
            record(Ref, out, "m8192", fs, [f], [spectrum_of(f)])
        except AssertionError:
            continue
        print("m8192 seed", seed)
        break
    else:
        raise AssertionError("m8192: no seed keeps the margins")
    for name, rate in (("fs44", 44100), ("fs16", 16000), ("fs8", 8000)):
        f = vowel(rate, 2048, 180.0, 8)
        r = record(Ref, out, name, rate, [f], [spectrum_of(f)])[0]
        assert not int(r[0, 0]), (name, r)
    assert out["fs8/row"][0, 9] == 0 and out["fs8/row"][0, 5] >= 1

    # plateau: exactly representable values
    sp = np.full(64, 1.0, np.float32)
    sp[1] = 9.0                     # a peak on the first interior bin
    sp[30:33] = 8.0                 # a flat top
    sp[62] = 7.0                    # a peak on the last interior bin
    sp2 = np.full(1025, 2.0, np.float32)
    sp2[20:24] = 16.0               # an even plateau: (left + right) // 2
    sp2[60] = 12.0
    sp2[100:103] = 12.0
    au = np.zeros(2048)
    au[0], au[150], au[300] = 4.0, 2.0, 0.0   # c[150] = 8 alone
    au2 = np.zeros(2048)
    au2[[0, 200, 500]] = 2.0                   # c[200] = c[300] = c[500] = 4: the first wins
    spa = np.zeros((2, 1025), np.float32)
    spa[0, :64] = sp
    spa[1] = sp2
    r = record(Ref, out, "plateau", fs, np.stack([au, au2]).astype(np.float32), spa, audio=np.stack([au, au2]))[0]
    assert r[1, 15] == 200 and r[1, 16] == 4.0 and r[0, 15] == 150, r[:, 14:]

    z = np.zeros(1025, np.float32)
    r = record(Ref, out, "zero", fs, [v, np.zeros(2048, np.float32)], [z, spectrum_of(v)])[0]
    assert int(r[0, 0]) == VR.FLAG_NO_ENERGY and r[1, 14] == 0 and r[1, 15] == 120, r
    bad_s = spectrum_of(v).copy()
    bad_s[700] = np.nan
    bad_a = v.copy()
    bad_a[5] = np.inf
    r = record(Ref, out, "nonfinite", fs, [v, bad_a], [bad_s, spectrum_of(v)])[0]
    assert np.all(r[:, 0] == VR.FLAG_NONFINITE) and not np.any(r[:, 1:])
    nz = noise(2048, 21)
    r, a, c, p = record(Ref, out, "weak", fs, [nz], [spectrum_of(v)])
    assert a[0] and p[0] == 0.0

    # seq: one reference object over a pool of 2048-sample frames
    pool = [(vow[i], spectrum_of(vow[i])) for i in range(5)]
    pool += [(app[5], spectrum_of(app[5])), (app[6], spectrum_of(app[6])),   # 5 noise, 6 tone
             (v, out["k11/spec"][0]),                                        # 7 the failed range check
             (nz, spectrum_of(v)),                                           # 8 weak
             (v, z)]                                                         # 9 the all-zero spectrum
    rng = np.random.default_rng(99)
    idx = rng.integers(0, 5, 300)
    idx[[9, 10, 11]] = 6, 7, 7        # inactive, then the stale state after a failed range
    idx[[21, 23, 25]] = 8, 9, 6       # the pitch carried across a weak frame
    idx[41:49] = [0, 0, 6, 6, 7, 7, 8, 8]
    frozen = np.zeros(300, np.int8)
    frozen[60:66] = 1
    ref = Ref(fs)
    st = {k_: [] for k_ in ("active", "conf", "conf_int", "pitch", "type", "nform", "form", "lens")}
    for s in range(300):
        ref.is_frozen = bool(frozen[s])
        fr, spc = pool[idx[s]]
        ref.update(windowed(fr), spc)
        g = ref.get_status()
        assert list(g) == ["active", "confidence", "pitch", "voice_type", "formants"]
        st["active"].append(bool(g["active"]))
        st["conf"].append(float(g["confidence"]))
        st["conf_int"].append(isinstance(g["confidence"], int))
        st["pitch"].append(float(g["pitch"]))
        st["type"].append(VOICE_TYPES.index(g["voice_type"]))
        st["nform"].append(len(g["formants"]))
        st["form"].append(list(g["formants"]) + [np.nan] * (4 - len(g["formants"])))
        st["lens"].append([len(ref.voice_history), len(ref.formant_history), len(ref.pitch_history)])
    lens = np.array(st["lens"])
    assert lens[-1, 0] == 120 and lens[-1, 1] == 60 and lens[-1, 2] == 120, lens[-1]
    out["seq/idx"] = idx.astype(np.int32)
    out["seq/frozen"] = frozen
    out["seq/pool_group"] = np.array(["app"] * 7 + ["k11", "weak", "zero"])
    out["seq/pool_frame"] = np.array([0, 1, 2, 3, 4, 5, 6, 0, 0, 0], np.int32)
    out["seq/active"] = np.array(st["active"], np.int8)
    out["seq/confidence"] = np.array(st["conf"])
    out["seq/confidence_is_int"] = np.array(st["conf_int"], np.int8)
    out["seq/pitch"] = np.array(st["pitch"])
    out["seq/voice_type"] = np.array(st["type"], np.int8)
    out["seq/n_formants"] = np.array(st["nform"], np.int8)
    out["seq/formants"] = np.array(st["form"])
    out["seq/lens"] = lens.astype(np.int32)
    out["voice_types"] = np.array(VOICE_TYPES)
    out["versions"] = np.array([np.__version__, scipy.__version__])
    for m_ in (64, 1024, 2048, 8192):
        out[f"hanning_sha/{m_}"] = np.array(hashlib.sha256(np.hanning(m_).tobytes()).hexdigest())
    path = os.path.join(HERE, "voice.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
