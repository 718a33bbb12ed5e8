"""A restatement of HipHopDetector.analyze's array work (omega4/panels/hip_hop_detector.py:94-384) for the
tests: the same numpy and scipy operations in the same order, so that it reproduces the reference's
features bit for bit (numpy >= 2 promotion: float32 magnitudes stay float32 against Python scalars), and
returns the intermediate values the device publishes (filtered RMS values, float32 power sums, envelope
threshold, kept peaks, branches). tests/test_hiphop.py pins it to tests/golden/hiphop.npz on the CPU.
`butter4_bandpass_sos` is scipy's butter(4, [lo, hi], 'bandpass', output='sos') written out step by step
(the cross-check of the library's C++ design); `sosfilt_seq` is the sequential DF2T cascade in any float
type (the library's sections are run through it on the CPU, and np.longdouble gives the yardstick the
generator records scipy's own deviation against).
"""
import numpy as np
from scipy import signal as scipy_signal

COLUMNS = ("rms", "sub_bass_presence", "kick_peak_count", "kick_pattern_factor", "hihat_zero_crossings",
           "hihat_density", "spectral_tilt", "vocal_peak_count", "vocal_presence", "flags", "sub_bass_rms",
           "hihat_rms", "envelope_threshold", "sub_bass_power", "bass_power", "total_power", "low_energy",
           "mid_energy", "high_energy", "vocal_energy", "core_vocal_energy", "total_energy", "tilt_branch",
           "vocal_branch")
# exact on the device: the integer decisions and the float32-path values
EXACT = ("rms", "kick_peak_count", "hihat_zero_crossings", "spectral_tilt", "vocal_peak_count", "vocal_presence",
         "flags", "sub_bass_power", "bass_power", "total_power", "low_energy", "mid_energy", "high_energy",
         "vocal_energy", "core_vocal_energy", "total_energy", "tilt_branch", "vocal_branch")
# float64 columns that pass through the filters: 1e-9 relative
FILTERED = ("sub_bass_presence", "kick_pattern_factor", "hihat_density", "sub_bass_rms", "hihat_rms",
            "envelope_threshold")
N_PEAKS = 16
FLAG_SILENT, FLAG_NONFINITE = 1, 2
MIN_RATE, MIN_BINS, MAX_BINS = 8000, 16, 8193
BANDS = ("sub_bass", "kick", "hihat")


def band_edges(fs):
    """The reference's filter bank (:70-92, without the unused bass filter)."""
    return {"sub_bass": (20, 60), "kick": (40, 100), "hihat": (3000, min(10000, fs / 2 * 0.9))}


def scipy_sos(fs):
    return {k: scipy_signal.butter(4, list(e), btype="bandpass", fs=fs, output="sos") for k, e in band_edges(fs).items()}


def butter4_bandpass_sos(lo, hi, fs):
    """scipy.signal.butter(4, [lo, hi], 'bandpass', fs=fs, output='sos') in closed steps: buttap, lp2bp_zpk,
    bilinear_zpk at scipy's internal rate 2 with prewarped edges, zpk2sos(pairing='nearest')."""
    w = 4.0 * np.tan(np.pi * (2.0 * np.array([lo, hi], float) / fs) / 2.0)
    bw, wo = w[1] - w[0], np.sqrt(w[0] * w[1])
    lp = -np.exp(1j * np.pi * np.arange(-3, 4, 2) / 8.0) * bw / 2
    r = np.sqrt(lp ** 2 - wo ** 2)
    p = np.concatenate((lp + r, lp - r))
    gain = bw ** 4 * np.real(256.0 / np.prod(4.0 - p))
    pz = [z for z in (4.0 + p) / (4.0 - p) if z.imag > 0]
    zeros = {-1.0: 4, 1.0: 4}
    sos = np.zeros((4, 6))
    for si in range(4):
        i = int(np.argmin([abs(1 - abs(z)) for z in pz]))
        p1 = pz.pop(i)
        zz = []
        for _ in range(2):
            minus = zeros[-1.0] > 0 and (zeros[1.0] == 0 or abs(p1 + 1) <= abs(p1 - 1))
            z = -1.0 if minus else 1.0
            zeros[z] -= 1
            zz.append(z)
        sos[3 - si] = [1.0, -(zz[0] + zz[1]), zz[0] * zz[1], 1.0, -2 * p1.real, p1.real ** 2 + p1.imag ** 2]
    sos[0, :3] *= gain
    return sos


def sosfilt_seq(sos, x, dtype=np.float64):
    """Sequential DF2T cascade from the zero state (what scipy's sosfilt computes) in `dtype`."""
    y = np.asarray(x).astype(dtype)
    for sec in np.asarray(sos):
        b0, b1, b2, _, a1, a2 = (dtype(v) for v in sec)
        z0 = z1 = dtype(0)
        out = np.empty_like(y)
        for i, u in enumerate(y):
            v = b0 * u + z0
            z0 = b1 * u + z1 - a1 * v
            z1 = b2 * u - a2 * v
            out[i] = v
        y = out
    return y


def band_ranges(freqs, fs):
    """The reference's masks as (first bin, count) over the increasing table, in the kernel's order."""
    f = np.asarray(freqs, np.float64)
    masks = [(f >= 20) & (f <= 60), (f >= 60) & (f <= 250), f < fs / 2, (f >= 20) & (f <= 500),
             (f >= 500) & (f <= 2000), (f >= 2000) & (f <= 8000), (f >= 200) & (f <= 3000), (f >= 300) & (f <= 2000),
             np.ones(len(f), bool)]
    out = []
    for m in masks:
        idx = np.nonzero(m)[0]
        assert len(idx) == 0 or (np.diff(idx) == 1).all()
        out.append((int(idx[0]) if len(idx) else 0, len(idx)))
    return out


def spectrum_side(spec, freqs, fs, select=None):
    """select: None for scipy's own distance rule, or select(x, candidates, distance) -> the kept peaks (the
    rule of tools/model/peaks_model.py, for spectra with equal heights where scipy has no rule of its own)."""
    fft_data = np.asarray(spec, np.float32)
    freqs = np.asarray(freqs, np.float64)
    e = {}

    def power(mask):
        return np.sum(np.abs(fft_data[mask]) ** 2)
    sub_mask, bass_mask, total_mask = (freqs >= 20) & (freqs <= 60), (freqs >= 60) & (freqs <= 250), freqs < fs / 2
    e["sub_bass_power"], e["bass_power"], e["total_power"] = power(sub_mask), power(bass_mask), power(total_mask)
    # _detect_sub_bass' frequency-domain part (:177-205)
    fdr, sbr = 0.0, 0.0
    if np.any(sub_mask) and e["total_power"] > 0:
        fdr = e["sub_bass_power"] / e["total_power"]
        sbr = e["sub_bass_power"] / (e["bass_power"] + 1e-10)
    e["freq_domain_ratio"], e["sub_to_bass_ratio"] = fdr, sbr
    # _analyze_spectral_tilt (:293-330)
    low_mask, mid_mask, high_mask = (freqs >= 20) & (freqs <= 500), (freqs >= 500) & (freqs <= 2000), \
        (freqs >= 2000) & (freqs <= 8000)
    low, mid, high = power(low_mask), power(mid_mask), power(high_mask)
    e["low_energy"], e["mid_energy"], e["high_energy"] = low, mid, high
    e["spectral_tilt"], e["tilt_branch"], e["low_ratio"] = 0.0, 0, None
    if np.any(low_mask) and np.any(mid_mask) and np.any(high_mask):
        total = low + mid + high
        if not total == 0:
            low_ratio, high_ratio = low / total, high / total
            tilt = (low_ratio - high_ratio + 1.0) / 2.0
            e["tilt_branch"], e["low_ratio"] = 1, float(low_ratio)
            if low_ratio > 0.5:
                e["tilt_branch"] = 3 if 1.0 < tilt * 1.2 else 2
                tilt = min(tilt * 1.2, 1.0)
            e["spectral_tilt"] = tilt
    # _detect_rap_vocals (:332-384)
    vocal_mask, core_mask = (freqs >= 200) & (freqs <= 3000), (freqs >= 300) & (freqs <= 2000)
    ve, ce, te = power(vocal_mask), power(core_mask), np.sum(np.abs(fft_data) ** 2)
    e["vocal_energy"], e["core_vocal_energy"], e["total_energy"] = ve, ce, te
    e["vocal_presence"], e["vocal_branch"], e["vocal_peak_count"] = 0.0, 0, 0
    e["vocal_peaks"], e["vocal_distance_peaks"], e["vocal_bins"] = np.zeros(0, int), np.zeros(0, int), int(vocal_mask.sum())
    if np.any(vocal_mask) and not (te == 0 or ve == 0):
        vm = np.abs(fft_data[vocal_mask])
        if len(vm) > 10:
            peaks, _ = scipy_signal.find_peaks(vm, prominence=np.max(vm) * 0.3, distance=20)
            if select is not None:  # find_peaks' order: the distance rule over all maxima, then the prominences
                kept = np.asarray(select(vm, list(scipy_signal.find_peaks(vm)[0]), 20), np.intp)
                peaks = kept[scipy_signal.peak_prominences(vm, kept)[0] >= np.max(vm) * 0.3]
            e["vocal_peaks"] = peaks
            e["vocal_distance_peaks"] = scipy_signal.find_peaks(vm, distance=20)[0]
            e["vocal_pmin"] = float(np.max(vm) * 0.3)
            presence = 0.4 * (ve / te) + 0.3 * (ce / ve) + 0.3 * (len(peaks) / len(vm))
            e["vocal_branch"] = 2 if 1.0 < presence * 2.5 else 1
            e["vocal_presence"] = min(presence * 2.5, 1.0)
            e["vocal_peak_count"] = len(peaks)
    return e


def audio_side(audio, sos, fs):
    """`audio` float32 or float64; `sos` the three cascades by name."""
    x = np.asarray(audio)
    e = {"rms": np.sqrt(np.mean(x ** 2))}
    total = e["rms"]
    sub = scipy_signal.sosfilt(sos["sub_bass"], x)
    e["sub_bass_rms"] = np.sqrt(np.mean(sub ** 2))
    e["time_domain_ratio"] = e["sub_bass_rms"] / total
    # _analyze_kick_pattern (:224-253), without the caller's kick magnitude
    kick = scipy_signal.sosfilt(sos["kick"], x)
    env = np.abs(scipy_signal.hilbert(kick))
    thr = np.mean(env) + 1.5 * np.std(env)
    peaks = scipy_signal.find_peaks(env, height=thr, distance=int(0.1 * fs))[0]
    e["envelope"], e["envelope_threshold"], e["kick_peaks"] = env, thr, peaks
    e["kick_peak_count"] = len(peaks)
    e["syncopation"] = 0.0
    if len(peaks) > 1:
        spacings = np.diff(peaks)
        reg = 1.0 - (np.std(spacings) / (np.mean(spacings) + 1e-10))
        reg = max(0, min(reg, 1))
        expected = np.median(spacings)
        sync = np.sum(np.abs(spacings - expected) > expected * 0.2) / len(spacings)
        e["kick_pattern_factor"], e["syncopation"] = 0.6 * reg + 0.4 * (1 - sync), float(sync)
    else:
        e["kick_pattern_factor"] = 0.5
    # _analyze_hihat_density (:261-291)
    hat = scipy_signal.sosfilt(sos["hihat"], x)
    e["hihat"] = hat
    e["hihat_zero_crossings"] = len(np.where(np.diff(np.sign(hat)))[0])
    zcr = e["hihat_zero_crossings"] / len(hat)
    e["hihat_rms"] = np.sqrt(np.mean(hat ** 2))
    e["hihat_density"] = min(zcr * 10, 1.0) * min(e["hihat_rms"] / total * 5, 1.0)
    return e


def features(spec, freqs, audio, fs, sos=None):
    """Everything the device row holds, plus the intermediates, for one frame."""
    spec, audio = np.asarray(spec), np.asarray(audio)
    e = dict.fromkeys(COLUMNS, 0.0)
    e["kick_peaks"] = np.zeros(0, int)
    if not (np.isfinite(spec).all() and np.isfinite(audio).all()):
        e["flags"] = FLAG_NONFINITE
        return e
    e["rms"] = np.sqrt(np.mean(audio ** 2))
    if e["rms"] < 0.001:
        e["flags"] = FLAG_SILENT
        return e
    e.update(spectrum_side(spec, freqs, fs))
    e.update(audio_side(audio, sos or scipy_sos(fs), fs))
    presence = (0.3 * e["time_domain_ratio"] + 0.5 * e["freq_domain_ratio"] + 0.2 * min(e["sub_to_bass_ratio"], 1.0))
    e["sub_bass_presence"] = min(presence * 3.0, 1.0)
    e["flags"] = 0
    return e


def row(e):
    return np.array([float(e[k]) for k in COLUMNS], np.float64)


def peaks_row(e):
    out = np.full(N_PEAKS, -1, np.int32)
    out[:len(e["kick_peaks"])] = e["kick_peaks"]
    return out


def reference_features(e, drum_info):
    """The reference's `features` dict from a restated frame and the caller's drum_info."""
    kick = drum_info.get("kick", {})
    detected, mag = kick.get("kick_detected", False), kick.get("magnitude", 0.0)
    return {"sub_bass_presence": e["sub_bass_presence"],
            "kick_pattern_score": min(e["kick_pattern_factor"] * mag, 1.0) if detected else 0.0,
            "hihat_density": e["hihat_density"], "spectral_tilt": e["spectral_tilt"],
            "vocal_presence": e["vocal_presence"], "tempo_match": 0.8 if detected else 0.3}
