"""A restatement of GenreClassifier.extract_features' array work
(omega4/panels/genre_classification.py:256-422 and :600-783) for the tests: the same numpy operations in
the same order, so that with f64=False it reproduces the reference bit for bit (numpy's own promotion:
float32 magnitudes stay float32 against Python scalars), and with f64=True it evaluates the same formulas
from the same float32 inputs in float64 -- the yardstick the float32-path columns are measured against.
tests/test_genre.py pins it to tests/golden/genre.npz on the CPU. It also returns the intermediate
decisions the device publishes (rolloff index, crossing count, percentile ranks, peak bins).
"""
import numpy as np

COLUMNS = ("spectral_centroid", "spectral_rolloff", "rolloff_index", "zero_crossings", "spectral_bandwidth",
           "dynamic_range", "loud", "quiet", "rms", "spectral_complexity", "bass_emphasis", "vocal_presence",
           "high_freq_energy", "spectral_flux", "distortion_count", "mid_frequency_dominance", "flags")
# the columns whose reference arithmetic is float32: compared through the float64 evaluation
F32_PATH = ("rms", "spectral_complexity", "bass_emphasis", "vocal_presence", "high_freq_energy", "spectral_flux",
            "mid_frequency_dominance")
MIN_BINS, MAX_BINS, MIN_AUDIO, MAX_AUDIO = 16, 8193, 15, 8192


def percentile_parts(a, q):
    """np.percentile(a, q) as numpy 2.x forms it for a 1-D float array (method 'linear'): the virtual index
    (n - 1) * (q / 100) in a's precision, the two order statistics and _lerp with its t >= 0.5 branch.
    Returns (rank, lower, upper, value)."""
    dt = a.dtype.type
    v = dt(len(a) - 1) * (dt(q) / dt(100))
    r = int(np.floor(v))
    g = dt(v - np.floor(v))
    s = np.sort(a)
    lo, hi = s[r], s[r + 1]
    d = hi - lo
    res = lo + d * g
    if g >= 0.5:
        res = hi - d * (dt(1) - g)
    return r, lo, hi, res


def band_ranges(freqs):
    """The reference's masks as (first bin, count) over the increasing table, in the kernel's order."""
    f = np.asarray(freqs, np.float64)
    masks = [(f >= 20) & (f <= 250), (f > 250) & (f <= 2000), (f >= 200) & (f <= 4000), (f >= 300) & (f <= 3000),
             (f >= 4000) & (f <= 10000), f <= 10000, (f >= 20) & (f < 500), (f >= 500) & (f <= 2000),
             (f > 2000) & (f <= 8000), (f >= 100) & (f <= 4000)]
    out = []
    for m in masks:
        idx = np.nonzero(m)[0]
        assert len(idx) == 0 or (np.diff(idx) == 1).all()
        out.append((int(idx[0]) if len(idx) else 0, len(idx)))
    return out


def distortion(magnitude):
    """:278-317: (qualifying count, the five largest peaks' bins padded with -1)."""
    K = len(magnitude)
    thr = np.mean(magnitude) * 2
    peaks = [(i, magnitude[i]) for i in range(1, K - 1)
             if magnitude[i] > magnitude[i - 1] and magnitude[i] > magnitude[i + 1] and magnitude[i] > thr]
    peaks.sort(key=lambda x: x[1], reverse=True)
    count = 0
    for peak_idx, peak_mag in peaks[:5]:
        if peak_idx < 5:
            continue
        harmonic_count = 0
        for n in range(2, 6):
            h = peak_idx * n
            if h < K and np.max(magnitude[max(0, h - 3):min(K, h + 4)]) > peak_mag * 0.1:
                harmonic_count += 1
        if harmonic_count >= 2:
            count += 1
    bins = [p[0] for p in peaks[:5]]
    return count, np.array(bins + [-1] * (5 - len(bins)), np.int32)


def spectrum_side(spec, freqs, prev_mag=None, f64=False):
    dt = np.float64 if f64 else np.float32
    freqs = np.asarray(freqs, np.float64)
    magnitude = np.abs(np.asarray(spec, np.float32)).astype(dt)
    K = len(magnitude)
    e = {}
    total = np.sum(magnitude)
    e["spectral_centroid"] = float(np.sum(freqs * magnitude) / total) if total != 0 else 0.0
    cumsum = np.cumsum(magnitude)
    if cumsum[-1] == 0:
        e["rolloff_index"], e["spectral_rolloff"] = 0, 0.0
    else:
        idx = int(np.where(cumsum >= 0.85 * cumsum[-1])[0][0])
        e["rolloff_index"], e["spectral_rolloff"] = idx, float(freqs[min(idx, K - 1)])
    e["spectral_bandwidth"] = float(np.sqrt(np.sum(((freqs - e["spectral_centroid"]) ** 2) * magnitude) / total)) \
        if total != 0 else 0.0

    def energy(mask):
        return np.sum(magnitude[mask] ** 2)
    f = freqs
    total_energy = np.sum(magnitude ** 2)
    # bass_emphasis (:709-739)
    bass_mask, mid_mask = (f >= 20) & (f <= 250), (f > 250) & (f <= 2000)
    if not np.any(bass_mask) or not np.any(mid_mask) or total_energy == 0:
        e["bass_emphasis"] = 0.0
    else:
        bass_energy, mid_energy = energy(bass_mask), energy(mid_mask)
        bass_ratio = bass_energy / total_energy
        bass_to_mid = bass_energy / (mid_energy + 1e-10)
        e["bass_emphasis"] = float(min(bass_ratio * min(bass_to_mid / 2.0, 1.0), 1.0))
    # vocal_presence (:753-783)
    vocal_mask, core_mask = (f >= 200) & (f <= 4000), (f >= 300) & (f <= 3000)
    if not np.any(vocal_mask) or total_energy == 0:
        e["vocal_presence"] = 0.0
    else:
        vocal_energy = energy(vocal_mask)
        core_energy = energy(core_mask) if np.any(core_mask) else 0
        vocal_ratio = vocal_energy / total_energy
        core_ratio = core_energy / vocal_energy if vocal_energy > 0 else 0
        e["vocal_presence"] = float(min(vocal_ratio * (0.5 + 0.5 * core_ratio) * 2.0, 1.0))
    # high_freq_energy (:406-422)
    high_mask, upto_mask = (f >= 4000) & (f <= 10000), f <= 10000
    e["high_freq_energy"] = 0.0
    if np.any(high_mask) and np.any(upto_mask):
        he, te = energy(high_mask), energy(upto_mask)
        if te > 0:
            e["high_freq_energy"] = float(he / te)
    # mid_frequency_dominance (:319-349); branch 0: no value, 1: the boosted ratio, 2: the plain ratio
    low_mask, mid_mask, high_mask = (f >= 20) & (f < 500), (f >= 500) & (f <= 2000), (f > 2000) & (f <= 8000)
    e["mid_frequency_dominance"], e["mid_branch"], e["mid_margin"] = 0.0, 0, np.inf
    if np.any(mid_mask):
        le = energy(low_mask) if np.any(low_mask) else 0
        me = energy(mid_mask)
        he = energy(high_mask) if np.any(high_mask) else 0
        te = le + me + he
        if te != 0:
            ratio = me / te
            # (the distance of the two comparisons from equality, relative: the generator asserts a margin)
            e["mid_margin"] = min(abs(float(me) - float(le) * 1.2), abs(float(me) - float(he) * 1.5)) / float(me) \
                if me > 0 else 0.0
            if me > le * 1.2 and me > he * 1.5:
                e["mid_frequency_dominance"], e["mid_branch"] = float(min(ratio * 1.5, 1.0)), 1
            else:
                e["mid_frequency_dominance"], e["mid_branch"] = float(ratio), 2
    # compute_spectral_complexity (:382-404)
    harmonic_mask = (f >= 100) & (f <= 4000)
    e["spectral_complexity"] = 0.3
    if np.any(harmonic_mask):
        hm = magnitude[harmonic_mask]
        safe = hm[hm > 1e-10] if f64 else hm[hm > np.float32(1e-10)]
        if len(safe) > 0:
            gm, am = np.exp(np.mean(np.log(safe))), np.mean(safe)
            if am > 0:
                e["spectral_complexity"] = float(np.clip(1.0 - gm / am, 0.0, 1.0))
    # spectral_flux (:256-276); non-finite stored bins are left out (the device's rule)
    e["spectral_flux"], e["prev_nonfinite"] = 0.0, False
    if prev_mag is not None:
        prev = np.abs(np.asarray(prev_mag, np.float32)).astype(dt)
        ok = np.isfinite(prev)
        e["prev_nonfinite"] = not ok.all()
        diff = magnitude - np.where(ok, prev, dt(0))
        flux = np.sum(np.where(ok, np.maximum(0, diff), dt(0)))
        if total > 0:
            e["spectral_flux"] = float(min(flux / total, 1.0))
    e["distortion_count"], e["peak_bins"] = distortion(magnitude)
    return e


def audio_side(audio, f64=False):
    """`audio` float32 or float64; f64=True widens float32 input first."""
    x = np.asarray(audio)
    if f64:
        x = x.astype(np.float64)
    e = {"zero_crossings": int(len(np.where(np.diff(np.sign(x)))[0]))}
    a = np.abs(x)
    r95, lo95, hi95, loud = percentile_parts(a, 95)
    r20, lo20, hi20, quiet = percentile_parts(a, 20)
    e["ranks"] = (r95, r20)
    e["order_stats"] = (float(lo95), float(hi95), float(lo20), float(hi20))
    e["loud"], e["quiet"] = float(loud), float(quiet)
    e["dynamic_range"] = float(min(1.0, (loud - quiet) / loud)) if quiet > 0 else 0.0
    e["rms"] = float(np.sqrt(np.mean(x ** 2)))
    return e


def features(spec, freqs, audio, prev_mag=None, f64=False):
    spec, audio = np.asarray(spec), np.asarray(audio)
    if not (np.isfinite(spec).all() and np.isfinite(audio).all()):
        e = dict.fromkeys(COLUMNS, 0.0)
        e.update(flags=2, peak_bins=np.full(5, -1, np.int32), rolloff_index=0, zero_crossings=0, distortion_count=0)
        return e
    e = spectrum_side(spec, freqs, prev_mag, f64)
    e.update(audio_side(audio, f64))
    e["flags"] = 2 if e["prev_nonfinite"] else 0
    return e


def row(e):
    return np.array([float(e[k]) for k in COLUMNS], np.float64)
