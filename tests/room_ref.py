"""RoomModeAnalyzer (omega4/analyzers/room_modes.py:71-239, :356-458) restated in numpy, in the project's own
code: what csrc/room.hip computes, in the same operation order. TEST INFRASTRUCTURE ONLY. Pinned to the
reference's own outputs (tests/golden/room.npz) on the CPU by tests/test_room.py: counts, flags, bins, types,
order, crossing indices and frequency / magnitude / prominence / q_factor / bandwidth bit for bit.

find_peaks(x, height=, prominence=) is restated from scipy's documented algorithm: _local_maxima_1d (strict
rise on the left, strict fall on the right, a plateau gives (left + right) // 2, never the first or last
sample), then x[p] >= height, then _peak_prominences with wlen=None (walk out while x[i] <= x[p], keep the
minimum on each side, prominence = x[p] - max(left_min, right_min)) >= prominence.
"""
import numpy as np

MAX_MODES, ROWS, COLS, RT60_COLS = 64, 65, 8, 8
MODE_COLUMNS = ("frequency", "magnitude", "q_factor", "severity", "type", "prominence", "bandwidth", "bin")
CFG_KEYS = ("sample_rate", "min_frequency", "max_frequency", "peak_threshold_multiplier", "minimum_prominence_std",
            "min_q_factor", "max_q_factor", "minimum_severity")
DEFAULT_CFG = (48000.0, 30.0, 300.0, 2.0, 1.0, 0.5, 100.0, 0.3)
TYPE_NAMES = ("axial_length", "axial_width", "axial_height", "tangential", "oblique")


def type_name(code):
    base, harmonic = int(code) & 7, int(code) >> 3
    return f"{TYPE_NAMES[base]}_H{harmonic}" if harmonic else TYPE_NAMES[base]


def type_code(name):
    base, _, h = name.partition("_H")
    return TYPE_NAMES.index(base) + 8 * (int(h) if h else 0)


def bin_range(freqs, lo, hi):
    idx = np.flatnonzero((freqs >= lo) & (freqs <= hi))
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


def speed_of_sound(temp=20.0, humidity=50.0):
    return 331.3 * np.sqrt(1 + temp / 273.15) + 0.02 * humidity


def expected_frequencies(length, width, height, temp=20.0, humidity=50.0):
    """The six doubles the host hands the device: axial fundamentals, then the tangential frequencies."""
    c = speed_of_sound(temp, humidity)
    out = [c / (2 * length), c / (2 * width), c / (2 * height)]
    for a, b in ((length, width), (length, height), (width, height)):
        out.append(c * np.sqrt((1 / (2 * a)) ** 2 + (1 / (2 * b)) ** 2))
    return np.asarray(out, np.float64)


def classify(f, exp=None):
    if exp is not None and exp[0] > 0:
        for h in (1, 2, 3):
            for d in range(3):
                if abs(f - exp[d] * h) < 5:
                    return d + 8 * h
        for d in range(3, 6):
            if abs(f - exp[d]) < 10:
                return 3
    for code, (lo, hi) in enumerate(((30, 80), (80, 120), (120, 200), (200, 300))):
        if lo <= f <= hi:
            return code
    return 4


def local_maxima(x):
    out, n = [], len(x)
    for i in range(1, n - 1):
        if x[i - 1] < x[i]:
            ahead = i + 1
            while ahead < n - 1 and x[ahead] == x[i]:
                ahead += 1
            if x[ahead] < x[i]:
                out.append((i + ahead - 1) // 2)
    return out


def prominence(x, p):
    lmin = rmin = x[p]
    i = p
    while i >= 0 and x[i] <= x[p]:
        lmin = min(lmin, x[i])
        i -= 1
    i = p
    while i < len(x) and x[i] <= x[p]:
        rmin = min(rmin, x[i])
        i += 1
    return x[p] - max(lmin, rmin)


def q_factor(x, fr, p, min_q, max_q):
    half = x[p] / np.sqrt(2)
    lf = rf = fr[p]
    for i in range(p - 1, -1, -1):
        if x[i] <= half:
            lf = fr[i] + (half - x[i]) * (fr[i + 1] - fr[i]) / (x[i + 1] - x[i])
            break
    for i in range(p + 1, len(x)):
        if x[i] <= half:
            rf = fr[i - 1] + (half - x[i - 1]) * (fr[i] - fr[i - 1]) / (x[i] - x[i - 1])
            break
    bw = rf - lf
    q = fr[p] / bw if bw > 0 else 50.0
    q = q if q > min_q else min_q
    return q if q < max_q else max_q


def detect(spectrum, freqs, cfg=DEFAULT_CFG, exp=None, decisions=None):
    """(header [count, flags, mean, std], modes [count, 8] in MODE_COLUMNS order, all of them). `decisions`, a
    list, receives every (value, threshold) pair a keep / drop decision compared."""
    _, fmin, fmax, mult, pstd, min_q, max_q, min_sev = cfg
    x = np.asarray(spectrum, np.float64)
    freqs = np.asarray(freqs, np.float64)
    none = np.zeros((0, COLS))
    if not (np.isfinite(x).all() and np.isfinite(freqs).all()):
        return np.array([0.0, 1.0, 0.0, 0.0]), none
    first, last = bin_range(freqs, fmin, fmax)
    if last == first:
        return np.array([0.0, 2.0, 0.0, 0.0]), none
    x, fr = x[first:last], freqs[first:last]
    mean, std = np.mean(x), np.std(x)
    if mean == 0 or std == 0:
        return np.array([0.0, 2.0, mean, std]), none
    height, pmin = mean * mult, std * pstd
    modes = []
    for p in local_maxima(x):
        if decisions is not None:
            decisions.append((x[p], height))
        if not x[p] >= height:
            continue
        prom = prominence(x, p)
        if decisions is not None:
            decisions.append((prom, pmin))
        if not prom >= pmin:
            continue
        q = q_factor(x, fr, p, min_q, max_q)
        q10 = q / 10.0
        s = (x[p] / mean) * (1.0 if 1.0 < q10 else q10) * 0.5
        s = s if s < 1.0 else 1.0
        if decisions is not None:
            decisions.append((s, min_sev))
        if s > min_sev:
            modes.append([fr[p], x[p], q, s, classify(fr[p], exp), prom, fr[p] / q if q > 0 else 0.0, first + p])
    modes.sort(key=lambda m: -m[3])  # (stable: ties keep ascending bin order)
    flags = 4.0 if len(modes) > MAX_MODES else 0.0
    return np.array([float(len(modes)), flags, mean, std]), np.asarray(modes, np.float64).reshape(-1, COLS)


def rows_from(header, modes):
    """The device's [65, 8] block of one frame."""
    out = np.zeros((ROWS, COLS))
    out[0, :4] = header
    n = min(len(modes), MAX_MODES)
    out[1:1 + n] = modes[:n]
    return out


def curve_db(audio):
    curve = np.cumsum((np.asarray(audio, np.float64) ** 2)[::-1])[::-1]
    floored = np.maximum(curve, 1e-10)
    return curve[0], 10 * np.log10(floored / floored[0])


def rt60_row(audio, fs):
    """[curve0, idx5, idx10, idx35, slope, intercept, r_squared, flags] of one history."""
    audio = np.asarray(audio, np.float64)
    L = len(audio)
    if not np.isfinite(audio ** 2).all():
        return np.array([0, 0, 0, 0, 0, 0, 0, 1.0])
    c0, db = curve_db(audio)
    i5, i10, i35 = (int(np.sum(db > t)) for t in (-5, -10, -35))
    row = np.array([c0, i5, i10, i35, 0, 0, 0, 0], np.float64)
    if i5 >= L or i35 >= L or i35 <= i5:
        row[7] = 2
        return row
    if i35 - i5 < 3:
        row[7] = 4
        return row
    t, d = np.arange(i5, i35) / fs, db[i5:i35]
    mt, md = np.mean(t), np.mean(d)
    sxx, sxy, sst = np.sum((t - mt) ** 2), np.sum((t - mt) * (d - md)), np.sum((d - md) ** 2)
    slope = sxy / sxx
    icpt = md - slope * mt
    row[4:7] = slope, icpt, 1 - np.sum((d - (slope * t + icpt)) ** 2) / sst
    row[7] = 8 if slope >= 0 else 0
    return row


def frame_energies(audio, W):
    return np.sum(np.asarray(audio, np.float64).reshape(-1, W) ** 2, axis=1)


def decay_stream(noise, L, r, roll, rising):
    """The large RT60 inputs from the golden's noise table, in exact IEEE steps (a serial cumprod envelope)."""
    base = np.roll(np.asarray(noise, np.float32), int(roll)).astype(np.float64)
    x = np.tile(base, -(-int(L) // len(base)))[:int(L)] * np.cumprod(np.full(int(L), float(r)))
    return (x[::-1] if rising else x).astype(np.float32)
