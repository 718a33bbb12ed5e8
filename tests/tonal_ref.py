"""A numpy restatement of what omega_tonal_features computes per frame (include/omega.h): the temporal blend,
detect_key's 24 adjusted correlations, get_alternative_keys' 24 plain ones, detect_chord's two score matrices and
analyze_mode for every root (omega4/panels/chromagram.py:215-339, :396-418, :670-812; music_theory.py:175-200),
with the decisions taken as the reference takes them. TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

COLS = 52
STATE_LEN = 13
FLAG_NONFINITE, FLAG_ZERO, FLAG_FLAT = 1, 2, 4
GENRES = ["pop", "jazz", "classical", "metal", "rock", "other"]
NOTES = ['C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B']
MAJOR = np.array([6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88])
MINOR = np.array([6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17])
WEIGHTS = {  # major_weights, minor_weights, chromatic_tolerance
    'jazz': ([1.0, 0.8, 1.0, 0.9, 1.0, 1.0, 0.9, 1.0, 0.8, 1.0, 0.8, 1.0], [1.0, 0.8, 1.0, 1.0, 0.9, 1.0, 0.8, 1.0, 1.0, 0.9, 1.0, 0.9], 0.8),
    'classical': ([1.2, 0.7, 1.0, 0.7, 1.1, 1.0, 0.7, 1.1, 0.7, 1.0, 0.7, 0.9], [1.2, 0.8, 1.0, 1.1, 0.8, 1.0, 0.8, 1.1, 1.0, 0.8, 1.0, 0.9], 0.3),
    'pop': ([1.5, 0.5, 1.0, 0.5, 1.2, 1.0, 0.5, 1.2, 0.5, 1.0, 0.5, 0.8], [1.5, 0.6, 1.0, 1.2, 0.6, 1.0, 0.6, 1.2, 1.0, 0.6, 1.0, 0.8], 0.2),
    'metal': ([1.8, 0.4, 1.2, 0.4, 1.0, 1.2, 0.6, 1.4, 0.4, 1.0, 0.4, 0.6], [1.8, 0.6, 1.2, 1.4, 0.5, 1.2, 0.5, 1.4, 1.2, 0.5, 1.2, 0.7], 0.6),
    'rock': ([1.6, 0.5, 1.1, 0.5, 1.1, 1.1, 0.6, 1.3, 0.5, 1.0, 0.5, 0.7], [1.6, 0.6, 1.1, 1.3, 0.6, 1.1, 0.6, 1.3, 1.1, 0.6, 1.1, 0.8], 0.4),
}
CHORD_TYPES = [('major', [0, 4, 7]), ('minor', [0, 3, 7]), ('dim', [0, 3, 6]), ('aug', [0, 4, 8]),
               ('maj7', [0, 4, 7, 11]), ('min7', [0, 3, 7, 10]), ('dom7', [0, 4, 7, 10]), ('maj9', [0, 4, 7, 11, 2]),
               ('min9', [0, 3, 7, 10, 2]), ('13', [0, 4, 7, 10, 2, 5, 9]), ('power', [0, 7]), ('sus2', [0, 2, 7]),
               ('sus4', [0, 5, 7])]
TYPE_NAMES = [n for n, _ in CHORD_TYPES]
MODES = [('Ionian (Major)', [0, 2, 4, 5, 7, 9, 11]), ('Dorian', [0, 2, 3, 5, 7, 9, 10]),
         ('Phrygian', [0, 1, 3, 5, 7, 8, 10]), ('Lydian', [0, 2, 4, 6, 7, 9, 11]),
         ('Mixolydian', [0, 2, 4, 5, 7, 9, 10]), ('Aeolian (Natural Minor)', [0, 2, 3, 5, 7, 8, 10]),
         ('Locrian', [0, 1, 3, 5, 6, 8, 10])]
MODE_NAMES = [n for n, _ in MODES]


def blend_factor(genre):
    return 0.7 if genre in ('metal', 'rock') else (0.5 if genre == 'jazz' else 0.3)


def tested_types(genre):
    if genre == 'jazz':
        return TYPE_NAMES
    if genre in ('metal', 'rock'):
        return ['power', 'major', 'minor', 'sus2', 'sus4', 'dom7']
    return ['major', 'minor', 'dim', 'aug', 'maj7', 'min7']


def key_name(k):
    return f"{NOTES[k // 2]} {'Minor' if k % 2 else 'Major'}"


def chord_name(cell):
    if cell < 0:
        return 'N/A'
    r, t = divmod(cell, 13)
    return NOTES[r] + ('5' if TYPE_NAMES[t] == 'power' else TYPE_NAMES[t])


def corr(a, b):
    with np.errstate(all='ignore'):
        return np.corrcoef(a, b)[0, 1]


def key_corr(x, genre):
    mw, nw, _ = WEIGHTS.get(genre, WEIGHTS['pop'])
    mw, nw = np.array(mw), np.array(nw)
    sq = np.sqrt(x)
    w = (sq / (np.sum(sq) + 1e-10)) * (mw + nw) / 2
    out = np.zeros(24)
    live = np.std(w) > 0
    for i in range(12):
        pm = np.roll(MAJOR, i) * np.roll(mw, i)
        pn = np.roll(MINOR, i) * np.roll(nw, i)
        pm = pm / (np.sum(pm) + 1e-10)
        pn = pn / (np.sum(pn) + 1e-10)
        a = corr(w, pm) if live else 0.0
        b = corr(w, pn) if live else 0.0
        if genre == 'jazz' and NOTES[i] == 'F':
            a, b = a * 1.1, b * 1.1
        elif genre == 'classical' and NOTES[i] in ('C', 'G', 'D', 'A', 'F'):
            a = a * 1.05
        elif genre == 'rock' and NOTES[i] in ('E', 'A', 'D', 'G'):
            a, b = a * 1.05, b * 1.05
        out[2 * i], out[2 * i + 1] = a, b
    return out


def alt_corr(x):
    out = np.zeros(24)
    if np.std(x) > 0:
        for i in range(12):
            out[2 * i] = corr(x, np.roll(MAJOR, i))
            out[2 * i + 1] = corr(x, np.roll(MINOR, i))
    return out


def chord_matrices(x, genre):
    out = np.full((2, 12, 13), np.nan)
    metal = genre in ('metal', 'rock')
    tol = WEIGHTS.get(genre, WEIGHTS['pop'])[2]
    tested = tested_types(genre)
    for v in range(2 if metal else 1):
        for r in range(12):
            thr = 0.02 if metal else 0.03
            if metal and r == 2 and v == 0:
                thr = 0.15
            if x[r] < thr:
                continue
            for t, (name, iv) in enumerate(CHORD_TYPES):
                if name not in tested:
                    continue
                pitches = [(r + k) % 12 for k in iv]
                score = 0.0
                for i, p in enumerate(pitches):
                    if i == 0:
                        score += x[p] * 2.0
                    elif i == 1 and name == 'power':
                        score += x[p] * 1.8
                    else:
                        score += x[p]
                pen = tol * 0.5 if name == 'power' else tol
                for p in range(12):
                    if p not in pitches:
                        score -= x[p] * pen
                score /= len(pitches)
                if v == 1:
                    if name == 'power':
                        score *= 1.5
                    elif name in ('minor', 'sus2', 'sus4'):
                        score *= 1.2
                elif genre == 'jazz' and name in ('maj7', 'min7', 'dom7', '13'):
                    score *= 1.2
                elif metal:
                    if name == 'power':
                        score *= 1.5
                        if r == 2 and x[2] > 0.15:
                            score *= 2.0 if x[9] > 0.05 else 1.5
                    elif name in ('minor', 'sus2', 'sus4'):
                        score *= 1.2
                elif genre == 'pop' and name in ('major', 'minor'):
                    score *= 1.1
                elif genre == 'classical' and name in ('major', 'minor', 'dim'):
                    score *= 1.1
                out[v, r, t] = score
    return out


def mode_matrix(x):
    out = np.zeros((12, 7))
    for r in range(12):
        rx = np.roll(x, -r)
        if not np.std(rx) > 0:
            continue
        for m, (_, iv) in enumerate(MODES):
            t = np.zeros(12)
            t[iv] = 1.0
            out[r, m] = corr(rx, t / np.sum(t))
    return out


def stable_desc(v):
    """Indices of the non-NaN entries by a stable descending sort (list.sort(reverse=True) keeps equals in order)."""
    idx = [i for i in range(len(v)) if v[i] == v[i]]
    return sorted(idx, key=lambda i: -v[i])


def frame(x, genre):
    """Row tail (cols 12..51) and the detail matrices of one blended chroma."""
    row = np.zeros(COLS)
    row[:12] = x
    finite = bool(np.all(np.isfinite(x)))
    xs = x if finite else np.zeros(12)
    var = float(np.var(xs))
    row[12] = (0 if finite else FLAG_NONFINITE) | (FLAG_ZERO if np.sum(xs) == 0 else 0) | (FLAG_FLAT if var < 0.001 else 0)
    row[13] = var
    with np.errstate(all='ignore'):
        kc, ac, ch, mo = key_corr(xs, genre), alt_corr(xs), chord_matrices(xs, genre), mode_matrix(xs)
    k = int(np.argmax(kc))
    row[14], row[15] = k, kc[k]
    top = stable_desc(ac)[:3]
    row[16:19], row[19:22] = top, ac[top]
    best, bv = -1, 0.0
    for i, s in enumerate(ch[0].ravel()):
        if s > bv:
            best, bv = i, s
    row[22], row[23] = best, bv
    order = stable_desc(ch[1].ravel())
    row[24:28] = [-1, 0, -1, 0]
    for q, i in enumerate(order[:2]):
        row[24 + 2 * q], row[25 + 2 * q] = i, ch[1].ravel()[i]
    for r in range(12):
        bm, bs = 0, 0.0
        for m in range(7):
            if mo[r, m] > bs:
                bm, bs = m, mo[r, m]
        row[28 + r], row[40 + r] = bm, bs
    return row, kc, ac, ch, mo


def features(raw, genre, roll=None, first=None, state=None):
    """omega_tonal_features on raw [F, 12]: (rows, key_corr, alt_corr, chord, mode, state_out)."""
    raw = np.asarray(raw, np.float64)
    F = len(raw)
    a = blend_factor(genre)
    rows, kc, ac = np.zeros((F, COLS)), np.zeros((F, 24)), np.zeros((F, 24))
    ch, mo = np.zeros((F, 2, 12, 13)), np.zeros((F, 12, 7))
    prev = None if state is None or state[0] == 0 else np.asarray(state[1:], np.float64)
    for f in range(F):
        cur = np.roll(raw[f], int(roll[f])) if roll is not None else raw[f]
        if first is not None and first[f]:
            prev = None
        x = cur if prev is None else prev * (1 - a) + cur * a
        rows[f], kc[f], ac[f], ch[f], mo[f] = frame(x, genre)
        prev = cur
    out = np.zeros(STATE_LEN)
    if state is not None:
        out[:] = state
    if prev is not None and F:
        out[0], out[1:] = 1.0, prev
    return rows, kc, ac, ch, mo, out
