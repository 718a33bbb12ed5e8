"""Makes tests/golden/tonal.npz by calling the reference's ChromagramAnalyzer, ChromagramPanel.update and MusicTheory
(omega4/panels/chromagram.py, music_theory.py) themselves (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_tonal.py <reference checkout>

The reference's panels are loaded by path as a package of their own with ``pygame`` stubbed (nothing is drawn).

  rows/<genre>   designed chroma rows (all six genres; `other` is the unknown name 'techno'): 1..6 strong pitch
                 classes over a noise floor of at most 0.05, normalised; triads, sevenths and power chords on every
                 root; D5 on both sides of the 0.15 / 0.10 / 0.05 thresholds; the metal riff pairs (both power
                 chords, each alone, the F# interference over either, a strong F# over neither); rows with a
                 variance just above and just below 0.001; the all-zero row; the flat row 0.25. Per row, from a new
                 reference analyzer: detect_key, get_alternative_keys (top 3), detect_chord, and analyze_mode for
                 every root; for metal also detect_chord behind the chord history C#5, C#5, D5
                 (`chord_after_history`), where the riff pattern alternates the other way. tests/tonal_ref.py is asserted against all of it here: names exactly, values to 1e-12.
  seq/<genre>    300 ChromagramPanel.update steps of one reference panel over a pool of spectra (K 1025, 48 kHz),
                 with silent frames, a genre change to `<genre>` after 40 steps of another, a tuning offset of -2
                 set on the analyzer for steps 200..235 (the detector finds no peak at this K and keeps it), and a
                 chord held long enough for anti-stick. After every step: get_results() as JSON (the chromagram beside it as an array), the analyzer's newest raw row,
                 its transposition offset, the five history lengths, and `mode_tie`: where the averaged mode is a tie
                 between equally frequent modes, which the reference breaks by set order (the string hash), their
                 names (JSON, [] elsewhere).
  theory         recorded MusicTheory calls.

Margins, asserted here on every frame that is not degenerate (conditions on the inputs, not measurements): at least
1e-9 between the best and the second key, between neighbours of the top four alternatives, between the best and the
second chord, between the anti-stick second and 0.85 x first, between the best and the second mode of every root,
between every chroma value and 0.02, 0.03, 0.05, 0.08, 0.10, 0.15 and 0.2, between the variance and 0.001, and
(seq) between `confidence` and 0.3. No row is left out: a row that misses a margin stops the generator.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import tonal_ref as T  # noqa: E402

GENRE_NAME = {"pop": "pop", "jazz": "jazz", "classical": "classical", "metal": "metal", "rock": "rock", "other": "techno"}
MARGIN = 1e-9
BAR = 1e-12


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = types.ModuleType("pygame")
    pg.font = types.ModuleType("pygame.font")
    pg.font.Font = object
    pg.Surface = object
    sys.modules.setdefault("pygame", pg)
    pkg = types.ModuleType("ref_panels")
    pkg.__path__ = [os.path.join(path, "omega4", "panels")]
    sys.modules["ref_panels"] = pkg
    chroma = importlib.import_module("ref_panels.chromagram")
    theory = importlib.import_module("ref_panels.music_theory")
    return chroma.ChromagramAnalyzer, chroma.ChromagramPanel, theory.MusicTheory


def gaps_ok(x, genre):
    """The margins of one blended chroma; False where one is missed."""
    if not np.all(np.isfinite(x)) or np.sum(x) == 0 or np.std(x) == 0:
        return True
    row, kc, ac, ch, mo = T.frame(x, genre)
    if abs(row[13] - 0.001) < MARGIN:
        return False
    for thr in (0.02, 0.03, 0.05, 0.08, 0.10, 0.15, 0.2):
        if np.min(np.abs(x - thr)) < MARGIN:
            return False
    s = np.sort(kc)[::-1]
    if s[0] - s[1] < MARGIN:
        return False
    s = np.sort(ac)[::-1]
    if np.min(s[:4][:-1] - s[:4][1:]) < MARGIN:
        return False
    for v in range(2):
        c = np.sort(ch[v][np.isfinite(ch[v])])[::-1]
        if len(c) > 1 and c[0] - c[1] < MARGIN and c[0] > 0:
            return False
        if v == 1 and len(c) > 1 and abs(c[1] - 0.85 * c[0]) < MARGIN:
            return False
        if len(c) and abs(c[0]) < MARGIN:
            return False
    for r in range(12):
        m = np.sort(mo[r])[::-1]
        if m[0] > 0 and (m[0] - m[1] < MARGIN or m[0] < MARGIN):
            return False
    return True


RIFF_HISTORY = ["C#5", "C#5", "D5"]  # the second detect_chord of every metal row starts from this chord history


def riff_branch(x):
    """Which return of _detect_metal_riff_pattern (chromagram.py:549-579) a chroma row reaches, whatever the history:
    'both', 'cs', 'd', 'fs' (the F# interference), or None."""
    cs, d, fs, gs, a = x[1], x[2], x[6], x[8], x[9]
    cs_power, d_power = cs > 0.1 and gs > 0.05, d > 0.1 and a > 0.05
    if cs_power and d_power:
        return "both"
    if cs_power and cs > d * 1.5:
        return "cs"
    if d_power and d > cs * 1.5:
        return "d"
    if fs > 0.2 and (cs_power or d_power) and (cs > 0.08 or d > 0.08):
        return "fs"
    return None


def designed_rows(rng):
    """(rows, named): named[i] says which designed case row i is, '' for a random one."""
    rows, named = [], []

    def add(strong, floor=0.05):
        x = rng.uniform(0.2 * floor, floor, 12)
        for p, a in strong:
            x[p % 12] = a
        rows.append(x / np.sum(x))
        named.append("")

    for n in range(1, 7):
        for _ in range(4):
            add([(p, rng.uniform(0.5, 1.0)) for p in rng.choice(12, n, replace=False)])
    for r in range(12):
        for iv in ([0, 4, 7], [0, 3, 7], [0, 4, 7, 10], [0, 3, 7, 10], [0, 4, 7, 11], [0, 7]):
            add([(r + k, rng.uniform(0.6, 1.0)) for k in iv])
    # D5 around the thresholds: D at 0.16 / 0.14 / 0.11 / 0.09 with A at 0.06 / 0.04 of the normalised row
    for d in (0.16, 0.14, 0.11, 0.09):
        for a in (0.06, 0.04):
            x = rng.uniform(0.2, 1.0, 12)
            x[[2, 9]] = 0
            x = x / np.sum(x) * (1 - d - a)
            x[2], x[9] = d, a
            rows.append(x)
            named.append(f"D5 grid {d} / {a}")
    # the metal riff pairs, every value off the thresholds: C#5 and D5 together, each alone, the F# interference
    # with the C# and with the D power chord, and a strong F# over neither (no pattern)
    for cs, gs, d, a, fs, branch in ((0.21, 0.11, 0.22, 0.12, 0.025, "both"), (0.31, 0.11, 0.12, 0.035, 0.025, "cs"),
                                     (0.12, 0.035, 0.31, 0.11, 0.025, "d"), (0.12, 0.07, 0.09, 0.025, 0.31, "fs"),
                                     (0.09, 0.025, 0.12, 0.07, 0.31, "fs"), (0.07, 0.11, 0.07, 0.11, 0.31, None)):
        x = rng.uniform(0.5, 1.0, 12)
        x[[1, 8, 2, 9, 6]] = 0
        x = x / np.sum(x) * (1 - cs - gs - d - a - fs)
        x[[1, 8, 2, 9, 6]] = cs, gs, d, a, fs
        assert riff_branch(x) == branch, (cs, d, branch)
        rows.append(x)
        named.append(f"riff {branch}")
    # variance just above and just below 0.001: a flat row with one raised class, scaled to the variance wanted
    for target in (0.00105, 0.00095):
        x = np.full(12, 1 / 12.0) + rng.uniform(-0.004, 0.004, 12)
        x[4] += 0.05
        x = x / np.sum(x)
        dev = x - np.mean(x)
        x = np.mean(x) + dev * np.sqrt(target / np.var(x))
        rows.append(x)
        named.append(f"variance {target}")
    rows.append(np.zeros(12))
    rows.append(np.full(12, 0.25))
    named += ["zero", "flat"]
    return rows, named


def record_rows(Analyzer, Theory, out, genre, designed):
    name = GENRE_NAME[genre]
    rows, named = designed
    # every row keeps the margins: none is left out
    missed = [(i, n) for i, (x, n) in enumerate(zip(rows, named)) if not gaps_ok(x, genre)]
    assert not missed, (genre, missed)
    X = np.array(rows)
    F = len(X)
    chord2, chord2_score = [], np.zeros(F)
    key, key_corr = [], np.zeros(F)
    alt, alt_corr = [], np.zeros((F, 3))
    chord, chord_score = [], np.zeros(F)
    mode, mode_score = np.zeros((F, 12), np.int8), np.zeros((F, 12))
    worst = 0.0
    for f, x in enumerate(X):
        with np.errstate(all="ignore"):
            an = Analyzer(48000)
            an.set_genre_context(name)
            k, c = an.detect_key(x.copy())
            a3 = an.get_alternative_keys(x.copy(), 3)
            an2 = Analyzer(48000)
            an2.set_genre_context(name)
            ch, cs = an2.detect_chord(x.copy())
            an3 = Analyzer(48000)   # the same behind a chord history: the riff pattern's other outcomes
            an3.set_genre_context(name)
            an3.chord_history.extend(RIFF_HISTORY)
            ch2, cs2 = an3.detect_chord(x.copy())
            for r in range(12):
                m, ms = Theory.analyze_mode(x.copy(), r)
                mode[f, r], mode_score[f, r] = T.MODE_NAMES.index(m), ms
        key.append(k)
        key_corr[f] = c
        alt.append([n for n, _ in a3])
        alt_corr[f] = [v for _, v in a3]
        chord.append(ch)
        chord_score[f] = cs
        chord2.append(ch2)
        chord2_score[f] = cs2
        assert (cs2 == 0.9) == (cs == 0.9) and (cs == 0.9 or (ch2, cs2) == (ch, cs)), (genre, f)
        assert (cs == 0.9) == (genre == "metal" and riff_branch(x) is not None), (genre, f)
        # tests/tonal_ref.py against the reference
        row = T.frame(x, genre)[0]
        flags = int(row[12])
        if not flags & (T.FLAG_ZERO | T.FLAG_FLAT):
            assert k == T.key_name(int(row[14])), (genre, f, k, row[14])
            worst = max(worst, abs(c - row[15]))
        else:
            assert k == "Unknown" and c == 0.0
        assert [T.key_name(int(i)) for i in row[16:19]] == alt[-1] or np.std(x) == 0, (genre, f)
        worst = max(worst, float(np.max(np.abs(alt_corr[f] - row[19:22]))))
        if not (cs == 0.9 and genre == "metal"):
            assert ch == T.chord_name(int(row[22])), (genre, f, ch, row[22])
            worst = max(worst, abs(cs - row[23]))
        assert np.array_equal(mode[f], row[28:40].astype(np.int8)), (genre, f)
        worst = max(worst, float(np.max(np.abs(mode_score[f] - row[40:52]))))
    assert worst <= BAR, (genre, worst)
    out[f"rows/{genre}/chroma"] = X
    out[f"rows/{genre}/key"] = np.array(key)
    out[f"rows/{genre}/key_corr"] = key_corr
    out[f"rows/{genre}/alt"] = np.array(alt)
    out[f"rows/{genre}/alt_corr"] = alt_corr
    out[f"rows/{genre}/chord"] = np.array(chord)
    out[f"rows/{genre}/chord_score"] = chord_score
    if genre == "metal":
        out["rows/metal/chord_after_history"] = np.array(chord2)
    out[f"rows/{genre}/mode"] = mode
    out[f"rows/{genre}/mode_score"] = mode_score
    print(f"rows/{genre}: {F} rows, tonal_ref within {worst:.2e}")


def spectrum(notes, rng, K=1025, fs=48000, bass=None):
    """A magnitude spectrum with a partial series on each MIDI note (and a bass peak for the tuning detector)."""
    f = np.arange(K) * (fs / 2 / (K - 1))
    s = 0.002 * rng.uniform(0.5, 1.0, K)
    for n, amp in notes:
        f0 = 440.0 * 2 ** ((n - 69) / 12)
        for h, w in ((1, 1.0), (2, 0.4), (3, 0.2)):
            s += amp * w * np.exp(-0.5 * ((f - h * f0) / 14.0) ** 2)
    if bass:
        s += 1.5 * np.exp(-0.5 * ((f - bass) / 9.0) ** 2)
    return s.astype(np.float32)


def jsonable(v):
    if isinstance(v, np.ndarray):
        return [float(a) for a in v]
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.integer, int)) and not isinstance(v, bool):
        return int(v)
    if isinstance(v, (list, tuple)):
        return [jsonable(a) for a in v]
    if isinstance(v, dict):
        return {k: jsonable(a) for k, a in v.items()}
    return v


def record_seq(Panel, out, genre, pool, rng):
    name = GENRE_NAME[genre]
    before = "jazz" if genre != "jazz" else "pop"
    P = len(pool)
    idx = rng.integers(0, P - 2, 300)
    idx[60:80] = 3                 # one chord held: anti-stick's repeat count passes 10
    idx[150:156] = rng.integers(0, 4, 6)
    idx[200:230] = P - 2           # the drop-tuned frames (a bass peak near 73.4 Hz)
    idx[230:236] = P - 1           # the standard-tuned bass peak
    silent = np.zeros(300, np.int8)
    silent[[0, 25, 26, 100, 299]] = 1
    quiet = np.zeros(512, np.float32)
    loud = (0.1 * np.sin(np.arange(512) * 0.05)).astype(np.float32)
    freqs = np.linspace(0, 24000, 1025)
    p = Panel(48000)
    res, chroma, raw, offs, lens, used, tie = [], np.zeros((300, 12)), np.zeros((300, 12)), np.zeros(300, np.int8), [], [], []
    for s in range(300):
        g = before if s < 40 else name
        if s == 120:
            g = None               # the default to pop
        used.append("" if g is None else g)
        if s in (200, 236):        # (at K 1025 the 70-100 Hz band holds two bins: the detector keeps what is set)
            p.analyzer.transposition_offset = -2 if s == 200 else 0
        with np.errstate(all="ignore"):
            p.update(pool[idx[s]], quiet if silent[s] else loud, freqs, g)
        r = p.get_results()
        chroma[s] = r["chromagram"]
        an = p.analyzer
        if len(an.chroma_history):
            raw[s] = an.chroma_history[-1]
        offs[s] = an.transposition_offset
        lens.append([len(an.key_history), len(an.chord_history), len(an.mode_history), len(an.modulation_history),
                     len(an.roman_numeral_sequence)])
        # the averaged mode is max() over a set: among modes of equal count the winner follows the string hash
        counts = {x: sum(1 for m, _ in an.mode_history if m == x) for x in set(m for m, _ in an.mode_history)}
        top = sorted(x for x in counts if counts[x] == max(counts.values()))
        tie.append(top if len(an.mode_history) > 5 and len(top) > 1 and not silent[s] else [])
        d = {k: v for k, v in r.items() if k != "chromagram"}
        res.append(jsonable(d))
        if not silent[s]:
            eff = an.current_genre.lower()
            eff = eff if eff in T.GENRES[:5] else "other"
            assert gaps_ok(chroma[s], eff), (genre, s)
            assert abs(r["confidence"] - 0.3) >= MARGIN, (genre, s, r["confidence"])
    out[f"seq/{genre}/idx"] = idx.astype(np.int16)
    out[f"seq/{genre}/silent"] = silent
    out[f"seq/{genre}/genre"] = np.array(used)
    out[f"seq/{genre}/results"] = np.array(json.dumps(res, ensure_ascii=False))
    out[f"seq/{genre}/chroma"] = chroma
    out[f"seq/{genre}/raw"] = raw
    out[f"seq/{genre}/offset"] = offs
    out[f"seq/{genre}/mode_tie"] = np.array(json.dumps(tie))
    out[f"seq/{genre}/lens"] = np.array(lens, np.int16)
    chords = [r["current_chord"] for r in res]
    print(f"seq/{genre}: {len(set(chords))} chords, {len(set(r['key'] for r in res))} keys, offsets {sorted(set(offs))}")


def record_theory(Theory, out):
    keys = [f"{n} {q}" for n in T.NOTES for q in ("Major", "Minor")] + ["Unknown", "Am", "Bb Major", "H Minor"]
    chords = ["Cmajor", "A#minor", "D5", "F#dom7", "Gmaj9", "N/A", "Ebmajor", "B13", "Esus4"]
    calls = {
        "circle": [[k, list(Theory.get_circle_position(k))] for k in keys],
        "relative_major": [[n, Theory.relative_major(n)] for n in T.NOTES + ["X"]],
        "relative_minor": [[n, Theory.relative_minor(n)] for n in T.NOTES + ["X"]],
        "roman": [[c, k, Theory.chord_to_roman(c, k)] for c in chords for k in keys[:24:5] + ["Unknown"]],
        "function": [[r, Theory.get_chord_function(r), Theory.get_tsd_group(r)] for r in
                     ["I", "ii7", "V7", "vii°", "VI9", "♭D", "iv", "x"]],
        "modulation": [[a, b, Theory.detect_key_modulation(a, b)] for a in keys[:24:3] for b in keys[:24:2]],
        "transitions": [[s, Theory.create_chord_transition_matrix(s)] for s in
                        (["I", "V", "vi", "IV", "I", "V", "I"], ["i"], [], ["I", "I", "I", "V7"])],
    }
    out["theory"] = np.array(json.dumps(calls, ensure_ascii=False))


def main(ref_path):
    Analyzer, Panel, Theory = import_reference(ref_path)
    out = {}
    for gi, genre in enumerate(T.GENRES):
        record_rows(Analyzer, Theory, out, genre, designed_rows(np.random.default_rng(100 + gi)))
    rng = np.random.default_rng(7)
    chords = [[(48, 1.0), (52, 0.8), (55, 0.9)], [(45, 1.0), (48, 0.8), (52, 0.9)], [(53, 1.0), (57, 0.8), (60, 0.9)],
              [(43, 1.0), (50, 0.9)], [(50, 1.0), (57, 0.9)], [(52, 1.0), (55, 0.8), (59, 0.9), (62, 0.6)],
              [(47, 1.0), (50, 0.8), (54, 0.9)], [(57, 1.0), (60, 0.7), (64, 0.9), (67, 0.5)]]
    pool = [spectrum(c, rng) for c in chords]
    pool += [np.zeros(1025, np.float32)]
    pool += [spectrum(chords[3], rng, bass=73.4), spectrum(chords[4], rng, bass=82.4)]
    out["seq/pool"] = np.array(pool)
    for gi, genre in enumerate(T.GENRES):
        record_seq(Panel, out, genre, pool, np.random.default_rng(200 + gi))
    record_theory(Theory, out)
    out["versions"] = np.array([np.__version__])
    path = os.path.join(HERE, "tonal.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
