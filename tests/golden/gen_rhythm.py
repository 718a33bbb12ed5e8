"""Makes tests/golden/rhythm.npz by calling the reference's BeatDetectionPanel (omega4/panels/beat_detection.py) and
FrequencyBandTrackerPanel (omega4/panels/frequency_band_tracker.py) themselves (build container only; TEST
INFRASTRUCTURE ONLY). Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_rhythm.py <reference checkout>

The two reference modules are loaded by path with ``pygame`` stubbed (they import it at the top; nothing is drawn)
and the beat module's ``time`` replaced by a deterministic stepping clock. Each group is ONE stream: one reference
object of each class is fed the group's float32 spectra (and, the beat panel, its frames) in order; a frame with a
non-finite value is not fed (this project's rule: it changes nothing; the tracker, which takes no audio, is still
fed a frame whose only non-finite value is a sample). Written per group: the frames (float32) and
spectra (float32), `freqs`, the rows in tests/rhythm_ref.py's COLUMNS order chained through the state blob from the
stream's start, and after every step every public attribute of both reference objects (`beat`, `track`; the names
are in `beat_names`, `track_names`). The rows are tests/rhythm_ref.py's and are asserted here against the reference
objects after every frame: prev_spectrum, the last onset strength, each energy_history tail, band_energies,
spectral_centroid and spectral_spread; and through the facades' host logic (omega_gpu on _host_init, no device)
every recorded attribute.

  app        48 kHz, K 513 (rfftfreq), m 2048, 6 frames        k2     K 2, m 1: every band is empty (lo >= hi)
  k8193      K 8193, m 16384, 2 frames                          lin    the app's linspace(0, 20000, 512), K 512
  fs8        8000 Hz: 8000 and 20000 Hz lie beyond the spectrum (upper edge -> len; as a lower edge 8000 Hz stays
             0 and the last band is the whole spectrum, as in the reference)
  (lin, fs8 and the groups below: m 64)
  zero       an all-zero spectrum between two others
  nonfinite  a NaN sample and an infinite bin between finite frames
  gated      7 frames, gated (rms < 0.001) at the start, twice in the middle and at the end
  allgated   3 frames, all gated
  seq_kick   300 update() steps, kicks every 24 frames, the clock stepping 1/60 s (0.4 s, 150 BPM)
  seq_irreg  300 update() steps, irregular kicks, a long pause of identical frames and three gated frames, the clock
             stepping 1/30 s

The sequences draw their spectra from a pool (`seq_*/pool`, `seq_*/idx`) whose values are multiples of 2^-10 with
sums below 2^14: every float32 sum over them is exact in any order, so the reference's float32 pairwise sums are the
device's float64 sums bit for bit and the onset strengths are the reference's own float32 values. That is what lets
rhythmic_complexity and spectral_spread be held to 1e-9 there: both descend from float32 totals, and a summation-
order difference of a few float32 ulps would show in them at 1e-7. The groups above carry unquantised spectra.

Conditions asserted here on the inputs (not measurements; a seed that misses one is not recorded): every rms at
least 1e-4 relative away from 0.001; in the sequences every comparison of detect_beats (the threshold, 0.5, 0.2 s),
of calculate_bpm (0.3, 1.0, 0.3) and of the peak hold at least 1e-4 relative away from its threshold (or, in the
peak hold, an exact tie of two exact sums: a band of one bin on the 2^-10 grid repeats its values); seq_kick
yields at least 8 beats and a current_bpm that has left 120; seq_irreg reaches every reachable branch of
analyze_rhythmic_patterns (the early return, regularity clamped at 0 and not, syncopation clipped to 1, below 1 and
the 0.0 return of a silent beat grid).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "audio-analyzer-omega_amd"))
import rhythm_ref as RR  # noqa: E402

F32_BAR = 64 * 2.0 ** -24  # tests/test_rhythm.py derives it
F64_BAR = 1e-9
BEAT_BANDS = ("sub_bass", "bass", "low_mid", "mid", "high_mid", "high")
TRACK_BANDS = BEAT_BANDS[:5] + ("presence", "brilliance")
PATTERNS = ("regularity", "complexity", "syncopation", "groove_strength")


class Clock:
    """The time of update() step i is T0 + i * step, however often it is read."""
    T0 = 1000.0

    def __init__(self, step):
        self.t, self.step = self.T0, step

    def at(self, i):
        self.t = self.T0 + i * self.step

    def time(self):
        return self.t

    __call__ = time


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    pg.font = types.SimpleNamespace(Font=object)  # (named in the modules' annotations)
    pg.Surface = object
    mods = []
    for name in ("beat_detection", "frequency_band_tracker"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(path, "omega4", "panels", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_" + name] = mod  # (dataclasses looks the module up)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def beat_attrs(p):
    """Every public attribute of a beat panel and its detector (the reference's or the facade's) as numbers."""
    d, info = p.detector, p.beat_info
    pat = info['rhythmic_patterns']
    v = {"current_bpm": d.current_bpm, "bpm_confidence": d.bpm_confidence, "beat_phase": d.beat_phase,
         "rhythmic_complexity": d.rhythmic_complexity, "beat_strength": d.beat_strength,
         "beat_regularity": d.beat_regularity, "syncopation_level": d.syncopation_level,
         "n_onsets": len(d.onset_strength_history),
         "last_onset": d.onset_strength_history[-1] if d.onset_strength_history else 0.0,
         "n_beats": len(d.beat_times), "last_beat_time": d.beat_times[-1] if d.beat_times else 0.0,
         "n_tempo_history": len(d.tempo_history), "has_prev": d.prev_spectrum is not None,
         "n_energy_history": len(d.energy_history["bass"]),
         "info_current_bpm": info['current_bpm'], "info_bpm_confidence": info['bpm_confidence'],
         "is_beat": info['is_beat'], "info_beat_strength": info['beat_strength'], "info_beat_phase": info['beat_phase'],
         "info_last_beat_time": info['last_beat_time'], "n_patterns": len(pat),
         "beat_flash_time": p.beat_flash_time, "n_bpm_history_display": len(p.bpm_history_display)}
    for b in BEAT_BANDS:
        v["energy_" + b] = d.energy_history[b][-1] if d.energy_history[b] else 0.0
    for k in PATTERNS:
        v["pattern_" + k] = pat.get(k, 0.0)
    return v


def track_attrs(p):
    t, info = p.tracker, p.band_info
    v = {"total_energy": t.total_energy, "spectral_centroid": t.spectral_centroid, "spectral_spread": t.spectral_spread,
         "reference_level": t.reference_level, "n_history": len(t.band_history["bass"]),
         "n_total_history": len(t.total_energy_history) if hasattr(t, "total_energy_history") else -1,
         "dominant_band": TRACK_BANDS.index(t.get_dominant_band()[0]), "spectral_tilt": t.get_spectral_tilt(),
         "info_dominant_band": -1 if info['dominant_band'] == 'none' else TRACK_BANDS.index(info['dominant_band']),
         "info_spectral_centroid": info['spectral_centroid'], "info_spectral_spread": info['spectral_spread'],
         "info_spectral_tilt": info['spectral_tilt'], "info_total_energy_db": info['total_energy_db']}
    for b in TRACK_BANDS:
        v["energy_" + b] = t.band_energies[b]
        v["rms_" + b] = t.band_rms[b]
        v["peak_" + b] = t.band_peaks[b]['value']
        v["hold_time_" + b] = t.band_peaks[b]['hold_time']
        v["balance_" + b] = t.spectral_balance.get(b, 0.0)
        v["db_" + b] = t.get_band_db(b)
        v["normalized_" + b] = t.get_band_normalized(b)
    return v


EXACT = ("n_", "is_beat", "last_beat_time", "info_last_beat_time", "has_prev", "beat_flash_time", "dominant_band",
         "info_dominant_band", "hold_time_")
F64 = ("current_bpm", "bpm_confidence", "beat_phase", "rhythmic_complexity", "beat_regularity", "info_current_bpm",
       "info_bpm_confidence", "info_beat_phase", "pattern_regularity", "pattern_complexity", "spectral_spread",
       "info_spectral_spread")


def bar_of(name):
    """0: equal; else the relative bar (tests/test_rhythm.py states the classes)."""
    if any(name == e or (e.endswith("_") and name.startswith(e)) for e in EXACT):
        return 0.0
    return F64_BAR if name in F64 else F32_BAR


def same(what, ref, host, spread_bar=None):
    for k, a in ref.items():
        a, b = float(a), float(host[k])
        bar = bar_of(k)
        if spread_bar is not None and k.endswith("spectral_spread"):
            bar = spread_bar
        assert (a == b) if bar == 0.0 else abs(a - b) <= bar * abs(a), (what, k, a, b)


def far(a, b, what, rel=1e-4):
    a, b = float(a), float(b)
    assert abs(a - b) >= rel * max(abs(a), abs(b)) and a != b, (what, a, b)


def best_confidence(beat_times):
    """calculate_bpm's clustering (:159-199) -> best_confidence, or None where it returns early."""
    bl = list(beat_times)
    if len(bl) < 4:
        return None
    iv = [bl[i] - bl[i - 1] for i in range(1, len(bl))]
    for v in iv:
        far(v, 0.3, "interval 0.3")
        far(v, 1.0, "interval 1.0")
    iv = [v for v in iv if 0.3 <= v <= 1.0]
    if not iv:
        return None
    bpms = [60.0 / v for v in iv]
    groups = {}
    for bpm in bpms:
        groups.setdefault(round(bpm * 2) / 2, []).append(bpm)
    best = 0.0
    for lst in groups.values():
        if len(lst) >= 2:
            best = max(best, len(lst) / len(bpms) * max(0.1, 1.0 - np.var(lst) / 100.0))
    return best


def step_margins(what, before, det, row, clock):
    """The decisions of one live row, from the facade detector's state before (`before`) and after it (`det`)."""
    hist = list(det.onset_strength_history)
    if len(hist) > 10:
        recent = hist[-10:]
        thr = np.mean(recent) + 0.3 * np.std(recent)
        if hist[-1] != 0 or thr != 0:  # (identical frames: the flux and the whole window are exactly 0 on both sides)
            far(hist[-1], thr, (what, "threshold"))
        far(hist[-1], 0.5, (what, "peak pick"))
        if hist[-1] > thr and hist[-1] > 0.5 and before["beat_times"]:
            far(clock() - before["beat_times"][-1], 0.2, (what, "0.2 s"))
    bc = best_confidence(det.beat_times)
    if bc is not None:
        far(bc, 0.3, (what, "confidence"))


def peak_margins(what, peaks_before, trk):
    for b in TRACK_BANDS:
        e, pk = float(trk.band_energies[b]), peaks_before[b]
        if e != float(pk['value']):  # (an exact tie of two exact sums is decided alike on both sides)
            far(e, pk['value'], (what, "peak hold", b))
        if not e > pk['value'] and pk['hold_time'] == 0:
            far(e, np.float32(pk['value']) * 0.95 if isinstance(pk['value'], np.floating) else pk['value'] * 0.95,
                (what, "peak decay", b))


def host_panels(fs, clock):
    from omega_gpu.beat_detection import BeatDetectionPanel
    from omega_gpu.frequency_band_tracker import FrequencyBandTrackerPanel
    bp = BeatDetectionPanel.__new__(BeatDetectionPanel)
    bp._host_init(fs, clock)
    tp = FrequencyBandTrackerPanel.__new__(FrequencyBandTrackerPanel)
    tp._host_init(fs)
    return bp, tp


def run_stream(mods, what, fs, freqs, spectra, frames, clock_step, check_steps):
    """Feeds one stream to the reference objects. Returns the rows and both attribute tables; asserts the
    reference against tests/rhythm_ref.py and the facades' host logic throughout."""
    from omega_gpu import _rhythm as R
    beat_mod, track_mod = mods
    clock, hclock = Clock(clock_step), Clock(clock_step)
    beat_mod.time = clock
    rb, rt = beat_mod.BeatDetectionPanel(fs), track_mod.FrequencyBandTrackerPanel(fs)
    hb, ht = host_panels(fs, hclock)
    empty = R.empty_bands(freqs)
    assert R.edges(freqs) == RR.edges(freqs)
    state, rows, battrs, tattrs = None, [], [], []
    exact = check_steps  # (the sequences' sums are exact)
    for i, (spec, x) in enumerate(zip(spectra, frames)):
        w = (what, i)
        clock.at(i)
        hclock.at(i)
        r, new = RR.row(spec, x, freqs, state)
        rt_row, _ = RR.row(spec, None, freqs, None)  # the tracker's call: no audio, no gate
        flags = int(r[0])
        # the beat panel's stream: spectrum and audio
        if not flags & RR.FLAG_NONFINITE:
            rms = float(np.sqrt(np.mean(x ** 2)))
            far(rms, RR.GATE, (w, "gate"))
            assert (rms < RR.GATE) == bool(flags & RR.FLAG_GATED), w
            before = {"beat_times": list(hb.detector.beat_times)}
            with np.errstate(all="ignore"):
                rb.update(spec, x, freqs)
            assert hb._apply_row(r), w
            hb.detector._state = new
            prev_state, state = state, new
            d = rb.detector
            if not flags & RR.FLAG_GATED:  # the reference's own intermediates against the row
                assert np.array_equal(d.prev_spectrum, new[2:].astype(np.float32)), w
                tot = np.float32(r[2])
                onset = 0.0 if flags & RR.FLAG_NO_FLUX else (np.float32(r[3]) / tot if tot > 0 else np.float32(r[3]))
                ref_on = float(d.onset_strength_history[-1])
                assert abs(ref_on - float(onset)) <= (0.0 if exact else F32_BAR) * abs(ref_on), (w, ref_on, onset)
                for b, name in enumerate(BEAT_BANDS):
                    a = float(d.energy_history[name][-1])
                    assert abs(a - r[5 + b]) <= F32_BAR * abs(a), (w, name, a, r[5 + b])
                if check_steps:
                    step_margins(w, before, hb.detector, r, hclock)
            else:  # a gated frame leaves the state as it was
                assert prev_state is None and new[0] == 0 or np.array_equal(new, prev_state), w
        else:
            assert not np.any(r[1:]) and not hb._apply_row(r), w
            assert np.array_equal(new, state if state is not None else new) and (state is not None or new[0] == 0), w
        # the tracker's stream: the spectrum alone (a non-finite sample does not reach it)
        if not int(rt_row[0]) & RR.FLAG_NONFINITE:
            peaks_before = {b: dict(ht.tracker.band_peaks[b]) for b in TRACK_BANDS}
            with np.errstate(all="ignore"):
                rt.update(spec, freqs)
            assert ht._apply_row(rt_row, empty), w
            t = rt.tracker
            for b, name in enumerate(TRACK_BANDS):
                a = float(t.band_energies[name])
                assert abs(a - rt_row[5 + b]) <= F32_BAR * abs(a), (w, name)
            tot = float(np.float32(rt_row[2]))
            if tot > 0:
                assert abs(float(t.spectral_centroid) - rt_row[12] / tot) <= F32_BAR * abs(t.spectral_centroid), w
                want = np.sqrt(rt_row[13] / tot) if rt_row[12] / tot > 0 else 0.0
                assert abs(float(t.spectral_spread) - want) <= F32_BAR * abs(want), (w, t.spectral_spread, want)
            if check_steps:
                peak_margins(w, peaks_before, ht.tracker)
        else:
            assert not ht._apply_row(rt_row, empty), w
        a, b = beat_attrs(rb), track_attrs(rt)
        # (outside the sequences the spread divides by a float32 total that differs by the summation order)
        same(w, a, beat_attrs(hb))
        same(w, b, track_attrs(ht), None if exact else F32_BAR)
        rows.append(r)
        battrs.append([float(v) for v in a.values()])
        tattrs.append([float(v) for v in b.values()])
    names = (list(a), list(b))
    return np.array(rows), np.array(battrs), np.array(tattrs), names, rb, rt


def random_spectra(rng, n, K):
    s = rng.random((n, K)) ** 3 * np.linspace(2.0, 0.2, K)
    return s.astype(np.float32)


def audio(rng, n, m, amp=0.1):
    return (amp * rng.standard_normal((n, m))).astype(np.float32)


def record(mods, out, group, fs, freqs, spectra, frames):
    spectra = np.asarray(spectra, np.float32)
    frames = np.asarray(frames, np.float32)
    rows, ba, ta, names, _, _ = run_stream(mods, group, fs, freqs, spectra, frames.astype(np.float64), 1 / 60, False)
    out[f"{group}/fs"] = np.int64(fs)
    out[f"{group}/freqs"] = np.asarray(freqs, np.float64)
    out[f"{group}/spec"] = spectra
    out[f"{group}/frame"] = frames
    out[f"{group}/row"] = rows
    out[f"{group}/beat"] = ba
    out[f"{group}/track"] = ta
    return rows, names


def first_seed(fn, what, seeds=range(1, 200)):
    for seed in seeds:
        try:
            r = fn(seed)
        except AssertionError as e:
            print(what, "seed", seed, "misses a condition:", str(e)[:140])
            continue
        print(what, "seed", seed)
        return r
    raise AssertionError(f"{what}: no seed keeps the conditions")


def quantised_pool(rng, K):
    """16 spectra on the 2^-10 grid: 8 floors that differ by a small jitter, 4 kicks, 4 broadband hits."""
    q = lambda a: np.round(np.asarray(a) * 1024) / 1024  # noqa: E731
    base = 0.004 + 0.012 * rng.random(K)
    pool = [q(base + 0.003 * rng.random(K)) for _ in range(8)]
    for j in range(4):
        k = pool[j].copy()
        k[1:6] += q(6.0 + 3.0 * rng.random(5))  # 47..234 Hz at 46.875 Hz a bin
        pool.append(k)
    for j in range(4):
        h = pool[4 + j].copy()
        h[40:200] += q(0.1 + 0.1 * rng.random(160))
        pool.append(h)
    pool = np.array(pool)
    assert np.all(pool * 1024 == np.round(pool * 1024)) and pool.sum(axis=1).max() < 2 ** 14
    return pool.astype(np.float32)


def sequence(mods, out, name, seed, clock_step, irregular):
    rng = np.random.default_rng(seed)
    K, m, fs = 513, 2048, 48000
    freqs = np.fft.rfftfreq(1024, 1 / fs)
    pool = quantised_pool(rng, K)
    apool = np.concatenate([audio(rng, 2, m), audio(rng, 1, m, 2e-4)])  # two live frames and a gated one
    idx = rng.integers(0, 8, 300)
    aidx = rng.integers(0, 2, 300)
    if not irregular:
        kicks = np.arange(24, 300, 24)
    else:
        kicks, t = [], 12
        while t < 150:
            kicks.append(t)
            t += int(rng.integers(10, 21))
        idx[152:272] = 3  # identical frames: flux 0, and a pause of 4 s between two beats
        t = 272
        while t < 300:
            kicks.append(t)
            t += int(rng.integers(10, 21))
        kicks = np.array(kicks)
        aidx[[40, 41, 200]] = 2
    idx[kicks] = 8 + rng.integers(0, 8 if irregular else 4, len(kicks))  # (irregular: kicks and broadband hits)
    spectra, frames = pool[idx], apool[aidx].astype(np.float64)
    rows, ba, ta, names, rb, rt = run_stream(mods, name, fs, freqs, spectra, frames, clock_step, True)
    bn = names[0]
    d = rb.detector
    assert len(d.beat_times) >= 8 and d.current_bpm != 120.0, (name, len(d.beat_times), d.current_bpm)
    if irregular:
        reg, sync, npat = ba[:, bn.index("pattern_regularity")], ba[:, bn.index("pattern_syncopation")], ba[:, bn.index("n_patterns")]
        nb = ba[:, bn.index("n_beats")]
        full = (nb >= 8) & (npat == 4)
        assert np.any((nb < 8) & (npat == 4)), (name, "early return")
        assert np.any(full & (reg == 0.0)) and np.any(full & (reg > 0.0)), (name, "regularity", reg.min(), reg.max())
        assert np.any(full & (sync == 1.0)) and np.any(full & (sync > 0) & (sync < 1)) and np.any(full & (sync == 0.0)), \
            (name, "syncopation", np.unique(sync)[:5])
        assert np.any(npat == 0), (name, "gated")
    out[f"{name}/fs"] = np.int64(fs)
    out[f"{name}/freqs"] = freqs
    out[f"{name}/pool"] = pool
    out[f"{name}/idx"] = idx.astype(np.int32)
    out[f"{name}/audio_pool"] = apool
    out[f"{name}/audio_idx"] = aidx.astype(np.int32)
    out[f"{name}/clock_step"] = np.float64(clock_step)
    out[f"{name}/row"] = rows
    out[f"{name}/beat"] = ba
    out[f"{name}/track"] = ta
    print(name, "beats", len(d.beat_times), "bpm", d.current_bpm, "confidence", d.bpm_confidence)
    return names


def main(ref_path):
    mods = import_reference(ref_path)
    out = {}
    rng = np.random.default_rng(2024)
    f48 = np.fft.rfftfreq(1024, 1 / 48000)
    record(mods, out, "app", 48000, f48, random_spectra(rng, 6, 513), audio(rng, 6, 2048))
    r, _ = record(mods, out, "k2", 48000, np.array([0.0, 24000.0]), random_spectra(rng, 3, 2), np.full((3, 1), 0.5))
    assert not np.any(r[:, 4:12]) and np.all(r[:, 2] > 0), r
    record(mods, out, "k8193", 48000, np.fft.rfftfreq(16384, 1 / 48000), random_spectra(rng, 2, 8193), audio(rng, 2, 16384))
    lin = np.linspace(0, 20000, 512)
    record(mods, out, "lin", 48000, lin, random_spectra(rng, 3, 512), audio(rng, 3, 64))
    f8 = np.fft.rfftfreq(1024, 1 / 8000)
    r, _ = record(mods, out, "fs8", 8000, f8, random_spectra(rng, 3, 513), audio(rng, 3, 64))
    e = RR.edges(f8)
    assert e[8] == 0 and e[9] == 513 and e[7] == 512 and np.all(r[:, 11] == r[:, 2]), (e, r[:, (2, 11)])
    z = random_spectra(rng, 3, 513)
    z[1] = 0
    r, _ = record(mods, out, "zero", 48000, f48, z, audio(rng, 3, 64))
    assert not np.any(r[1, 2:]) and r[2, 3] > 0, r[1]
    s, x = random_spectra(rng, 5, 513), audio(rng, 5, 64)
    x[1, 7] = np.nan
    s[3, 100] = np.inf
    r, _ = record(mods, out, "nonfinite", 48000, f48, s, x)
    assert list(r[:, 0].astype(int)) == [4, 1, 0, 1, 0], r[:, 0]
    x = audio(rng, 7, 64)
    for i in (0, 2, 3, 6):
        x[i] *= 2e-3
    r, _ = record(mods, out, "gated", 48000, f48, random_spectra(rng, 7, 513), x)
    assert list(r[:, 0].astype(int)) == [6, 4, 2, 2, 0, 0, 2], r[:, 0]
    r, _ = record(mods, out, "allgated", 48000, f48, random_spectra(rng, 3, 513), audio(rng, 3, 64, 2e-4))
    assert list(r[:, 0].astype(int)) == [6, 6, 6], r[:, 0]
    names = first_seed(lambda sd: sequence(mods, out, "seq_kick", sd, 1 / 60, False), "seq_kick")
    first_seed(lambda sd: sequence(mods, out, "seq_irreg", sd, 1 / 30, True), "seq_irreg")
    out["beat_names"] = np.array(names[0])
    out["track_names"] = np.array(names[1])
    out["versions"] = np.array([np.__version__])
    path = os.path.join(HERE, "rhythm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
