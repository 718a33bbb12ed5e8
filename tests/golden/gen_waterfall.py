"""Makes tests/golden/waterfall.npz by calling the reference's SpectrogramWaterfall and SpectrogramWaterfallPanel
(omega4/panels/spectrogram_waterfall.py) themselves (build container only; TEST INFRASTRUCTURE ONLY). Run from the
repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_waterfall.py <reference checkout>

The reference module is loaded by path with ``pygame`` stubbed (it imports it at the top; nothing is drawn). Each
group is ONE stream fed to one reference panel, once as float32 (`<group>/spec`, stored) and once as float64
(tests/waterfall_ref.py widen() of the stored spectra: not stored). Written per group and precision p in (f32, f64):
`row_p` (the rows appended to waterfall_data, concatenated; `row_off` gives each frame's start), `stat_p` [F, 6]:
max dB, min dB, current_peak, current_floor, the panel's peak_freq and peak_magnitude after the frame; and per
group `lohi` [F, 2] (freq_indices at the frame), `auto` and `gain` [F] (auto_gain and gain_adjustment at the frame).

  a2048    30 frames, fft_size 2048 at 48 kHz (1025 bins, cells [1, 854))
  k129     60 frames, fft_size 256 (129 bins), amplitudes spanning 1e-4..10
  toggle   24 frames of 129 bins: auto_gain off for frames 8..15, gain_adjustment 0, then 6.0, then -3.5
  range    20 frames of 129 bins: set_frequency_range(1000, 8000) before frame 10
  const    6 frames of one constant spectrum: peak == floor, zero rows
  short    8 frames of 513 bins against fft_size 2048's mapping: shorter than max_idx
Every group has several frames with exact zeros among their bins.

Colours: per precision the intensity grid `grid_p` -- 0, 1, the breakpoints 0.25, 0.5, 0.75, 0.33, 0.66 each with its
two nextafter neighbours in that precision, k / 255 for k = 0..255, 2000 seeded uniform values -- and `color_p`
[5, n, 3]: _spectrum_to_color of every grid value (a numpy scalar, as the reference's draw loop hands them over) in
the schemes spectrum, hot, cool, viridis and the fallback (color_scheme set to another name).
`map_rates`, `map_sizes`, `map_idx`: freq_indices at four (sample rate, fft_size) pairs.

Printed and asserted: the worst difference between the reference's float32 rows (the C library's log10f) and
tests/waterfall_ref.py's model (log10 in float64, rounded once) on these sequences, which must stay within
4 * 2^-24 (the tests' bar is 8 * 2^-24); the float64 rows equal the model's to 1e-12.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import waterfall_ref as WR  # noqa: E402

BREAKS = (0.25, 0.5, 0.75, 0.33, 0.66)


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    pg.font = types.SimpleNamespace(Font=object)  # (named in the module's annotations)
    pg.Surface = object
    spec = importlib.util.spec_from_file_location(
        "ref_spectrogram_waterfall", os.path.join(path, "omega4", "panels", "spectrogram_waterfall.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_spectrogram_waterfall"] = mod
    spec.loader.exec_module(mod)
    return mod


def spectra(rng, F, n, lo_amp=1e-3, hi_amp=1.0):
    """Amplitudes log-uniform in [lo_amp, hi_amp] under a sloping envelope, exact zeros in every third frame."""
    a = np.exp(rng.uniform(np.log(lo_amp), np.log(hi_amp), (F, n))) * np.linspace(1.0, 0.3, n)
    a *= rng.uniform(0.5, 1.5, (F, 1))
    for f in range(0, F, 3):
        a[f, rng.integers(0, n, 5)] = 0.0
    return a.astype(np.float32)


def run_reference(mod, fft_size, spec, steps):
    """One stream through a reference panel; steps[f] is a function applied to the panel before frame f (or None)."""
    panel = mod.SpectrogramWaterfallPanel(48000)
    panel.waterfall = mod.SpectrogramWaterfall(48000, fft_size)
    w = panel.waterfall
    rows, stat, lohi, auto, gain = [], [], [], [], []
    for f, x in enumerate(spec):
        if steps.get(f):
            steps[f](panel)
        freqs = w.freq_bins[:len(x)]
        panel.update(x, freqs)
        r = w.waterfall_data[-1]
        assert r.dtype == x.dtype and isinstance(w.peak_history[-1][0], x.dtype.type), (r.dtype, x.dtype)
        if w.auto_gain:
            assert isinstance(w.current_peak, x.dtype.type) and isinstance(w.current_floor, x.dtype.type)
        rows.append(r)
        mx, mn = w.peak_history[-1]
        stat.append([mx, mn, w.current_peak, w.current_floor, panel.waterfall_info['peak_freq'],
                     panel.waterfall_info['peak_magnitude']])
        lohi.append(w.freq_indices)
        auto.append(w.auto_gain)
        gain.append(w.gain_adjustment)
    assert len(w.waterfall_data) == len(spec)
    return rows, np.array(stat, np.float64), np.array(lohi, np.int32), np.array(auto, np.int32), np.array(gain, np.float64)


def model(spec, lohi, auto, gain):
    """tests/waterfall_ref.py over the same stream."""
    wf, rows, stat = WR.Waterfall(), [], []
    for x, (lo, hi), a, g in zip(spec, lohi, auto, gain):
        st, r = WR.run(x[None, :], int(lo), int(hi), bool(a), float(g), wf)
        rows.append(r[0])
        stat.append(st[0])
    return rows, np.array(stat)


WORST = {"f32": 0.0, "f64": 0.0}


def record(mod, out, group, fft_size, spec, steps=None):
    out[f"{group}/spec"] = spec
    out[f"{group}/fft_size"] = np.int64(fft_size)
    for p, s in (("f32", spec), ("f64", WR.widen(spec))):
        rows, stat, lohi, auto, gain = run_reference(mod, fft_size, s, steps or {})
        mrows, mstat = model(s, lohi, auto, gain)
        for f, (a, b) in enumerate(zip(rows, mrows)):
            assert a.shape == b.shape and a.dtype == b.dtype, (group, p, f)
            WORST[p] = max(WORST[p], float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))))
        assert np.array_equal(mstat[:, 5], [np.argmax(x) for x in s]), group
        out[f"{group}/row_{p}"] = np.concatenate(rows)
        out[f"{group}/stat_{p}"] = stat
    out[f"{group}/row_off"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    out[f"{group}/lohi"] = lohi
    out[f"{group}/auto"] = auto
    out[f"{group}/gain"] = gain
    return rows, stat


def grid(dt, rng):
    v = [dt(0.0), dt(1.0)]
    for b in BREAKS:
        v += [np.nextafter(dt(b), dt(0.0)), dt(b), np.nextafter(dt(b), dt(1.0))]
    v += [dt(k) / dt(255) for k in range(256)]
    v += list(rng.random(2000).astype(dt))
    return np.array(v, dt)


def main(ref_path):
    mod = import_reference(ref_path)
    out = {}
    rng = np.random.default_rng(2025)
    record(mod, out, "a2048", 2048, spectra(rng, 30, 1025))
    record(mod, out, "k129", 256, spectra(rng, 60, 129, 1e-4, 10.0))

    def auto_off(p):
        p.waterfall.toggle_auto_gain()
        p.adjust_gain(6.0)

    def auto_on(p):
        p.waterfall.toggle_auto_gain()
        p.adjust_gain(-9.5)
    _, st = record(mod, out, "toggle", 256, spectra(rng, 24, 129), {8: auto_off, 16: auto_on})
    assert list(out["toggle/auto"]) == [1] * 8 + [0] * 8 + [1] * 8 and list(out["toggle/gain"][[0, 8, 16]]) == [0.0, 6.0, -3.5]
    assert np.all(st[8:16, 2] == st[7, 2]) and st[16, 2] != st[7, 2]
    rows, _ = record(mod, out, "range", 256, spectra(rng, 20, 129),
                     {10: lambda p: p.waterfall.set_frequency_range(1000, 8000)})
    assert len(rows[0]) != len(rows[-1]) and tuple(out["range/lohi"][0]) == (1, 107)
    c = np.full((6, 129), 0.37, np.float32)
    rows, st = record(mod, out, "const", 256, c)
    assert not np.any(np.concatenate(rows)) and np.all(st[:, 2] == st[:, 3])
    rows, _ = record(mod, out, "short", 2048, spectra(rng, 8, 513))
    assert tuple(out["short/lohi"][0]) == (1, 854) and len(rows[0]) == 512
    for g in ("a2048", "k129", "toggle", "range", "short"):
        assert np.sum(np.any(out[f"{g}/spec"] == 0, axis=1)) >= 3, g
    print("float32 rows, reference against the float64-log10 model: worst", WORST["f32"], "=", WORST["f32"] * 2 ** 24,
          "* 2^-24; float64 rows: worst", WORST["f64"])
    assert WORST["f32"] <= 4 * 2.0 ** -24 and WORST["f64"] <= 1e-12
    out["model_worst"] = np.array([WORST["f32"], WORST["f64"]])

    w = mod.SpectrogramWaterfall(48000)
    names = list(WR.SCHEMES) + ["grey"]
    for p, dt in (("f32", np.float32), ("f64", np.float64)):
        g = grid(dt, np.random.default_rng(7))
        col = np.zeros((len(names), len(g), 3), np.uint8)
        for s, name in enumerate(names):
            w.color_scheme = name
            for i, v in enumerate(g):
                col[s, i] = w._spectrum_to_color(v)
        out[f"grid_{p}"] = g
        out[f"color_{p}"] = col
    rates, sizes = [48000, 96000, 44100, 32000], [2048, 16384, 2048, 2048]
    out["map_rates"] = np.array(rates, np.int64)
    out["map_sizes"] = np.array(sizes, np.int64)
    out["map_idx"] = np.array([mod.SpectrogramWaterfall(r, n).freq_indices for r, n in zip(rates, sizes)], np.int32)
    print("mapping", out["map_idx"].tolist(), "cells at 48 kHz / 2048:", len(mod.SpectrogramWaterfall(48000).display_freqs))
    out["versions"] = np.array([np.__version__])
    path = os.path.join(HERE, "waterfall.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
