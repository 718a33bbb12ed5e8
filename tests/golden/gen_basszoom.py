"""Makes tests/golden/basszoom.npz by calling the reference's BassZoomPanel (omega4/panels/bass_zoom.py:15-232)
itself (build container only; TEST INFRASTRUCTURE ONLY). Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_basszoom.py <reference checkout>

The reference module is loaded by path with ``pygame`` stubbed (the module imports it at the top; nothing is
drawn) and ``time.time`` replaced by a deterministic stepping clock. Each group is ONE stream: one reference panel
is built, and _process_bass_detail_internal and apply_bass_results are called here for every frame in order, so
that no thread timing enters; shutdown() ends the panel's worker. Frames hold 16-bit PCM values (k / 32768,
float32-representable) and are stored as float32. tests/basszoom_ref.py is asserted against the reference object
after every frame: bars and peaks bitwise, timestamps equal, and the mapping's freq_ranges bitwise.

Written per group g: g/fs, g/frame [P, m] float32 (the pool), g/idx [F] (the stream's frames as indices into the
pool), g/clock_step, g/row [F, 3 + bars], g/bars, g/peaks [F, bars] float32, g/peak_times [F, bars] float64. Per
rate: map<fs>/freq_ranges, /first_bin, /bins_per_bar, /n_valid.

  app        48 kHz, 8192 samples: a kick-like 55 Hz tone at 0.5 with a 110 Hz body (drives bars into the
             compression and the clamp), the same at 0.01, a frame whose bass_max lands in (0.1, 1), one with
             bass_max < 0.1 (scale factor exactly 0), 30 / 80 / 120 / 170 Hz tones (one per compensation class),
             white noise, exact silence (bass_max 0, scale 1.0), and three tones under white noise (for the sequences)
  short      frame_len 512 and 1000 (s512, s1000): zero-padded, hanning(n)
  long       frame_len 16384: truncated to the first 8192 samples
  one        frame_len 1
  fs44, fs22, fs16, fs8, fs96, fs192   34 x 1, 34 x 2, 46 x 2, 37 x 5 (184 bins, a short last bar), 16 and 8 bars
  nonfinite  a NaN sample and an infinite sample between finite frames: flags only, the stream passes them over
             (the reference is not fed them)
  seq_hold   300 steps over the app pool, the clock stepping 1001/60000 s (a 59.94 Hz display; at exactly 1/60 s the
             180th step after a peak would have an age within 1e-13 of 3.0, against the margin below): a loud
             stretch, then more than 3 s of quiet frames; peaks are set, held, and decay by 0.95 per step (all three
             asserted)
  seq_slow   the clock stepping 0.5 s: the hold expires after 7 steps

Margins, asserted here (conditions on the inputs, not measurements; a seed that misses one is skipped): every
non-silent frame has bass_max >= 1e-3 sum |x_n w_n|; every bar > peak comparison has its operands at least 2^-18
apart, or both clamped from pre-clamp values at least that far above 1.0, or both exactly 0; every now - timestamp
is at least 1e-6 s away from 3.0 -- or, in seq_slow alone, exactly 3.0: its times are multiples of 0.5 s from 1000.0,
so every time and every difference is exact in float64 and the sixth step's `> 3.0` is decided without rounding.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import basszoom_ref as BR  # noqa: E402

GAP = 2.0 ** -18
RATES = (8000, 16000, 22050, 44100, 48000, 96000, 192000)
EXPECT = {48000: (31, 1), 44100: (34, 1), 22050: (34, 2), 16000: (46, 2), 8000: (37, 5), 96000: (16, 1),
          192000: (8, 1)}


class Clock:
    """The time of step i is T0 + i * step, however often it is read."""
    T0 = 1000.0

    def __init__(self, step):
        self.t, self.step = self.T0, step

    def at(self, i):
        self.t = self.T0 + i * self.step

    def __call__(self):
        return self.t


def import_reference(path):
    sys.dont_write_bytecode = True
    pg = sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    pg.font = types.SimpleNamespace(Font=object)  # (named in the module's annotations only)
    pg.Surface = object
    spec = importlib.util.spec_from_file_location("ref_bass_zoom", os.path.join(path, "omega4", "panels", "bass_zoom.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BassZoomPanel


def pcm(x):
    return (np.round(np.asarray(x) * 32768) / 32768).astype(np.float32)


def run_stream(Ref, what, fs, pool, idx, clock_step):
    """One reference panel over pool[idx]; returns rows, bars, peaks, timestamps and the (set, held, decayed)
    counts. Non-finite frames are not fed to the reference."""
    import time
    clock = Clock(clock_step)
    time.time = clock
    ref = Ref(fs)
    try:
        mp = BR.Mapping(fs)
        assert ref.bass_detail_bars == mp.n_bars and ref.bass_bin_mapping == mp.groups, what
        assert [tuple(float(v).hex() for v in r) for r in ref.bass_freq_ranges] == \
            [tuple(float(v).hex() for v in r) for r in mp.freq_ranges], what
        state = BR.new_state()
        out = [[], [], [], []]
        seen = np.zeros(3, np.int64)
        for i, k in enumerate(idx):
            w = (what, i)
            clock.at(i)
            x = pool[k].astype(np.float64)
            row = BR.frame_row(x, mp)
            before_peaks = state[BR.MAX_BARS:BR.MAX_BARS + mp.n_bars].copy()
            before_stamps = state[2 * BR.MAX_BARS:2 * BR.MAX_BARS + mp.n_bars].copy()
            before_bars = state[:mp.n_bars].copy()
            bars, peaks, stamps, state = BR.step(state, row, clock(), mp.n_bars)
            if not int(row[0]):
                res = ref._process_bass_detail_internal(x)
                ref.latest_bass_result = res
                ref.apply_bass_results()
                assert ref.bass_bar_values.dtype == np.float32 and ref.bass_peak_values.dtype == np.float32, w
                assert np.array_equal(ref.bass_bar_values.view(np.uint32), bars.view(np.uint32)), w
                assert np.array_equal(ref.bass_peak_values.view(np.uint32), peaks.view(np.uint32)), w
                assert np.array_equal(ref.bass_peak_timestamps, stamps), w
                # the margins
                n = min(len(x), BR.N_FFT)
                l1 = np.sum(np.abs(x[:n] * np.hanning(n)))
                assert row[1] == 0 and l1 == 0 or row[1] >= 1e-3 * l1, (w, "bass_max against sum |x w|", row[1], l1)
                c = row[BR.ROW_HEAD:]
                rising = c > before_bars
                pre = np.where(rising, 0.1 * before_bars + 0.9 * c, 0.6 * before_bars + 0.4 * c)
                far = np.abs(bars.astype(np.float64) - before_peaks) >= GAP
                clamped = (pre >= 1.0 + GAP) & (before_peaks == 1.0)
                zero = (bars == 0) & (before_peaks == 0)
                assert np.all(far | clamped | zero), (w, "bar against peak")
                age = clock() - before_stamps
                exact = (age == 3.0) & (clock_step == 0.5)  # (multiples of 0.5 s: every time and difference is exact)
                assert np.all((np.abs(age - 3.0) >= 1e-6) | exact), (w, "hold time")
                higher = bars.astype(np.float64) > before_peaks
                seen += [np.count_nonzero(higher), np.count_nonzero(~higher & (age <= 3.0) & (before_peaks > 0)),
                         np.count_nonzero(~higher & (age > 3.0) & (before_peaks > 0))]
            else:
                assert np.array_equal(bars, before_bars.astype(np.float32)) and not np.any(row[1:]), w
            for o, v in zip(out, (row, bars, peaks, stamps)):
                o.append(v)
        return [np.array(o) for o in out], seen
    finally:
        ref.shutdown()


def record(Ref, out, group, fs, pool, idx=None, clock_step=1 / 60):
    pool = np.stack([np.asarray(x, np.float32) for x in pool])
    idx = np.arange(len(pool)) if idx is None else np.asarray(idx)
    (rows, bars, peaks, stamps), seen = run_stream(Ref, group, fs, pool, idx, clock_step)
    out[f"{group}/fs"] = np.int64(fs)
    out[f"{group}/frame"] = pool
    out[f"{group}/idx"] = idx.astype(np.int32)
    out[f"{group}/clock_step"] = np.float64(clock_step)
    out[f"{group}/row"] = rows
    out[f"{group}/bars"] = bars
    out[f"{group}/peaks"] = peaks
    out[f"{group}/peak_times"] = stamps
    return rows, bars, peaks, seen


def tone(fs, m, f, amp, rng, floor=0.01):
    """A tone over a noise floor (relative to the tone) that keeps every bar well away from 0."""
    t = np.arange(m) / fs
    return amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) + amp * floor * rng.standard_normal(m)


def app_pool(fs, m, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(m) / fs
    kick = 0.5 * np.sin(2 * np.pi * 55 * t + 0.3) + 0.8 * np.sin(2 * np.pi * 110 * t + 1.1) \
        + 0.004 * rng.standard_normal(m)
    return [pcm(kick), pcm(0.02 * kick), pcm(tone(fs, m, 120, 0.0004, rng, 0.05)),
            pcm(tone(fs, m, 120, 0.00004, rng, 0.05)), pcm(tone(fs, m, 30, 0.4, rng)), pcm(tone(fs, m, 80, 0.3, rng)),
            pcm(tone(fs, m, 120, 0.6, rng)), pcm(tone(fs, m, 170, 0.3, rng)), pcm(0.1 * rng.standard_normal(m)),
            np.zeros(m, np.float32)] + \
        [pcm(tone(fs, m, f, 0.01, rng, 0.0) + 0.1 * rng.standard_normal(m)) for f in (55, 120, 170)]


# the sequences' frames: broadband ones keep every bar's distance to its peak large; the tones and the kick move
# single bars through the compression and the clamp
LOUD, QUIET = (0, 4, 5, 6, 7, 8, 10, 11, 12), (3, 9)
DISPLAY_STEP = 1001 / 60000  # 59.94 frames per second


def first_seed(fn, what, seeds=range(1, 60)):
    for seed in seeds:
        try:
            r = fn(seed)
        except AssertionError as e:
            print(what, "seed", seed, "misses a margin:", str(e)[:160])
            continue
        print(what, "seed", seed)
        return r
    raise AssertionError(f"{what}: no seed keeps the margins")


def main(ref_path):
    Ref = import_reference(ref_path)
    out = {}
    for fs in RATES:
        mp = BR.Mapping(fs)
        assert (mp.n_bars, mp.bins_per_bar) == EXPECT[fs], (fs, mp.n_bars, mp.bins_per_bar)
        out[f"map{fs}/freq_ranges"] = np.array(mp.freq_ranges, np.float64)
        out[f"map{fs}/first_bin"] = np.int64(mp.first_bin)
        out[f"map{fs}/bins_per_bar"] = np.int64(mp.bins_per_bar)
        out[f"map{fs}/n_valid"] = np.int64(mp.n_valid)
    assert BR.Mapping(8000).n_valid == 184 and len(BR.Mapping(8000).groups[-1]) == 4

    def app(seed):
        rows, bars, _, _ = record(Ref, out, "app", 48000, app_pool(48000, 8192, seed))
        assert rows[0, 1] > 1000 and np.any(rows[0, 3:] > 1.0), rows[0, :3]          # compression past the clamp
        assert 0.1 < rows[2, 1] < 1 and 0 < rows[2, 2], rows[2, :3]
        assert 0 < rows[3, 1] < 0.1 and rows[3, 2] == 0, rows[3, :3]
        assert rows[9, 1] == 0 and rows[9, 2] == 1.0 and not np.any(rows[9, 3:]), rows[9, :3]
        comp = BR.Mapping(48000).comp
        assert [comp[int(np.argmax(rows[k, 3:]))] for k in (4, 5, 6, 7)] == [0.3, 0.6, 1.0, 0.8]
        return seed
    first_seed(app, "app")
    pool = list(out["app/frame"])
    for m in (512, 1000):
        first_seed(lambda s, m=m: record(Ref, out, f"s{m}", 48000, [p[:m] for p in app_pool(48000, 8192, s)[4:8]]),
                   f"s{m}")

    def long_(seed):
        rng = np.random.default_rng(seed)
        a, b = pcm(tone(48000, 16384, 120, 0.5, rng)), pcm(tone(48000, 16384, 60, 0.4, rng))
        a[8192:] = pcm(0.9 * rng.standard_normal(8192))  # the tail must not count
        rows, _, _, _ = record(Ref, out, "long", 48000, [a, b])
        assert np.array_equal(rows[0], BR.frame_row(a[:8192].astype(np.float64), BR.Mapping(48000)))
    first_seed(long_, "long")
    record(Ref, out, "one", 48000, [np.array([0.5], np.float32), np.array([-0.25], np.float32)])
    for name, fs in (("fs44", 44100), ("fs22", 22050), ("fs16", 16000), ("fs8", 8000), ("fs96", 96000),
                     ("fs192", 192000)):
        first_seed(lambda s, fs=fs, name=name: record(
            Ref, out, name, fs, [pcm(tone(fs, 4096, f, a, np.random.default_rng(s + j), 0.05))
                                 for j, (f, a) in enumerate(((45, 0.5), (130, 0.6), (90, 0.002)))]), name)
    bad_a, bad_b = pool[5].copy()[:2048], pool[6].copy()[:2048]
    bad_a[7] = np.nan
    bad_b[2047] = np.inf
    rows, _, _, _ = record(Ref, out, "nonfinite", 48000,
                           [pool[4][:2048], bad_a, pool[5][:2048], bad_b, pool[6][:2048], pool[9][:2048]])
    assert list(rows[:, 0].astype(int)) == [0, 1, 0, 1, 0, 0], rows[:, 0]

    def sequence(name, clock_step, seed, n_loud, n):
        rng = np.random.default_rng(seed)
        idx = np.concatenate([[8, 0, 0, 0], rng.choice(LOUD, n_loud - 4), rng.choice(QUIET, n - n_loud - 20),
                              rng.choice(LOUD, 20)])
        (rows, bars, peaks, stamps), seen = run_stream(Ref, name, 48000, out["app/frame"], idx, clock_step)
        assert np.all(seen > 0), (name, seen)
        assert np.any(bars == 1.0), (name, "a clamped bar")
        out[f"{name}/idx"] = idx.astype(np.int32)
        out[f"{name}/clock_step"] = np.float64(clock_step)
        out[f"{name}/bars"] = bars
        out[f"{name}/peaks"] = peaks
        out[f"{name}/peak_times"] = stamps
        print(name, "peaks set / held / decayed:", seen)
    first_seed(lambda s: sequence("seq_hold", DISPLAY_STEP, s, 60, 300), "seq_hold")
    first_seed(lambda s: sequence("seq_slow", 0.5, s, 10, 60), "seq_slow")
    out["versions"] = np.array([np.__version__])
    path = os.path.join(HERE, "basszoom.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
