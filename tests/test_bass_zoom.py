"""The bass zoom panel: tests/basszoom_ref.py and the library's mapping against tests/golden/basszoom.npz (recorded
from the reference's own BassZoomPanel by tests/golden/gen_basszoom.py), the facade's host logic against the two
recorded sequences, and omega_basszoom_features on the device against the golden rows.

Bars on the device. Flags and peak timestamps: equal. bass_max, scale_factor and each compressed value: 1e-9
relative to the row's own largest value, the project's float64 bar for transform-derived values. The generator
keeps every non-silent frame's bass_max at or above 1e-3 sum |x_n w_n|; a float64 evaluation of a bin in any
summation order is within about 8192 * 2^-53 = 9.1e-13 of sum |x_n w_n|, so within 9.1e-10 of bass_max at the very
worst and, with the errors of 8192 terms adding like a random walk, some 1e-14 in practice; log10 adds an ulp.
Bar values: 2^-21 absolute. Per step at most one float32 rounding can fall differently on a value below 2
(2^-23), one on 0.1 * bar (2^-26), plus 0.9e-9 from the input; these are carried forward with a factor of at most
0.6, so the total stays under 2.5 times the per-step sum, 3.4e-7 < 2^-21 = 4.8e-7. Peak values: 2^-19 absolute: a
peak starts with a bar's deviation and adds at most one 2^-24 rounding per 0.95 decay step, a geometric series
under 20 * 2^-24, together 1.7e-6 < 2^-19 = 1.9e-6. The generator keeps every bar > peak comparison's operands 2^-18
apart (or both clamped, or both zero) and every age 1e-6 s from the 3.0 s hold, so the timestamps are decidable.
Variants (float32 copies, device memory, strided and overlapping rows, another rate in between) and chained calls:
bitwise equal to the contiguous host float64 call.

The observed worst deviation per column is printed (run with -s).
Observed on an MI355X over all golden groups, host and device memory, float32 and float64 frames, strided and
overlapping rows (worst per column): bass_max 3.8e-16, scale_factor 1.65e-18, compressed 1.08e-16 of the row's
largest (bar 1e-9); bars 0 (bar 2^-21) and peaks 0 (bar 2^-19): every bar and peak bit-equal to the reference's;
flags and timestamps equal; the variants and chained calls bit-equal; both sequences through update() matched the
reference bit for bit after every step.
"""
import ctypes as C

import numpy as np
import pytest

import basszoom_ref as BR
from conftest import load_golden

RATES = (8000, 16000, 22050, 44100, 48000, 96000, 192000)
GROUPS = ("app", "s512", "s1000", "long", "one", "fs44", "fs22", "fs16", "fs8", "fs96", "fs192", "nonfinite")
SEQS = ("seq_hold", "seq_slow")
ROW_TOL, BAR_TOL, PEAK_TOL = 1e-9, 2.0 ** -21, 2.0 ** -19
WORST = {}


@pytest.fixture(scope="module")
def G():
    return load_golden("basszoom")


class Clock:
    T0 = 1000.0

    def __init__(self, step):
        self.t, self.step = self.T0, step

    def at(self, i):
        self.t = self.T0 + i * self.step

    def __call__(self):
        return self.t


def stream(G, g):
    """(fs, frames float64 [F, m], times [F]) of a group."""
    idx = G[f"{g}/idx"]
    pool = G["app/frame"] if g in SEQS else G[f"{g}/frame"]
    fs = 48000 if g in SEQS else int(G[f"{g}/fs"])
    return fs, pool[idx].astype(np.float64), Clock.T0 + np.arange(len(idx)) * float(G[f"{g}/clock_step"])


def host_panel(fs, clock):
    from omega_gpu.bass_zoom import BassZoomPanel
    p = BassZoomPanel.__new__(BassZoomPanel)
    p._host_init(fs, clock)
    return p


def note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))


def check(got, want, what):
    """(rows, bars, peaks, peak_times) against the golden's."""
    rows, bars, peaks, stamps = (np.asarray(v, np.float64) for v in got)
    wrows, wbars, wpeaks, wstamps = (np.asarray(v, np.float64) for v in want)
    assert rows.shape == wrows.shape and bars.shape == wbars.shape, what
    np.testing.assert_array_equal(rows[:, 0], wrows[:, 0], err_msg=f"{what}: flags")
    top = np.max(np.abs(wrows[:, 1:]), axis=1, keepdims=True)
    dev = np.abs(rows[:, 1:] - wrows[:, 1:]) / np.where(top > 0, top, 1.0)
    note("bass_max", dev[:, 0].max())
    note("scale_factor", dev[:, 1].max())
    note("compressed", dev[:, 2:].max())
    note("bars", np.abs(bars - wbars).max())
    note("peaks", np.abs(peaks - wpeaks).max())
    print(f"{what}: worst so far " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    assert dev.max() <= ROW_TOL, (what, "row", dev.max())
    assert np.abs(bars - wbars).max() <= BAR_TOL, (what, "bars", np.abs(bars - wbars).max())
    assert np.abs(peaks - wpeaks).max() <= PEAK_TOL, (what, "peaks", np.abs(peaks - wpeaks).max())
    np.testing.assert_array_equal(stamps, wstamps, err_msg=f"{what}: peak timestamps")


def golden_of(G, g):
    rows = G["app/row"][G[f"{g}/idx"]] if g in SEQS else G[f"{g}/row"]
    return rows, G[f"{g}/bars"], G[f"{g}/peaks"], G[f"{g}/peak_times"]


def library_mapping(fs):
    from omega_gpu import _lib as L
    n = (C.c_int32 * 4)()
    ranges, comp = np.zeros(128), np.zeros(64)
    a = C.addressof(n)
    code = L.lib().omega_basszoom_mapping(float(fs), a, a + 4, a + 8, a + 12, ranges.ctypes.data, comp.ctypes.data)
    return code, [int(v) for v in n], ranges, comp


# ---- CPU ----

@pytest.mark.parametrize("fs", RATES)
def test_mapping_matches_the_recorded_one(G, fs):
    want = G[f"map{fs}/freq_ranges"]
    first, per, valid = (int(G[f"map{fs}/{k}"]) for k in ("first_bin", "bins_per_bar", "n_valid"))
    code, (bars, lfirst, lper, lvalid), ranges, comp = library_mapping(fs)
    assert code == 0 and (bars, lfirst, lper, lvalid) == (len(want), first, per, valid)
    assert ranges[:2 * bars].tobytes() == want.tobytes()
    mp = BR.Mapping(fs)
    assert np.array(mp.freq_ranges).tobytes() == want.tobytes()
    np.testing.assert_array_equal(comp[:bars], mp.comp)
    p = host_panel(fs, Clock(1.0))
    assert p.bass_detail_bars == len(want) and np.array(p.bass_freq_ranges).tobytes() == want.tobytes()
    assert p.bass_bin_mapping == mp.groups
    assert p.bass_bin_mapping[0][0] == first and sum(len(g) for g in p.bass_bin_mapping) == valid
    assert p.bass_bar_values.dtype == np.float32 and p.bass_bar_values.shape == (len(want),)
    assert p.bass_peak_timestamps.dtype == np.float64
    assert list(p.get_results()) == ['bar_values', 'peak_values', 'freq_ranges', 'detail_bars']


def test_mapping_bar_and_bin_counts(G):
    counts = {fs: (len(G[f"map{fs}/freq_ranges"]), int(G[f"map{fs}/bins_per_bar"])) for fs in RATES}
    assert counts == {48000: (31, 1), 44100: (34, 1), 22050: (34, 2), 16000: (46, 2), 8000: (37, 5), 96000: (16, 1),
                      192000: (8, 1)}
    assert int(G["map8000/n_valid"]) == 184 and int(G["map48000/first_bin"]) == 4


def test_mapping_refusals():
    from omega_gpu import _lib as L
    from omega_gpu.bass_zoom import bass_mapping
    assert library_mapping(2.0e6)[0] == L.EUNSUP   # no bin in 20..200 Hz
    assert library_mapping(4000)[0] == L.EUNSUP    # 369 bins: over the cap
    for bad in (0.0, -48000.0, float("nan"), float("inf")):
        assert library_mapping(bad)[0] == L.EINVAL
    p = host_panel(2000000, Clock(1.0))
    assert p.bass_detail_bars == 1 and p.bass_freq_ranges == [(20, 200)] and p.bass_bin_mapping == [[]]
    assert len(p.bass_bar_values) == 64
    p.update(np.ones(8192))  # one bar that never moves, no device
    assert not np.any(p.bass_bar_values) and not np.any(p.bass_peak_values)
    with pytest.raises(L.UnsupportedError):
        bass_mapping(4000)


@pytest.mark.parametrize("g", GROUPS + SEQS)
def test_ref_equals_golden(G, g):
    fs, frames, times = stream(G, g)
    rows, bars, peaks, stamps, _ = BR.run(frames, times, BR.Mapping(fs))
    want = golden_of(G, g)
    np.testing.assert_array_equal(rows, want[0])
    assert bars.dtype == np.float32 and bars.tobytes() == np.ascontiguousarray(want[1]).tobytes()
    assert peaks.tobytes() == np.ascontiguousarray(want[2]).tobytes()
    np.testing.assert_array_equal(stamps, want[3])


def test_golden_covers_the_cases(G):
    r = G["app/row"]
    assert r[3, 2] == 0 and 0 < r[3, 1] < 0.1                    # scale factor exactly 0
    assert r[9, 1] == 0 and r[9, 2] == 1.0                        # exact silence
    assert 0.1 < r[2, 1] < 1
    assert np.any(r[0, 3:] > 1.0) and np.any(G["seq_hold/bars"] == 1.0)   # past the clamp; a clamped bar
    comp = BR.Mapping(48000).comp
    assert {comp[int(np.argmax(r[k, 3:]))] for k in (4, 5, 6, 7)} == {0.3, 0.6, 1.0, 0.8}
    assert list(G["nonfinite/row"][:, 0].astype(int)) == [0, 1, 0, 1, 0, 0]
    for seq in SEQS:
        pk, ts = G[f"{seq}/peaks"], G[f"{seq}/peak_times"]
        same = (ts[1:] == ts[:-1]) & (pk[:-1] > 0)
        assert np.any(same & (pk[1:] == pk[:-1])), (seq, "held")
        assert np.any(same & (pk[1:] == pk[:-1] * np.float32(0.95)) & (pk[1:] < pk[:-1])), (seq, "decaying")
    assert [G[f"{g}/frame"].shape[1] for g in ("s512", "s1000", "long", "one")] == [512, 1000, 16384, 1]


@pytest.mark.parametrize("seq", SEQS)
def test_host_logic_reproduces_sequence(G, seq):
    """The facade's host path on the recorded rows gives the reference's arrays after every step, bit for bit."""
    clock = Clock(float(G[f"{seq}/clock_step"]))
    p = host_panel(48000, clock)
    rows, bars, peaks, stamps = golden_of(G, seq)
    for i, row in enumerate(rows):
        clock.at(i)
        assert p._apply_row(row, clock())
        assert p.bass_bar_values.dtype == np.float32 and p.bass_bar_values.tobytes() == bars[i].tobytes(), (seq, i)
        assert p.bass_peak_values.tobytes() == peaks[i].tobytes(), (seq, i)
        np.testing.assert_array_equal(p.bass_peak_timestamps, stamps[i])
    bad = np.zeros(len(rows[0]))
    bad[0] = 1
    assert not p._apply_row(bad, clock()) and p.bass_bar_values.tobytes() == bars[-1].tobytes()


# ---- GPU ----

@pytest.fixture(scope="module")
def panels():
    from omega_gpu.bass_zoom import BassZoomPanel
    cache = {}

    def get(fs):
        if fs not in cache:
            cache[fs] = BassZoomPanel(fs)
        return cache[fs]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_device_rows(G, panels, g):
    fs, frames, times = stream(G, g)
    got = panels(fs).analyze_frames(frames, times)
    check(got[:4], golden_of(G, g), f"device {g}")
    nb = got[1].shape[1]
    state = got[4]
    np.testing.assert_array_equal(state[:nb], got[1][-1])
    np.testing.assert_array_equal(state[64:64 + nb], got[2][-1])
    np.testing.assert_array_equal(state[128:128 + nb], got[3][-1])
    assert not np.any(state[nb:64]) and not np.any(state[64 + nb:128]) and not np.any(state[128 + nb:])


def same(a, b):
    for x, y in zip(a, b):
        x = x.cpu().numpy() if hasattr(x, "cpu") else x
        y = y.cpu().numpy() if hasattr(y, "cpu") else y
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_device_variants(G, panels):
    """float32 copies of the (float32-representable) frames, device memory, strided and overlapping rows, and
    another rate configured in between give the contiguous host float64 call's bits."""
    import torch
    from omega_gpu import _lib as L
    fs, frames, times = stream(G, "app")
    p = panels(fs)
    base = p.analyze_frames(frames, times)
    same(p.analyze_frames(G["app/frame"], times), base)
    fs2, frames2, times2 = stream(G, "fs8")
    check(panels(fs2).analyze_frames(frames2, times2)[:4], golden_of(G, "fs8"), "device fs8 in between")
    # another rate through this very context, then back
    assert L.lib().omega_basszoom_configure(p._eng._ctx, C.byref(L.BassZoomConfig(8000.0, 4096))) == 0
    p._configured = None
    same(p.analyze_frames(frames, times), base)
    dfr = torch.zeros((len(frames), 8192 + 64), dtype=torch.float64, device="cuda:0")
    dfr[:, :8192] = torch.from_numpy(frames)
    same(p.analyze_frames(dfr[:, :8192], times), base)                       # strided rows, device memory
    same(p.analyze_frames(dfr[:, :8192].float(), torch.from_numpy(times).to("cuda:0")), base)
    line = torch.from_numpy(np.concatenate(frames[4:7])).to("cuda:0")
    view = line.unfold(0, 8192, 2048)                                         # overlapping rows
    tv = times[:view.shape[0]]
    got = p.analyze_frames(view, tv)
    same(got, p.analyze_frames(view.contiguous().cpu().numpy(), tv))
    want = BR.run(view.cpu().numpy(), tv, BR.Mapping(fs))
    check(tuple(v.cpu().numpy() for v in got[:4]), want[:4], "device overlapping")


@pytest.mark.gpu
@pytest.mark.parametrize("g", ("app", "nonfinite", "fs8"))
def test_chaining_is_bit_equal(G, panels, g):
    """F frames in one call against F one-frame calls chained through the blob, and against two halves."""
    fs, frames, times = stream(G, g)
    p = panels(fs)
    whole = p.analyze_frames(frames, times)
    st, parts = None, []
    for i in range(len(frames)):
        r = p.analyze_frames(frames[i:i + 1], times[i:i + 1], st)
        st = r[4]
        parts.append(r[:4])
    same([np.concatenate([q[k] for q in parts]) for k in range(4)] + [st], whole)
    a = p.analyze_frames(frames[:2], times[:2])
    b = p.analyze_frames(frames[2:], times[2:], a[4])
    same([np.concatenate([a[k], b[k]]) for k in range(4)] + [b[4]], whole)


@pytest.mark.gpu
@pytest.mark.parametrize("seq", SEQS)
def test_update_sequence_on_device(G, seq):
    from omega_gpu.bass_zoom import BassZoomPanel
    clock = Clock(float(G[f"{seq}/clock_step"]))
    p = BassZoomPanel(48000, clock=clock)
    _, frames, _ = stream(G, seq)
    _, bars, peaks, stamps = golden_of(G, seq)
    for i, x in enumerate(frames):
        clock.at(i)
        p.update(x, {"kick": 0.5})
        assert p.bass_bar_values.dtype == np.float32 and p.bass_peak_values.dtype == np.float32
        d = np.abs(p.bass_bar_values.astype(np.float64) - bars[i]).max()
        e = np.abs(p.bass_peak_values.astype(np.float64) - peaks[i]).max()
        note("seq bars", d)
        note("seq peaks", e)
        assert d <= BAR_TOL and e <= PEAK_TOL, (seq, i, d, e)
        np.testing.assert_array_equal(p.bass_peak_timestamps, stamps[i])
    print(f"{seq}: worst so far " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    assert p.drum_info == {"kick": 0.5} and p.get_results()["detail_bars"] == 31
    p.shutdown()


@pytest.mark.gpu
def test_nonfinite_update_leaves_state(G):
    from omega_gpu.bass_zoom import BassZoomPanel
    _, frames, _ = stream(G, "nonfinite")
    p = BassZoomPanel(48000, clock=Clock(1.0))
    p.update(frames[0])
    before = (p.bass_bar_values.copy(), p.bass_peak_values.copy(), p.bass_peak_timestamps.copy(), p._state.copy())
    assert np.any(before[0] > 0)
    p.update(frames[1])
    for got, want in zip((p.bass_bar_values, p.bass_peak_values, p.bass_peak_timestamps, p._state), before):
        np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_unsupported_shapes_leave_the_configured_one(G, panels):
    import omega_gpu
    from omega_gpu import _lib as L
    fs, frames, times = stream(G, "app")
    p = panels(fs)
    base = p.analyze_frames(frames, times)
    with pytest.raises(omega_gpu.UnsupportedError):
        p.analyze_frames(np.zeros((1, 0)), [0.0])
    for rate, m in ((48000.0, 0), (4000.0, 8192)):
        cfg = L.BassZoomConfig(rate, m)
        assert L.lib().omega_basszoom_configure(p._eng._ctx, C.byref(cfg)) == L.EUNSUP
    assert L.lib().omega_basszoom_configure(p._eng._ctx, C.byref(L.BassZoomConfig(-1.0, 8192))) == L.EINVAL
    assert p._configured == 8192
    same(p.analyze_frames(frames, times), base)
