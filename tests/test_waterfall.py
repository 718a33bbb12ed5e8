"""The spectrogram waterfall: tests/waterfall_ref.py against tests/golden/waterfall.npz (recorded from the reference's
own SpectrogramWaterfall and SpectrogramWaterfallPanel by tests/golden/gen_waterfall.py), the facade's host logic
against a fake library call, the ABI's argument checks, and omega_waterfall_rows / omega_waterfall_colors on the
device.

Bars. Exact: the mapping, the percentile stage on given (max, min) pairs, the colours on given intensities, flags and
argmax, chained against single calls. float64 rows: 1e-12 absolute (rows lie in [0, 1]; the device's log10 and the C
library's differ near 1e-15, a float32 slip would show at 1e-7); float64 dB values, peak and floor: 1e-12 of
max(1, |v|) (|dB| <= 200, a log10 ulp there is 3e-14). float32: the reference's chain uses the C library's log10f,
which is not correctly rounded, so bitwise parity is out of reach. The model (log10 in float64, rounded once) was
measured against the reference on 400 frames of 853 cells, amplitudes 1e-4..10 with zeros: worst 3 * 2^-24, and the
generator measures the same 3 * 2^-24 on the committed sequences. The bar on float32 rows is 8 * 2^-24 absolute -- room
for one more ulp in the percentile that sets the range, a hundred times below a wrong-bin or wrong-range error --
and float32 dB maxima, minima, peak and floor are held to the recorded values within 4 float32 ulps of their magnitude.

Observed on an MI355X over all golden groups (run with -s): float32 rows worst 3 * 2^-24, float32 stats worst 3 ulps;
float64 rows worst 2.2e-16, float64 stats worst 2.1e-16; every exact comparison equal.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import waterfall_ref as WR
from conftest import REPO, load_golden
from host_program import compile_host_program

GROUPS = ("a2048", "k129", "toggle", "range", "const", "short")
PREC = (("f32", np.float32), ("f64", np.float64))
F32_BAR = 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def G():
    return load_golden("waterfall")


def seq(G, g, p):
    """One recorded stream: spectra in precision p, the rows frame by frame, the stats and the settings."""
    spec = G[f"{g}/spec"]
    spec = spec if p == "f32" else WR.widen(spec)
    off, flat = G[f"{g}/row_off"], G[f"{g}/row_{p}"]
    rows = [flat[off[i]:off[i + 1]] for i in range(len(spec))]
    return spec, rows, G[f"{g}/stat_{p}"], G[f"{g}/lohi"], G[f"{g}/auto"], G[f"{g}/gain"]


def segments(lohi, auto, gain):
    """Runs of frames with one setting: (start, end, lo, hi, auto, gain)."""
    key = [(int(a), int(b), int(c), float(d)) for (a, b), c, d in zip(lohi, auto, gain)]
    out, s = [], 0
    for i in range(1, len(key) + 1):
        if i == len(key) or key[i] != key[s]:
            out.append((s, i) + key[s])
            s = i
    return out


def ulps32(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def check_against_golden(p, rows, stats, want_rows, want_stat, what):
    """Rows and stats (columns 1..4: dB max, dB min, peak, floor) against the recorded ones, at the module's bars."""
    worst = max(float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) for a, b in zip(rows, want_rows))
    got, want = np.asarray(stats)[:, 1:5], want_stat[:, 0:4]
    if p == "f64":
        sw = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
        print(f"{what}: rows worst {worst:.3g} (bar 1e-12), stats worst {sw:.3g} (bar 1e-12)")
        assert worst <= 1e-12 and sw <= 1e-12, (what, worst, sw)
    else:
        u = float(np.max(ulps32(got, want)))
        print(f"{what}: rows worst {worst * 2 ** 24:.3g} * 2^-24 (bar 8), stats worst {u:.3g} float32 ulps (bar 4)")
        assert worst <= F32_BAR and u <= 4, (what, worst, u)
    for a, b in zip(rows, want_rows):
        assert a.dtype == b.dtype and a.shape == b.shape, what


# ---- CPU ----

def test_ref_mapping_equals_golden(G):
    got = [WR.mapping(int(r), int(n), 20, 20000) for r, n in zip(G["map_rates"], G["map_sizes"])]
    assert got == [tuple(v) for v in G["map_idx"].tolist()] == [(1, 854), (4, 3414), (1, 929), (2, 1024)]


def test_library_mapping_equals_golden(G):
    from omega_gpu.spectrogram_waterfall import frequency_mapping
    for r, n, want in zip(G["map_rates"], G["map_sizes"], G["map_idx"]):
        assert frequency_mapping(int(r), int(n), 20, 20000) == tuple(want)
    rng = np.random.default_rng(4)
    for _ in range(200):  # any range, any rate: numpy's linspace and argmax
        fs, n = int(rng.choice([8000, 22050, 44100, 48000, 96000, 192000])), int(rng.choice([2, 3, 256, 1000, 2048, 16384]))
        lo, hi = float(rng.uniform(0, fs)), float(rng.uniform(0, fs))
        assert frequency_mapping(fs, n, lo, hi) == WR.mapping(fs, n, lo, hi), (fs, n, lo, hi)


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("p,dt", PREC)
def test_ref_percentile_stage_equals_golden(G, g, p, dt):
    """np.percentile's types on the recorded (max, min) pairs: peak and floor bit for bit."""
    _, _, stat, _, auto, _ = seq(G, g, p)
    peak, floor = WR.percentile_stage(stat[:, 0], stat[:, 1], dt)
    on = auto != 0
    assert peak.dtype == dt
    np.testing.assert_array_equal(peak[on].astype(np.float64), stat[on, 2])
    np.testing.assert_array_equal(floor[on].astype(np.float64), stat[on, 3])


@pytest.mark.parametrize("p", ("f32", "f64"))
def test_ref_colors_equal_golden(G, p):
    g = G[f"grid_{p}"]
    assert len(g) == 2 + 15 + 256 + 2000 and g[0] == 0 and g[1] == 1
    for s in range(5):
        np.testing.assert_array_equal(WR.colors(g, s), G[f"color_{p}"][s], err_msg=f"scheme {s}")


def ref_stream(spec, lohi, auto, gain):
    wf, rows, stats = WR.Waterfall(), [], []
    for s, e, lo, hi, a, g in segments(lohi, auto, gain):
        st, r = WR.run(spec[s:e], lo, hi, bool(a), g, wf)
        rows += list(r)
        stats.append(st)
    return rows, np.concatenate(stats)


@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("p", ("f32", "f64"))
def test_ref_rows_against_golden(G, g, p):
    spec, want_rows, want_stat, lohi, auto, gain = seq(G, g, p)
    rows, stats = ref_stream(spec, lohi, auto, gain)
    check_against_golden(p, rows, stats, want_rows, want_stat, f"ref {g} {p}")
    freqs = np.linspace(0, 24000, int(G[f"{g}/fft_size"]) // 2 + 1)
    np.testing.assert_array_equal(freqs[stats[:, 5].astype(int)], want_stat[:, 4])
    np.testing.assert_array_equal(stats[:, 6], want_stat[:, 5])


def test_golden_covers_the_cases(G):
    assert G["a2048/spec"].shape == (30, 1025) and tuple(G["a2048/lohi"][0]) == (1, 854)
    assert G["k129/spec"].shape == (60, 129) and G["k129/spec"].max() > 5 and 0 < G["k129/spec"][G["k129/spec"] > 0].min() < 1e-3
    assert list(G["toggle/auto"]) == [1] * 8 + [0] * 8 + [1] * 8 and sorted(set(G["toggle/gain"])) == [-3.5, 0.0, 6.0]
    assert len(set(map(tuple, G["range/lohi"]))) == 2
    assert not np.any(G["const/row_f32"]) and np.all(G["const/stat_f64"][:, 2] == G["const/stat_f64"][:, 3])
    assert G["short/spec"].shape[1] == 513 and tuple(G["short/lohi"][0]) == (1, 854)
    for g in GROUPS[:4] + ("short",):
        assert np.sum(np.any(G[f"{g}/spec"] == 0, axis=1)) >= 3
    assert G["model_worst"][0] <= 4 * 2.0 ** -24
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "waterfall.npz")) < 1 << 20


class FakeLibrary:
    """Stands in for the facade's two library calls: tests/waterfall_ref.py on the host."""

    def __init__(self, w):
        self.w, self.ref, self.color_calls = w, WR.Waterfall(), []
        w._rows = self.rows
        w._colorize_rows = self.colorize

    def rows(self, spectra):
        from omega_gpu.spectrogram_waterfall import scheme_id
        spectra = np.asarray(spectra)
        if spectra.dtype not in (np.float32, np.float64):
            spectra = spectra.astype(np.float64)
        lo, hi = self.w.freq_indices
        stats, rows = WR.run(spectra, lo, hi, self.w.auto_gain, self.w.gain_adjustment, self.ref)
        return stats, rows, WR.colors(rows, scheme_id(self.w.color_scheme)), np.zeros(45)

    def colorize(self, rows, sid):
        self.color_calls.append((rows.shape, sid))
        return WR.colors(rows, sid)


def host_panel():
    from omega_gpu.spectrogram_waterfall import SpectrogramWaterfall, SpectrogramWaterfallPanel
    p = SpectrogramWaterfallPanel.__new__(SpectrogramWaterfallPanel)
    p._host_init(48000)
    p.waterfall = SpectrogramWaterfall.__new__(SpectrogramWaterfall)
    p.waterfall._host_init(48000, 256)
    return p, FakeLibrary(p.waterfall)


def test_facade_host_logic(G):
    spec = G["k129/spec"]
    freqs = np.linspace(0, 24000, 129)
    p, fake = host_panel()
    w = p.waterfall
    assert w.freq_indices == (1, 107) and len(w.display_freqs) == 106 and w.waterfall_data.maxlen == 200
    assert (w.current_peak, w.current_floor, w.auto_gain, w.gain_adjustment, w.color_scheme) == (0.0, -80.0, True, 0.0, 'spectrum')
    # update_interval: every third call reaches the library; empty input and None count but do nothing
    w.update_interval = 3
    for i in range(7):
        p.update(spec[i], freqs)
    assert w.update_counter == 7 and len(w.waterfall_data) == 2 and len(w.peak_history) == 2
    np.testing.assert_array_equal(w.waterfall_data[1], WR.run(spec[[2, 5]], 1, 107)[1][1])
    assert p.get_results()['peak_freq'] == freqs[np.argmax(spec[6])] and p.get_results()['peak_magnitude'] == spec[6].max()
    w.update(np.zeros(0, np.float32), freqs)
    w.update(None, freqs)
    assert w.update_counter == 9 and len(w.waterfall_data) == 2
    w.update_interval = 1
    # pause: nothing moves, not even the counter
    p.toggle_pause()
    p.update(spec[7], freqs)
    assert p.paused and w.update_counter == 9
    p.toggle_pause()
    # the deque keeps 200 rows, peak_history 100; the types are the input's
    for i in range(205):
        p.update(spec[i % 60], freqs)
    assert len(w.waterfall_data) == 200 and len(w.peak_history) == 100 and len(w._colors) == 200
    assert w.waterfall_data[-1].dtype == np.float32 and isinstance(w.current_peak, np.float32)
    assert isinstance(w.peak_history[-1][0], np.float32)
    assert p.get_image().shape == (200, 106, 3) and not fake.color_calls
    # scheme cycling, and the colours made again in one call
    seen = []
    for _ in range(4):
        p.cycle_color_scheme()
        seen.append((w.color_scheme, p.get_results()['color_scheme']))
    assert seen == [(s, s) for s in ('hot', 'cool', 'viridis', 'spectrum')]
    w.set_color_scheme('nope')
    assert w.color_scheme == 'spectrum'
    p.cycle_color_scheme()
    img = p.get_image()
    assert fake.color_calls == [((200, 106), 1)]
    np.testing.assert_array_equal(img, WR.colors(np.stack(list(w.waterfall_data)), 1))
    p.get_image()
    assert len(fake.color_calls) == 1  # (cached)
    # a range change: rows of two lengths, the shorter padded with black; the history stays
    w.set_frequency_range(1000, 8000)
    assert w.freq_indices == WR.mapping(48000, 256, 1000, 8000) and w.min_freq == 1000
    p.update(spec[0], freqs)
    img = p.get_image()
    k = w.freq_indices[1] - w.freq_indices[0]
    assert img.shape == (200, 106, 3) and len(w.waterfall_data[-1]) == k and not np.any(img[-1, k:]) and len(w.peak_history) == 100
    p.reset_view()
    assert w.freq_indices == (1, 107) and w.gain_adjustment == 0.0
    # gain, auto gain, scale, labels
    p.adjust_gain(2.5)
    p.adjust_gain(1.0)
    assert w.gain_adjustment == 3.5
    w.toggle_auto_gain()
    before = (w.current_peak, w.current_floor)
    p.update(spec[3], freqs)
    assert not w.auto_gain and (w.current_peak, w.current_floor) == before
    labels = w.get_frequency_labels(300)
    assert [t for _, _, t in labels] == ['20', '50', '100', '200', '500', '1k', '2k', '5k', '10k', '20k']
    assert labels[0][1] == 300 and labels[-1][1] == 0 and labels[5][1] == int(300 * (1.0 - (math.log10(1000) - math.log10(20)) / (math.log10(20000) - math.log10(20))))
    p.toggle_frequency_scale()
    assert w.freq_scale == 'linear' and w._frequency_to_display_y(10010.0, 100) == 50
    assert [t for _, _, t in w.get_frequency_labels(100)][:2] == ['20', '2.2k']
    w.set_frequency_scale('bark')
    assert w.freq_scale == 'linear'
    # a non-finite frame is skipped
    n = len(w.peak_history), w.update_counter
    bad = spec[1].copy()
    bad[5] = np.inf
    info = p.get_results()
    p.update(bad, freqs)
    assert w.skipped_nonfinite == 1 and len(w.peak_history) == n[0] and w.update_counter == n[1] + 1 and p.get_results() == info
    w.clear_waterfall()
    assert len(w.waterfall_data) == 0 and p.get_image().shape == (0, 0, 3)
    w.reset()
    assert (w.current_peak, w.current_floor, len(w.peak_history), w._state) == (0.0, -80.0, 0, None)
    with pytest.raises(ValueError):
        w._configure(1)  # a one-bin spectrum leaves [1:1]


def test_facade_update_batch_equals_updates_on_the_host(G):
    spec = WR.widen(G["toggle/spec"])
    freqs = np.linspace(0, 24000, 129)
    (a, _), (b, _) = host_panel(), host_panel()
    a.waterfall.update_interval = b.waterfall.update_interval = 2
    for x in spec:
        a.waterfall.update(x, freqs)
    b.waterfall.update_batch(spec[:5])
    b.waterfall.update_batch(spec[5:])
    assert len(a.waterfall.waterfall_data) == 12 == len(b.waterfall.waterfall_data) and a.waterfall.update_counter == b.waterfall.update_counter
    for x, y in zip(a.waterfall.waterfall_data, b.waterfall.waterfall_data):
        np.testing.assert_array_equal(x, y)
    assert a.waterfall.current_peak == b.waterfall.current_peak and isinstance(b.waterfall.current_peak, np.float64)
    b.waterfall.update_batch(spec[:4].astype(np.float16).astype(np.int32) + 1)  # integers are widened to float64
    assert b.waterfall.waterfall_data[-1].dtype == np.float64


def test_abi_checks_its_arguments_without_a_device(tmp_path):
    """tests/abi/waterfall_args.cpp: the mapping, the refusals of configure, rows and colors, and the state size."""
    lib = os.path.join(REPO, "audio-analyzer-omega_amd", "lib")
    exe = compile_host_program(os.path.join(REPO, "tests", "abi", "waterfall_args.cpp"), str(tmp_path / "waterfall_args"))
    env = dict(os.environ, LD_LIBRARY_PATH=lib + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, os.path.join(lib, "libomega.so")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout


# ---- GPU ----

@pytest.fixture(scope="module")
def wf():
    from omega_gpu import SpectrogramWaterfall
    return SpectrogramWaterfall(48000)


def dev_rows(wf, spec, lo, cells, auto=True, gain=0.0, scheme=0, state=None, rgb=True, stride=None, n_bins=None,
             state_out=True, code=0):
    """omega_waterfall_rows on host memory through the C entry point -> (stats, rows, rgb, state)."""
    from omega_gpu import _lib as L
    eng = wf._eng
    n = spec.shape[1] if n_bins is None else n_bins
    F = len(spec) if stride is None else (spec.size - n) // stride + 1
    eng._check(L.lib().omega_waterfall_configure(eng._ctx, C.byref(L.WaterfallConfig(n, lo, cells))))
    wf._configured = None
    spec = np.ascontiguousarray(spec)
    f64 = int(spec.dtype == np.float64)
    stats = np.full((F, 7), -7.0)
    rows = np.full((F, cells), -7, spec.dtype)
    img = np.full((F, cells, 3), 7, np.uint8) if rgb else None
    new = np.full(45, -7.0) if state_out is True else state_out
    r = L.lib().omega_waterfall_rows(eng._ctx, spec.ctypes.data, n if stride is None else stride, f64, F, int(auto), float(gain),
                                     scheme, None if state is None else state.ctypes.data,
                                     None if new is None else new.ctypes.data, stats.ctypes.data, rows.ctypes.data,
                                     None if img is None else img.ctypes.data, L.MEM_HOST)
    assert r == code, (r, L.lib().omega_last_error(eng._ctx))
    return stats, rows, img, new


def dev_colors(wf, x, scheme):
    from omega_gpu import _lib as L
    x = np.ascontiguousarray(x)
    out = np.empty(x.shape + (3,), np.uint8)
    wf._eng._check(L.lib().omega_waterfall_colors(wf._eng._ctx, x.ctypes.data, x.shape[1], int(x.dtype == np.float64),
                                                  x.shape[0], x.shape[1], scheme, out.ctypes.data, L.MEM_HOST))
    return out


def dev_stream(wf, spec, lohi, auto, gain, scheme=3):
    state, rows, stats, imgs = None, [], [], []
    for s, e, lo, hi, a, g in segments(lohi, auto, gain):
        n = spec.shape[1]
        lo, hi = min(lo, n), min(hi, n)
        st, r, img, state = dev_rows(wf, spec[s:e], lo, hi - lo, a, g, scheme, state)
        rows += list(r)
        imgs += list(img)
        stats.append(st)
    return rows, np.concatenate(stats), imgs


def check_percentiles(stats, dt, auto=True):
    """stats' peak and floor are the restatement's percentile of stats' own maxima and minima, bit for bit."""
    live = stats[:, 0] == 0
    peak, floor = WR.percentile_stage(stats[live, 1], stats[live, 2], dt)
    np.testing.assert_array_equal(stats[live, 3], peak.astype(np.float64))
    np.testing.assert_array_equal(stats[live, 4], floor.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("p,dt", PREC)
def test_device_rows_against_golden(G, wf, g, p, dt):
    spec, want_rows, want_stat, lohi, auto, gain = seq(G, g, p)
    rows, stats, imgs = dev_stream(wf, spec, lohi, auto, gain)
    check_against_golden(p, rows, stats, want_rows, want_stat, f"device {g} {p}")
    assert not np.any(stats[:, 0])
    np.testing.assert_array_equal(stats[:, 5], [np.argmax(x) for x in spec])
    np.testing.assert_array_equal(stats[:, 6], [x[np.argmax(x)] for x in spec])
    assert all(r.min() >= 0 and r.max() <= 1 for r in rows)
    if g != "toggle":
        check_percentiles(stats, dt)
    for r, img in zip(rows, imgs):  # the rows' colours: the colour kernel's and the restatement's on the device's rows
        np.testing.assert_array_equal(img, WR.colors(r, 3))
    np.testing.assert_array_equal(dev_colors(wf, np.stack(rows[:5]), 3), np.stack(imgs[:5]))


@pytest.mark.gpu
@pytest.mark.parametrize("p", ("f32", "f64"))
def test_device_colors_equal_golden(G, wf, p):
    g = G[f"grid_{p}"]
    for s in (0, 1, 2, 3, 4, 99, -1):
        want = G[f"color_{p}"][min(s, 4) if s >= 0 else 4]
        for width in (len(g), 7):  # one long row; rows of 7 cells, whose bytes start at every alignment
            x = g[:len(g) // width * width].reshape(-1, width)
            np.testing.assert_array_equal(dev_colors(wf, x, s).reshape(-1, 3), want[:x.size], err_msg=f"scheme {s} width {width}")
    import torch
    x = torch.from_numpy(np.stack([g, g[::-1]])).to("cuda:0")
    got = wf.colorize(x[:, 3:], 'hot').cpu().numpy()  # device memory, a strided view
    np.testing.assert_array_equal(got[0], G[f"color_{p}"][1][3:])
    np.testing.assert_array_equal(got[1], G[f"color_{p}"][1][::-1][3:])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", (np.float32, np.float64))
def test_device_rows_colours_in_every_scheme(G, wf, dt):
    spec = G["k129/spec"][:9].astype(dt)
    for s in range(5):
        st, rows, img, _ = dev_rows(wf, spec, 1, 106, scheme=s)
        np.testing.assert_array_equal(img, WR.colors(rows, s))
        np.testing.assert_array_equal(img, dev_colors(wf, rows, s))
    _, rows2, none, _ = dev_rows(wf, spec, 1, 106, rgb=False, scheme=77)
    np.testing.assert_array_equal(rows2, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("F", (1, 19, 20, 21, 45))
@pytest.mark.parametrize("dt", (np.float32, np.float64))
def test_chaining_is_bit_equal(G, wf, F, dt):
    """F frames in one call against the same frames split every 1, 7 and 20 frames through the blob; every output
    and the blob bit for bit, state_in and state_out in one buffer included."""
    spec = G["k129/spec"][:F].astype(dt)
    spec[F // 2, 3] = np.nan if F > 2 else spec[F // 2, 3]
    one = dev_rows(wf, spec, 1, 106, gain=1.5, scheme=1)
    for step in (1, 7, 20):
        buf, parts = None, []
        for s in range(0, F, step):
            if buf is None:
                out = dev_rows(wf, spec[s:s + step], 1, 106, gain=1.5, scheme=1)
                buf = out[3]
            else:
                out = dev_rows(wf, spec[s:s + step], 1, 106, gain=1.5, scheme=1, state=buf, state_out=buf)
            parts.append(out)
        for k in range(3):
            np.testing.assert_array_equal(np.concatenate([q[k] for q in parts]), one[k], err_msg=f"step {step} output {k}")
        np.testing.assert_array_equal(buf, one[3])
    if F == 45:
        assert np.count_nonzero(one[0][:, 0]) == 1
        check_percentiles(one[0], dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", (np.float32, np.float64))
def test_shapes(wf, dt):
    import torch
    from omega_gpu import SpectrogramWaterfall
    from omega_gpu import _lib as L
    rng = np.random.default_rng(21)
    for n, lo, cells in ((1, 0, 1), (70, 3, 63), (64, 0, 64), (70, 5, 65), (1025, 1, 853), (300, 0, 17), (300, 283, 17),
                         (8193, 0, 8193)):
        spec = (rng.random((3, n)) ** 4 * 3).astype(dt)
        spec[1, rng.integers(0, n)] = 0
        stats, rows, img, _ = dev_rows(wf, spec, lo, cells, scheme=0)
        want_stats, want_rows = WR.run(spec, lo, lo + cells)
        np.testing.assert_array_equal(stats[:, (0, 5, 6)], want_stats[:, (0, 5, 6)])
        bar = 1e-12 if dt == np.float64 else F32_BAR
        assert np.max(np.abs(rows.astype(np.float64) - want_rows)) <= bar, (n, lo, cells)
        check_percentiles(stats, dt)
        np.testing.assert_array_equal(img, WR.colors(rows, 0))
    # strided and overlapping rows, host and device memory
    n, lo, cells = 129, 1, 106
    flat = (rng.random(4000) ** 3).astype(dt)
    for stride in (200, 57):
        F = (flat.size - n) // stride + 1
        view = np.lib.stride_tricks.as_strided(flat, (F, n), (stride * flat.itemsize, flat.itemsize))
        base = dev_rows(wf, np.ascontiguousarray(view), lo, cells)
        got = dev_rows(wf, flat[None, :], lo, cells, stride=stride, n_bins=n)
        for a, b in zip(got, base):
            np.testing.assert_array_equal(a, b)
        w256 = SpectrogramWaterfall(48000, 256)  # (its mapping is [1, 107))
        t = torch.from_numpy(flat).to("cuda:0").unfold(0, n, stride)
        st, rw, im, state = w256.analyze_frames(t)
        for a, b in zip((st, rw, im, state), base):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
        st2, _, _, state2 = w256.analyze_frames(t, state)  # a device blob goes back in
        assert st2.shape == st.shape and state2[2] == 20
    assert L.lib().omega_waterfall_state_size() == 45


@pytest.mark.gpu
@pytest.mark.parametrize("dt", (np.float32, np.float64))
def test_cases(G, wf, dt):
    spec = G["k129/spec"][:30].astype(dt)
    # a flat spectrum: a zero row
    flat = np.full((4, 129), 0.125, dt)
    stats, rows, _, _ = dev_rows(wf, flat, 1, 106)
    assert not np.any(rows) and np.all(stats[:, 3] == stats[:, 4]) and np.all(stats[:, 1] == stats[:, 2])
    # all-zero input: -200 dB, peak == floor, a zero row, argmax 0
    stats, rows, img, _ = dev_rows(wf, np.zeros((3, 129), dt), 1, 106, scheme=2)
    assert np.all(stats[:, 1:5] == -200.0) and not np.any(rows) and not np.any(stats[:, 5:])
    np.testing.assert_array_equal(img, WR.colors(rows, 2))
    # a non-finite bin in the middle frame of five, outside the slice: flagged, zero row, the others as without it
    for badv in (np.nan, np.inf, -np.inf):
        five = spec[:5].copy()
        five[2, 120] = badv
        stats, rows, img, state = dev_rows(wf, five, 1, 106, scheme=0)
        s4, r4, i4, state4 = dev_rows(wf, five[[0, 1, 3, 4]], 1, 106, scheme=0)
        assert list(stats[:, 0]) == [0, 0, 1, 0, 0] and not np.any(stats[2, 1:]) and not np.any(rows[2])
        np.testing.assert_array_equal(img[2], WR.colors(rows[2], 0))
        for a, b in ((stats, s4), (rows, r4), (img, i4)):
            np.testing.assert_array_equal(a[[0, 1, 3, 4]], b)
        np.testing.assert_array_equal(state, state4)
    # every frame non-finite: no state yet
    allbad = spec[:2].copy()
    allbad[:, 0] = np.nan
    stats, _, _, state = dev_rows(wf, allbad, 1, 106)
    assert list(stats[:, 0]) == [1, 1] and not np.any(state)
    # auto_gain off from the start: peak 0, floor -80; a gain
    stats, rows, _, _ = dev_rows(wf, spec[:3], 1, 106, auto=False, gain=12.0)
    assert np.all(stats[:, 3] == 0.0) and np.all(stats[:, 4] == -80.0)
    want = WR.run(spec[:3], 1, 107, False, 12.0)[1]
    assert np.max(np.abs(rows.astype(np.float64) - want)) <= (1e-12 if dt == np.float64 else F32_BAR)
    assert np.any(rows == 1) and np.any((rows > 0) & (rows < 1))
    # a gain with auto gain, against the restatement; more than 20 frames of history
    stats, rows, _, state = dev_rows(wf, spec, 1, 106, gain=-7.25)
    want = WR.run(spec, 1, 107, True, -7.25)[1]
    assert np.max(np.abs(rows.astype(np.float64) - want)) <= (1e-12 if dt == np.float64 else F32_BAR)
    check_percentiles(stats, dt)
    assert state[0] == 1 and state[1] == (dt == np.float64) and state[2] == 20
    np.testing.assert_array_equal(state[3:23], stats[10:, 1])
    np.testing.assert_array_equal(state[23:43], stats[10:, 2])
    np.testing.assert_array_equal(state[43:], stats[-1, 3:5])
    # auto gain off behind a state: its peak and floor stay, the history goes on
    s2, _, _, state2 = dev_rows(wf, spec[:2], 1, 106, auto=False, state=state)
    assert np.all(s2[:, 3] == state[43]) and np.all(s2[:, 4] == state[44])
    np.testing.assert_array_equal(state2[3:21], state[5:23])
    # the state survives another slice
    s3, _, _, _ = dev_rows(wf, spec[:1], 40, 20, state=state)
    pk, fl = WR.percentile_pair([dt(v) for v in list(state[4:23]) + [s3[0, 1]]], [dt(v) for v in list(state[24:43]) + [s3[0, 2]]])
    assert s3[0, 3] == pk and s3[0, 4] == fl
    # ties in argmax take the first, anywhere in the spectrum
    tie = spec[:2].copy()
    tie[0, [7, 100, 128]] = 50
    tie[1, [128]] = 50
    tie[1, 0] = 50
    stats, _, _, _ = dev_rows(wf, tie, 1, 106)
    assert list(stats[:, 5]) == [7, 0] and list(stats[:, 6]) == [50, 50]
    # n_frames 0: the state passes through
    out = np.zeros(45)
    dev_rows(wf, spec[:0], 1, 106, state=state, state_out=out)
    np.testing.assert_array_equal(out, state)


@pytest.mark.gpu
def test_multi_launch_chain_is_bit_equal(wf):
    """A call of more than 65536 frames takes two launch pairs that hand the state on through the context's blobs:
    65537 frames of one bin, non-finite on both sides of the boundary."""
    F = 65537
    spec = (np.random.default_rng(5).random((F, 1), dtype=np.float32) + 0.01)
    spec[[65530, 65535, 65536], 0] = np.nan
    one = dev_rows(wf, spec, 0, 1, rgb=False)
    assert sorted(np.flatnonzero(one[0][:, 0])) == [65530, 65535, 65536]
    a = dev_rows(wf, spec[:65536], 0, 1, rgb=False)
    b = dev_rows(wf, spec[65536:], 0, 1, rgb=False, state=a[3])
    np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), one[0])
    np.testing.assert_array_equal(b[3], one[3])
    live = np.flatnonzero(one[0][:, 0] == 0)[-20:]
    np.testing.assert_array_equal(one[3][3:23], one[0][live, 1])


@pytest.mark.gpu
def test_refusals_leave_shape_and_outputs(G, wf):
    from omega_gpu import OmegaError, SpectrogramWaterfall, UnsupportedError
    from omega_gpu import _lib as L
    spec = G["k129/spec"][:4]
    base = dev_rows(wf, spec, 1, 106)
    eng = wf._eng
    fresh = SpectrogramWaterfall(48000)  # (a context of its own)
    assert fresh._eng is not eng
    with pytest.raises(OmegaError):  # unconfigured
        fresh._eng._check(L.lib().omega_waterfall_rows(fresh._eng._ctx, spec.ctypes.data, 129, 0, 4, 1, 0.0, 0, None, None,
                                                       base[0].ctypes.data, base[1].ctypes.data, None, L.MEM_HOST))
    for n, lo, cells in ((0, 0, 1), (8194, 0, 1), (129, 1, 129), (129, -1, 5), (129, 4, 0)):
        assert L.lib().omega_waterfall_configure(eng._ctx, C.byref(L.WaterfallConfig(n, lo, cells))) == L.EUNSUP
    with pytest.raises(UnsupportedError):
        wf.analyze_frames(np.zeros((1, 8194), np.float32))
    # the configured shape is still (129, 1, 106): a call without configuring again
    stats, rows = np.full((4, 7), -7.0), np.full((4, 106), -7, np.float32)
    args = (eng._ctx, spec.ctypes.data, 129, 0, 4, 1, 0.0, 0)
    assert L.lib().omega_waterfall_rows(*args, None, None, stats.ctypes.data, rows.ctypes.data, None, L.MEM_HOST) == 0
    np.testing.assert_array_equal(stats, base[0])
    np.testing.assert_array_equal(rows, base[1])
    # a blob of the other precision, and missing outputs: the stated code, nothing written
    stats[:], rows[:] = -7, -7
    out = np.full(45, -7.0)
    s64 = dev_rows(wf, spec.astype(np.float64), 1, 106)[3]
    assert L.lib().omega_waterfall_rows(*args, s64.ctypes.data, out.ctypes.data, stats.ctypes.data, rows.ctypes.data, None,
                                        L.MEM_HOST) == L.EUNSUP
    assert L.lib().omega_waterfall_rows(*args, None, out.ctypes.data, None, rows.ctypes.data, None, L.MEM_HOST) == L.EINVAL
    assert L.lib().omega_waterfall_rows(*args, None, out.ctypes.data, stats.ctypes.data, None, None, L.MEM_HOST) == L.EINVAL
    assert np.all(stats == -7) and np.all(rows == -7) and np.all(out == -7)
    import torch
    t64 = torch.from_numpy(s64).to("cuda:0")
    with pytest.raises(UnsupportedError):  # the same refusal for a blob in device memory
        wf.analyze_frames(torch.from_numpy(spec).to("cuda:0"), t64)
    np.testing.assert_array_equal(dev_rows(wf, spec, 1, 106)[1], base[1])


@pytest.mark.gpu
@pytest.mark.parametrize("p,dt", PREC)
def test_facade_on_device(G, p, dt):
    """update() frame by frame and update_batch() give the same deque as the golden; get_image() survives a scheme
    change and a range change; a precision change wants reset()."""
    from omega_gpu import SpectrogramWaterfallPanel, UnsupportedError
    spec, want_rows, want_stat, _, _, _ = seq(G, "a2048", p)
    freqs = np.linspace(0, 24000, 1025)
    a, b = SpectrogramWaterfallPanel(48000), SpectrogramWaterfallPanel(48000)
    for x in spec:
        a.update(x, freqs)
    b.waterfall.update_batch(spec[:11])
    b.waterfall.update_batch(spec[11:])
    assert len(a.waterfall.waterfall_data) == 30 == len(b.waterfall.waterfall_data)
    for x, y in zip(a.waterfall.waterfall_data, b.waterfall.waterfall_data):
        np.testing.assert_array_equal(x, y)
    hist = np.array([[0.0, float(h[0]), float(h[1]), want_stat[i, 2], want_stat[i, 3]]
                     for i, h in enumerate(a.waterfall.peak_history)])
    hist[-1, 3:] = float(a.waterfall.current_peak), float(a.waterfall.current_floor)
    check_against_golden(p, list(a.waterfall.waterfall_data), hist, want_rows, want_stat, f"facade {p}")
    assert a.waterfall.current_peak == b.waterfall.current_peak and isinstance(a.waterfall.current_peak, dt)
    assert a.get_results()['peak_freq'] == want_stat[-1, 4] and a.get_results()['peak_magnitude'] == want_stat[-1, 5]
    np.testing.assert_array_equal(a.get_image(), b.get_image())
    np.testing.assert_array_equal(a.get_image(), WR.colors(np.stack(list(a.waterfall.waterfall_data)), 0))
    a.cycle_color_scheme()
    a.cycle_color_scheme()
    a.cycle_color_scheme()
    np.testing.assert_array_equal(a.get_image(), WR.colors(np.stack(list(a.waterfall.waterfall_data)), 3))
    a.waterfall.set_frequency_range(200, 2000)
    a.update(spec[0], freqs)
    img = a.get_image()
    k = len(a.waterfall.waterfall_data[-1])
    assert img.shape == (31, 853, 3) and k == a.waterfall.freq_indices[1] - a.waterfall.freq_indices[0] < 853
    np.testing.assert_array_equal(img[-1, :k], WR.colors(a.waterfall.waterfall_data[-1], 3))
    assert not np.any(img[-1, k:])
    np.testing.assert_array_equal(img[:30], WR.colors(np.stack(list(a.waterfall.waterfall_data)[:30]), 3))
    other = spec[0].astype(np.float32 if dt == np.float64 else np.float64)
    with pytest.raises(UnsupportedError):
        a.update(other, freqs)
    a.waterfall.reset()
    a.update(other, freqs)
    assert len(a.waterfall.waterfall_data) == 1 and a.waterfall.waterfall_data[0].dtype == other.dtype
