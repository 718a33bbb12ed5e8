"""The professional meters panel: tests/meterpanel_ref.py and the library's pure entry points against
tests/golden/meterpanel.npz (recorded from the reference's own ProfessionalMetersPanel by
tests/golden/gen_meterpanel.py), and omega_meterpanel_update and the facade on the device.

Device rows against the recorded ones: hold value and counter, attack time, transients detected, flags, fill, sum
and histogram equal; the punch factor bitwise for float32 frames and within 1e-12 relative for float64 frames (the
project's float64 bar: the device's pairwise sum runs numpy's order, so what is left is the rounding of the square
root and the divide). End to end (the device's calculate_lufs feeds the panel) the momentary is held to 0.01 LU
(tests/test_gpu_parity.py:297, float64 Hann-windowed frames) and the true peak to 0.01 dB (tests/test_gpu_parity.py:18,
:298); the generator keeps every momentary ten times that from every edge and every compared pair of true peaks equal
or ten times that apart, so integers, histograms and counters are decidable. The worst float64 punch deviation seen is
printed (run with -s).
"""
import ctypes as C
import logging
import os
import subprocess

import numpy as np
import pytest

import meterpanel_ref as MR
from conftest import REPO, load_golden
from host_program import compile_host_program

LENS = (1, 2, 7, 8, 9, 129, 4800, 16383, 16384)
GROUPS = ("app", "app_f32", "edge", "edge_f32", "bins", "seq_hold", "seq_small") + \
    tuple(f"len{m}{s}" for m in LENS for s in ("", "_f32"))
LU_TOL, TP_TOL, PUNCH_TOL = 0.01, 0.01, 1e-12
WORST = {"punch64": 0.0}


@pytest.fixture(scope="module")
def G():
    return load_golden("meterpanel")


def stream(G, g):
    """The group's frames [F, m] in its dtype."""
    pool = G[str(G[f"{g}/pool"]) + "/frame"]
    return pool[G[f"{g}/idx"]].astype(np.float64 if int(G[f"{g}/f64"]) else np.float32)


def config(lens=(600, 300, 300), frame_len=2048, n_bins=60, lo=-60.0, hi=0.0, fs=48000.0):
    from omega_gpu import _lib as L
    return L.MeterPanelConfig(fs, frame_len, lens[0], lens[1], lens[2], n_bins, lo, hi)


def unpack(cfg, blob):
    from omega_gpu import _lib as L
    lv, pk, rg = (np.full(max(1, n), -7.0) for n in (cfg.level_len, cfg.peak_len, cfg.range_len))
    n = (C.c_int32 * 3)(-1, -1, -1)
    hold, tr = np.full(2, -7.0), np.full(3, -7.0)
    a = C.addressof(n)
    code = L.lib().omega_meterpanel_unpack(C.byref(cfg), blob.ctypes.data, lv.ctypes.data, a, pk.ctypes.data, a + 4,
                                           rg.ctypes.data, a + 8, hold.ctypes.data, tr.ctypes.data)
    return code, lv, pk, rg, list(n), hold, tr


# ---- CPU ----

@pytest.mark.parametrize("g", GROUPS)
def test_ref_equals_golden(G, g):
    rows, hist, p = MR.run(stream(G, g), G[f"{g}/meters"], G[f"{g}/hold_samples"], G[f"{g}/reset"],
                           level_len=int(G[f"{g}/lens"][0]), peak_len=int(G[f"{g}/lens"][1]),
                           range_len=int(G[f"{g}/lens"][2]))
    assert rows.tobytes() == G[f"{g}/rows"].tobytes() or np.array_equal(rows, G[f"{g}/rows"], equal_nan=True)
    np.testing.assert_array_equal(hist, G[f"{g}/hist"])
    for d, k in ((p.level, "level"), (p.peaks, "peaks"), (p.ranges, "ranges")):
        assert np.array(d, np.float64).tobytes() == G[f"{g}/{k}"].tobytes()


def test_golden_covers_the_cases(G):
    e = np.linspace(-60, 0, 61)
    m, h = G["bins/meters"][:, 0], G["bins/hist"].astype(np.int64)
    step = np.diff(np.vstack([np.zeros((1, 60), np.int64), h]), axis=0)  # (19 frames: the window never wraps)
    where = [int(np.argmax(s)) if s.any() else -1 for s in step]
    inf = np.inf
    want = {-60.0: 0, np.nextafter(-60.0, -inf): -1, np.nextafter(-60.0, inf): 0, -59.0: 1, np.nextafter(-59.0, -inf): 0,
            np.nextafter(-59.0, inf): 1, 0.0: 59, np.nextafter(0.0, -inf): 59, np.nextafter(0.0, inf): -1, 1e-9: -1,
            -100.0: -1, -23.0: 37, -59.999: 0}
    seen = set()
    for v, b in zip(m, where):
        if v != v:
            assert b == -1
            seen.add("nan")
        else:
            assert want[float(v)] == b, (v, b)
            seen.add(float(v))
    assert seen >= set(want) | {"nan"} and np.any(np.signbit(m) & (m == 0)) and e[37] == -23.0
    # the hold machine's branches: set, tie (counted down), one ulp above (set), expiry, NaN
    r, tp = G["bins/rows"], G["bins/meters"][:, 4]
    assert r[0, 0] == -10.0 and r[0, 1] == 3 and r[1, 1] == 2 and tp[1] == tp[0]
    assert r[2, 0] == np.nextafter(-10.0, inf) and r[2, 1] == 3
    assert np.any(np.isnan(tp)) and np.any(np.isnan(r[:, 0])) and np.any((r[1:, 1] <= 0) & (r[1:, 0] < r[:-1, 0]))
    c = G["seq_hold/rows"][:, 1]
    assert np.any(c == 0) and c.min() < -50 and np.any(c == 180) and G["seq_hold/reset"].sum() == 1
    assert set(G["seq_hold/hold_samples"]) == {60, 180, 0} and len(c) == 700
    assert list(G["seq_small/lens"]) == [5, 3, 3] and set(G["seq_small/hold_samples"]) == {2}
    # the carry: a frame without an attack repeats the three values of the one before
    er = G["edge/rows"]
    quiet = np.flatnonzero((er[1:, 5].astype(int) & 1) == 0) + 1
    assert len(quiet) >= 4 and np.array_equal(er[quiet, 2:5], er[quiet - 1, 2:5], equal_nan=True) and np.any(er[quiet, 4] > 0)
    assert G["edge/rows"][0, 5] == 1 and G["edge_f32/rows"][0, 5] == 0    # a difference of exactly float32(0.1)
    fl = G["edge_f32/rows"][:, 5].astype(int)
    assert np.any(fl & 2) and np.any(np.isnan(G["edge_f32/rows"][:, 3]))   # NaN: punch 0; infinite: punch NaN
    idx = list(G["edge/idx"])
    assert G["edge/rows"][idx.index(2), 2] == 0.0 and G["edge/rows"][idx.index(3), 2] == 14 / 48000 * 1000
    assert not np.any(G["len1/rows"][:, 5]) and np.all(G["len1/rows"][:, 6] == [1, 2, 3])
    for m_ in LENS[1:]:
        assert G[f"len{m_}/frame"].shape[1] == m_
    assert int(G["app/f64"]) == 1 and int(G["app_f32/f64"]) == 0 and G["app/frame"].shape[1] == 2048


@pytest.mark.parametrize("kw", [{}, {"n_bins": 61, "lo": -60.0, "hi": 0.1}, {"n_bins": 7, "lo": -1e-3, "hi": 5e9}])
def test_edges_equal_linspace(kw):
    from omega_gpu import _lib as L
    cfg = config(**kw)
    out = np.zeros(cfg.n_bins + 1)
    assert L.lib().omega_meterpanel_edges(C.byref(cfg), out.ctypes.data) == 0
    assert out.tobytes() == np.linspace(cfg.hist_lo, cfg.hist_hi, cfg.n_bins + 1).tobytes()


@pytest.mark.parametrize("g", ("seq_small", "seq_hold", "edge_f32", "bins"))
def test_state_size_and_unpack_round_trip(G, g):
    from omega_gpu import _lib as L
    lens = [int(v) for v in G[f"{g}/lens"]]
    cfg = config(lens)
    assert L.lib().omega_meterpanel_state_size(C.byref(cfg)) == MR.HEAD + sum(lens)
    frames = stream(G, g)
    for n in (0, 2, len(frames)):
        _, _, p = MR.run(frames[:n], G[f"{g}/meters"], G[f"{g}/hold_samples"], G[f"{g}/reset"], level_len=lens[0],
                         peak_len=lens[1], range_len=lens[2])
        blob = p.blob()
        assert len(blob) == MR.HEAD + sum(lens)
        code, lv, pk, rg, ns, hold, tr = unpack(cfg, blob)
        assert code == 0 and ns == [len(p.level), len(p.peaks), len(p.ranges)]
        for got, k, d in ((lv, 0, p.level), (pk, 1, p.peaks), (rg, 2, p.ranges)):
            assert got[:ns[k]].tobytes() == np.array(d, np.float64).tobytes() and np.all(got[ns[k]:] == -7.0)
        np.testing.assert_array_equal(hold, [p.hold, p.counter])
        np.testing.assert_array_equal(tr, [p.attack, p.punch, p.count])


def test_pure_entry_points_refuse():
    from omega_gpu import _lib as L
    lib = L.lib()
    out = np.full(64, -7.0)
    bad = [dict(fs=0.0), dict(fs=float("nan")), dict(fs=float("inf")), dict(frame_len=-1), dict(lens=(0, 300, 300)),
           dict(lens=(600, 4097, 300)), dict(lens=(600, 300, -1)), dict(n_bins=0), dict(n_bins=63),
           dict(lo=0.0, hi=0.0), dict(lo=1.0, hi=0.0), dict(lo=float("nan")), dict(hi=float("inf")),
           dict(lo=1.0, hi=np.nextafter(1.0, 2.0))]
    blob = MR.Panel().blob()
    for kw in bad:
        cfg = config(**kw)
        assert lib.omega_meterpanel_state_size(C.byref(cfg)) == L.EINVAL, kw
        assert lib.omega_meterpanel_edges(C.byref(cfg), out.ctypes.data) == L.EINVAL, kw
        assert unpack(cfg, blob)[0] == L.EINVAL, kw
    for m in (0, 16385):
        cfg = config(frame_len=m)
        assert lib.omega_meterpanel_state_size(C.byref(cfg)) == L.EUNSUP
        assert lib.omega_meterpanel_edges(C.byref(cfg), out.ctypes.data) == L.EUNSUP
    assert lib.omega_meterpanel_state_size(None) == L.EINVAL and lib.omega_meterpanel_edges(None, out.ctypes.data) == L.EINVAL
    assert lib.omega_meterpanel_edges(C.byref(config()), None) == L.EINVAL
    assert lib.omega_meterpanel_unpack(C.byref(config()), None, *([None] * 8)) == L.EINVAL
    assert np.all(out == -7.0)
    # a blob whose fills and slots are no ring's: refused, nothing written
    for slot, v in ((5, 601.0), (5, -1.0), (6, 600.0), (5, 2.5), (7, 301.0), (10, 300.0), (6, 3.0)):
        b = blob.copy()
        b[slot] = v
        code, lv, pk, rg, ns, hold, tr = unpack(config(), b)
        assert code == L.EINVAL and ns == [-1, -1, -1] and np.all(hold == -7.0) and np.all(lv == -7.0), (slot, v)
    d = L.MeterPanelConfig()
    lib.omega_meterpanel_config_default(C.byref(d))
    assert (d.sample_rate, d.frame_len, d.level_len, d.peak_len, d.range_len, d.n_bins, d.hist_lo, d.hist_hi) == \
        (48000.0, 2048, 600, 300, 300, 60, -60.0, 0.0)


def host_panel(fs=48000, **kw):
    from omega_gpu.professional_meters import ProfessionalMetersPanel
    p = ProfessionalMetersPanel.__new__(ProfessionalMetersPanel)
    p._host_init(fs, **kw)
    return p


def test_facade_pure_parts():
    import omega_gpu
    assert omega_gpu.ProfessionalMetersPanel and not hasattr(omega_gpu.ProfessionalMetersPanel, 'panel_rows') and "ProfessionalMetersPanel" in omega_gpu.__all__
    p = host_panel()
    # recorded from the reference's get_lufs_color / get_peak_color
    assert [p.get_lufs_color(v) for v in (-5, -9, -10, -14, -20, -23, -30, -35, -50)] == [
        (255, 100, 100), (255, 200, 100), (255, 200, 100), (100, 255, 100), (100, 255, 100), (180, 180, 255),
        (180, 180, 255), (120, 120, 120), (120, 120, 120)]
    assert [p.get_peak_color(v) for v in (0, -0.1, -1, -3, -5, -6, -10, -20, -40)] == [
        (255, 50, 50), (255, 150, 50), (255, 150, 50), (100, 255, 100), (100, 255, 100), (180, 200, 220),
        (180, 200, 220), (120, 120, 120), (120, 120, 120)]
    for s, want in ((1.0, 60), (3.0, 180), (0, 0), (-2.0, 0), (0.29, 17), (2.999, 179)):
        p.set_peak_hold_time(s)
        assert p.peak_hold_samples == want == int(max(0.0, s) * 60) and p.peak_hold_time == max(0.0, s)
    assert p.histogram_bins.tobytes() == np.linspace(-60, 0, 61).tobytes()
    assert not hasattr(p, "lufs_info") and not hasattr(p, "draw") and p.get_results()["lufs"] is None
    assert p.transient_info == {'attack_time': 0.0, 'punch_factor': 0.0, 'transients_detected': 0}
    assert p.peak_hold_value == -100.0 and p.peak_hold_counter == 0 and p.use_gated_measurement is True
    assert [d.maxlen for d in (p.level_history, p.true_peak_history, p.loudness_range_history)] == [600, 300, 300]
    assert len(p.level_history) == 0
    bins, hist = p.get_level_histogram()
    assert bins.tobytes() == np.linspace(-60, 0, 61)[:-1].tobytes() and hist.shape == (60,) and not hist.any()
    p.toggle_gating()
    assert p.use_gated_measurement is False
    p.set_fonts({'large': 1, 'small': 3})
    assert (p.font_large, p.font_medium, p.font_small, p.font_meters) == (1, None, 3, 3)
    # the histories, the hold and the counter read from a blob
    q = MR.Panel()
    for i in range(4):
        q.step(np.zeros(4), [-20.0 - i, 0, 0, 1.0 + i, -3.0 - i], 60)
    p._state = q.blob()
    assert list(p.level_history) == [-20.0, -21.0, -22.0, -23.0] and list(p.loudness_range_history) == [1, 2, 3, 4]
    assert list(p.true_peak_history) == [-3, -4, -5, -6] and p.peak_hold_value == -3.0 and p.peak_hold_counter == 57
    p.reset_peak_hold()
    assert p.peak_hold_value == -100.0 and p.peak_hold_counter == 0


def test_abi_checks_its_arguments_without_a_device(tmp_path):
    """tests/abi/meterpanel_args.cpp: every null / negative / oversize argument returns its code with a message and
    writes nothing."""
    lib = os.path.join(REPO, "audio-analyzer-omega_amd", "lib")
    exe = compile_host_program(os.path.join(REPO, "tests", "abi", "meterpanel_args.cpp"), str(tmp_path / "meterpanel_args"))
    env = dict(os.environ, LD_LIBRARY_PATH=lib + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe, os.path.join(lib, "libomega.so")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok"), r.stdout


# ---- GPU ----

@pytest.fixture(scope="module")
def panels():
    from omega_gpu.professional_meters import ProfessionalMetersPanel
    cache = {}

    def get(lens):
        lens = tuple(int(v) for v in lens)
        if lens not in cache:
            cache[lens] = ProfessionalMetersPanel(48000, level_len=lens[0], peak_len=lens[1], range_len=lens[2])
        return cache[lens]
    return get


def device_run(p, frames, meters, hold_samples, resets, state=None, hist=True):
    """The stream through panel_rows, one call per stretch of equal peak_hold_samples (a reset starts a stretch)."""
    rows, hists = [], []
    cuts = [0] + [i for i in range(1, len(frames)) if hold_samples[i] != hold_samples[i - 1] or resets[i]] + [len(frames)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        p.peak_hold_samples = int(hold_samples[a])
        r, h, state = p._panel_rows(frames[a:b], meters[a:b], state, bool(resets[a]), hist)
        rows.append(r)
        hists.append(h)
    cat = (lambda v: np.concatenate([x.cpu().numpy() if hasattr(x, "cpu") else x for x in v]))
    return cat(rows), (cat(hists) if hist else None), (state.cpu().numpy() if hasattr(state, "cpu") else state)


def check_rows(G, g, rows, hist, f64):
    want = G[f"{g}/rows"]
    for col in (0, 1, 2, 4, 5, 6, 7):
        np.testing.assert_array_equal(rows[:, col], want[:, col], err_msg=f"{g}: column {col}")
    if hist is not None:
        np.testing.assert_array_equal(hist, G[f"{g}/hist"], err_msg=f"{g}: histogram")
    if f64:
        ok = np.isfinite(want[:, 3]) & (want[:, 3] != 0)
        np.testing.assert_array_equal(rows[~ok, 3], want[~ok, 3])
        dev = np.max(np.abs(rows[ok, 3] / want[ok, 3] - 1), initial=0.0)
        WORST["punch64"] = max(WORST["punch64"], float(dev))
        print(f"{g}: float64 punch factor deviation {dev:.3g}, worst so far {WORST['punch64']:.3g}")
        assert dev <= PUNCH_TOL, (g, dev)
    else:
        np.testing.assert_array_equal(rows[:, 3].astype(np.float32).view(np.uint32)[~np.isnan(want[:, 3])],
                                      want[:, 3].astype(np.float32).view(np.uint32)[~np.isnan(want[:, 3])], err_msg=g)
        np.testing.assert_array_equal(np.isnan(rows[:, 3]), np.isnan(want[:, 3]))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_device_rows(G, panels, g):
    import torch
    p = panels(G[f"{g}/lens"])
    frames, f64 = stream(G, g), bool(int(G[f"{g}/f64"]))
    args = (G[f"{g}/meters"], G[f"{g}/hold_samples"], G[f"{g}/reset"])
    rows, hist, state = device_run(p, frames, *args)
    check_rows(G, g, rows, hist, f64)
    _, _, q = MR.run(frames, *args, level_len=p._cfg.level_len, peak_len=p._cfg.peak_len, range_len=p._cfg.range_len)
    want = q.blob()
    want[3] = rows[-1, 3]
    np.testing.assert_array_equal(state, want)
    drows, dhist, dstate = device_run(p, torch.from_numpy(frames).to("cuda:0"), *args)
    np.testing.assert_array_equal(drows, rows)
    np.testing.assert_array_equal(dhist, hist)
    np.testing.assert_array_equal(dstate, state)


ODD = dict(n_bins=7, lo=-61.3, hi=2.45)   # fractional edges, eight of them; 5 bins: tonal's genre keys 1..5


@pytest.mark.gpu
@pytest.mark.parametrize("kw", (ODD, dict(n_bins=5, lo=-47.25, hi=-3.5), dict(n_bins=62, lo=-60.5, hi=0.25)))
@pytest.mark.parametrize("g", ("seq_hold", "bins"))
def test_device_rows_other_edges(G, g, kw):
    """Edges that are no integers and other bin counts, on a context whose tonal table is configured first and read
    afterwards: the edges and the tonal tables do not share a slot of the context's table cache."""
    import torch
    from omega_gpu import _lib as L
    from omega_gpu.professional_meters import ProfessionalMetersPanel
    p = ProfessionalMetersPanel(48000, _n_bins=kw["n_bins"], _hist_lo=kw["lo"], _hist_hi=kw["hi"])
    lib, ctx = L.lib(), p._eng._ctx
    raw = np.abs(np.random.default_rng(3).standard_normal((4, 12)))
    raw /= raw.max(axis=1, keepdims=True)

    def tonal(genre):
        p._eng._check(lib.omega_tonal_configure(ctx, C.byref(L.TonalConfig(genre))))
        rows = np.empty((4, 52))
        p._eng._check(lib.omega_tonal_features(ctx, raw.ctypes.data, 4, None, None, None, None, rows.ctypes.data, None,
                                               None, None, None, L.MEM_HOST))
        return rows
    before = [tonal(gn) for gn in range(1, 6)]
    frames = stream(G, g)
    meters = G[f"{g}/meters"].copy()
    if g == "bins":  # the designed values moved onto these edges: each edge, its neighbours, outside, NaN
        e = np.linspace(kw["lo"], kw["hi"], kw["n_bins"] + 1)
        vals = [f(v) for v in (e[0], e[1], e[-1], e[len(e) // 2]) for f in
                (lambda v: v, lambda v: np.nextafter(v, -np.inf), lambda v: np.nextafter(v, np.inf))]
        meters[:, 0] = (vals + [np.nan, -100.0, 1e9, e[0] - 1.0, e[1], e[-1], 0.5 * (e[0] + e[1])])[:len(meters)]
    hs, rs = G[f"{g}/hold_samples"], G[f"{g}/reset"]
    want_rows, want_hist, q = MR.run(frames, meters, hs, rs, **kw)
    assert want_hist.shape[1] == kw["n_bins"] and want_hist.any()
    for fr in (frames, torch.from_numpy(frames).to("cuda:0")):
        rows, hist, state = device_run(p, fr, meters, hs, rs)
        np.testing.assert_array_equal(rows, want_rows)
        np.testing.assert_array_equal(hist, want_hist)
        np.testing.assert_array_equal(state, q.blob())
    for gn, b in zip(range(1, 6), before):
        np.testing.assert_array_equal(tonal(gn), b)
    assert p.histogram_bins.tobytes() == np.linspace(kw["lo"], kw["hi"], kw["n_bins"] + 1).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("g", ("seq_small", "seq_hold", "edge"))
def test_chaining_is_bit_equal(G, panels, g):
    import torch
    from omega_gpu import _lib as L
    p = panels(G[f"{g}/lens"])
    frames = stream(G, g)
    F = len(frames)
    meters, hs, rs = G[f"{g}/meters"], G[f"{g}/hold_samples"].copy(), np.zeros(F, np.int32)
    hs[:] = 2  # one peak_hold_samples for the whole stream: every split below is the same stream
    p.peak_hold_samples = 2
    whole = p._panel_rows(frames, meters)

    def chained(cuts):
        st, rows, hists = None, [], []
        for a, b in zip([0] + cuts, cuts + [F]):
            r, h, st = p._panel_rows(frames[a:b], meters[a:b], st)
            rows.append(r)
            hists.append(h)
        return np.concatenate(rows), np.concatenate(hists), st

    lens = sorted(set(int(v) for v in G[f"{g}/lens"]))
    splits = [list(range(1, F))] + [[c] for n in [1] + lens for c in (n, n + 1) if 0 < c < F]
    for cuts in splits:
        for got, want in zip(chained(cuts), whole):
            np.testing.assert_array_equal(got, want, err_msg=f"{g}: cuts {cuts[:3]}")
    # no histogram wanted: the rows and the state stay
    r, h, st = p._panel_rows(frames, meters, hist=False)
    assert h is None
    np.testing.assert_array_equal(r, whole[0])
    np.testing.assert_array_equal(st, whole[2])
    # state_out == state_in, in device memory
    half = F // 2
    a = p._panel_rows(frames[:half], meters[:half])
    blob = torch.from_numpy(a[2]).to("cuda:0")
    fr, mt = torch.from_numpy(frames[half:]).to("cuda:0"), torch.from_numpy(meters[half:]).to("cuda:0")
    rows = torch.empty((F - half, 8), dtype=torch.float64, device="cuda:0")
    hist = torch.empty((F - half, 60), dtype=torch.int32, device="cuda:0")
    p._eng._bind_stream(fr)
    p._eng._check(L.lib().omega_meterpanel_update(p._eng._ctx, fr.data_ptr(), frames.shape[1], int(frames.dtype == np.float64),
                                                  mt.data_ptr(), F - half, 2, 0, blob.data_ptr(), rows.data_ptr(),
                                                  hist.data_ptr(), blob.data_ptr(), L.MEM_DEVICE))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rows.cpu().numpy(), whole[0][half:])
    np.testing.assert_array_equal(hist.cpu().numpy(), whole[1][half:])
    np.testing.assert_array_equal(blob.cpu().numpy(), whole[2])


@pytest.mark.gpu
@pytest.mark.parametrize("g", ("seq_hold", "app"))
def test_update_sequence_on_device(G, g):
    from omega_gpu.professional_meters import ProfessionalMetersPanel
    frames = stream(G, g)
    want, wm, whist = G[f"{g}/rows"], G[f"{g}/meters"], G[f"{g}/hist"]
    hs, rs = G[f"{g}/hold_samples"], G[f"{g}/reset"]
    p, b = ProfessionalMetersPanel(48000), ProfessionalMetersPanel(48000)
    for i, x in enumerate(frames):
        if rs[i]:
            p.reset_peak_hold()
        p.peak_hold_samples = int(hs[i])
        p.update(x)
        w = (g, i)
        assert p.peak_hold_counter == want[i, 1], w
        assert abs(p.peak_hold_value - want[i, 0]) <= TP_TOL, (w, p.peak_hold_value, want[i, 0])
        assert abs(p.lufs_info["momentary"] - wm[i, 0]) <= LU_TOL and p.lufs_info is p.metering.current_lufs, w
        t = p.transient_info
        assert t['transients_detected'] == want[i, 4] and type(t['transients_detected']) is int, w
        assert t['attack_time'] == want[i, 2] and (want[i, 4] == 0 or type(t['attack_time']) is np.float64), w
        assert abs(t['punch_factor'] - want[i, 3]) <= PUNCH_TOL * abs(want[i, 3]), w
        if want[i, 3] != 0:
            assert type(t['punch_factor']) is np.float64, w
        counts = whist[i].astype(np.int64)
        np.testing.assert_array_equal(p.get_level_histogram()[1], counts / counts.sum() if counts.sum() else counts)
    for d, k, tol in ((p.level_history, "level", LU_TOL), (p.true_peak_history, "peaks", TP_TOL),
                      (p.loudness_range_history, "ranges", LU_TOL)):
        assert len(d) == len(G[f"{g}/{k}"]) and np.max(np.abs(np.array(d) - G[f"{g}/{k}"])) <= tol, (g, k)
    # update_batch over the stretches of equal settings equals the loop of update, bit for bit
    cuts = [0] + [i for i in range(1, len(frames)) if hs[i] != hs[i - 1] or rs[i]] + [len(frames)]
    for a, c in zip(cuts[:-1], cuts[1:]):
        if rs[a]:
            b.reset_peak_hold()
        b.peak_hold_samples = int(hs[a])
        rows, hist = b.update_batch(frames[a:c])
        assert rows.shape == (c - a, 8) and hist.shape == (c - a, 60)
    assert b._state.tobytes() == p._state.tobytes() and b.transient_info == p.transient_info
    assert b.lufs_info == p.lufs_info and list(b.level_history) == list(p.level_history)
    np.testing.assert_array_equal(b.get_level_histogram()[1], p.get_level_histogram()[1])
    np.testing.assert_array_equal(rows[-1, [1, 2, 4, 6, 7]], want[-1, [1, 2, 4, 6, 7]])


@pytest.mark.gpu
def test_panel_surface(G, caplog):
    from omega_gpu.professional_meters import ProfessionalMetersPanel
    frames = stream(G, "app")
    p, q = ProfessionalMetersPanel(48000), ProfessionalMetersPanel(48000)
    assert not hasattr(p, "lufs_info") and p.get_results() == {'lufs': None, 'transient': p.transient_info}
    assert not p.get_level_histogram()[1].any() and len(p.true_peak_history) == 0
    for x in frames[:3]:
        p.update(x)
    assert p.get_results()['lufs'] is p.lufs_info and set(p.lufs_info) == set(MR.KEYS)
    assert len(p.level_history) == 3 and len(q.level_history) == 0 and not hasattr(q, "lufs_info")  # no shared state
    assert p.peak_hold_value > -100.0 and p.transient_info['transients_detected'] > 0
    # an error path: the reference's filtfilt raises for a 5-sample frame; so does a frame above the cap
    before = (p._state.copy(), dict(p.transient_info), dict(p.lufs_info), p.get_level_histogram()[1].copy())
    for bad in (np.ones(5), np.zeros(16385)):
        with caplog.at_level(logging.ERROR):
            caplog.clear()
            p.update(bad)
        assert caplog.records, len(bad)
        assert p._state.tobytes() == before[0].tobytes() and p.transient_info == before[1] and p.lufs_info == before[2]
        np.testing.assert_array_equal(p.get_level_histogram()[1], before[3])
    q.update(frames[0])   # the failed updates left the stream where it was: p's next frame is q's second
    p.reset_peak_hold()
    assert p.peak_hold_value == -100.0 and p.peak_hold_counter == 0 and len(p.level_history) == 3
    p.update(frames[3])
    assert p.peak_hold_counter == p.peak_hold_samples == 60 or p.peak_hold_value == p.lufs_info["true_peak"]
    p.reset()
    assert not hasattr(p, "lufs_info") and len(p.level_history) == 0 and p.peak_hold_value == -100.0
    assert p.transient_info == {'attack_time': 0.0, 'punch_factor': 0.0, 'transients_detected': 0}
    p.update(frames[0])
    assert p._state.tobytes() == q._state.tobytes() and p.lufs_info == q.lufs_info


@pytest.mark.gpu
def test_unsupported_shapes_leave_the_configured_one(G, panels):
    import omega_gpu
    from omega_gpu import _lib as L
    p = panels((600, 300, 300))
    frames, meters = stream(G, "app"), G["app/meters"]
    p.peak_hold_samples = 60
    base = p._panel_rows(frames, meters)
    for m in (0, 16385):
        with pytest.raises(omega_gpu.UnsupportedError):
            p._panel_rows(np.zeros((1, m)), meters[:1])
        assert L.lib().omega_meterpanel_configure(p._eng._ctx, C.byref(config(frame_len=m))) == L.EUNSUP
        assert b"1..16384" in L.lib().omega_last_error(p._eng._ctx)
    for kw in (dict(fs=-1.0), dict(n_bins=63), dict(lens=(600, 300, 5000)), dict(lo=0.0, hi=-60.0)):
        assert L.lib().omega_meterpanel_configure(p._eng._ctx, C.byref(config(**kw))) == L.EINVAL, kw
    assert p._configured == 2048
    for got, want in zip(p._panel_rows(frames, meters), base):
        np.testing.assert_array_equal(got, want)
