"""§8(f) row 9: stereo phase correlation on the device (omega_phase_correlation through
omega_gpu.phase_correlation) against the reference's own outputs (tests/golden/phase.npz, recorded by
tests/golden/gen_phase.py with the group assertions and margins listed there) and the restatement
tests/phase_ref.py, which is pinned to the golden on the CPU.

Tolerances. Flags, the band mask and the goniometer points are exact (the points bit for bit); stereo_width
equals 1 - |correlation| of the device's own correlation. Correlation, the band correlations and balance are
held to 1e-9 absolute against the golden, the RMS columns to 1e-9 relative: the project's float64 bar for
device-FFT results (test_transients.py, test_hiphop.py). A float64 transform's error of about 1e-15 log2(m),
normwise, against the asserted 1e-5 magnitude-std margin moves a band correlation by about 1e-10. The observed
deviation is printed per column (run with -s).
Observed on an MI355X over all golden frames (worst per column): correlation 3.33e-16, balance 1.70e-16,
rms_left 1.79e-16 and rms_right 1.82e-16 relative, band correlations 1.19e-13 (the hard-panned app frame,
whose right channel lies 54 dB below the left; 1.42e-14 elsewhere); flags, mask and points equal on every
frame. The FFT error supposition held with four orders to spare.
"""
import ctypes as C
import functools
import hashlib
import json

import numpy as np
import pytest

import phase_ref as PR
from conftest import load_golden

GROUPS = ("app", "m64", "m512", "m8192", "fs44", "fs16", "zero", "nonfinite", "seq")
ATOL = RTOL = 1e-9
SIZES = ((48000, 64), (48000, 512), (48000, 2048), (48000, 8192), (44100, 2048), (16000, 1024))
SIZE_GROUP = dict(zip(SIZES, ("m64", "m512", "app", "m8192", "fs44", "fs16")))


@functools.lru_cache(maxsize=None)
def G():
    return load_golden("phase")


def group(name):
    g = G()
    return int(g[f"{name}/fs"]), int(g[f"{name}/m"]), [
        (g[f"{name}/{i}/left"], g[f"{name}/{i}/right"], g[f"{name}/{i}/row"], g[f"{name}/{i}/points"])
        for i in range(int(g[f"{name}/n"]))]


def check_row(tag, row, pts, ref_row, ref_pts, worst=None):
    """One device row and its points against the golden's."""
    assert row[5] == ref_row[5] and row[6] == ref_row[6], (tag, row[5:7], ref_row[5:7])
    np.testing.assert_array_equal(pts, ref_pts, err_msg=f"{tag} points")
    if int(ref_row[5]) & 1:  # non-finite input: the whole row is 0 beside the flag
        assert not np.delete(row, 5).any(), tag
        return
    assert row[1] == 1.0 - abs(row[0]), tag
    d = {"correlation": abs(row[0] - ref_row[0]), "balance": abs(row[2] - ref_row[2]),
         "bands": float(np.max(np.abs(row[7:] - ref_row[7:])))}
    for k, c in (("rms_left", 3), ("rms_right", 4)):
        d[k] = abs(row[c] - ref_row[c]) / ref_row[c] if ref_row[c] else abs(row[c])
    print(f"{tag} deviation from the golden:", {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
        assert v <= ATOL, (tag, k, v)
    assert np.all(np.abs(row[7:]) <= 1.0) and abs(row[0]) <= 1.0


def host_panel(fs=48000, m=2048):
    from omega_gpu.phase_correlation import PhaseCorrelation
    pc = PhaseCorrelation.__new__(PhaseCorrelation)  # (the constructor opens the device)
    pc._host_init(fs, m)
    return pc


# ---- CPU ----

@pytest.mark.parametrize("name", GROUPS)
def test_phase_ref_matches_reference_golden(name):
    """tests/phase_ref.py against the reference: every row and every point bit for bit."""
    fs, m, frames = group(name)
    np.testing.assert_array_equal(PR.band_edges(fs), G()[f"{name}/edges"])
    np.testing.assert_array_equal(PR.band_ranges(fs, m), G()[f"{name}/ranges"])
    for i, (l, r, row, pts) in enumerate(frames):
        got = PR.features(l, r, fs)
        np.testing.assert_array_equal(got[0], row, err_msg=f"{name} {i}")
        np.testing.assert_array_equal(got[1], pts, err_msg=f"{name} {i}")
        assert not pts[PR.n_points(m):].any()


@pytest.mark.parametrize("fs,m", SIZES)
def test_phase_band_ranges_are_numpys(fs, m):
    """omega_phase_band_ranges (no context, no device) against the recorded ranges of the numpy masks."""
    from omega_gpu import _lib as L
    g, name = G(), SIZE_GROUP[fs, m]
    assert (int(g[f"{name}/fs"]), int(g[f"{name}/m"])) == (fs, m)
    edges = np.ascontiguousarray(g[f"{name}/edges"], np.float64)
    out = np.full((10, 2), -1, np.int32)
    assert L.lib().omega_phase_band_ranges(fs, m, edges.ctypes.data, out.ctypes.data) == 0
    np.testing.assert_array_equal(out, g[f"{name}/ranges"])
    np.testing.assert_array_equal(host_panel(fs, m).band_frequencies, edges)


def test_phase_hanning_is_numpys():
    """The window the library uploads (numpy's route, 0.5 + 0.5 cos(pi k / (m - 1))) is np.hanning bit for bit:
    against the recorded sha256 of numpy's table for every recorded length."""
    from omega_gpu import _lib as L
    g = G()
    for m in (64, 512, 1024, 2048, 8192):
        w = np.empty(m)
        assert L.lib().omega_phase_hanning(m, w.ctypes.data) == 0
        assert hashlib.sha256(w.tobytes()).hexdigest() == str(g[f"hanning/{m}"]), m
    assert L.lib().omega_phase_hanning(1, w.ctypes.data) == L.EINVAL
    assert L.lib().omega_phase_hanning(64, None) == L.EINVAL


def test_phase_golden_group_assertions():
    """Each group does on the committed golden what it was made for."""
    g = G()
    rows = {n: [f[2] for f in group(n)[2]] for n in GROUPS}
    assert group("app")[:2] == (48000, 2048) and len(rows["app"]) == 6
    a = rows["app"]
    assert 0.2 < a[0][0] < 0.98 and a[1][0] == 1.0 and a[2][0] == -1.0 and 0 < a[3][0] < 0.999
    assert np.all(a[1][8:] >= 1 - 1e-12) and np.all(a[2][8:] >= 1 - 1e-12) and all(r[7] == 0.0 for r in a)
    assert a[4][2] < -0.99 and abs(a[5][2]) < 0.01 and abs(a[5][3] - 0.5) < 0.01
    assert all(r[5] == 0 and r[6] == 1023 for r in a)
    assert [group(n)[:2] for n in ("m64", "m512", "m8192", "fs44", "fs16")] == [
        (48000, 64), (48000, 512), (48000, 8192), (44100, 2048), (16000, 1024)]
    rg = g["m64/ranges"]
    assert all(rg[b, 0] == rg[b, 1] for b in range(5)) and rg[5, 1] - rg[5, 0] == 1
    assert all(int(r[6]) == 0b1111100000 and r[12] == 0.0 and not r[7:12].any() for r in rows["m64"])
    assert int(g["fs16/nyquist_in_band9"]) == int(g["fs16/ranges"][9, 1] == 513)
    z = rows["zero"]
    assert [r[5] for r in z] == [4, 4, 6] and all(r[0] == 0 and r[1] == 1 and not r[7:].any() for r in z)
    assert z[0][2] == -1 and z[1][2] == 1 and z[2][2] == 0
    assert all(r[5] == 1 and not np.delete(r, 5).any() for r in rows["nonfinite"])
    # the margins, on every frame with two live channels
    for n in GROUPS:
        fs, m, frames = group(n)
        for l, r, row, _ in frames:
            if int(row[5]) & 1 or not l.any() or not r.any():
                continue
            l, r = l.astype(np.float64), r.astype(np.float64)
            for x in (l, r):
                assert np.std(x) >= 1e-3 * np.sqrt(np.mean(x ** 2))
            w = np.hanning(m)
            ml, mr = np.abs(np.fft.rfft(l * w)), np.abs(np.fft.rfft(r * w))
            top = max(ml.max(), mr.max())
            for lo, hi in g[f"{n}/ranges"]:
                if hi - lo >= 2:
                    assert np.std(ml[lo:hi]) >= 1e-5 * top and np.std(mr[lo:hi]) >= 1e-5 * top
    # the sequences
    assert len(g["seq/idx"]) == 320 and g["seq/hist_len"].max() == 300 and (g["seq/hist_len"] == 300).sum() > 15
    assert (g["seq/warn"] & 1).any() and (g["seq/warn"] & 2).any() and (g["seq/warn"] == 0).any()
    assert np.all(g["seq/bands"][:, :5] == g["seq/init"][:5]) and g["seq/init"][:5].all()
    assert len(g["seq2048/idx"]) == 40 and g["seq2048/pers_len"].max() == 30
    assert json.loads(str(g["versions"]))["numpy"]


@pytest.mark.parametrize("name", ("seq", "seq2048"))
def test_phase_facade_host_state_machine(name):
    """The facade's host state from _host_init (no device), fed the golden rows and points of the recorded
    sequence, against the reference's recorded state after every frame: correlation_stats with the warnings
    verbatim, the history length, the kept balance, the kept bands, the persistence length and intensities,
    get_status()."""
    from omega_gpu.phase_correlation import COLUMNS, WARN_CANCEL, WARN_HIGH
    assert tuple(COLUMNS) == tuple(PR.COLUMNS)
    g = G()
    warn = json.loads(str(g["warnings"]))
    assert [WARN_HIGH, WARN_CANCEL] == warn
    pool = str(g[f"{name}/pool"])
    fs, m, frames = group(pool)
    pc = host_panel(fs, m)
    assert pc.correlation_history.maxlen == 300 and pc.gonio_max_frames == 30 and pc.gonio_decay_rate == 0.95
    assert pc.get_status() == {"correlation": 0.0, "stereo_width": 0.0, "balance": 0.0, "mono_compatible": True}
    pc.band_correlations = g[f"{name}/init"].copy()
    kept = 0
    for i, k in enumerate(g[f"{name}/idx"]):
        _, _, row, pts = frames[k]
        before = pc.balance
        pc._apply_row(row, pts, m)
        st = pc.correlation_stats
        assert list(st) == ["min", "max", "avg", "peak_hold_time", "warnings"] and st["peak_hold_time"] == 0
        assert (st["min"], st["max"], float(st["avg"])) == tuple(g[f"{name}/stats"][i]), i
        assert st["warnings"] == [w for b, w in enumerate(warn) if int(g[f"{name}/warn"][i]) >> b & 1], i
        assert len(pc.correlation_history) == g[f"{name}/hist_len"][i]
        np.testing.assert_array_equal(pc.band_correlations, g[f"{name}/bands"][i])
        s = pc.get_status()
        assert list(s) == ["correlation", "stereo_width", "balance", "mono_compatible"]
        assert (s["correlation"], s["stereo_width"], s["balance"], int(s["mono_compatible"])) == (
            g[f"{name}/corr"][i], g[f"{name}/width"][i], g[f"{name}/balance"][i], g[f"{name}/mono"][i]), i
        if int(row[5]) & 2:
            kept += pc.balance == before != 0
        assert len(pc.gonio_persistence) == g[f"{name}/pers_len"][i]
        assert [f["intensity"] for f in pc.gonio_persistence] == list(g[f"{name}/pers_int"][i][:len(pc.gonio_persistence)])
        cur = pc.gonio_persistence[-1]["points"]
        assert len(cur) == PR.n_points(m) and isinstance(cur[0], tuple)
        np.testing.assert_array_equal(np.asarray(cur), pts[:len(cur)])
    if name == "seq":
        assert kept >= 3
    # a non-finite row leaves the state as it was; a short frame is a no-op; reset_statistics
    row = np.zeros(17)
    row[5] = 1
    n = len(pc.correlation_history)
    pc._apply_row(row, np.zeros((128, 2)), m)
    pc.update(np.ones(100), np.ones(100))  # (returns before any device call)
    assert len(pc.correlation_history) == n
    pc.reset_statistics()
    assert not pc.correlation_history
    assert pc.correlation_stats == {"min": 0.0, "max": 0.0, "avg": 0.0, "peak_hold_time": 0, "warnings": []}


def test_phase_abi_argument_checks():
    """The entry points' argument checks that run before any device call, and the documented defaults."""
    from omega_gpu import _lib as L
    lib = L.lib()
    cfg = L.PhaseConfig()
    lib.omega_phase_config_default(C.byref(cfg))
    assert (cfg.sample_rate, cfg.m) == (48000, 2048)
    edges = PR.band_edges(48000)
    rg, x, out = np.empty((10, 2), np.int32), np.zeros(2048, np.float32), np.empty((1, 17))
    assert lib.omega_phase_band_ranges(0, 2048, edges.ctypes.data, rg.ctypes.data) == L.EINVAL
    assert lib.omega_phase_band_ranges(48000, 1, edges.ctypes.data, rg.ctypes.data) == L.EINVAL
    assert lib.omega_phase_band_ranges(48000, 2048, None, rg.ctypes.data) == L.EINVAL
    bad = edges.copy()
    bad[3] = np.nan
    assert lib.omega_phase_band_ranges(48000, 2048, bad.ctypes.data, rg.ctypes.data) == L.EINVAL
    assert lib.omega_phase_configure(None, C.byref(cfg), edges.ctypes.data) == L.EINVAL
    assert lib.omega_phase_correlation(None, x.ctypes.data, x.ctypes.data, 0, 2048, 1, out.ctypes.data, None,
                                       L.MEM_HOST) == L.EINVAL
    assert b"ABI 5" in lib.omega_version()  # (the entry points are additive)
    assert max(PR.n_points(1 << b) for b in range(6, 14)) == PR.N_POINTS == 128 and len(PR.COLUMNS) == 17


# ---- GPU ----

WORST = {}


def panel(name):
    from omega_gpu import PhaseCorrelation
    fs, m, _ = group(name)
    return PhaseCorrelation(fs, m)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUPS)
def test_phase_golden_parity(name):
    """Every frame of the group through omega_phase_correlation, singly and as one batch."""
    fs, m, frames = group(name)
    pc = panel(name)
    for i, (l, r, row, pts) in enumerate(frames):
        got = pc.analyze_frames(l[None], r[None])
        check_row(f"{name}[{i}]", got[0][0], got[1][0], row, pts, WORST)
    rows, points = pc.analyze_frames(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
    for i, (l, r, row, pts) in enumerate(frames):
        check_row(f"{name}[{i}] batched", rows[i], points[i], row, pts)
    assert not pc.correlation_history  # (analyze_frames keeps no state)
    print("worst so far:", {k: f"{v:.2e}" for k, v in WORST.items()})


@pytest.mark.gpu
def test_phase_constant_channel_is_finite():
    """A constant non-zero channel (left out of the parity groups: the reference's answer is rounding residue
    of its summation order) gives finite values in [-1, 1]."""
    _, m, frames = group("app")
    pc = panel("app")
    for c in (0.3, np.float32(0.1), 1e-30):
        k = np.full(m, c, np.float32)
        for l, r in ((k, frames[0][1]), (frames[0][0], k), (k, k)):
            row = pc.analyze_frames(l[None], r[None])[0][0]
            assert np.isfinite(row).all() and abs(row[0]) <= 1 and np.all(np.abs(row[7:]) <= 1) and not int(row[5]) & 1


@pytest.mark.gpu
def test_phase_batch_and_layouts():
    """One planar [64, 2, 2048] device-resident batch equals the same frames sent singly from the host, bit
    for bit; overlapping rows (frame_stride < m); a float64 call equals its float32-widened twin."""
    import torch
    _, m, frames = group("app")
    rng = np.random.default_rng(11)
    x = np.empty((64, 2, m), np.float32)
    for i in range(64):
        l, r = frames[i % 6][:2]
        x[i, 0], x[i, 1] = np.roll(l, 31 * i) * np.float32(0.5 + rng.random()), np.roll(r, 17 * i)
    pc = panel("app")
    xd = torch.from_numpy(x).cuda()
    rows, pts = pc.analyze_frames(xd[:, 0], xd[:, 1])
    assert rows.is_cuda and rows.shape == (64, 17) and pts.shape == (64, 128, 2)
    rows, pts = rows.cpu().numpy(), pts.cpu().numpy()
    for i in range(64):
        one = pc.analyze_frames(x[i, 0][None], x[i, 1][None])
        np.testing.assert_array_equal(one[0][0], rows[i], err_msg=f"frame {i}")
        np.testing.assert_array_equal(one[1][0], pts[i], err_msg=f"frame {i}")
    want = PR.features(x[63, 0], x[63, 1], 48000)
    check_row("batch[63]", rows[63], pts[63], want[0], want[1])
    # overlapping rows of two streams
    sl, sr = np.concatenate([x[0, 0], x[1, 0]]), np.concatenate([x[0, 1], x[1, 1]])
    vl, vr = (torch.from_numpy(s).cuda().unfold(0, m, 512) for s in (sl, sr))
    assert vl.stride(0) == 512 < m
    got = pc.analyze_frames(vl, vr)
    want = pc.analyze_frames(np.stack([sl[k * 512:k * 512 + m] for k in range(5)]),
                             np.stack([sr[k * 512:k * 512 + m] for k in range(5)]))
    for k in range(2):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k])
    # float64 input
    a = pc.analyze_frames(x[:3, 0].astype(np.float64), x[:3, 1].astype(np.float64))
    for k in range(2):
        np.testing.assert_array_equal(a[k], pc.analyze_frames(x[:3, 0], x[:3, 1])[k])
    y = x[5].astype(np.float64) * 1.000000123  # (not representable in float32)
    row, p = (v[0] for v in pc.analyze_frames(y[0][None], y[1][None]))
    want = PR.features(y[0], y[1], 48000)
    check_row("float64", row, p, want[0], want[1])


@pytest.mark.gpu
def test_phase_rejections_and_isolation():
    """OMEGA_EUNSUP for m 48 and 16384; a call before configure returns an error code; a non-finite frame in
    mid-batch is the zero row with flag bit 0 and leaves its neighbours' rows bit-equal."""
    from omega_gpu import PhaseCorrelation, UnsupportedError
    from omega_gpu import _lib as L
    lib = L.lib()
    pc = PhaseCorrelation(48000, 2048)
    ctx = pc._eng._ctx
    x, out = np.ones(16384, np.float32), np.empty((1, 17))
    assert lib.omega_phase_correlation(ctx, x.ctypes.data, x.ctypes.data, 0, 2048, 1, out.ctypes.data, None,
                                       L.MEM_HOST) == L.EINVAL
    assert b"omega_phase_configure" in lib.omega_last_error(ctx)
    edges = PR.band_edges(48000)
    for m in (48, 16384):
        cfg = L.PhaseConfig(48000, m)
        assert lib.omega_phase_configure(ctx, C.byref(cfg), edges.ctypes.data) == L.EUNSUP
        assert str(m).encode() in lib.omega_last_error(ctx)
        with pytest.raises(UnsupportedError, match=str(m)):
            pc.analyze_frames(np.ones((1, m), np.float32), np.ones((1, m), np.float32))
    _, m, frames = group("app")
    l = np.stack([f[0] for f in frames])
    r = np.stack([f[1] for f in frames])
    clean = pc.analyze_frames(l, r)
    l2, r2 = l.copy(), r.copy()
    l2[2, 1000] = np.nan
    r2[4, 0] = -np.inf
    got = pc.analyze_frames(l2, r2)
    for i in range(6):
        if i in (2, 4):
            assert got[0][i, 5] == 1 and not np.delete(got[0][i], 5).any() and not got[1][i].any()
        else:
            np.testing.assert_array_equal(got[0][i], clean[0][i])
            np.testing.assert_array_equal(got[1][i], clean[1][i])
    # points may be NULL
    out = np.empty((6, 17))
    assert lib.omega_phase_correlation(ctx, l.ctypes.data, r.ctypes.data, 0, m, 6, out.ctypes.data, None,
                                       L.MEM_HOST) == 0
    np.testing.assert_array_equal(out, clean[0])


@pytest.mark.gpu
def test_phase_facade_sequence_on_device():
    """PhaseCorrelation.update over seq2048 on the device: the reference's recorded get_status() and
    band_correlations per frame within the bars, the statistics and the persistence as recorded."""
    g = G()
    fs, m, frames = group("app")
    pc = panel("app")
    for i, k in enumerate(g["seq2048/idx"]):
        l, r, _, pts = frames[k]
        pc.update(l, r)
        s = pc.get_status()
        assert abs(s["correlation"] - g["seq2048/corr"][i]) <= ATOL and abs(s["balance"] - g["seq2048/balance"][i]) <= ATOL
        assert abs(s["stereo_width"] - g["seq2048/width"][i]) <= ATOL and s["mono_compatible"] == bool(g["seq2048/mono"][i])
        assert np.max(np.abs(pc.band_correlations - g["seq2048/bands"][i])) <= ATOL
        st = pc.correlation_stats
        np.testing.assert_allclose([st["min"], st["max"], st["avg"]], g["seq2048/stats"][i], rtol=0, atol=ATOL)
        assert len(pc.correlation_history) == g["seq2048/hist_len"][i]
        assert len(pc.gonio_persistence) == g["seq2048/pers_len"][i]
        np.testing.assert_array_equal(np.asarray(pc.gonio_persistence[-1]["points"]), pts[:PR.n_points(m)])
    n = len(pc.correlation_history)
    pc.update(frames[0][0][:100], frames[0][1][:100])   # shorter than 101 samples: a no-op
    pc.update(np.ones(3000, np.float32))                # an unsupported length: logged, state unchanged
    assert len(pc.correlation_history) == n
    pc.update(frames[1][0])                             # right=None: both channels are left
    assert pc.correlation == 1.0 and len(pc.correlation_history) == n + 1
