"""Makes tests/golden/phase.npz by calling the reference's PhaseCorrelationPanel
(omega4/panels/phase_correlation.py:11-252, :934-941) itself (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_phase.py <reference checkout>

The reference module is loaded by path with ``pygame`` stubbed (the module imports it at the top; nothing is
drawn). update() is never called: it fabricates a right channel with np.random. The reference's own
_calculate_correlation, balance expressions (:132-136), _update_goniometer_enhanced,
_calculate_band_correlations and _update_statistics are called on real channels, as float64 arrays (what the
app passes). Written per frame: the float32 inputs, the row in tests/phase_ref.py's COLUMNS order and the
points; per (fs, m): band_frequencies and the numpy masks' ranges; np.hanning's sha256 per m; the numpy and
scipy versions. The groups, each asserted here for what it is for:

  app        48 kHz, m 2048: partially correlated programme material; an in-phase pair; an inverted pair
             (correlation -1 after the clip); a delayed pair; a hard-panned pair; a DC offset of 0.5 on 0.1 of
             signal
  m64, m512, m8192   48 kHz; at m 64 bands 0-4 have no bin and band 5 has one
  fs44       44100 Hz, m 2048
  fs16       16000 Hz, m 1024; `fs16/nyquist_in_band9` records whether the Nyquist bin falls in band 9
  zero       one channel all zeros (all correlations 0, flag bit 2); both all zeros (flag bits 1 and 2)
  nonfinite  flags only
  seq        a pool of m 64 stereo frames and 320 steps over it (`seq/idx`) through ONE reference object
             whose band_correlations start at 0.05 (b + 1), with silent pairs in between: the 300-deep history
             wraps, both warnings fire, balance survives a silent pair, the empty bands keep their value.
             After every step: correlation_stats, the history length, balance, band_correlations, the
             persistence length and intensities, get_status()
  seq2048    40 steps over the app frames: gonio_persistence reaches its 30-frame cap. The decay cut
             (intensity <= 0.1) cannot fire in the reference: 0.95^30 = 0.21, the cap drops a frame first
             (asserted: the smallest intensity stays above 0.1)

Margins asserted on every frame (frames with a silent channel are exempt): every band with at least 2 bins
has a magnitude standard deviation, in both channels, of at least 1e-5 of the frame's largest magnitude;
both time-domain stds are at least 1e-3 of the channel's RMS.
`<group>/dev`: the reference's largest deviation from a long-double evaluation of the same formulas (a
direct long-double DFT, m <= 2048 only) as [overall correlation, bands]. For the record; it is not the bar.
"""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import phase_ref as PR  # noqa: E402

WARN = ["High correlation - check mono compatibility", "Phase cancellation detected"]


def import_reference(path):
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    spec = importlib.util.spec_from_file_location("ref_phase_correlation",
                                                  os.path.join(path, "omega4", "panels", "phase_correlation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PhaseCorrelationPanel


def programme(fs, m, seed, share=0.7, gain_r=1.0):
    """Tones and coloured noise common to both channels plus independent noise per channel."""
    rng = np.random.default_rng(seed)
    t = np.arange(m) / fs
    mid = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in
              ((0.2, 110.0, 0.1), (0.15, 440.0, 1.0), (0.1, 1760.0, 2.0), (0.05, 5300.0, 0.5)))
    mid = mid + 0.08 * np.cumsum(rng.standard_normal(m)) / np.sqrt(m) + 0.05 * rng.standard_normal(m)
    l = share * mid + (1 - share) * 0.2 * rng.standard_normal(m)
    r = gain_r * (share * mid + (1 - share) * 0.2 * rng.standard_normal(m))
    return l.astype(np.float32), r.astype(np.float32)


def ref_frame(panel, l32, r32):
    """The reference's outputs for one stereo frame as (row, points); the panel's state advances like
    update()'s :124-145."""
    left, right = l32.astype(np.float64), r32.astype(np.float64)
    row = np.zeros(PR.N_COLS)
    if not (np.isfinite(left).all() and np.isfinite(right).all()):
        row[5] = PR.FLAG_NONFINITE
        return row, np.zeros((PR.N_POINTS, 2))
    panel.correlation = panel._calculate_correlation(left, right)
    panel.correlation_history.append(panel.correlation)
    panel.stereo_width = 1.0 - abs(panel.correlation)
    left_energy = np.sqrt(np.mean(left ** 2))
    right_energy = np.sqrt(np.mean(right ** 2))
    total_energy = left_energy + right_energy
    if total_energy > 0:
        panel.balance = (right_energy - left_energy) / total_energy
    panel._update_goniometer_enhanced(left, right)
    before = panel.band_correlations.copy()
    panel.band_correlations[:] = np.nan  # (to see which bands the reference writes)
    panel._calculate_band_correlations(left, right)
    written = ~np.isnan(panel.band_correlations)
    bands = np.where(written, panel.band_correlations, 0.0)
    panel.band_correlations = np.where(written, panel.band_correlations, before)
    panel._update_statistics()
    flat = not (np.std(left - np.mean(left)) > 0 and np.std(right - np.mean(right)) > 0)
    row[0], row[1] = panel.correlation, panel.stereo_width
    row[2] = (right_energy - left_energy) / total_energy if total_energy > 0 else 0.0
    row[3], row[4] = left_energy, right_energy
    row[5] = (0 if total_energy > 0 else PR.FLAG_NO_ENERGY) + (PR.FLAG_FLAT if flat else 0)
    row[6] = sum(1 << b for b in range(10) if written[b])
    row[7:] = bands
    pts = np.zeros((PR.N_POINTS, 2))
    cur = panel.gonio_persistence[-1]["points"]
    assert len(cur) == PR.n_points(len(left)) <= PR.N_POINTS
    pts[:len(cur)] = np.asarray(cur, np.float64).reshape(-1, 2)
    return row, pts


def margins(l32, r32, fs, ranges):
    left, right = l32.astype(np.float64), r32.astype(np.float64)
    if not left.any() or not right.any():
        return
    for x in (left, right):
        assert np.std(x) >= 1e-3 * np.sqrt(np.mean(x ** 2))
    w = np.hanning(len(left))
    ml, mr = np.abs(np.fft.rfft(left * w)), np.abs(np.fft.rfft(right * w))
    top = max(ml.max(), mr.max())
    for lo, hi in ranges:
        if hi - lo >= 2:
            assert np.std(ml[lo:hi]) >= 1e-5 * top and np.std(mr[lo:hi]) >= 1e-5 * top, (lo, hi)


def long_double_dev(row, l32, r32, ranges):
    """[overall, bands]: the row against a long-double evaluation (direct DFT) of the same formulas."""
    ld = np.longdouble
    left, right = l32.astype(ld), r32.astype(ld)
    m = len(left)

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        sa, sb = np.sqrt((a * a).mean()), np.sqrt((b * b).mean())
        return float(np.clip((a * b).mean() / (sa * sb), -1, 1)) if sa > 0 and sb > 0 else 0.0

    d0 = abs(corr(left, right) - row[0])
    if m > 2048:
        return [d0, 0.0]
    ang = 2 * np.pi * np.arange(m, dtype=ld) / m
    ct, st = np.cos(ang), np.sin(ang)
    w = np.hanning(m).astype(ld)
    kn = (np.arange(m // 2 + 1)[:, None] * np.arange(m)[None, :]) % m
    mags = []
    for x in (left * w, right * w):
        mags.append(np.sqrt((ct[kn] * x).sum(1) ** 2 + (st[kn] * x).sum(1) ** 2))
    d1 = max([abs(corr(mags[0][lo:hi], mags[1][lo:hi]) - row[7 + b]) for b, (lo, hi) in enumerate(ranges) if hi > lo]
             or [0.0])
    return [d0, d1]


def main(ref_path):
    Panel = import_reference(ref_path)
    out = {}
    import scipy
    out["versions"] = json.dumps({"numpy": np.__version__, "scipy": scipy.__version__})
    out["warnings"] = json.dumps(WARN)

    def numpy_ranges(panel, m):
        freqs = np.fft.rfftfreq(m, 1 / panel.sample_rate)
        rg = np.zeros((10, 2), np.int32)
        for b in range(10):
            idx = np.flatnonzero((freqs >= panel.band_frequencies[b]) & (freqs < panel.band_frequencies[b + 1]))
            if len(idx):
                assert np.array_equal(idx, np.arange(idx[0], idx[-1] + 1))
                rg[b] = idx[0], idx[-1] + 1
        return rg

    def group(name, fs, frames, dev=True):
        m = len(frames[0][0])
        rg = numpy_ranges(Panel(fs), m)
        out[f"{name}/fs"], out[f"{name}/m"], out[f"{name}/n"] = fs, m, len(frames)
        out[f"{name}/edges"], out[f"{name}/ranges"] = np.asarray(Panel(fs).band_frequencies, np.float64), rg
        out[f"hanning/{m}"] = hashlib.sha256(np.hanning(m).tobytes()).hexdigest()
        rows, worst = [], [0.0, 0.0]
        for i, (l, r) in enumerate(frames):
            assert l.dtype == r.dtype == np.float32 and len(l) == len(r) == m
            row, pts = ref_frame(Panel(fs), l, r)
            mine = PR.features(l, r, fs)
            assert np.array_equal(mine[0], row) and np.array_equal(mine[1], pts), (name, i)
            assert int(row[5]) & 1 or int(row[6]) == sum(1 << b for b in range(10) if rg[b, 1] > rg[b, 0])
            out[f"{name}/{i}/left"], out[f"{name}/{i}/right"] = l, r
            out[f"{name}/{i}/row"], out[f"{name}/{i}/points"] = row, pts
            if not int(row[5]) & 1:
                margins(l, r, fs, rg)
                if dev and l.any() and r.any():
                    worst = [max(a, b) for a, b in zip(worst, long_double_dev(row, l, r, rg))]
            rows.append(row)
        out[f"{name}/dev"] = np.asarray(worst)
        print(name, "dev", worst)
        return rows, rg

    # app
    l0, r0 = programme(48000, 2048, 1)
    l1, _ = programme(48000, 2048, 2)
    l3, _ = programme(48000, 2048, 3)
    d = np.concatenate([np.zeros(7, np.float32), l3[:-7]])
    l4, r4 = programme(48000, 2048, 4, share=0.5, gain_r=0.002)
    l5, r5 = programme(48000, 2048, 5)
    l5, r5 = (np.float32(0.5) + np.float32(0.1) * l5), (np.float32(0.5) + np.float32(0.1) * r5)
    app = [(l0, r0), (l1, l1.copy()), (l1, -l1), (l3, d), (l4, r4), (l5, r5)]
    rows, _ = group("app", 48000, app)
    assert 0.2 < rows[0][0] < 0.98 and rows[1][0] == 1.0 and rows[2][0] == -1.0 and 0 < rows[3][0] < 0.999
    # (magnitudes: an inversion is invisible; band 0 has the one bin at 23.4 Hz: 0.0)
    assert np.all(rows[1][8:] >= 1 - 1e-12) and np.all(rows[2][8:] >= 1 - 1e-12) and all(r[7] == 0.0 for r in rows)
    assert rows[4][2] < -0.99 and abs(rows[5][2]) < 0.01 and abs(rows[5][3] - 0.5) < 0.01
    assert all(r[5] == 0 and r[6] == 1023 for r in rows)

    rows, rg = group("m64", 48000, [programme(48000, 64, 10 + i) for i in range(3)])
    assert all(rg[b, 0] == rg[b, 1] for b in range(5)) and rg[5, 1] - rg[5, 0] == 1
    assert all(int(r[6]) == 0b1111100000 and r[12] == 0.0 and not r[7:12].any() for r in rows)
    group("m512", 48000, [programme(48000, 512, 20 + i) for i in range(2)])
    group("m8192", 48000, [programme(48000, 8192, 30)])
    group("fs44", 44100, [programme(44100, 2048, 40 + i) for i in range(2)])
    rows, rg = group("fs16", 16000, [programme(16000, 1024, 50 + i) for i in range(2)])
    out["fs16/nyquist_in_band9"] = int(rg[9, 1] == 513)
    print("fs16: top edge", repr(float(Panel(16000).band_frequencies[-1])), "Nyquist bin in band 9:", rg[9, 1] == 513)

    lz, rz = programme(48000, 512, 60)
    z = np.zeros(512, np.float32)
    rows, _ = group("zero", 48000, [(lz, z), (z, rz), (z, z)])
    assert rows[0][5] == 4 and rows[1][5] == 4 and rows[2][5] == 6
    assert all(r[0] == 0 and r[1] == 1 and not r[7:].any() for r in rows) and rows[0][2] == -1 and rows[1][2] == 1

    ln, rn = programme(48000, 512, 61)
    a, b = ln.copy(), rn.copy()
    a[100] = np.nan
    b[511] = np.inf
    rows, _ = group("nonfinite", 48000, [(a, rn), (ln, b)])
    assert all(r[5] == 1 and not np.delete(r, 5).any() for r in rows)

    # seq: pool 0-4 programme, 5 in-phase, 6 inverted, 7 silent
    pool = [programme(48000, 64, 70 + i, share=0.3 + 0.1 * i, gain_r=0.5 + 0.2 * i) for i in range(5)]
    pool += [(pool[0][0], pool[0][0].copy()), (pool[1][0], -pool[1][0]), (np.zeros(64, np.float32),) * 2]
    group("seq", 48000, pool, dev=False)
    idx = [7 if i in (20, 40) else 5 for i in range(60)]
    cyc = [0, 1, 2, 7, 3, 4, 6, 0, 2, 7, 7, 1, 5]
    idx += [cyc[i % len(cyc)] for i in range(260)]
    sequence("seq", Panel, out, pool, idx, init=0.05 * (np.arange(10) + 1))
    st = out["seq/warn"]
    assert (st & 1).any() and (st & 2).any() and (st == 0).any() and out["seq/hist_len"].max() == 300
    assert (out["seq/hist_len"] == 300).sum() > 15
    k = idx.index(7, 60)  # (the first silent pair after programme material)
    assert idx[k - 1] == 2 and out["seq/balance"][k] == out["seq/balance"][k - 1] != 0
    assert np.all(out["seq/bands"][:, :5] == 0.05 * (np.arange(5) + 1)) and np.ptp(out["seq/bands"][:, 6]) > 0
    sequence("seq2048", Panel, out, app, [i % 6 for i in range(40)], init=np.zeros(10))
    assert out["seq2048/pers_len"].max() == 30 and (out["seq2048/pers_len"] == 30).sum() >= 10
    pi = out["seq2048/pers_int"]
    assert pi[pi > 0].min() > 0.1

    path = os.path.join(HERE, "phase.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def sequence(name, Panel, out, pool, idx, init):
    fs = 48000
    panel = Panel(fs)
    panel.band_correlations = np.asarray(init, np.float64).copy()
    n = len(idx)
    rec = {k: np.zeros((n,) + s) for k, s in (("stats", (3,)), ("balance", ()), ("bands", (10,)), ("corr", ()),
                                               ("width", ()), ("pers_int", (30,)))}
    rec.update({k: np.zeros(n, np.int32) for k in ("warn", "hist_len", "pers_len", "mono")})
    for i, k in enumerate(idx):
        row, _ = ref_frame(panel, *pool[k])
        assert np.array_equal(row, out[f"{name if name == 'seq' else 'app'}/{k}/row"])
        st = panel.correlation_stats
        assert st["peak_hold_time"] == 0 and all(w in WARN for w in st["warnings"])
        rec["stats"][i] = st["min"], st["max"], st["avg"]
        rec["warn"][i] = sum(1 << WARN.index(w) for w in st["warnings"])
        rec["hist_len"][i] = len(panel.correlation_history)
        rec["bands"][i] = panel.band_correlations
        s = panel.get_status()
        assert list(s) == ["correlation", "stereo_width", "balance", "mono_compatible"]
        rec["corr"][i], rec["width"][i], rec["balance"][i], rec["mono"][i] = (
            s["correlation"], s["stereo_width"], s["balance"], s["mono_compatible"])
        rec["pers_len"][i] = len(panel.gonio_persistence)
        rec["pers_int"][i, :len(panel.gonio_persistence)] = [f["intensity"] for f in panel.gonio_persistence]
    out[f"{name}/idx"] = np.asarray(idx, np.int32)
    out[f"{name}/init"] = np.asarray(init, np.float64)
    out[f"{name}/pool"] = "seq" if name == "seq" else "app"
    for k, v in rec.items():
        out[f"{name}/{k}"] = v


if __name__ == "__main__":
    main(sys.argv[1])
