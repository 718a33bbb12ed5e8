"""Makes tests/golden/room.npz by calling the reference's RoomModeAnalyzer
(omega4/analyzers/room_modes.py:19-499, room_mode_config.py:9-74) itself (build container only; TEST
INFRASTRUCTURE ONLY). Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_room.py <reference checkout>

The two reference modules are loaded by path as a throw-away package (room_modes.py imports its config
relatively; the real package's __init__ would pull in every analyzer). The reference is called on float64
arrays, with its hash cache off (it returns what a recomputation would); inputs are stored as float32. Per
group: the frequency table as (n, top) of np.linspace(0, top, n) with its sha256, the config as
tests/room_ref.py's CFG_KEYS, the six hint frequencies (0: none), the numpy mask's range, the spectra, and per
frame the header [count, flags, mean, std] and all modes in MODE_COLUMNS order. The groups, each asserted here
for what it is for:

  app        the app's shape: 512-bin spectra over linspace(0, 24000, 512), 6 in-range bins; also the reference's
             results when called on the float32 arrays (`app/<i>/modes_f32call`), for the record only
  k11, k46, k92   |rfft(x blackman)| of 2048, 8192, 16384 points at 48 kHz, tones at 47, 94, 141, 230 Hz plus
             noise: 0, 4 and 4 modes; at 16384 length, width, height, tangential with severity tied at 1.0
  k300       more in-range bins than the workgroup has lanes
  k4096      the cap (max_frequency is the table's entry at first + 4095)
  plateau    flat-topped peaks of width 2, 3 and 4
  edgewalk   peaks whose prominence walk reaches either end; equal-height neighbours the walk passes over
  noq        no half-power crossing on one side and on both (50.0), Q clamped at both limits
  ties       equal severities below 1.0, out of bin order
  many       more than 64 modes: truncated
  hints      room 5 x 4 x 2.5 m: each H1-H3 branch, the tangential branch and the frequency fallback
  empty      zero, constant (std 0) and non-finite frames (in and out of range) among live ones
  fs44       44.1 kHz, 8192 points
`host/...`: the reference's get_speed_of_sound at four (temperature, humidity) pairs and its
estimate_room_dimensions of frame 0 of hints, k92 and app as [length, width, height, confidence].

RT60 (`rt/<i>/...`): decaying noise at (W, frames) = (64, 30), (100, 30), (2048, 30), (2048, 60); a stream
without a -35 dB crossing; an all-zero stream; a two-point regression; a rising signal; a non-finite stream.
The large inputs are stored as a recipe over one 8192-sample noise table (room_ref.decay_stream: exact IEEE
steps) with the sha256 of the float32 samples. Per stream: the reference's dict for each of the three methods
(`<method>` = [rt60, confidence, slope, r_squared], NaN where the dict has no such key), the expected device
row, and the frames' energies.

Margins asserted on every frame, so that the reference alone stays inside them: std >= 1e-3 mean; every
height, prominence and severity decision at least 1e-9 relative from its threshold; distinct severities of a
frame at least 1e-9 apart; each dB crossing sample and its predecessor at least 1e-9 dB from the threshold
(`rt/<i>/margin_db` records the smallest distance).
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
import room_ref as RR  # noqa: E402

REL = 1e-9


def import_reference(path):
    sys.dont_write_bytecode = True
    d = os.path.join(path, "omega4", "analyzers")
    pkg = types.ModuleType("ref_room_pkg")
    pkg.__path__ = [d]
    sys.modules["ref_room_pkg"] = pkg
    mods = {}
    for name in ("room_mode_config", "room_modes"):
        spec = importlib.util.spec_from_file_location(f"ref_room_pkg.{name}", os.path.join(d, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["room_modes"].RoomModeAnalyzer, mods["room_mode_config"].RoomModeConfig


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def blackman_mag(fs, m, seed, noise=0.02):
    rng = np.random.default_rng(seed)
    t = np.arange(m) / fs
    x = sum(np.sin(2 * np.pi * f * t + 0.3 * k) for k, f in enumerate((47.0, 94.0, 141.0, 230.0)))
    x = x + noise * rng.standard_normal(m)
    return np.abs(np.fft.rfft(x * np.blackman(m))).astype(np.float32)


def main(ref_path):
    Ref, RefConfig = import_reference(ref_path)
    import scipy
    out = {"versions": json.dumps({"numpy": np.__version__, "scipy": scipy.__version__})}
    groups = []

    def make_ref(cfg, dims=None):
        kw = dict(zip(RR.CFG_KEYS[1:], cfg[1:]))
        if dims:
            kw.update(room_length_hint=dims[0], room_width_hint=dims[1], room_height_hint=dims[2])
        return Ref(int(cfg[0]) if cfg[0] == int(cfg[0]) else cfg[0], RefConfig(enable_caching=False, **kw))

    def group(name, n, top, spectra, cfg=RR.DEFAULT_CFG, dims=None, margins=True):
        freqs = np.linspace(0.0, top, n)
        spectra = np.asarray(spectra, np.float32)
        assert spectra.shape[1] == n
        exp = RR.expected_frequencies(*dims) if dims else np.zeros(6)
        rg = RR.bin_range(freqs, cfg[1], cfg[2])
        ref = make_ref(cfg, dims)
        if dims:  # the host's six doubles are the reference's own expressions
            c = ref.get_speed_of_sound()
            assert exp[0] == c / (2 * dims[0]) and exp[3] == c * np.sqrt((1 / (2 * dims[0])) ** 2 + (1 / (2 * dims[1])) ** 2)
        out[f"{name}/freq_n"], out[f"{name}/freq_top"], out[f"{name}/freq_sha"] = n, float(top), sha(freqs)
        out[f"{name}/cfg"], out[f"{name}/hints"] = np.asarray(cfg, np.float64), exp
        out[f"{name}/dims"] = np.asarray(dims or (0, 0, 0), np.float64)
        out[f"{name}/range"], out[f"{name}/spectra"] = np.asarray(rg, np.int32), spectra
        res = []
        for i, s32 in enumerate(spectra):
            x = s32.astype(np.float64)
            got = ref.detect_room_modes(x, freqs)
            dec = []
            header, modes = RR.detect(x, freqs, cfg, exp if dims else None, dec)
            # the restatement against the reference, bit for bit
            assert len(got) == int(header[0]), (name, i, len(got), header)
            for g, m in zip(got, modes):
                assert [g[k] for k in ("frequency", "magnitude", "q_factor", "severity", "prominence", "bandwidth")] == [
                    m[0], m[1], m[2], m[3], m[5], m[6]], (name, i, g, m)
                assert g["type"] == RR.type_name(m[4]), (name, i, g, m)
            out[f"{name}/{i}/header"], out[f"{name}/{i}/modes"] = header, modes
            if margins and not int(header[1]):
                assert header[3] >= 1e-3 * abs(header[2]), (name, i, header)
                for v, thr in dec:
                    assert thr == 0 or abs(v - thr) >= REL * abs(thr), (name, i, v, thr)
                sev = np.unique(modes[:, 3])
                assert len(sev) < 2 or np.min(np.diff(sev)) >= REL, (name, i)
            res.append((header, modes))
        groups.append(name)
        print(name, "K", rg[1] - rg[0], "counts", [int(h[0]) for h, _ in res])
        return res, freqs, rg

    # app
    rng = np.random.default_rng(100)
    app = 0.02 + 0.01 * rng.random((5, 512))
    app[0, 1:7] = [0.1, 0.2, 1.5, 0.2, 0.1, 0.12]
    app[1, 1:7] = [0.1, 0.9, 0.1, 0.1, 1.1, 0.1]
    app[2, 1:7] = [1.0, 0.8, 0.6, 0.4, 0.3, 0.2]
    app[4, 1:7] = [0.1, 0.1, 0.1, 0.1, 2.0, 0.1]
    res, freqs, rg = group("app", 512, 24000.0, app)
    assert tuple(rg) == (1, 7) and [int(h[0]) for h, _ in res] == [1, 2, 0, 0, 1]
    ref = make_ref(RR.DEFAULT_CFG)
    for i, s in enumerate(np.asarray(app, np.float32)):
        got = ref.detect_room_modes(s, freqs.astype(np.float32))
        out[f"app/{i}/modes_f32call"] = np.asarray(
            [[g[k] for k in ("frequency", "magnitude", "q_factor", "severity", "prominence", "bandwidth")] for g in got],
            np.float64).reshape(-1, 6)

    # Blackman magnitudes
    for name, m, want in (("k11", 2048, 0), ("k46", 8192, 4), ("k92", 16384, 4)):
        res, _, rg = group(name, m // 2 + 1, 24000.0, [blackman_mag(48000, m, 7 + k) for k in range(2)])
        assert rg[1] - rg[0] == int(name[1:]) and all(int(h[0]) == want for h, _ in res), (name, rg)
    for h, modes in res:
        assert sorted(RR.type_name(t) for t in modes[:, 4]) == ["axial_height", "axial_length", "axial_width", "tangential"]
        assert np.all(modes[:, 3] == 1.0) and np.all(np.diff(modes[:, 7]) > 0)
    res, _, rg = group("fs44", 4097, 22050.0, [blackman_mag(44100, 8192, 20 + k) for k in range(2)])
    assert all(int(h[0]) >= 3 for h, _ in res)

    # k300: a 1 Hz table; tones of noise-like material
    def bumps(n, centres, heights, width=3.0, floor=0.05, seed=0):
        k = np.arange(n, dtype=np.float64)
        x = floor * (1 + 0.5 * np.random.default_rng(seed).random(n))
        for c, h in zip(centres, heights):
            x = x + h * np.exp(-0.5 * ((k - c) / width) ** 2)
        return x

    res, _, rg = group("k300", 400, 332.5, [bumps(400, (60, 130, 215, 300, 340), (3, 2.5, 4, 2, 3.5), seed=s)
                                            for s in (1, 2)])
    assert rg[1] - rg[0] > 256 and all(int(h[0]) >= 3 for h, _ in res)

    # k4096: the cap
    f5 = np.linspace(0.0, 400.0, 5000)
    first = int(np.flatnonzero(f5 >= 30.0)[0])
    cap_cfg = (48000.0, 30.0, float(f5[first + 4095]), 2.0, 1.0, 0.5, 100.0, 0.3)
    cent = (first + 3, 900, 2047, 3111, first + 4092)
    res, _, rg = group("k4096", 5000, 400.0, [bumps(5000, cent, (30, 25, 40, 20, 35), width=w, seed=s)
                                              for w, s in ((2.0, 3), (9.0, 4))], cfg=cap_cfg)
    assert rg[1] - rg[0] == 4096 and all(int(h[0]) >= 3 for h, _ in res)
    out["k4096/over_max_frequency"] = float(f5[first + 4096])

    # designed shapes on a 1 Hz table (401 bins, in-range bins 30..300)
    def flat(v=0.1):
        return np.full(401, v)

    p = flat()
    p[49], p[50:52], p[52] = 2.0, 5.0, 2.0       # width 2
    p[99], p[100:103], p[103] = 2.0, 4.0, 2.0    # width 3
    p[149], p[150:154], p[154] = 2.0, 6.0, 2.0   # width 4
    p2 = flat()
    p2[200:203] = 3.0                            # a plateau then a rise: no peak of its own
    p2[203] = 7.0
    p2[296:301] = 5.0                            # a plateau reaching the last in-range bin: no peak
    res, _, _ = group("plateau", 401, 400.0, [p, p2])
    assert [int(b) for b in res[0][1][:, 7]] == [151, 50, 101] or sorted(int(b) for b in res[0][1][:, 7]) == [50, 101, 151]
    assert [int(b) for b in res[1][1][:, 7]] == [203]

    e = flat()
    e[80], e[120], e[200], e[290] = 5.0, 5.0, 9.0, 4.0
    e[31], e[299] = 3.0, 3.5                     # next to the ends of the range
    e2 = flat()
    e2[30:300] = np.linspace(0.2, 0.4, 270)      # a ramp: the walks end on different floors
    e2[100], e2[180], e2[181], e2[260] = 6.0, 6.0, 0.2, 8.0
    res, _, _ = group("edgewalk", 401, 400.0, [e, e2])
    m0 = {int(r[7]): r for r in res[0][1]}
    lowf = float(np.float32(0.1))
    assert m0[200][5] == 9.0 - lowf and m0[80][5] == m0[120][5] == 5.0 - lowf and 31 in m0 and 299 in m0, m0

    noq_cfg = (48000.0, 30.0, 300.0, 1.1, 0.5, 8.0, 100.0, 0.3)
    q0 = flat(3.0)
    q0[150] = 4.0                                # no crossing on either side: 50.0
    q1 = flat()
    q1[30:71] = np.linspace(3.0, 4.0, 41)        # no crossing on the left; wide: Q clamps to min_q_factor
    q1[71:111] = np.linspace(3.9, 0.1, 40)
    q1[250] = 9.0                                # narrow at 250 Hz: Q clamps to max_q_factor
    res, _, _ = group("noq", 401, 400.0, [q0, q1], cfg=noq_cfg)
    assert res[0][1][0, 2] == 50.0 and int(res[0][0][0]) == 1
    m1 = {int(r[7]): r for r in res[1][1]}
    assert m1[70][2] == 8.0 and m1[250][2] == 100.0, m1

    tie_cfg = (48000.0, 30.0, 300.0, 1.2, 1.0, 0.5, 100.0, 0.3)
    t0 = flat(1.0)
    t0[50], t0[120], t0[200], t0[260] = 1.5, 1.75, 1.5, 1.5
    res, _, _ = group("ties", 401, 400.0, [t0], cfg=tie_cfg)
    assert [int(b) for b in res[0][1][:, 7]] == [120, 50, 200, 260] and res[0][1][1, 3] == res[0][1][2, 3] < 1.0

    s0 = flat(1.0)
    s0[31:299:2] = 3.0 + 0.015625 * (np.arange(134) % 7)
    res, _, _ = group("many", 401, 400.0, [s0], cfg=tie_cfg)
    assert int(res[0][0][0]) == 134 and int(res[0][0][1]) == 4

    dims = (5.0, 4.0, 2.5)
    exp = RR.expected_frequencies(*dims)
    hz = [round(exp[0]), round(exp[1]), round(exp[2]), round(2 * exp[1]), round(3 * exp[0]), round(3 * exp[1]),
          round(2 * exp[2]), round(3 * exp[2]), round(exp[3]), 170, 250, 290]
    h0 = flat()
    for k, b in enumerate(hz):
        h0[b] = 4.0 + 0.25 * k
    res, _, _ = group("hints", 401, 400.0, [h0], dims=dims)
    names = {int(r[7]): RR.type_name(r[4]) for r in res[0][1]}
    assert len(names) == len(hz), names
    assert [names[b] for b in hz] == [
        "axial_length_H1", "axial_width_H1", "axial_height_H1", "axial_width_H2", "axial_length_H3",
        "axial_width_H3", "axial_height_H2", "axial_height_H3", "tangential", "axial_height", "tangential",
        "tangential"], [names[b] for b in hz]

    live = bumps(401, (60, 130, 215), (3, 2.5, 4), seed=9)
    nanf, inff = live.copy(), live.copy()
    nanf[100], inff[350] = np.nan, np.inf        # in range; out of range
    res, _, _ = group("empty", 401, 400.0, [live, flat(0.0), live[::-1].copy(), flat(0.7), live, nanf, inff, live])
    assert [int(h[1]) for h, _ in res] == [0, 2, 0, 2, 0, 1, 1, 0] and int(res[0][0][0]) >= 2

    out["groups"] = json.dumps(groups)

    # the reference's host scalar methods, for the facade's restatements
    ref = make_ref(RR.DEFAULT_CFG)
    out["host/speed_args"] = np.asarray([[20.0, 50.0], [0.0, 0.0], [35.0, 90.0], [-10.0, 20.0]])
    out["host/speed"] = np.asarray([ref.get_speed_of_sound(t, h) for t, h in out["host/speed_args"]])
    assert ref.get_speed_of_sound() == out["host/speed"][0]
    for name, dm in (("hints", dims), ("k92", None), ("app", None)):
        r = make_ref(tuple(out[f"{name}/cfg"]), dm)
        fr = np.linspace(0.0, float(out[f"{name}/freq_top"]), int(out[f"{name}/freq_n"]))
        got = r.detect_room_modes(out[f"{name}/spectra"][0].astype(np.float64), fr)
        est = r.estimate_room_dimensions(got)
        out[f"host/dims/{name}"] = np.asarray([est[k] for k in ("length", "width", "height", "confidence")], np.float64)
    assert out["host/dims/hints"][:3].all() and out["host/dims/hints"][3] > 0

    # ---- RT60 ----
    noise = np.random.default_rng(2024).standard_normal(8192).astype(np.float32)
    out["rt/noise"] = noise
    streams = []

    def recipe(W, frames, depth, roll, rising=0):
        L = W * frames
        r = float(np.exp(-depth / L))
        return dict(x=RR.decay_stream(noise, L, r, roll, rising), W=W, recipe=[L, r, roll, rising])

    for k, (W, fr) in enumerate(((64, 30), (100, 30), (2048, 30), (2048, 60))):
        streams.append(recipe(W, fr, 7.0, 100 * k))
    tail = recipe(100, 30, 1.5, 55)                       # no -35 dB crossing: the last sample holds 1 % of the energy
    tail["x"][-1] = np.float32(np.sqrt(0.01 * np.sum(tail["x"].astype(np.float64) ** 2)))
    streams.append(tail)
    streams.append(dict(x=np.zeros(1920, np.float32), W=64))
    db = np.array([0.0, -2.0, -6.0, -20.0, -36.0, -50.0])
    cv = np.append(10 ** (db / 10), 0.0)
    streams.append(dict(x=np.sqrt(cv[:-1] - cv[1:]).astype(np.float32), W=3, min_history=1))
    streams.append(recipe(64, 30, 7.0, 300, rising=1))
    bad = recipe(64, 30, 7.0, 400)["x"].copy()
    bad[1000] = np.nan
    streams.append(dict(x=bad, W=64))
    out["rt/n"] = len(streams)
    for i, st in enumerate(streams):
        x32, W = st["x"], st["W"]
        x = x32.astype(np.float64)
        mh = st.get("min_history", 30)
        ref = Ref(48000, RefConfig(min_audio_history=mh))
        for fr in x.reshape(-1, W):
            ref.update_audio_history(fr)
        assert len(ref._audio_history) == len(x) // W
        out[f"rt/{i}/W"], out[f"rt/{i}/L"], out[f"rt/{i}/min_history"], out[f"rt/{i}/sha"] = W, len(x), mh, sha(x32)
        if "recipe" in st and len(x32) > 4096:
            out[f"rt/{i}/recipe"] = np.asarray(st["recipe"], np.float64)
        else:
            out[f"rt/{i}/x"] = x32
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for method in ("schroeder", "edt", "simple"):
                    d = ref.calculate_rt60_estimate(method)
                    assert d["method"] == method and "error" not in d, d
                    out[f"rt/{i}/{method}"] = np.asarray(
                        [d["rt60"], d["confidence"], d.get("slope", np.nan), d.get("r_squared", np.nan)], np.float64)
                row = RR.rt60_row(x, 48000)
        out[f"rt/{i}/row"] = row
        out[f"rt/{i}/energies"] = np.asarray([np.sum(fr ** 2) for fr in x.reshape(-1, W)])
        flags = int(row[7])
        margin = np.inf
        if not flags & 1:
            _, dbc = RR.curve_db(x)
            assert np.all(np.diff(dbc) <= 0)
            for thr, idx in zip((-5, -10, -35), row[1:4]):
                for j in (int(idx) - 1, int(idx)):
                    if 0 <= j < len(x):
                        margin = min(margin, abs(dbc[j] - thr))
            assert margin >= 1e-9, (i, margin)
        out[f"rt/{i}/margin_db"] = margin
        sch = out[f"rt/{i}/schroeder"]
        if not flags & 7:  # the centred fit against the reference's polyfit
            assert abs(row[4] - sch[2]) <= 1e-9 * abs(sch[2]) and abs(row[6] - sch[3]) <= 1e-9, (i, row, sch)
        print("rt", i, "L", len(x), "row", row, "margin", margin, "schroeder", sch)
    rows = [out[f"rt/{i}/row"] for i in range(len(streams))]
    assert [int(r[7]) for r in rows] == [0, 0, 0, 0, 2, 2, 4, int(rows[7][7]), 1], [r[7] for r in rows]
    assert all(out[f"rt/{i}/margin_db"] >= 8e-5 for i in range(4))
    assert rows[4][3] == 3000 and rows[4][1] < 3000 and rows[5][1] == 1920 and rows[6][3] - rows[6][1] == 2

    path = os.path.join(HERE, "room.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
