"""§8(f) row 10: room acoustics on the device (omega_room_modes and omega_room_decay through
omega_gpu.room_modes) against the reference's own outputs (tests/golden/room.npz, recorded by
tests/golden/gen_room.py with the group assertions and margins listed there) and the restatement
tests/room_ref.py, which is pinned to the golden on the CPU.

Bars on the device. Exact: count, flags, bins, types and order, the crossing indices. Bit-equal: frequency,
magnitude and prominence (compares and one subtraction), q_factor and bandwidth (IEEE operations on exact
inputs, contraction off). Mean, std and severity: 1e-12 relative -- any summation order of K <= 4096 float64
terms is within about log2(K) 2^-53 = 1.3e-15 of exact, and the asserted std margin of 1e-3 of the mean
amplifies that to about 1e-12. slope, intercept, curve[0], the frame energies and RT60: 1e-9 relative, the
project's float64 bar; r_squared and the confidences: 1e-9 absolute. The observed worst deviation per column is
printed (run with -s).
Observed on an MI355X over all golden frames and streams (worst per column): mean 0, std 2.01e-16, severity 0
(bar 1e-12); curve[0] 2.63e-14, slope 8.97e-16, intercept 7.41e-13, frame energies 3.75e-16, RT60 8.79e-16
relative, r_squared and the confidences 0 (bar 1e-9); counts, flags, bins, types, order, crossing indices and
the five bit-equal columns equal on every frame, for float32 and float64 input, host and device memory.
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import room_ref as RR
from conftest import load_golden

SUM_RTOL, FIT_RTOL, R2_ATOL = 1e-12, 1e-9, 1e-9
METHODS = ("schroeder", "edt", "simple")


@functools.lru_cache(maxsize=None)
def G():
    return load_golden("room")


def groups():
    return json.loads(str(load_golden("room")["groups"]))


GROUPS = groups()


@functools.lru_cache(maxsize=None)
def group(name):
    """(freqs, cfg, hints, dims, range, spectra float32 [F, n], [(header, modes)])."""
    import hashlib
    g = G()
    freqs = np.linspace(0.0, float(g[f"{name}/freq_top"]), int(g[f"{name}/freq_n"]))
    assert hashlib.sha256(freqs.tobytes()).hexdigest() == str(g[f"{name}/freq_sha"])
    spectra = g[f"{name}/spectra"]
    frames = [(g[f"{name}/{i}/header"], g[f"{name}/{i}/modes"]) for i in range(len(spectra))]
    return (freqs, tuple(float(v) for v in g[f"{name}/cfg"]), g[f"{name}/hints"], tuple(g[f"{name}/dims"]),
            tuple(g[f"{name}/range"]), spectra, frames)


@functools.lru_cache(maxsize=None)
def stream(i):
    """(x float32, W, min_history, row, energies, {method: [rt60, confidence, slope, r_squared]})."""
    import hashlib
    g = G()
    if f"rt/{i}/x" in g.files:
        x = g[f"rt/{i}/x"]
    else:
        L, r, roll, rising = g[f"rt/{i}/recipe"]
        x = RR.decay_stream(g["rt/noise"], L, r, roll, rising)
    assert x.dtype == np.float32 and hashlib.sha256(x.tobytes()).hexdigest() == str(g[f"rt/{i}/sha"])
    x.setflags(write=False)
    return (x, int(g[f"rt/{i}/W"]), int(g[f"rt/{i}/min_history"]), g[f"rt/{i}/row"], g[f"rt/{i}/energies"],
            {m: g[f"rt/{i}/{m}"] for m in METHODS})


N_STREAMS = 9


def make_config(cfg, dims=(0, 0, 0), **kw):
    from omega_gpu.room_modes import RoomModeConfig
    return RoomModeConfig(**dict(zip(RR.CFG_KEYS[1:], cfg[1:])), room_length_hint=dims[0], room_width_hint=dims[1],
                          room_height_hint=dims[2], **kw)


def host_analyzer(cfg=RR.DEFAULT_CFG, dims=(0, 0, 0), **kw):
    from omega_gpu.room_modes import RoomModeAnalyzer
    rm = RoomModeAnalyzer.__new__(RoomModeAnalyzer)  # (the constructor opens the device)
    rm._host_init(int(cfg[0]), make_config(cfg, dims, **kw))
    return rm


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def check_rows(tag, got, header, modes, worst=None):
    """One frame's device rows [65, 8] against the golden's header and modes."""
    assert got.shape == (RR.ROWS, RR.COLS)
    assert (got[0, 0], got[0, 1]) == (header[0], header[1]), (tag, got[0], header)
    assert not got[0, 4:].any(), tag
    n = min(int(header[0]), RR.MAX_MODES)
    assert not got[1 + n:].any(), tag
    if int(header[1]) & 1:
        assert not got[0, 2:].any(), tag
        return
    d = {"mean": rel(got[0, 2], header[2]), "std": rel(got[0, 3], header[3]), "severity": 0.0}
    m = got[1:1 + n]
    np.testing.assert_array_equal(m[:, 7], modes[:n, 7], err_msg=f"{tag} bins / order")
    np.testing.assert_array_equal(m[:, 4], modes[:n, 4], err_msg=f"{tag} types")
    for col in (0, 1, 5, 2, 6):
        np.testing.assert_array_equal(m[:, col], modes[:n, col], err_msg=f"{tag} {RR.MODE_COLUMNS[col]}")
    for a, b in zip(m[:, 3], modes[:n, 3]):
        d["severity"] = max(d["severity"], rel(a, b))
    print(f"{tag} deviation from the golden:", {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
        assert v <= SUM_RTOL, (tag, k, v)


def check_rt_row(tag, got, want, worst=None):
    assert got[7] == want[7], (tag, got, want)
    if int(want[7]) & 1:
        assert not got[:7].any(), tag
        return
    np.testing.assert_array_equal(got[1:4], want[1:4], err_msg=f"{tag} crossings")
    d = {"curve0": rel(got[0], want[0]), "slope": rel(got[4], want[4]), "intercept": rel(got[5], want[5]),
         "r_squared": abs(got[6] - want[6])}
    print(f"{tag} deviation from the golden:", {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
        assert v <= (R2_ATOL if k == "r_squared" else FIT_RTOL), (tag, k, v)


def check_dict(tag, d, want, method, worst=None):
    assert d["method"] == method and "error" not in d, (tag, d)
    assert ("slope" in d) == (not np.isnan(want[2])) and ("r_squared" in d) == (not np.isnan(want[3])), (tag, d)
    dev = {"rt60": rel(d["rt60"], want[0]), "confidence": abs(d["confidence"] - want[1])}
    if "slope" in d:
        dev["slope"], dev["r_squared"] = rel(d["slope"], want[2]), abs(d["r_squared"] - want[3])
    for k, v in dev.items():
        if worst is not None:
            worst[f"{method} {k}"] = max(worst.get(f"{method} {k}", 0.0), v)
        assert v <= FIT_RTOL, (tag, k, v, d, want)


# ---- CPU ----

@pytest.mark.parametrize("name", GROUPS)
def test_room_ref_matches_reference_golden(name):
    """tests/room_ref.py against the reference's recorded modes: everything bit for bit (np.mean and np.std are
    the reference's own calls)."""
    freqs, cfg, hints, dims, rg, spectra, frames = group(name)
    assert RR.bin_range(freqs, cfg[1], cfg[2]) == rg
    if any(dims):
        np.testing.assert_array_equal(RR.expected_frequencies(*dims), hints)
    for i, (header, modes) in enumerate(frames):
        h, m = RR.detect(spectra[i].astype(np.float64), freqs, cfg, hints if any(dims) else None)
        np.testing.assert_array_equal(h, header, err_msg=f"{name} {i}")
        np.testing.assert_array_equal(m, modes, err_msg=f"{name} {i}")


@pytest.mark.parametrize("i", range(N_STREAMS))
def test_room_ref_rt60_matches_reference_golden(i):
    """The centred fit over the counted crossings against the reference's polyfit / polyval results."""
    x, W, _, row, energies, dicts = stream(i)
    got = RR.rt60_row(x, 48000)
    assert got[7] == row[7]
    np.testing.assert_array_equal(got[1:4], row[1:4])
    np.testing.assert_allclose(got, row, rtol=1e-12, atol=0)
    np.testing.assert_allclose(RR.frame_energies(x, W), energies, rtol=1e-12, atol=0)
    sch = dicts["schroeder"]
    if not int(row[7]) & 7:
        assert rel(row[4], sch[2]) <= FIT_RTOL and abs(row[6] - sch[3]) <= R2_ATOL
        assert sch[0] == min(5.0, max(0.05, -60.0 / sch[2]))


@pytest.mark.parametrize("name", GROUPS)
def test_room_bin_range_is_the_numpy_mask(name):
    """omega_room_bin_range (no context, no device) against the recorded ranges of the numpy masks."""
    from omega_gpu import _lib as L
    freqs, cfg, _, _, rg, _, _ = group(name)
    out = np.full(2, -1, np.int32)
    assert L.lib().omega_room_bin_range(freqs.ctypes.data, len(freqs), cfg[1], cfg[2], out.ctypes.data) == 0
    assert tuple(out) == rg


def test_room_bin_range_rejections():
    from omega_gpu import _lib as L
    lib = L.lib()
    f, out = np.linspace(0.0, 24000.0, 512), np.zeros(2, np.int32)
    call = lambda fr, n, lo=30.0, hi=300.0, o=out: lib.omega_room_bin_range(  # noqa: E731
        fr.ctypes.data if fr is not None else None, n, lo, hi, o.ctypes.data if o is not None else None)
    assert call(f, 512) == 0 and tuple(out) == (1, 7)
    assert call(None, 512) == L.EINVAL and call(f, 0) == L.EINVAL and call(f, 512, o=None) == L.EINVAL
    assert call(f, 512, lo=float("nan")) == L.EINVAL
    for bad in (f[::-1].copy(), np.where(np.arange(512) == 9, f[8], f), np.where(np.arange(512) == 100, np.nan, f)):
        assert call(bad, 512) == L.EINVAL
    assert call(f, 512, lo=30000.0, hi=40000.0) == 0 and out[0] == out[1]  # (no bin in range)
    assert call(np.array([100.0]), 1) == 0 and tuple(out) == (0, 1)
    cfg = L.RoomConfig()
    lib.omega_room_config_default(C.byref(cfg))
    assert tuple(getattr(cfg, k) for k in RR.CFG_KEYS) == RR.DEFAULT_CFG
    x, o = np.zeros(512, np.float32), np.empty((1, 65, 8))
    assert lib.omega_room_configure(None, C.byref(cfg), f.ctypes.data, 512, None) == L.EINVAL
    assert lib.omega_room_modes(None, x.ctypes.data, 0, 512, 1, o.ctypes.data, L.MEM_HOST) == L.EINVAL
    assert lib.omega_room_decay(None, x.ctypes.data, 0, 512, 512, 0, 1, o.ctypes.data, None, L.MEM_HOST) == L.EINVAL
    assert b"ABI 5" in lib.omega_version()  # (the entry points are additive)


def test_room_golden_group_assertions():
    """Each group does on the committed golden what it was made for, inside the margins."""
    g = G()
    fr = {n: group(n) for n in GROUPS}
    counts = {n: [int(h[0]) for h, _ in fr[n][6]] for n in GROUPS}
    K = {n: fr[n][4][1] - fr[n][4][0] for n in GROUPS}
    assert set(GROUPS) >= {"app", "k11", "k46", "k92", "k300", "k4096", "plateau", "edgewalk", "noq", "ties", "many",
                           "hints", "empty", "fs44"}
    assert fr["app"][4] == (1, 7) and len(fr["app"][0]) == 512 and counts["app"] == [1, 2, 0, 0, 1]
    assert (K["k11"], K["k46"], K["k92"]) == (11, 46, 92)
    assert counts["k11"] == [0, 0] and counts["k46"] == [4, 4] and counts["k92"] == [4, 4]
    for _, modes in fr["k92"][6]:
        assert [RR.type_name(t) for t in modes[:, 4]] == ["axial_length", "axial_width", "axial_height", "tangential"]
        assert np.all(modes[:, 3] == 1.0)
    assert K["k300"] > 256 and K["k4096"] == 4096 and fr["fs44"][0][-1] == 22050.0
    assert float(g["k4096/over_max_frequency"]) == fr["k4096"][0][fr["k4096"][4][1]]
    assert sorted(int(b) for b in fr["plateau"][6][0][1][:, 7]) == [50, 101, 151]
    assert [int(b) for b in fr["plateau"][6][1][1][:, 7]] == [203]
    m0 = {int(r[7]): r for r in fr["edgewalk"][6][0][1]}
    low = float(np.float32(0.1))
    assert m0[200][5] == 9.0 - low and m0[80][5] == m0[120][5] == 5.0 - low and 31 in m0 and 299 in m0
    assert fr["noq"][6][0][1][0, 2] == 50.0
    m1 = {int(r[7]): r for r in fr["noq"][6][1][1]}
    assert m1[70][2] == fr["noq"][1][5] == 8.0 and m1[250][2] == fr["noq"][1][6] == 100.0
    t = fr["ties"][6][0][1]
    assert [int(b) for b in t[:, 7]] == [120, 50, 200, 260] and t[1, 3] == t[2, 3] == t[3, 3] < 1.0
    assert counts["many"] == [134] and int(fr["many"][6][0][0][1]) == 4
    names = {RR.type_name(c) for c in fr["hints"][6][0][1][:, 4]}
    assert names >= {f"axial_{d}_H{h}" for d in ("width", "height") for h in (1, 2, 3)} | {
        "axial_length_H1", "axial_length_H3", "tangential", "axial_height"}
    assert [int(h[1]) for h, _ in fr["empty"][6]] == [0, 2, 0, 2, 0, 1, 1, 0]
    # the margins
    for n in GROUPS:
        freqs, cfg, hints, dims, _, spectra, frames = fr[n]
        for i, (header, modes) in enumerate(frames):
            if int(header[1]):
                continue
            dec = []
            RR.detect(spectra[i].astype(np.float64), freqs, cfg, hints if any(dims) else None, dec)
            assert header[3] >= 1e-3 * abs(header[2])
            assert all(thr == 0 or abs(v - thr) >= 1e-9 * abs(thr) for v, thr in dec), (n, i)
            sev = np.unique(modes[:, 3])
            assert len(sev) < 2 or np.min(np.diff(sev)) >= 1e-9
    rows = [stream(i)[3] for i in range(N_STREAMS)]
    assert [(len(stream(i)[0]) // stream(i)[1], stream(i)[1]) for i in range(4)] == [(30, 64), (30, 100), (30, 2048),
                                                                                     (60, 2048)]
    assert [int(r[7]) for r in rows] == [0, 0, 0, 0, 2, 2, 4, 2, 1]
    assert rows[4][3] == 3000 > rows[4][2] and rows[5][1] == 1920 and rows[6][3] - rows[6][1] == 2
    assert all(float(g[f"rt/{i}/margin_db"]) >= (8e-5 if i < 4 else 1e-9) for i in range(N_STREAMS))
    assert json.loads(str(g["versions"]))["numpy"]


def test_room_facade_host_methods():
    """The facade's host scalar methods from _host_init (no device) against the reference's recorded values."""
    from omega_gpu.room_modes import type_name
    g = G()
    rm = host_analyzer()
    assert rm.sustained_peaks_history.maxlen == 300 and rm._audio_history.maxlen == 60
    got = [rm.get_speed_of_sound(t, h) for t, h in g["host/speed_args"]]
    assert got == list(g["host/speed"]) and rm.get_speed_of_sound() == g["host/speed"][0]
    # estimate_q_factor and classify_room_mode on every recorded mode
    for name in GROUPS:
        freqs, cfg, hints, dims, (first, last), spectra, frames = group(name)
        rm = host_analyzer(cfg, dims)
        exp = rm._expected_frequencies(rm._get_room_dimensions())
        assert (exp is None and not any(dims)) or list(exp) == list(hints)
        for i, (_, modes) in enumerate(frames):
            x = spectra[i].astype(np.float64)[first:last]
            for m in modes:
                assert rm.estimate_q_factor(x, freqs[first:last], int(m[7]) - first) == m[2]
                assert rm.classify_room_mode(m[0], rm._get_room_dimensions()) == RR.type_name(m[4]) == type_name(m[4])
        assert rm.estimate_q_factor(np.ones(5), np.arange(5.0), 0) == 1.0 == rm.estimate_q_factor(np.ones(5), np.arange(5.0), 4)
    # estimate_room_dimensions
    from omega_gpu.room_modes import RoomModeAnalyzer
    for name in ("hints", "k92", "app"):
        _, cfg, _, dims, _, _, frames = group(name)
        rm = host_analyzer(cfg, dims)
        est = rm.estimate_room_dimensions(RoomModeAnalyzer.modes_from_rows(RR.rows_from(*frames[0])))
        assert list(est) == ["length", "width", "height", "confidence"]
        assert [est[k] for k in est] == list(g[f"host/dims/{name}"]), name
    assert rm.estimate_room_dimensions([]) == {"length": 0.0, "width": 0.0, "height": 0.0, "confidence": 0.0}
    # the RT60 ends from the recorded rows and energies
    for i in range(N_STREAMS):
        x, W, mh, row, energies, dicts = stream(i)
        rm = host_analyzer(min_audio_history=mh)
        x64 = x.astype(np.float64)
        with np.errstate(all="ignore"):
            check_dict(f"rt {i}", rm.finish_schroeder(row, x64), dicts["schroeder"], "schroeder")
            check_dict(f"rt {i}", rm.finish_edt(row, len(x), x64), dicts["edt"], "edt")
            en = energies if not int(row[7]) & 1 else RR.frame_energies(x64, W)
            check_dict(f"rt {i}", rm.finish_simple(en, W), dicts["simple"], "simple")
    # too little history, the deque
    rm = host_analyzer()
    rm.update_audio_history(None)
    rm.update_audio_history(np.zeros(0))
    chunk = np.ones(8, np.float32)
    rm.update_audio_history(chunk)
    chunk[:] = 2.0
    assert len(rm._audio_history) == 1 and rm._audio_history[0][0] == 1.0
    assert rm.calculate_rt60_estimate() == {"rt60": 0.0, "confidence": 0.0, "method": "schroeder"}
    assert rm.calculate_rt60_estimate("edt") == {"rt60": 0.0, "confidence": 0.0, "method": "edt"}
    assert rm.detect_room_modes(None, None) == [] and rm.detect_room_modes(np.ones(3), np.ones(4)) == []
    assert rm.detect_room_modes(np.ones(0), np.ones(0)) == []


@pytest.mark.parametrize("kw,msg", [
    (dict(min_frequency=300.0), "min_frequency must be less than max_frequency"),
    (dict(peak_threshold_multiplier=0.0), "peak_threshold_multiplier must be positive"),
    (dict(minimum_prominence_std=-0.1), "minimum_prominence_std must be non-negative"),
    (dict(min_q_factor=100.0), "min_q_factor must be less than max_q_factor"),
    (dict(minimum_severity=1.5), "minimum_severity must be between 0 and 1"),
    (dict(minimum_severity=-0.5), "minimum_severity must be between 0 and 1"),
    (dict(temperature_celsius=60.0), "temperature_celsius must be between -50 and 50"),
    (dict(humidity_percent=101.0), "humidity_percent must be between 0 and 100"),
    (dict(cache_max_age_frames=-1), "cache_max_age_frames must be non-negative"),
    (dict(rt60_method="sabine"), "rt60_method must be one of: schroeder, edt, simple"),
    (dict(min_audio_history=0), "min_audio_history must be at least 1"),
])
def test_room_config_value_errors(kw, msg):
    from omega_gpu import RoomModeConfig
    with pytest.raises(ValueError, match=msg):
        RoomModeConfig(**kw)
    c = RoomModeConfig()
    assert (c.min_frequency, c.max_frequency, c.peak_threshold_multiplier, c.minimum_prominence_std, c.min_q_factor,
            c.max_q_factor, c.minimum_severity, c.temperature_celsius, c.humidity_percent, c.enable_caching,
            c.cache_max_age_frames, c.rt60_method, c.min_audio_history, c.room_length_hint, c.room_width_hint,
            c.room_height_hint) == (30.0, 300.0, 2.0, 1.0, 0.5, 100.0, 0.3, 20.0, 50.0, True, 10, "schroeder", 30, 0.0,
                                    0.0, 0.0)


# ---- GPU ----

WORST, WORST_RT = {}, {}


def analyzer(name=None, **kw):
    from omega_gpu import RoomModeAnalyzer
    if name is None:
        return RoomModeAnalyzer(48000, make_config(RR.DEFAULT_CFG, **kw))
    _, cfg, _, dims, _, _, _ = group(name)
    return RoomModeAnalyzer(int(cfg[0]), make_config(cfg, dims, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUPS)
def test_room_modes_golden_parity(name):
    """Every frame of the group through omega_room_modes: host and device memory, float32 and float64, singly
    and as one batch."""
    import torch
    freqs, _, _, _, _, spectra, frames = group(name)
    rm = analyzer(name)
    for i, (header, modes) in enumerate(frames):
        check_rows(f"{name}[{i}]", rm.analyze_spectra(spectra[i][None], freqs)[0], header, modes, WORST)
    variants = {"host f32": rm.analyze_spectra(spectra, freqs),
                "host f64": rm.analyze_spectra(spectra.astype(np.float64), freqs),
                "device f32": rm.analyze_spectra(torch.from_numpy(spectra).cuda(), freqs).cpu().numpy(),
                "device f64": rm.analyze_spectra(torch.from_numpy(spectra).double().cuda(), freqs).cpu().numpy()}
    for tag, rows in variants.items():
        for i, (header, modes) in enumerate(frames):
            check_rows(f"{name}[{i}] {tag}", rows[i], header, modes)
        np.testing.assert_array_equal(rows, variants["host f32"], err_msg=tag)
    print("worst so far:", {k: f"{v:.2e}" for k, v in WORST.items()})


@pytest.mark.gpu
def test_room_modes_layouts_and_float64():
    """Overlapping rows of one device buffer equal the same rows sent singly; float64 values that float32
    cannot hold, against the restatement."""
    import torch
    freqs, cfg, _, _, _, spectra, _ = group("k300")
    rm = analyzer("k300")
    n = len(freqs)
    v = np.concatenate([spectra[0], spectra[1], spectra[0]])
    step = 37
    view = torch.from_numpy(v).cuda().unfold(0, n, step)
    assert view.stride(0) == step < n and view.shape[0] > 10
    got = rm.analyze_spectra(view, freqs).cpu().numpy()
    want = rm.analyze_spectra(np.stack([v[k * step:k * step + n] for k in range(view.shape[0])]), freqs)
    np.testing.assert_array_equal(got, want)
    assert len({int(r[0, 0]) for r in got}) > 1  # (the shifted rows are different frames)
    y = spectra.astype(np.float64) * 1.000000123
    rows = rm.analyze_spectra(y, freqs)
    for i in range(len(y)):
        check_rows(f"float64[{i}]", rows[i], *RR.detect(y[i], freqs, cfg))


@pytest.mark.gpu
def test_room_modes_row_independence():
    """The zero, constant and non-finite frames of `empty` leave their neighbours' rows bit-equal to a batch of
    the live frames alone."""
    freqs, _, _, _, _, spectra, frames = group("empty")
    rm = analyzer("empty")
    flags = [int(h[1]) for h, _ in frames]
    live = [i for i, f in enumerate(flags) if not f]
    assert 0 < len(live) < len(flags)
    rows = rm.analyze_spectra(spectra, freqs)
    alone = rm.analyze_spectra(spectra[live], freqs)
    np.testing.assert_array_equal(rows[live], alone)
    for i, f in enumerate(flags):
        if f:
            assert rows[i, 0, 1] == f and rows[i, 0, 0] == 0 and not rows[i, 1:].any()
    assert rm.detect_room_modes(spectra[5], freqs) == [] and rm.detect_room_modes(spectra[1], freqs) == []


@pytest.mark.gpu
def test_room_rejections():
    """OMEGA_EUNSUP above 4096 in-range bins; OMEGA_EINVAL with a last-error text before configure, for a table
    that does not increase and for bad layouts."""
    from omega_gpu import RoomModeAnalyzer, UnsupportedError
    from omega_gpu import _lib as L
    lib = L.lib()
    rm = RoomModeAnalyzer(48000)
    ctx = rm._eng._ctx
    x, out = np.ones(8192, np.float32), np.empty((1, 65, 8))
    assert lib.omega_room_modes(ctx, x.ctypes.data, 0, 512, 1, out.ctypes.data, L.MEM_HOST) == L.EINVAL
    assert b"omega_room_configure" in lib.omega_last_error(ctx)
    assert lib.omega_room_decay(ctx, x.ctypes.data, 0, 512, 512, 0, 1, out.ctypes.data, None, L.MEM_HOST) == L.EINVAL
    assert b"omega_room_configure" in lib.omega_last_error(ctx)
    freqs, cfg, _, _, _, spectra, frames = group("k4096")
    over = float(G()["k4096/over_max_frequency"])
    c = L.RoomConfig(*cfg)
    c.max_frequency = over
    assert lib.omega_room_configure(ctx, C.byref(c), freqs.ctypes.data, len(freqs), None) == L.EUNSUP
    assert b"4097" in lib.omega_last_error(ctx)
    big = RoomModeAnalyzer(48000, make_config(cfg[:2] + (over,) + cfg[3:]))
    with pytest.raises(UnsupportedError, match="4097"):
        big.analyze_spectra(spectra, freqs)
    c.max_frequency = cfg[2]
    bad = freqs.copy()
    bad[7] = bad[6]
    assert lib.omega_room_configure(ctx, C.byref(c), bad.ctypes.data, len(bad), None) == L.EINVAL
    c.minimum_severity = 2.0
    assert lib.omega_room_configure(ctx, C.byref(c), freqs.ctypes.data, len(freqs), None) == L.EINVAL
    c.minimum_severity = cfg[7]
    assert lib.omega_room_configure(ctx, C.byref(c), freqs.ctypes.data, len(freqs), None) == 0
    out = np.empty((2, 65, 8))
    assert lib.omega_room_modes(ctx, spectra.ctypes.data, 0, len(freqs), 2, out.ctypes.data, L.MEM_HOST) == 0
    check_rows("k4096 raw", out[1], *frames[1])
    assert lib.omega_room_modes(ctx, spectra.ctypes.data, 0, 0, 2, out.ctypes.data, L.MEM_HOST) == L.EINVAL
    assert lib.omega_room_modes(ctx, None, 0, len(freqs), 2, out.ctypes.data, L.MEM_HOST) == L.EINVAL
    r = np.empty((1, 8))
    for Ln, W, code in ((1, 0, L.EINVAL), (100, 7, L.EINVAL), (100, -1, L.EINVAL), ((1 << 20) + 1, 0, L.EUNSUP)):
        assert lib.omega_room_decay(ctx, x.ctypes.data, 0, Ln, Ln, W, 1, r.ctypes.data, None, L.MEM_HOST) == code, (Ln, W)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(N_STREAMS))
def test_room_rt60_golden_parity(i):
    """Every stream through omega_room_decay: host and device memory, float32 and float64; then the facade's
    three methods against the reference's dicts."""
    import torch
    x, W, mh, row, energies, dicts = stream(i)
    rm = analyzer(min_audio_history=mh)
    variants = {"host f32": rm.analyze_histories(x[None], W), "host f64": rm.analyze_histories(x.astype(np.float64)[None], W),
                "device f32": rm.analyze_histories(torch.from_numpy(x.copy()).cuda()[None], W),
                "device f64": rm.analyze_histories(torch.from_numpy(x.copy()).double().cuda()[None], W)}
    for tag, (rows, en) in variants.items():
        if tag.startswith("device"):
            rows, en = rows.cpu().numpy(), en.cpu().numpy()
        check_rt_row(f"rt[{i}] {tag}", rows[0], row, WORST_RT)
        if not int(row[7]) & 1:
            dev = max(rel(a, b) for a, b in zip(en[0], energies))
            WORST_RT["energies"] = max(WORST_RT.get("energies", 0.0), dev)
            assert dev <= FIT_RTOL, (tag, dev)
        np.testing.assert_array_equal(rows, variants["host f32"][0], err_msg=tag)
    assert rm.analyze_histories(x[None], 0)[1] is None
    for dtype in (np.float32, np.float64):
        rm._audio_history.clear()
        for fr in x.astype(dtype).reshape(-1, W):
            rm.update_audio_history(fr)
        with np.errstate(all="ignore"):
            for method in METHODS:
                check_dict(f"rt[{i}] {dtype.__name__}", rm.calculate_rt60_estimate(method), dicts[method], method, WORST_RT)
    print("worst so far:", {k: f"{v:.2e}" for k, v in WORST_RT.items()})


@pytest.mark.gpu
def test_room_rt60_batch_and_overlap():
    """Streams as overlapping rows of one device buffer equal the same rows sent singly."""
    import torch
    x = stream(1)[0]
    rm = analyzer()
    view = torch.from_numpy(x.copy()).cuda().unfold(0, 2000, 250)
    assert view.shape[0] == 5 and view.stride(0) == 250
    rows, en = rm.analyze_histories(view, 100)
    for k in range(5):
        one = rm.analyze_histories(x[k * 250:k * 250 + 2000][None], 100)
        np.testing.assert_array_equal(rows[k].cpu().numpy(), one[0][0])
        np.testing.assert_array_equal(en[k].cpu().numpy(), one[1][0])
        check_rt_row(f"overlap[{k}]", one[0][0], RR.rt60_row(x[k * 250:k * 250 + 2000], 48000))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUPS)
def test_room_facade_dicts(name):
    """detect_room_modes and detect_room_modes_batch against the reference's dicts: keys, type strings, order."""
    freqs, _, _, _, _, spectra, frames = group(name)
    rm = analyzer(name)
    batch = rm.detect_room_modes_batch(spectra, freqs)
    assert len(batch) == len(frames)
    for i, (header, modes) in enumerate(frames):
        one = rm.detect_room_modes(spectra[i], freqs)
        assert one == batch[i]
        n = min(int(header[0]), RR.MAX_MODES)
        assert len(one) == n
        for d, m in zip(one, modes):
            assert list(d) == ["frequency", "magnitude", "q_factor", "severity", "type", "prominence", "bandwidth"]
            assert all(isinstance(d[k], float) for k in d if k != "type")
            assert (d["frequency"], d["magnitude"], d["q_factor"], d["prominence"], d["bandwidth"]) == (
                m[0], m[1], m[2], m[5], m[6])
            assert d["type"] == RR.type_name(m[4]) and rel(d["severity"], m[3]) <= SUM_RTOL
