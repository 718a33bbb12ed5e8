"""§8(f) row 6: HarmonicAnalyzer.detect_harmonic_series on the device (omega_harmonic_analyze through
omega_gpu.harmonic_analysis) against the reference's own outputs (tests/golden/harmonic.npz, recorded by
tests/golden/gen_harmonic.py under the conditions listed there) and the restatement
tests/harmonic_ref.py, which is pinned to the golden on the CPU.

Tolerances. Every integer decision is exact: the series count and order, peak bins, harmonic bins,
the rolloff bin, the formant count. Values that are freqs entries or means of them (dominant
fundamental, rolloff, inharmonicity) match to 1e-12 relative, centroid and spread to 1e-9 (another
summation order). The float32-path values (strengths, thd, thd_plus_noise, flux relative; hnr_db
absolute) must lie within 4 x the reference's own recorded deviation from the float64 evaluation of the
same formulas (golden `dev`), the formants within 4 x its recorded relative deviation from the
extended-precision evaluation (golden `dev_formant`). The device's own deviations are printed per frame
(run with -s). Recorded reference deviations: strengths 2.4e-7, thd 9.2e-8, thd_plus_noise 7.0e-5, flux
8.0e-8, hnr_db 2.2e-5 dB, formants 9.5e-14. Observed on an MI355X over all 33 frames: strengths <= 2.4e-7
(the kernel forms the score in float32 like the reference, so it carries the reference's own deviation),
thd and flux 0, thd_plus_noise <= 3.3e-13, hnr_db <= 1.5e-14 dB, formants <= 2.7e-15.
"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import harmonic_ref as HR
from conftest import REPO, load_golden

sys.path.insert(0, os.path.join(REPO, "tools", "model"))
import peaks_model as M  # noqa: E402

GROUPS = ("app", "k1025", "k4097", "m1024", "m4096", "fs44", "pure", "plateau", "distance", "noseries", "offset",
          "silent", "realroot", "seq")


@functools.lru_cache(maxsize=None)
def G():
    return load_golden("harmonic")


def group(name):
    g = G()
    n = int(g[f"{name}/n"])
    fr = [(g[f"{name}/{i}/spec"], g[f"{name}/{i}/audio"].astype(np.float64)) for i in range(n)]
    return int(g[f"{name}/fs"]), g[f"{name}/freqs"], fr


@functools.lru_cache(maxsize=None)
def evals(name):
    """The float32-path restatement and the float64 evaluation of the group's frames (computed once)."""
    fs, freqs, frames = group(name)
    out, prev = [], None
    for spec, audio in frames:
        out.append((HR.analyze(spec, freqs, audio, fs, prev), HR.analyze(spec, freqs, audio, fs, prev, f64=True)))
        prev = spec if name == "seq" else None
    return out


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def check_frame(name, i, row, sbins, sstr):
    """One device (or restatement) row with its series arrays against frame i of the group's golden."""
    g, p = G(), f"{name}/{i}/"
    ref = g[p + "row"]
    dev = dict(zip([str(k) for k in g["dev_names"]], g["dev"]))
    e64 = evals(name)[i][1]
    fs, freqs, _ = group(name)
    n = int(ref[0])
    assert int(row[0]) == n, (name, i, row[0], n)
    k = min(n, sbins.shape[0])
    np.testing.assert_array_equal(sbins[:k, 0], g[p + "series_peak"][:k], err_msg=f"{name} {i} series order")
    np.testing.assert_array_equal(sbins[:k, 1:], g[p + "series_bins"][:k], err_msg=f"{name} {i} harmonic bins")
    assert (sbins[k:] == -1).all() and (sstr[k:] == 0).all()
    d = {"strength": max([rel(a, b) for a, b in zip(sstr[:k], e64["series_strength"][:k])] or [0.0]),
         "thd": rel(row[2], e64["thd"]), "thd_plus_noise": rel(row[3], e64["thd_plus_noise"]),
         "spectral_flux": rel(row[6], e64["spectral_flux"]), "hnr_db": abs(row[9] - e64["hnr_db"])}
    print(f"{name}[{i}] deviation from the float64 evaluation:", {k_: f"{v:.2e}" for k_, v in d.items()})
    for k_, v in d.items():
        assert v <= 4 * dev[k_], (name, i, k_, v, dev[k_])
    np.testing.assert_allclose(row[[1, 7, 8]], ref[[1, 7, 8]], rtol=1e-12, err_msg=f"{name} {i} f0 / rolloff / inharmonicity")
    if n:
        assert row[7] == freqs[int(g[p + "rolloff_idx"])], (name, i)
    np.testing.assert_allclose(row[[4, 5]], ref[[4, 5]], rtol=1e-9, err_msg=f"{name} {i} centroid / spread")
    assert int(row[10]) == int(ref[10]), (name, i, row[10:15], ref[10:15])
    if int(ref[10]):
        ext = g[p + "formants_ext"]
        df = max(rel(a, b) for a, b in zip(row[11:11 + len(ext)], ext))
        print(f"{name}[{i}] formant deviation from the extended-precision evaluation: {df:.2e}")
        assert df <= 4 * float(g["dev_formant"]), (name, i, df, float(g["dev_formant"]))
    assert (row[11 + int(ref[10]):15] == 0).all()


def profiles():
    return json.loads(str(G()["instrument_profiles"]))


# ---- CPU ----

@pytest.mark.parametrize("name", GROUPS)
def test_harmonic_ref_matches_reference_golden(name):
    """tests/harmonic_ref.py against the reference: the float32 paths reproduce the recorded values
    exactly (numpy's own promotion), the lags and roots to rounding, and the recorded `dev` really is the
    reference's deviation from the float64 evaluation."""
    g = G()
    dev = dict(zip([str(k) for k in g["dev_names"]], g["dev"]))
    for i, (e, e64) in enumerate(evals(name)):
        p = f"{name}/{i}/"
        np.testing.assert_array_equal(HR.row(e), g[p + "row"])
        np.testing.assert_array_equal(e["peaks"], g[p + "peaks"])
        np.testing.assert_array_equal(e["series_strength"], g[p + "series_strength"])
        bins = np.concatenate([e["series_peak"][:, None], e["series_bins"]], axis=1).reshape(-1, 17)
        check_frame(name, i, HR.row(e), bins, e["series_strength"])
        for a, b in zip(e["series_strength"], e64["series_strength"]):
            assert rel(a, b) <= dev["strength"] * (1 + 1e-9)
        for k in ("thd", "thd_plus_noise", "spectral_flux"):
            assert e64[k] == 0 or rel(e[k], e64[k]) <= dev[k] * (1 + 1e-9), (name, i, k)
        assert abs(e["hnr_db"] - e64["hnr_db"]) <= dev["hnr_db"] * (1 + 1e-9)
        if e["roots"] is not None:
            np.testing.assert_allclose(e["lags"], g[p + "lags"], rtol=1e-13)
            ext, _ = HR.formants_ext(group(name)[2][i][1], group(name)[0])
            np.testing.assert_allclose(ext, g[p + "formants_ext"], rtol=1e-15)
            for a, b in zip(e["formants"], ext):
                assert rel(a, b) <= float(g["dev_formant"]) * (1 + 1e-6)
    if name == "realroot":
        assert any(z.imag == 0 and z.real < 0 for z in g["realroot/0/roots"])
    if name == "plateau":
        assert g["plateau/0/spec"][12] == g["plateau/0/spec"][13] == 1.0 and 12 in g["plateau/0/peaks"]
    if name == "distance":
        assert 15 not in g["distance/0/peaks"] and g["distance/0/spec"][15] > g["distance/0/spec"][14]
    if name == "offset":
        # the frames where the 5 % acceptance and the strength filter decide: a candidate with fewer than two
        # accepted harmonics is rejected beside kept ones; a kept series has rejected harmonics between
        # accepted ones and more than eight accepted; in-range peaks without any series
        e = evals(name)[0][0]
        cand = dict(e["candidates"])
        assert cand[340] == 0.0 and 340 in e["peaks"] and 340 not in e["series_peak"] and e["series_count"] >= 2
        b7 = e["series_bins"][list(e["series_peak"]).index(7)]
        acc = [n + 1 for n in range(16) if b7[n] >= 0]
        assert len(acc) > 8 and acc[:8] != list(range(1, 9))
        e = evals(name)[1][0]
        assert len(e["candidates"]) == 2 and e["series_count"] == 0


def test_harmonic_facade_host_logic():
    """The facade's host-side parts against the golden: the rebuilt series dicts, the instrument
    scoring with the recorded profile table, the vowel lookup and tables. No device is touched."""
    from omega_gpu.harmonic_analysis import HarmonicAnalyzer, HarmonicMetrics
    g = G()
    an = HarmonicAnalyzer.__new__(HarmonicAnalyzer)  # (the constructor opens the device)
    an.instrument_profiles = profiles()
    seen = 0
    for name in ("app", "k1025", "plateau", "distance", "noseries", "offset"):
        fs, freqs, frames = group(name)
        for i, (spec, _) in enumerate(frames):
            p = f"{name}/{i}/"
            bins = np.concatenate([g[p + "series_peak"][:, None], g[p + "series_bins"]], axis=1).reshape(-1, 17)
            found = HarmonicAnalyzer.series_dicts(spec, freqs, bins, g[p + "series_strength"], len(bins))
            for s, row in zip(found, bins):
                assert list(s) == ["fundamental", "harmonics", "strength", "harmonic_count"]
                assert s["harmonic_count"] == int((row[1:] >= 0).sum()) == len(s["harmonics"])
                assert all(list(h) == ["number", "expected_freq", "actual_freq", "magnitude", "relative_strength"]
                           for h in s["harmonics"])
                assert s["harmonics"][0]["relative_strength"].dtype == np.float32
            got = [[m["instrument"], float(m["confidence"]), m["match_count"]] for m in an.identify_instruments(found[:3])]
            want = json.loads(str(g[p + "matches"]))
            assert [m[0] for m in got] == [m[0] for m in want] and [m[2] for m in got] == [m[2] for m in want], (name, i)
            np.testing.assert_allclose([m[1] for m in got], [m[1] for m in want], rtol=1e-6)
            seen += len(want)
    assert seen > 0
    an.instrument_profiles = {}
    assert an.identify_instruments(found[:3]) == []
    hm = HarmonicMetrics(48000)
    fm, vowel, conf = json.loads(str(g["vowel"]))
    v = hm.detect_vowel_from_formants(fm)
    assert v[0] == vowel and abs(v[1] - conf) < 1e-12
    assert hm.detect_vowel_from_formants([500.0]) == ("unknown", 0.0)
    t = json.loads(str(g["tables"]))
    assert {k: {kk: list(vv) for kk, vv in d.items()} for k, d in hm.formant_ranges.items()} == t["formant_ranges"]
    assert hm.vowel_formants == t["vowel_formants"]
    with pytest.raises(ValueError):
        HarmonicMetrics(0)
    with pytest.raises(ValueError):
        HarmonicAnalyzer(0)


def test_harmonic_abi_argument_checks():
    """The entry points' argument checks that run before any device call."""
    from omega_gpu import _lib as L
    lib = L.lib()
    assert b"ABI 5" in lib.omega_version()
    cfg = L.HarmonicConfig()
    lib.omega_harmonic_config_default(C.byref(cfg))
    assert (cfg.sample_rate, cfg.n_bins, cfg.max_series) == (48000, 512, 16)
    fr = np.linspace(0, 24000, 512)
    out = np.empty((1, 16))
    spec = np.zeros(512, np.float32)
    assert lib.omega_harmonic_configure(None, C.byref(cfg), fr.ctypes.data) == L.EINVAL
    assert lib.omega_harmonic_analyze(None, spec.ctypes.data, 512, None, 0, 0, 1, 1, out.ctypes.data, None, None,
                                      L.MEM_HOST) == L.EINVAL
    assert lib.omega_harmonic_reset(None) == L.EINVAL


# ---- GPU ----

def analyzer(name, **kw):
    from omega_gpu.harmonic_analysis import HarmonicAnalyzer
    return HarmonicAnalyzer(group(name)[0], instrument_profiles=profiles(), **kw)


KEYS = ["harmonic_series", "instrument_matches", "dominant_fundamental", "thd", "thd_plus_noise", "spectral_centroid",
        "spectral_spread", "spectral_flux", "spectral_rolloff", "inharmonicity", "formants", "hnr_db"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in GROUPS if n != "seq"])
def test_harmonic_golden_parity(name):
    """Every frame of the group through analyze_frames (each on a fresh state, as recorded) and through
    detect_harmonic_series: the reference's dict, its instrument matches, the golden values."""
    g = G()
    fs, freqs, frames = group(name)
    an = analyzer(name)
    for i, (spec, audio) in enumerate(frames):
        an.reset()
        out, sb, ss = an.analyze_frames(spec[None], freqs, audio[None])
        check_frame(name, i, out[0], sb[0], ss[0])
        assert out[0, 15] == 0
        an.reset()
        r = an.detect_harmonic_series(spec, freqs, audio)
        assert list(r) == KEYS
        row = np.array([len(r["harmonic_series"]), r["dominant_fundamental"], r["thd"], r["thd_plus_noise"],
                        r["spectral_centroid"], r["spectral_spread"], r["spectral_flux"], r["spectral_rolloff"],
                        r["inharmonicity"], r["hnr_db"], len(r["formants"])] + r["formants"] + [0.0] * (4 - len(r["formants"])))
        np.testing.assert_array_equal(row, out[0, :15])
        want = json.loads(str(g[f"{name}/{i}/matches"]))
        assert [m["instrument"] for m in r["instrument_matches"]] == [m[0] for m in want], (name, i)
        for s, pk in zip(r["harmonic_series"], g[f"{name}/{i}/series_peak"]):
            assert s["fundamental"] == freqs[pk] and s["harmonic_count"] == len(s["harmonics"])
    if name == "pure":  # (the last frame: THD+N and HNR off their caps)
        assert out[0, 3] < 100 and 0 < out[0, 9] < 60
    if name in ("noseries", "silent"):
        assert not out[0].any()


@pytest.mark.gpu
def test_harmonic_sequence_state_split_and_reset():
    """The 12-frame stream as one call and as calls of 5 + 7: both equal the golden (flux against the
    previous frame, across the call boundary and across the two frames without a series); after
    omega_harmonic_reset the first frame's flux is 0 again; single calls keep the host histories."""
    g = G()
    fs, freqs, frames = group("seq")
    spec = np.stack([f[0] for f in frames])
    audio = np.stack([f[1] for f in frames])
    one = analyzer("seq").analyze_frames(spec, freqs, audio)
    an = analyzer("seq")
    a, b = an.analyze_frames(spec[:5], freqs, audio[:5]), an.analyze_frames(spec[5:], freqs, audio[5:])
    for k in range(3):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), one[k])
    for i in range(12):
        check_frame("seq", i, one[0][i], one[1][i], one[2][i])
    # 6 + 6: the first call ends on frame 5, which has no series; frame 6's flux compares with it
    an6 = analyzer("seq")
    a, b = an6.analyze_frames(spec[:6], freqs, audio[:6]), an6.analyze_frames(spec[6:], freqs, audio[6:])
    for k in range(3):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), one[k])
    assert one[0][0, 6] == 0 and one[0][6, 6] > 1 and not one[0][4].any()
    again = an.analyze_frames(spec[:1], freqs, audio[:1])[0]
    assert again[0, 6] > 0  # (against frame 11)
    an.reset()
    np.testing.assert_array_equal(an.analyze_frames(spec[:1], freqs, audio[:1])[0], one[0][:1])
    sn = analyzer("seq")
    for s, x in frames:
        sn.detect_harmonic_series(s, freqs, x)
    np.testing.assert_allclose(list(sn.spectral_centroid_history), g["seq/centroid_history"], rtol=1e-9)
    np.testing.assert_allclose(list(sn.thd_history), g["seq/thd_history"], rtol=4 * float(g["dev"][1]))


@pytest.mark.gpu
def test_harmonic_truncation_null_audio_and_pointers():
    """max_series below the count: the true count is reported and the top entries kept; NULL audio: no
    formants, the other columns bitwise unchanged; float32 audio, device pointers and an overlapping
    stream view give the host rows bitwise."""
    import torch
    fs, freqs, frames = group("k4097")
    spec = np.stack([f[0] for f in frames])
    audio = np.stack([f[1] for f in frames])
    full = analyzer("k4097").analyze_frames(spec, freqs, audio)
    assert full[0][0, 0] == 9
    cut = analyzer("k4097", max_series=4).analyze_frames(spec, freqs, audio)
    np.testing.assert_array_equal(cut[0], full[0])
    np.testing.assert_array_equal(cut[1], full[1][:, :4])
    np.testing.assert_array_equal(cut[2], full[2][:, :4])
    none = analyzer("k4097").analyze_frames(spec, freqs, None)
    np.testing.assert_array_equal(none[0][:, :10], full[0][:, :10])
    assert not none[0][:, 10:].any()
    f32 = analyzer("k4097").analyze_frames(spec, freqs, audio.astype(np.float32))
    np.testing.assert_array_equal(f32[0], full[0])
    dev = analyzer("k4097").analyze_frames(torch.from_numpy(spec).cuda(), freqs, torch.from_numpy(audio).cuda())
    assert dev[0].is_cuda and dev[1].dtype == torch.int32
    for k in range(3):
        np.testing.assert_array_equal(dev[k].cpu().numpy(), full[k])
    fs, freqs, frames = group("seq")
    spec = np.stack([f[0] for f in frames[:4]])
    audio = np.stack([f[1] for f in frames[:4]])
    host = analyzer("seq").analyze_frames(spec, freqs, audio)
    flat = torch.from_numpy(audio.reshape(-1)).cuda()
    view = flat.unfold(0, 2048, 2048)
    got = analyzer("seq").analyze_frames(torch.from_numpy(spec).cuda(), freqs, view)
    np.testing.assert_array_equal(got[0].cpu().numpy(), host[0])


@pytest.mark.gpu
def test_harmonic_broadcast_device_batch_is_copied():
    """A device batch built by ``expand`` of one row (row stride 0) takes the common row rule: it is copied
    and analysed, bit-equal to its ``.contiguous()`` copy. F = 3, K = 512 bins, m = 512 samples. (Before the
    facades shared their marshalling this facade tested stride(1) alone and the library refused the batch
    as a bad layout.)"""
    import torch
    fs, freqs, frames = group("app")
    spec, audio = frames[0]
    assert spec.shape == (512,)
    spectra = torch.from_numpy(spec).cuda()[None, :].expand(3, 512)
    batch = torch.from_numpy(audio[:512]).cuda()[None, :].expand(3, 512)
    assert spectra.stride(0) == 0 and batch.stride(0) == 0
    got = analyzer("app").analyze_frames(spectra, freqs, batch)
    want = analyzer("app").analyze_frames(spectra.contiguous(), freqs, batch.contiguous())
    for a, b in zip(got, want):
        assert a.is_cuda and a.shape[0] == 3
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    rows = got[0].cpu().numpy()
    assert (rows[:, 0] > 0).all()  # (a series is found in every row: none is the zero row)


@pytest.mark.gpu
def test_harmonic_unsupported_and_invalid_shapes():
    """Shapes outside the supported table return OMEGA_EUNSUP with the message (no CPU fallback), bad
    tables OMEGA_EINVAL; a non-finite spectrum is flagged and gives the zero row."""
    from omega_gpu import _lib as L
    from omega_gpu import UnsupportedError
    fs, freqs, frames = group("app")
    spec, audio = frames[0]
    an = analyzer("app")
    with pytest.raises(UnsupportedError, match="8193"):
        an.analyze_frames(np.zeros((1, 8194), np.float32), np.arange(8194.0), None)
    with pytest.raises(UnsupportedError, match="16"):
        an.analyze_frames(np.zeros((1, 8), np.float32), np.arange(8.0), None)
    with pytest.raises(UnsupportedError, match="9000"):
        an.analyze_frames(spec[None], freqs, np.zeros((1, 9000)))
    with pytest.raises(UnsupportedError, match="14"):
        an.analyze_frames(spec[None], freqs, np.ones((1, 14)))
    bad = freqs.copy()
    bad[7] = bad[6]
    with pytest.raises(L.OmegaError, match="increasing"):
        an.analyze_frames(spec[None], bad, None)
    lib, ctx = L.lib(), an._eng._ctx
    cfg = L.HarmonicConfig(48000, 512, 0)
    assert lib.omega_harmonic_configure(ctx, C.byref(cfg), freqs.ctypes.data) == L.EINVAL
    assert b"max_series" in lib.omega_last_error(ctx)
    assert an.detect_harmonic_series(spec, freqs, audio[:10])["formants"] == []  # (:258: len <= 14, no formants)
    x = spec.copy()
    x[100] = np.nan
    out = an.analyze_frames(np.stack([spec, x]), freqs, np.stack([audio, audio]))[0]
    assert out[1, 15] == 2 and not out[1, :15].any() and out[0, 0] > 0 and out[0, 15] == 0


@pytest.mark.gpu
def test_harmonic_metrics_methods():
    """HarmonicMetrics' methods, one frame each through omega_harmonic_metrics: on golden frames with the
    golden's dominant fundamental they give the golden values (same tolerances); for another fundamental
    and for a spectrum without a series they give the restatement's values (the reference computes them for
    any spectrum); they are stateless -- a call between two detect_harmonic_series frames leaves the next
    frame's flux as recorded."""
    from omega_gpu import UnsupportedError
    from omega_gpu.harmonic_analysis import HarmonicMetrics
    g = G()
    dev = dict(zip([str(k) for k in g["dev_names"]], g["dev"]))

    def close(got, want, tol):
        assert rel(got, want) <= tol, (got, want, tol)
    for name, i in (("pure", 1), ("k1025", 2), ("offset", 0)):
        fs, freqs, frames = group(name)
        spec, audio = frames[i]
        hm = HarmonicMetrics(fs)
        ref, e64 = g[f"{name}/{i}/row"], evals(name)[i][1]
        f0 = ref[1]
        close(hm.calculate_thd(spec, freqs, f0), e64["thd"], 4 * dev["thd"])
        close(hm.calculate_thd_plus_noise(spec, freqs, f0), e64["thd_plus_noise"], 4 * dev["thd_plus_noise"])
        assert abs(hm.calculate_harmonic_to_noise_ratio(spec, freqs, f0) - e64["hnr_db"]) <= 4 * dev["hnr_db"]
        close(hm.calculate_inharmonicity(spec, freqs, f0), ref[8], 1e-12)
        close(hm.calculate_spectral_centroid(spec, freqs), ref[4], 1e-9)
        close(hm.calculate_spectral_spread(spec, freqs), ref[5], 1e-9)
        assert hm.calculate_spectral_rolloff(spec, freqs) == ref[7]
        fm = hm.detect_formants_lpc(audio)
        assert len(fm) == int(ref[10])
        for a, b in zip(fm, g[f"{name}/{i}/formants_ext"]):
            close(a, b, 4 * float(g["dev_formant"]))
    # another fundamental than the dominant one, in float64 from the float32 bins like the kernel
    fs, freqs, frames = group("k1025")
    spec, audio = frames[0]
    x64, nyq = spec.astype(np.float64), fs / 2
    hm = HarmonicMetrics(fs)
    for f0 in (freqs[19], 3000.0, 30000.0, 0.0):
        close(hm.calculate_thd(spec, freqs, f0), float(HR.thd(x64, freqs, f0, nyq)), 1e-12)
        close(hm.calculate_thd_plus_noise(spec, freqs, f0), float(HR.thd_plus_noise(x64, freqs, f0, nyq)), 1e-9)
        if f0 > 0:
            close(hm.calculate_inharmonicity(spec, freqs, f0), float(HR.inharmonicity(x64, freqs, f0, nyq)), 1e-12)
            assert abs(hm.calculate_harmonic_to_noise_ratio(spec, freqs, f0) - float(HR.hnr(x64, freqs, f0, nyq))) <= 1e-9
        else:
            assert hm.calculate_inharmonicity(spec, freqs, f0) == 0 and hm.calculate_harmonic_to_noise_ratio(spec, freqs, f0) == 0
    # spectra without a harmonic series: the shape metrics and the formants are computed all the same
    for name, i in (("noseries", 0), ("offset", 1)):
        fs, freqs, frames = group(name)
        spec, audio = frames[i]
        hm = HarmonicMetrics(fs)
        c, sp, ro, _ = HR.centroid_spread_rolloff(spec, freqs)
        close(hm.calculate_spectral_centroid(spec, freqs), float(c), 1e-9)
        close(hm.calculate_spectral_spread(spec, freqs), float(sp), 1e-9)
        assert hm.calculate_spectral_rolloff(spec, freqs) == ro
        ext, _ = HR.formants_ext(audio, fs)
        fm = hm.detect_formants_lpc(audio)
        assert len(fm) == len(ext) > 0
        for a, b in zip(fm, ext):
            close(a, b, 4 * float(g["dev_formant"]))
    assert hm.detect_formants_lpc(np.ones(10)) == [] and hm.detect_formants_lpc(np.zeros(64)) == []
    # flux of two spectra; stateless between an analyzer's frames
    fs, freqs, frames = group("seq")
    e64 = evals("seq")
    hm = HarmonicMetrics(fs)
    close(hm.calculate_spectral_flux(frames[1][0], frames[0][0]), e64[1][1]["spectral_flux"], 4 * dev["spectral_flux"])
    an = analyzer("seq")
    r0 = an.detect_harmonic_series(frames[0][0], freqs, frames[0][1])
    an.metrics.calculate_thd(frames[5][0], freqs, 440.0)
    an.metrics.calculate_spectral_centroid(frames[3][0], np.linspace(0, 24000, 1025))
    assert an.metrics.calculate_spectral_flux(frames[2][0], frames[0][0]) > 0
    r1 = an.detect_harmonic_series(frames[1][0], freqs, frames[1][1])
    assert r0["spectral_flux"] == 0
    close(r1["spectral_flux"], e64[1][1]["spectral_flux"], 4 * dev["spectral_flux"])
    with pytest.raises(UnsupportedError):
        hm.calculate_spectral_rolloff(frames[0][0], freqs, 0.9)
    with pytest.raises(UnsupportedError):
        hm.calculate_thd(frames[0][0], freqs, 440.0, num_harmonics=7)
    with pytest.raises(UnsupportedError):
        hm.detect_formants_lpc(frames[0][1], order=10)


@pytest.mark.gpu
def test_harmonic_nonfinite_previous_and_window_cache():
    """A non-finite spectrum that ends a call is stored like any other: the next call's first frame leaves
    its non-finite bins out of the flux and carries the non-finite flag. Many audio lengths in turn (more
    than the window cache holds) give the rows of a fresh analyzer."""
    fs, freqs, frames = group("k1025")
    spec, audio = frames[0]
    bad = frames[1][0].copy()
    bad[200:210] = np.inf
    an = analyzer("k1025")
    out = an.analyze_frames(bad[None], freqs, None)[0]
    assert out[0, 15] == 2 and not out[0, :15].any()
    nxt = an.analyze_frames(spec[None], freqs, None)[0]
    want = frames[1][0].astype(np.float64)
    keep = np.ones(len(want), bool)
    keep[200:210] = False
    flux = np.sum(np.maximum(np.abs(spec.astype(np.float64)) - np.abs(want), 0)[keep])
    assert nxt[0, 15] == 2 and nxt[0, 0] > 0
    np.testing.assert_allclose(nxt[0, 6], flux, rtol=1e-12)
    assert an.analyze_frames(spec[None], freqs, None)[0][0, 15] == 0
    an = analyzer("k1025")
    first = {}
    for rnd in range(2):
        for m in (2048, 2000, 1900, 1800, 1700, 1600, 1500, 1400, 1300, 1200, 1100):
            an.reset()
            row = an.analyze_frames(spec[None], freqs, audio[None, :m])[0][0]
            assert row[10] > 0
            if rnd == 0:
                first[m] = row
            else:
                np.testing.assert_array_equal(row, first[m])
    check_frame("k1025", 0, first[2048], *[a[0] for a in analyzer("k1025").analyze_frames(spec[None], freqs, audio[None])[1:]])


@pytest.mark.gpu
def test_harmonic_series_with_equal_height_peaks_nine_bins_apart():
    """One 512-bin spectrum of spikes on a zero floor: a fundamental at bin 28 with its harmonics at 56 and 84,
    and an equally high peak 9 bins above it at 37 with harmonics at 74 and 111. The distance rule keeps one of
    the pair: the later one by the kernels' rule, so the series on bin 37 is found and the one on bin 28 is
    not. The expected series are the restatement's with the kept peaks from tools/model/peaks_model.py (scipy
    has no rule for equal heights), and they are not the series the opposite tie rule gives."""
    freqs = np.linspace(0.0, 24000.0, 512)
    spec = np.zeros(512, np.float32)
    spec[[28, 56, 84]] = 1.0, 0.8, 0.6
    spec[[37, 74, 111]] = 1.0, 0.8, 0.6

    def series(later):
        e = HR.analyze(spec, freqs, None, 48000,
                       select=lambda x, cand, d: M.select_by_distance(x, cand, d, later_wins=later)[0])
        return np.concatenate([e["series_peak"][:, None], e["series_bins"]], axis=1)
    want, other = series(True), series(False)
    assert list(want[:, 0]) == [37] and list(other[:, 0]) == [28]  # (a series either way, on another peak)
    assert list(want[0, 1:4]) == [37, 74, 111]
    out, sb, ss = analyzer("app").analyze_frames(spec[None], freqs, None)
    assert out[0, 0] == len(want) and out[0, 15] == 0
    np.testing.assert_array_equal(sb[0, :len(want)], want)
    assert (sb[0, len(want):] == -1).all() and ss[0, 0] > 0.3 and not ss[0, len(want):].any()
