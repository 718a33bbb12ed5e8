"""§8(f) row 7: GenreClassifier.extract_features on the device (omega_genre_features through
omega_gpu.genre_classification) against the reference's own outputs (tests/golden/genre.npz, recorded by
tests/golden/gen_genre.py with the group assertions listed there) and the restatement tests/genre_ref.py,
which is pinned to the golden on the CPU.

Tolerances. The integer decisions are exact: rolloff index, crossing count, distortion count, the five
peak bins, the flags; so are loud, quiet, dynamic_range and the rolloff frequency. Centroid and bandwidth
agree to 1e-9 relative (the float64 sums run in another order). Every float32-path column (rms,
spectral_complexity, bass_emphasis, vocal_presence, high_freq_energy, spectral_flux,
mid_frequency_dominance) must lie within 4 x the reference's own recorded deviation from the float64
evaluation of the same formulas (golden `dev`), with a floor of one float32 ulp, 6e-8 relative. The
device's deviation is printed per frame (run with -s). Recorded reference deviations: rms 5.0e-8,
spectral_complexity 1.7e-6, bass_emphasis 3.6e-7, vocal_presence 1.1e-7, high_freq_energy 2.4e-7,
spectral_flux 9.5e-8, mid_frequency_dominance 2.0e-7.
Observed on an MI355X over all 30 frames: rms, bass_emphasis, vocal_presence, high_freq_energy, spectral_flux
and mid_frequency_dominance are the reference's float32 values bit for bit on every frame (so their
deviation is exactly the reference's own: 5.0e-8, 3.6e-7, 1.1e-7, 2.4e-7, 9.5e-8, 2.0e-7);
spectral_complexity, evaluated in float64 on the device, deviates by at most 2.4e-15 (bit-equal to the
reference's float32 value on the 2 frames where that is the constant 0.3).
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import genre_ref as GR
from conftest import load_golden

GROUPS = ("app", "k1025", "k4097", "m1024", "m4096", "fs44", "offset", "k16a", "k16b", "k16c", "seq", "distort",
          "rolloff", "zeros", "silent", "mid")
COL = {k: i for i, k in enumerate(GR.COLUMNS)}
EXACT = ("rolloff_index", "zero_crossings", "distortion_count", "flags", "loud", "quiet", "dynamic_range",
         "spectral_rolloff")
FEATURE_KEYS = ["spectral_centroid", "spectral_rolloff", "zero_crossing_rate", "spectral_bandwidth", "dynamic_range",
                "percussion_strength", "harmonic_complexity", "estimated_tempo", "pitch_class_concentration",
                "pitch_class_entropy", "chord_change_rate", "key_stability", "bass_emphasis", "beat_regularity",
                "vocal_presence", "high_freq_energy", "spectral_flux", "harmonic_distortion",
                "mid_frequency_dominance", "power_chord_ratio"]


@functools.lru_cache(maxsize=None)
def G():
    return load_golden("genre")


def group(name):
    g = G()
    n = int(g[f"{name}/n"])
    return int(g[f"{name}/fs"]), g[f"{name}/freqs"], [(g[f"{name}/{i}/spec"], g[f"{name}/{i}/audio"]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def evals(name):
    """The float32-path restatement and the float64 evaluation of the group's frames (computed once)."""
    _, freqs, frames = group(name)
    out, prev = [], None
    for spec, audio in frames:
        out.append((GR.features(spec, freqs, audio, prev), GR.features(spec, freqs, audio, prev, f64=True)))
        prev = np.abs(spec) if name == "seq" else None
    return out


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def dev_table():
    g = G()
    return dict(zip([str(k) for k in g["dev_names"]], g["dev"]))


def host(name, i):
    h = json.loads(str(G()[f"{name}/{i}/host"]))
    return h["drum"], h["harmonic"], h["chroma"], h["chords"], h["keys"]


def check_frame(name, i, row, peaks):
    """One device (or restatement) row with its peak bins against frame i of the group's golden."""
    g, p = G(), f"{name}/{i}/"
    ref = g[p + "row"]
    e64 = evals(name)[i][1]
    for k in EXACT:
        assert row[COL[k]] == ref[COL[k]], (name, i, k, row[COL[k]], ref[COL[k]])
    np.testing.assert_array_equal(peaks, g[p + "peak_bins"], err_msg=f"{name} {i} peak bins")
    for k in ("spectral_centroid", "spectral_bandwidth"):
        np.testing.assert_allclose(row[COL[k]], ref[COL[k]], rtol=1e-9, atol=0, err_msg=f"{name} {i} {k}")
    d = {k: rel(row[COL[k]], e64[k]) for k in GR.F32_PATH}
    print(f"{name}[{i}] deviation from the float64 evaluation:", {k: f"{v:.2e}" for k, v in d.items()},
          "bit for bit:", [k for k in GR.F32_PATH if row[COL[k]] == ref[COL[k]]])
    dev = dev_table()
    for k, v in d.items():
        assert v <= max(4 * dev[k], 6e-8), (name, i, k, v, dev[k])


def patterns():
    return json.loads(str(G()["genre_patterns"]))


# ---- CPU ----

@pytest.mark.parametrize("name", GROUPS)
def test_genre_ref_matches_reference_golden(name):
    """tests/genre_ref.py against the reference: its float32 mode reproduces every recorded value exactly,
    its float64 mode deviates by at most the recorded `dev`."""
    g, dev = G(), dev_table()
    for i, (e, e64) in enumerate(evals(name)):
        p = f"{name}/{i}/"
        np.testing.assert_array_equal(GR.row(e), g[p + "row"])
        np.testing.assert_array_equal(e["peak_bins"], g[p + "peak_bins"])
        np.testing.assert_array_equal(e["ranks"], g[p + "ranks"])
        np.testing.assert_array_equal(e["order_stats"], g[p + "order_stats"])
        assert e["mid_branch"] == int(g[p + "mid_branch"]) and e64["rolloff_index"] == int(g[p + "rolloff_index64"])
        check_frame(name, i, GR.row(e), e["peak_bins"])
        for k in GR.F32_PATH:
            assert rel(e[k], e64[k]) <= dev[k] * (1 + 1e-9), (name, i, k)
        # the reference's own dict: the device-side entries are the row's
        ft = dict(json.loads(str(g[p + "features"])))
        assert list(ft) == FEATURE_KEYS
        assert ft["spectral_rolloff"] == e["spectral_rolloff"] and ft["bass_emphasis"] == e["bass_emphasis"]
        assert ft["zero_crossing_rate"] == e["zero_crossings"] / len(group(name)[2][i][1])


def test_genre_golden_group_assertions():
    """Each group does on the committed golden what it was made for."""
    g = G()
    rows = {n: [g[f"{n}/{i}/row"] for i in range(int(g[f"{n}/n"]))] for n in GROUPS}
    # 16-bin tables: bands without bins, the reference's early returns
    for n in ("k16a", "k16b", "k16c"):
        assert g[f"{n}/freqs"].shape == (16,) and any(c == 0 for _, c in GR.band_ranges(g[f"{n}/freqs"]))
    assert rows["k16a"][0][COL["bass_emphasis"]] == 0 and rows["k16a"][0][COL["vocal_presence"]] > 0
    assert rows["k16b"][0][COL["vocal_presence"]] == 0 and rows["k16b"][0][COL["spectral_complexity"]] == 0.3
    assert int(g["k16b/0/mid_branch"]) == 0 and int(g["k16c/0/mid_branch"]) == 0
    assert rows["k16c"][0][COL["high_freq_energy"]] == 0 and rows["k16c"][0][COL["bass_emphasis"]] > 0
    # the flux state
    flux = [r[COL["spectral_flux"]] for r in rows["seq"]]
    assert len(flux) >= 4 and flux[0] == 0 and min(flux[1:]) > 0
    # distortion
    cnt = [int(r[COL["distortion_count"]]) for r in rows["distort"]]
    pk = [g[f"distort/{i}/peak_bins"] for i in range(4)]
    assert any(0 < c < 5 for c in cnt)
    assert any(0 <= b < 5 for b in pk[1])
    assert any(b >= 5 and b * 2 < 512 <= b * 5 for b in pk[2])
    top = [g["distort/3/spec"][b] for b in pk[3]]
    assert len(set(top)) < 5 and list(pk[3]).index(25) < list(pk[3]).index(50) and top[1] == top[2]
    # the float64 running sum picks another rolloff bin
    for i in range(int(g["rolloff/n"])):
        assert int(rows["rolloff"][i][COL["rolloff_index"]]) != int(g[f"rolloff/{i}/rolloff_index64"])
    # exact zeros, runs of equal values, tied order statistics
    for i in range(2):
        x = g[f"zeros/{i}/audio"]
        assert (x == 0).sum() > 20 and len(np.unique(np.abs(x))) < 12
    assert any(g[f"zeros/{i}/order_stats"][0] == g[f"zeros/{i}/order_stats"][1] for i in range(2))
    assert not rows["silent"][0][[c for c in range(17) if c != COL["spectral_complexity"]]].any()
    assert sorted(int(g[f"mid/{i}/mid_branch"]) for i in range(2)) == [1, 2]
    for n in GROUPS:
        for i, (e, _) in enumerate(evals(n)):
            assert e["mid_branch"] == 0 or e["mid_margin"] >= 1e-4, (n, i)
    for i in range(2):
        assert int(g[f"nonfinite/{i}/flags"]) == 2
        assert not (np.isfinite(g[f"nonfinite/{i}/spec"]).all() and np.isfinite(g[f"nonfinite/{i}/audio"]).all())


def classifier_host():
    from omega_gpu.genre_classification import GenreClassifier
    clf = GenreClassifier.__new__(GenreClassifier)  # (the constructor opens the device)
    clf._host_init(48000, patterns())
    return clf


def test_genre_facade_host_logic():
    """The facade's host-side parts against the golden: the feature dict built from a recorded row and the
    recorded drum / harmonic / chroma / history inputs equals the reference's dict, key order included;
    classify with the recorded genre_patterns over a recorded sequence gives the reference's genre order
    and probabilities; the hip_hop_confidence override; no table, a clear error. No device is touched."""
    from omega_gpu.genre_classification import COLUMNS, GenreClassifier
    assert tuple(COLUMNS) == tuple(GR.COLUMNS)
    g = G()
    clf = classifier_host()
    seen = set()
    for name in GROUPS:
        for i, (_, audio) in enumerate(group(name)[2]):
            drum, harm, chroma, chords, keys = host(name, i)
            got = clf.features_from_row(g[f"{name}/{i}/row"], len(audio), drum, harm, chroma, chords, keys)
            want = json.loads(str(g[f"{name}/{i}/features"]))
            assert list(got) == [k for k, _ in want] == FEATURE_KEYS
            for k, v in want:
                assert abs(float(got[k]) - v) <= 1e-15 * abs(v), (name, i, k, got[k], v)
            seen.add((bool(harm.get("harmonic_series")), chroma is None, chords is None, keys is None, bool(drum)))
    assert len(seen) >= 8
    rec = json.loads(str(g["classify"]))
    assert len(rec["features"]) >= 5
    for ft, want in zip(rec["features"], rec["probabilities"]):
        pr = clf.classify(dict(ft))
        assert list(pr) == [k for k, _ in want]
        np.testing.assert_allclose(list(pr.values()), [v for _, v in want], rtol=0, atol=1e-12)
        assert [k for k, _ in clf.get_top_genres(pr)] == [k for k, _ in sorted(want, key=lambda x: x[1], reverse=True)[:3]]
    assert [k for k, _ in clf.get_top_genres(pr, 3)] == [k for k, _ in rec["top3"]]
    hh = json.loads(str(g["classify_hh"]))
    clf = classifier_host()
    plain = classifier_host()
    differs = False
    for ft, want in zip(rec["features"], hh["probabilities"]):
        pr = clf.classify(dict(ft), hip_hop_confidence=hh["confidence"])
        assert list(pr) == [k for k, _ in want]
        np.testing.assert_allclose(list(pr.values()), [v for _, v in want], rtol=0, atol=1e-12)
        differs = differs or pr != plain.classify(dict(ft))
    assert differs
    assert classifier_host().classify({}) != {}  # (every pattern row scores 0: the reference's 'Unknown')
    none = GenreClassifier.__new__(GenreClassifier)
    none._host_init(48000)
    with pytest.raises(ValueError, match="genre_patterns"):
        none.classify(dict(rec["features"][0]))
    with pytest.raises(ValueError):
        GenreClassifier(0)


def test_genre_abi_argument_checks():
    """The entry points' argument checks that run before any device call, and the documented defaults."""
    from omega_gpu import _lib as L
    lib = L.lib()
    cfg = L.GenreConfig()
    lib.omega_genre_config_default(C.byref(cfg))
    assert (cfg.sample_rate, cfg.n_bins) == (48000, 512)
    fr = np.linspace(0, 24000, 512)
    out, pb = np.empty((1, 17)), np.empty((1, 5), np.int32)
    spec, audio = np.zeros(512, np.float32), np.zeros(2048, np.float32)
    assert lib.omega_genre_configure(None, C.byref(cfg), fr.ctypes.data) == L.EINVAL
    assert lib.omega_genre_features(None, spec.ctypes.data, 512, audio.ctypes.data, 0, 2048, 2048, 1, out.ctypes.data,
                                    pb.ctypes.data, L.MEM_HOST) == L.EINVAL
    assert lib.omega_genre_reset(None) == L.EINVAL
    assert b"ABI 5" in lib.omega_version()  # (the entry points are additive)


# ---- GPU ----

def classifier(name):
    from omega_gpu.genre_classification import GenreClassifier
    return GenreClassifier(group(name)[0], genre_patterns=patterns())


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in GROUPS if n != "seq"])
def test_genre_golden_parity(name):
    """Every frame of the group through extract_features_frames (each on a fresh state, as recorded) and
    through extract_features: the reference's dict, the golden values."""
    g = G()
    _, freqs, frames = group(name)
    clf = classifier(name)
    for i, (spec, audio) in enumerate(frames):
        clf.reset()
        out, pb = clf.extract_features_frames(spec[None], freqs, audio[None])
        check_frame(name, i, out[0], pb[0])
        clf.reset()
        ft = clf.extract_features(spec, audio, freqs, *host(name, i))
        want = json.loads(str(g[f"{name}/{i}/features"]))
        assert list(ft) == [k for k, _ in want]
        assert ft == clf.features_from_row(out[0], len(audio), *host(name, i))
    if name == "silent":
        assert not out[0][[c for c in range(17) if c != COL["spectral_complexity"]]].any()
    if name == "rolloff":
        assert int(out[0, COL["rolloff_index"]]) != int(g[f"rolloff/{len(frames) - 1}/rolloff_index64"])


@pytest.mark.gpu
def test_genre_sequence_state_split_and_reset():
    """The stream as one call and split across two: identical rows, the flux carried across the call
    boundary; after reset() the first flux is 0 again."""
    _, freqs, frames = group("seq")
    spec = np.stack([f[0] for f in frames])
    audio = np.stack([f[1] for f in frames])
    one = classifier("seq").extract_features_frames(spec, freqs, audio)
    for i in range(len(frames)):
        check_frame("seq", i, one[0][i], one[1][i])
    clf = classifier("seq")
    a, b = clf.extract_features_frames(spec[:2], freqs, audio[:2]), clf.extract_features_frames(spec[2:], freqs, audio[2:])
    for k in range(2):
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), one[k])
    fl = COL["spectral_flux"]
    assert one[0][0, fl] == 0 and one[0][1:, fl].min() > 0
    again = clf.extract_features_frames(spec[:1], freqs, audio[:1])[0]
    assert again[0, fl] > 0  # (against the last frame)
    clf.reset()
    np.testing.assert_array_equal(clf.extract_features_frames(spec[:1], freqs, audio[:1])[0], one[0][:1])


@pytest.mark.gpu
def test_genre_input_forms():
    """Device tensors give the host rows bitwise: contiguous, an overlapping unfold view of a stream as
    frames, a strided view of wider spectra; float64 audio follows numpy's float64 percentile and rms."""
    import torch
    _, freqs, frames = group("seq")
    spec = np.stack([f[0] for f in frames])
    audio = np.stack([f[1] for f in frames])
    host_out = classifier("seq").extract_features_frames(spec, freqs, audio)
    dev = classifier("seq").extract_features_frames(torch.from_numpy(spec).cuda(), freqs, torch.from_numpy(audio).cuda())
    assert dev[0].is_cuda and dev[1].dtype == torch.int32
    for k in range(2):
        np.testing.assert_array_equal(dev[k].cpu().numpy(), host_out[k])
    # an overlapping stream: hop 512 over one buffer
    stream = np.concatenate([audio[0], audio[1][:512 * 4]]).astype(np.float32)
    view = torch.from_numpy(stream).cuda().unfold(0, 2048, 512)[:5]
    rows = np.stack([stream[i * 512:i * 512 + 2048] for i in range(5)])
    wide = torch.zeros(5, 1100, device="cuda")
    wide[:, :1025] = torch.from_numpy(spec).cuda()
    want = classifier("seq").extract_features_frames(spec, freqs, rows)
    got = classifier("seq").extract_features_frames(wide[:, :1025], freqs, view)
    for k in range(2):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k])
    # float64 audio: the restatement with float64 input (numpy's own float64 percentile, sign and rms)
    x64 = audio[0].astype(np.float64) * 1.000000123
    out = classifier("seq").extract_features_frames(spec[:1], freqs, x64[None])[0][0]
    e = GR.audio_side(x64)
    for k in ("zero_crossings", "loud", "quiet", "dynamic_range"):
        assert out[COL[k]] == e[k], (k, out[COL[k]], e[k])
    assert rel(out[COL["rms"]], e["rms"]) <= 1e-14


@pytest.mark.gpu
def test_genre_batch_independence():
    """33 frames over the k4097 table in one call equal the same frames one by one (the flux handed over
    by running them in order on one classifier)."""
    _, freqs, frames = group("k4097")
    rng = np.random.default_rng(3)
    base = np.stack([f[0] for f in frames] + [G()[f"rolloff/{i}/spec"] for i in range(2)])
    spec = (base[np.arange(33) % 4] * (0.5 + rng.random((33, 1)))).astype(np.float32)
    audio = np.stack([np.roll(frames[i % 2][1], 7 * i) for i in range(33)])
    one = classifier("k4097").extract_features_frames(spec, freqs, audio)
    clf = classifier("k4097")
    for i in range(33):
        r = clf.extract_features_frames(spec[i:i + 1], freqs, audio[i:i + 1])
        np.testing.assert_array_equal(r[0][0], one[0][i], err_msg=f"frame {i}")
        np.testing.assert_array_equal(r[1][0], one[1][i], err_msg=f"frame {i}")
    e = GR.features(spec[32], freqs, audio[32], np.abs(spec[31]))
    for k in EXACT:
        assert one[0][32, COL[k]] == e[k], k


@pytest.mark.gpu
def test_genre_unsupported_shapes_leave_state():
    """K = 15, K = 8194, m = 14 and m = 8193 raise UnsupportedError (no CPU fallback) and leave the flux
    state and the table untouched."""
    from omega_gpu import UnsupportedError
    _, freqs, frames = group("seq")
    spec = np.stack([f[0] for f in frames])
    audio = np.stack([f[1] for f in frames])
    want = classifier("seq").extract_features_frames(spec[:2], freqs, audio[:2])[0]
    clf = classifier("seq")
    clf.extract_features_frames(spec[:1], freqs, audio[:1])
    for K, m in ((15, 2048), (8194, 2048), (1025, 14), (1025, 8193)):
        with pytest.raises(UnsupportedError, match=str(K if K != 1025 else m)):
            clf.extract_features_frames(np.ones((1, K), np.float32), np.arange(float(K)) if K != 1025 else freqs,
                                        np.ones((1, m), np.float32))
    # the library's own checks (the facade's come first): the same codes
    from omega_gpu import _lib as L
    lib, ctx = L.lib(), clf._eng._ctx
    out, pb, one = np.empty((1, 17)), np.empty((1, 5), np.int32), np.ones(9000, np.float32)
    for K in (15, 8194):
        cfg = L.GenreConfig(48000, K)
        assert lib.omega_genre_configure(ctx, C.byref(cfg), np.arange(float(K)).ctypes.data) == L.EUNSUP
    for m in (14, 8193):
        assert lib.omega_genre_features(ctx, spec.ctypes.data, 1025, one.ctypes.data, 0, m, m, 1, out.ctypes.data,
                                        pb.ctypes.data, L.MEM_HOST) == L.EUNSUP
    got = clf.extract_features_frames(spec[1:2], freqs, audio[1:2])[0]
    np.testing.assert_array_equal(got[0], want[1])


@pytest.mark.gpu
def test_genre_nonfinite_frames():
    """A non-finite bin or sample: the flagged zero row, no peaks. The magnitude is stored like any other:
    the following frame's flux leaves the non-finite bins out and carries the flag; the one after is
    clean."""
    g = G()
    _, freqs, _ = group("nonfinite")
    good_s, good_a = g["nonfinite/1/spec"], g["nonfinite/0/audio"]
    clf = classifier("nonfinite")
    for i in range(2):
        clf.reset()
        out, pb = clf.extract_features_frames(np.stack([good_s, g[f"nonfinite/{i}/spec"]]), freqs,
                                              np.stack([good_a, g[f"nonfinite/{i}/audio"]]))
        assert out[1, 16] == int(g[f"nonfinite/{i}/flags"]) == 2 and not out[1, :16].any() and (pb[1] == -1).all()
        assert out[0, 16] == 0 and out[0, COL["zero_crossings"]] > 0
    clf.reset()
    bad = g["nonfinite/0/spec"]
    nxt = (good_s * np.float32(1.25)).astype(np.float32)
    out, _ = clf.extract_features_frames(bad[None], freqs, good_a[None])
    assert out[0, 16] == 2
    out, _ = clf.extract_features_frames(np.stack([nxt, good_s]), freqs, np.stack([good_a, good_a]))
    e = GR.features(nxt, freqs, good_a, np.abs(bad))
    assert e["flags"] == 2 and e["spectral_flux"] > 0
    assert out[0, 16] == 2 and out[0, COL["spectral_flux"]] == e["spectral_flux"]
    assert out[1, 16] == 0 and out[1, COL["spectral_flux"]] == GR.features(good_s, freqs, good_a, nxt)["spectral_flux"]
