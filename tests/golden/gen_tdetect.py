"""Makes tests/golden/tdetect.npz by calling the reference's TransientDetectionPanel
(omega4/panels/transient_detection.py:11-381, :559-574) itself (build container only; TEST INFRASTRUCTURE ONLY).
Run from the repo root with the reference checkout's path:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_tdetect.py <reference checkout>

The reference module is loaded by path with ``pygame`` stubbed (the module imports it at the top; nothing is
drawn) and ``time.time`` replaced by a deterministic stepping clock. Each group is ONE stream: one reference
object is fed the group's float64 frames and float32 spectra in order (the frames hold float32-representable
values and are stored as float32). Written per group: fs, the frames, the
spectra and the rows in tests/tdetect_ref.py's COLUMNS order, chained through the state blob from the stream's
start. The rows are tests/tdetect_ref.py's -- the reference's own numpy / scipy expressions with every sum that
the device forms in float64 taken by math.fsum -- and are asserted here against the reference object after
every frame: its envelope, peak level, last flux spectrum, previous phase row and last novelty, and through the
facade's host logic (omega_gpu.transient_detection on _host_init, no device) every public attribute.

  m256, m512, m1024   48 kHz, K = m / 2 + 1: no HF column and no novelty; no novelty; both
  app        48 kHz, m 2048, K 513: a kick, a quieter kick, white noise, a decaying burst, a 400 Hz tone, a
             snare-like mix, a click, silence
  m8192      2 frames, K 4097
  fs44, fs16 44100 and 16000 Hz, m 2048, K 513
  k2, k8193  K 2 and K 8193, m 2048
  zero       an all-zero frame between two others
  nonfinite  a NaN sample and an infinite bin between finite frames: flags only, the stream passes them over
             (the reference is not fed them)
  edge       a peak at index 0, a peak at the last index, a frame that never falls below a tenth of its peak
  seq_fast, seq_slow   300 update() steps each of ONE reference object over a pool of the app group's frames
             (`idx`), frozen over `frozen`, the clock stepping 1/60 s and 0.5 s: `sensitivity` rises in the
             first and falls in the second (asserted). After every step: the row and every public attribute.

Margins, asserted here (conditions on the inputs, not measurements; a frame or a seed that misses one is not
recorded): the rolloff prefix sums at least 1e-6 relative away from 0.85 of the total; every |x_i| at least
1e-9 peak away from a tenth of the peak; the best two |x| distinct or exactly equal; every novelty bin whose
magnitude exceeds 1e-9 / 2 of the magnitudes' sum has its phase 1e-6 rad away from the +-pi cut (DC and Nyquist
are such bins only with a real part that far from 0); in the sequences the energy ratio, the flux ratio, the
novelty ratio and hf_ratio at least 1e-6 relative away from their thresholds, and every comparison of the
classification ladder 1e-4 (its operands carry the reference's float32 sums).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "audio-analyzer-omega_amd"))
import tdetect_ref as TR  # noqa: E402

F64_BAR = 1e-9
F32_BAR = 64 * 2.0 ** -24  # tests/test_transient_detection.py derives it
TYPES = ["None", "Kick", "Snare", "Tom", "HiHat", "Cymbal", "Perc", "Other"]
FLOATS = ("transient_strength", "attack_time", "decay_time", "peak_level", "rms_level", "crest_factor", "envelope",
          "sensitivity", "prev_envelope", "last_zcr", "last_rolloff")
FLOATS32 = ("last_centroid",)


class Clock:
    """The time of update() step i is T0 + i * step, however often it is read."""
    T0 = 1000.0

    def __init__(self, step):
        self.t, self.step = self.T0, step

    def at(self, i):
        self.t = self.T0 + i * self.step

    def __call__(self):
        return self.t


def import_reference(path):
    sys.dont_write_bytecode = True
    sys.modules.setdefault("pygame", types.ModuleType("pygame"))
    spec = importlib.util.spec_from_file_location(
        "ref_transient_detection", os.path.join(path, "omega4", "panels", "transient_detection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TransientDetectionPanel


def host_panel(fs, clock):
    from omega_gpu.transient_detection import TransientDetectionPanel
    p = TransientDetectionPanel.__new__(TransientDetectionPanel)
    p._host_init(fs, clock)
    return p


def far(a, b, rel, what):
    assert abs(a - b) >= rel * max(abs(a), abs(b)) and a != b, (what, a, b)


def frame_margins(what, spec, x):
    ax = np.abs(x)
    pk = ax.max()
    if pk > 0:
        assert np.all(np.abs(ax - 0.1 * pk) >= 1e-9 * pk), (what, "tenth of the peak")
        top = np.sort(ax)[-2:]
        assert top[0] == top[1] or top[1] - top[0] >= 1e-12 * pk, (what, "argmax")
    s = spec.astype(np.float64)
    total = TR.fsum(s)
    if total > 0:
        cum = np.cumsum(s)
        assert np.all(np.abs(cum - 0.85 * total) >= 1e-6 * total), (what, "rolloff")
    if len(x) >= 1024:
        ph, mag = TR.phase_spectrum(x)
        big = mag * 2 > 1e-9 * TR.fsum(mag)
        assert np.all(np.pi - np.abs(ph[big][1:-1]) >= 1e-6), (what, "phase cut")


def same_state(what, ref, host):
    """Every public attribute of the reference object against the facade's host logic."""
    for k in ("transient_detected", "transient_type", "update_counter"):
        assert getattr(ref, k) == getattr(host, k), (what, k, getattr(ref, k), getattr(host, k))
    for k in FLOATS + FLOATS32:
        a, b = float(getattr(ref, k)), float(getattr(host, k))
        bar = F32_BAR if k in FLOATS32 else F64_BAR
        assert abs(a - b) <= bar * max(abs(a), 1e-300), (what, k, a, b)
    assert np.all(np.abs(ref.band_energies - host.band_energies) <= F32_BAR), (what, "band_energies")
    for k in ("transient_history", "envelope_history", "transient_events", "novelty_history"):
        assert len(getattr(ref, k)) == len(getattr(host, k)), (what, k)
    assert len(ref.spectral_flux_history) == len(host._flux_sums), what
    for a, b in zip(ref.transient_events, host.transient_events):
        assert a["time"] == b["time"] and a["type"] == b["type"], (what, a, b)
    assert list(ref.get_status()) == list(host.get_status()), what


def step_margins(what, host, row, before):
    """The decisions of one applied row, from the facade's state before (`before`) and after it."""
    flags = int(row[0])
    if before["prev_envelope"] > 0:
        far(row[1] / before["prev_envelope"], before["sensitivity"], 1e-6, (what, "energy ratio"))
    if not flags & TR.FLAG_NO_FLUX:
        avg = np.mean(before["flux_sums"])
        if avg > 0:
            far(row[5], avg * 1.8, 1e-6, (what, "flux"))
    if not flags & TR.FLAG_NO_NOVELTY:
        thr = np.median(list(host.novelty_history)) * 2.5
        far(row[6], thr if thr > 0 else 0.001, 1e-6, (what, "novelty"))
    if not flags & TR.FLAG_NO_HF and row[3] > 0:
        far(row[8] / row[3], 0.3, 1e-6, (what, "hf ratio"))
    if host.transient_detected:
        be, c = host.band_energies, float(host.last_centroid)
        for a, b in ((be[0], 0.7), (c, 150), (be[1], 0.4), (c, 200), (c, 800), (host.last_zcr, 0.1),
                     (host.last_zcr, 0.3), (host.last_rolloff, 5000), (c, 1000), (be[3], 0.4), (be[2], 0.5)):
            far(float(a), b, 1e-4, (what, "ladder", b))


def snapshot(p):
    return {"prev_envelope": float(p.prev_envelope), "sensitivity": float(p.sensitivity),
            "flux_sums": [float(v) for v in p._flux_sums]}


def attrs(ref):
    return [float(ref.transient_detected), float(ref.transient_strength), float(TYPES.index(ref.transient_type)),
            float(ref.attack_time), float(ref.decay_time), float(ref.peak_level), float(ref.rms_level),
            float(ref.crest_factor), float(ref.envelope), float(ref.sensitivity), float(ref.last_centroid),
            float(ref.last_zcr), float(ref.last_rolloff), *[float(v) for v in ref.band_energies],
            float(len(ref.transient_history)), float(len(ref.envelope_history)), float(len(ref.transient_events)),
            float(len(ref.spectral_flux_history)), float(len(ref.novelty_history)), float(ref.update_counter),
            float(ref.transient_events[-1]["time"]) if ref.transient_events else 0.0, float(ref.prev_envelope)]


ATTRS = ("detected", "strength", "type", "attack_time", "decay_time", "peak_level", "rms_level", "crest_factor",
         "envelope", "sensitivity", "centroid", "zcr", "rolloff", "band0", "band1", "band2", "band3",
         "n_transient_history", "n_envelope_history", "n_events", "n_flux_history", "n_novelty_history",
         "update_counter", "last_event_time", "prev_envelope")


def run_stream(Ref, what, fs, steps, clock_step, check_steps):
    """steps: (spectrum float32, frame float64, frozen). Returns the rows and the reference's attributes after
    every step; asserts the reference against tests/tdetect_ref.py and the facade's host logic throughout."""
    import time
    clock = Clock(clock_step)
    time.time = clock
    ref = Ref(fs)
    hclock = Clock(clock_step)
    host = host_panel(fs, hclock)
    state = None
    out_rows, out_attrs = [], []
    for i, (spec, x, frozen) in enumerate(steps):
        w = (what, i)
        clock.at(i)
        hclock.at(i)
        r, new = TR.row(spec, x, fs, state)
        ref.is_frozen = host.is_frozen = bool(frozen)
        finite = not int(r[0]) & TR.FLAG_NONFINITE
        if finite and not frozen:
            frame_margins(w, spec, x)
            before = snapshot(host)
            with np.errstate(all="ignore"):
                ref.update(x, spec)
            assert host._apply_row(r, len(spec), len(x), new)
            state = new
            # the reference's own intermediates
            assert float(ref.envelope) == r[1] and float(ref.peak_level) == r[2], w
            assert np.array_equal(ref.spectral_flux_history[-1], new[4:4 + TR.FLUX_BINS]), w
            if len(x) >= 1024:
                assert np.array_equal(ref.prev_phase, new[4 + TR.FLUX_BINS:4 + TR.FLUX_BINS + TR.PHASE_BINS]), w
                if not int(r[0]) & TR.FLAG_NO_NOVELTY:
                    assert abs(ref.novelty_history[-1] - r[6]) <= 1e-12 * np.pi * max(r[7], 1e-300), w
            if check_steps:
                step_margins(w, host, r, before)
        elif not finite:
            assert not np.any(r[1:])
            r_only_flag, same = r, np.array_equal(new, state if state is not None else np.zeros(TR.STATE_LEN))
            assert same and int(r_only_flag[0]) == TR.FLAG_NONFINITE, w
        else:
            ref.update(x, spec)  # frozen: nothing moves
            r = np.zeros(len(TR.COLUMNS))
        same_state(w, ref, host)
        out_rows.append(r)
        out_attrs.append(attrs(ref))
    return np.array(out_rows), np.array(out_attrs), ref


def spectrum_of(x, K):
    """K float32 magnitudes: the Hann spectrum of the first 2 (K - 1) samples (zero-padded; at least 1024)."""
    n = max(2 * (K - 1), 1024)
    seg = np.zeros(n)
    seg[:min(n, len(x))] = x[:n]
    return np.abs(np.fft.rfft(seg * np.hanning(n))).astype(np.float32)[:K]


def make_frames(fs, m, seed):
    """Eight frames of one stream: kick, quiet kick, noise, burst, tone, snare-like, click, near-silence."""
    rng = np.random.default_rng(seed)
    t = np.arange(m) / fs
    nz = lambda a: a * rng.standard_normal(m)  # noqa: E731
    dec = np.exp(-t * 8000.0 / m * 3)
    kick = 0.5 * np.sin(2 * np.pi * 55 * t + 0.3) + nz(2e-4)
    burst = np.zeros(m)
    burst[m // 4:] = (0.6 * np.sin(2 * np.pi * 900 * t) * dec)[:m - m // 4]
    click = np.zeros(m)
    click[m // 2] = 0.9
    click[m // 2 + 1] = -0.5
    return [kick, 0.25 * kick + nz(1e-4), nz(0.08), burst + nz(2e-4),
            0.3 * np.sin(2 * np.pi * 400 * t + 1.0) + nz(2e-4),
            0.3 * np.sin(2 * np.pi * 180 * t) * dec + nz(0.03) * dec + nz(1e-4), click + nz(2e-4), nz(1e-5)]


def record(Ref, out, group, fs, frames, K, feed=None):
    frames = np.asarray(frames, np.float32).astype(np.float64)  # (float32-representable: stored as float32)
    spectra = np.stack([spectrum_of(np.nan_to_num(x, posinf=0.0), K) for x in frames]) if feed is None else feed
    steps = [(s, x, False) for s, x in zip(spectra, frames)]
    rows, at, _ = run_stream(Ref, group, fs, steps, 1 / 60, False)
    out[f"{group}/fs"] = np.int64(fs)
    out[f"{group}/frame"] = frames.astype(np.float32)
    out[f"{group}/spec"] = spectra
    out[f"{group}/row"] = rows
    out[f"{group}/attrs"] = at
    return rows


def first_seed(fn, what, seeds=range(1, 60)):
    for seed in seeds:
        try:
            r = fn(seed)
        except AssertionError as e:
            print(what, "seed", seed, "misses a margin:", str(e)[:120])
            continue
        print(what, "seed", seed)
        return r
    raise AssertionError(f"{what}: no seed keeps the margins")


def main(ref_path):
    Ref = import_reference(ref_path)
    out = {}
    for m in (256, 512, 1024):
        first_seed(lambda s, m=m: record(Ref, out, f"m{m}", 48000, make_frames(48000, m, s)[:6], m // 2 + 1), f"m{m}")
    app = first_seed(lambda s: (record(Ref, out, "app", 48000, make_frames(48000, 2048, s), 513), s), "app")[1]
    pool = list(out["app/frame"].astype(np.float64))
    first_seed(lambda s: record(Ref, out, "m8192", 48000, make_frames(48000, 8192, s)[2:4], 4097), "m8192")
    first_seed(lambda s: record(Ref, out, "fs44", 44100, make_frames(44100, 2048, s)[:4], 513), "fs44")
    first_seed(lambda s: record(Ref, out, "fs16", 16000, make_frames(16000, 2048, s)[:4], 513), "fs16")
    first_seed(lambda s: record(Ref, out, "k2", 48000, make_frames(48000, 2048, s)[:3], 2), "k2")
    first_seed(lambda s: record(Ref, out, "k8193", 48000, make_frames(48000, 2048, s)[2:4], 8193), "k8193")
    r = record(Ref, out, "zero", 48000, [pool[2], np.zeros(2048), pool[3]], 513)
    assert r[1, 2] == 0 and r[1, 10] == 0 and r[1, 12] == 2047 and r[1, 13] == 0, r[1]
    bad_a = pool[4].copy()
    bad_a[7] = np.nan
    sp = np.stack([spectrum_of(x, 513) for x in (pool[2], bad_a * 0, pool[3], pool[4], pool[5])])
    sp[1] = sp[0]
    sp[3, 100] = np.inf
    r = record(Ref, out, "nonfinite", 48000, [pool[2], bad_a, pool[3], pool[4], pool[5]], 513, feed=sp)
    assert list(r[:, 0].astype(int) & 1) == [0, 1, 0, 1, 0] and not int(r[4, 0]) & TR.FLAG_NO_NOVELTY, r[:, 0]
    rng = np.random.default_rng(5)
    e0 = 0.01 * rng.standard_normal(2048)
    e0[0] = 0.8
    e1 = 0.01 * rng.standard_normal(2048)
    e1[-1] = -0.8
    e2 = 0.5 + 0.05 * rng.standard_normal(2048)  # never below a tenth of its peak
    r = record(Ref, out, "edge", 48000, [e0, e1, e2], 513)
    assert r[0, 10] == 0 and r[1, 10] == 2047 and r[2, 11] == 0 and r[2, 12] == 2047, r[:, 10:13]

    # the two update() sequences over the app group's frames
    specs = out["app/spec"]
    frames32 = out["app/frame"].astype(np.float64)

    def sequence(name, clock_step, seed, weights, rises):
        rng = np.random.default_rng(seed)
        if rises:
            idx = rng.choice(8, 300, p=np.array(weights) / np.sum(weights))
        else:
            idx = np.zeros(300, np.int64)
            idx[rng.choice(np.arange(4, 296, 8), 30, replace=False)] = rng.choice([2, 3, 5, 6], 30)
        frozen = np.zeros(300, np.int8)
        frozen[100:106] = 1
        frozen[200] = 1
        steps = [(specs[k], frames32[k], bool(z)) for k, z in zip(idx, frozen)]
        rows, at, ref = run_stream(Ref, name, 48000, steps, clock_step, True)
        sens = at[:, ATTRS.index("sensitivity")]
        assert (sens.max() > 1.5 and sens[-1] > 1.5) if rises else (sens.min() < 1.5 and sens[-1] < 1.5), (name, sens[-1])
        assert len(ref.transient_history) == 293 and len(ref.transient_events) >= 10, name
        out[f"{name}/idx"] = idx.astype(np.int32)
        out[f"{name}/frozen"] = frozen
        out[f"{name}/clock_step"] = np.float64(clock_step)
        out[f"{name}/row"] = rows
        out[f"{name}/attrs"] = at
        print(name, "sensitivity", sens[0], "->", sens[-1], "events", len(ref.transient_events),
              "types", sorted(set(TYPES[int(v)] for v in at[:, 2])))

    first_seed(lambda s: sequence("seq_fast", 1 / 60, s, [2, 2, 4, 2, 1, 2, 2, 1], True), "seq_fast")
    first_seed(lambda s: sequence("seq_slow", 0.5, s, None, False), "seq_slow")
    out["types"] = np.array(TYPES)
    out["attr_names"] = np.array(ATTRS)
    out["versions"] = np.array([np.__version__, scipy.__version__])
    path = os.path.join(HERE, "tdetect.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
