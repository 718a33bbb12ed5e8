"""The feature families' float64 host tables (csrc/design.cpp: twiddles64, np_window64, savgol_cubic; kept per
context in omega_ctx::tables, DESIGN.md "Host tables").

On the CPU: tests/abi/tables_dump.cpp, a stand-alone host program, prints the builders' outputs as bit patterns,
and each must equal, bit for bit, the expression of the call site that built the table before the builders were
shared, restated here with math.cos / math.sin (the same libm) and numpy:
  twiddles  pitch's cos(pi q / n), -sin(pi q / n) for q <= n; everyone else's cos(2 pi q / period),
            -sin(2 pi q / period) -- the real transform's two tables, phase's / hip-hop's, bass zoom's 8192 and one
            length that is no power of two;
  windows   np.hanning(M) and np.hamming(M), and np_window's own formula 0.5 + 0.5 cos(pi n / (M - 1)),
            n = 1 - M + 2 i (numpy's route; [1.0] for M = 1);
  weights   savgol_cubic(21) against the 441 values the (21, 3)-only function it replaced returned
            (tests/golden/savgol_21_3.npz, recorded from that function once), and savgol_cubic(5 / 7 / 9 / 11 / 21)
            against scipy's own savgol_coeffs rows to 1e-12 (another solver).

On the device: what only sharing can break -- equal periods asked for with different counts, and the order of
first use. One context runs phase, hip-hop, transients and transient detection at 256 and then 512 samples per
frame (period / 2 of one is the period of another's first table), pitch at 2048 (period 4096) and a transient at
4096; every output must equal, bit for bit, the same call in a context of its own. Then the same with the
families in the reverse order."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import signal

from conftest import REPO, load_golden
from host_program import compile_host_program

SRC = os.path.join(REPO, "tests", "abi", "tables_dump.cpp")
HANN, HAMMING = 1, 2  # OMEGA_WIN_*
WINDOW_LENGTHS = (1, 2, 15, 64, 512, 1024, 2048)
SAVGOL_WINDOWS = (5, 7, 9, 11, 21)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = compile_host_program(SRC, str(tmp_path_factory.mktemp("tables") / "tables_dump"))

    def run(lines):
        """one uint64 array of bit patterns per request line"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        out = [np.array([int(t, 16) for t in ln.split()], np.uint64) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def bits(values):
    return np.ascontiguousarray(values, np.float64).ravel().view(np.uint64)


def assert_bits(got, want, what):
    want = bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "first differing entry", int(bad[0]), hex(got[bad[0]]), hex(want[bad[0]]))


def twiddles(period, count):
    """The former call sites' loop: (cos(2 * M_PI * q / period), -sin(2 * M_PI * q / period)), interleaved."""
    return [v for q in range(count) for v in (math.cos(2 * math.pi * q / period), -math.sin(2 * math.pi * q / period))]


def test_twiddles_equal_every_former_site(dump):
    # (period, count) as the sites ask now; each former table is this one or a prefix of it
    asks = [(n // 2, n // 4 + 1) for n in (64, 256, 8192)]      # the real transform's first table (was n / 4 entries)
    asks += [(n, n // 2 + 1) for n in (64, 256, 8192)]          # its second; hip-hop's; phase's (was m / 2 entries)
    asks += [(8192, 8192), (1000, 1000)]                        # bass zoom's; a length that is no power of two
    got = dump([f"tw {p} {c}" for p, c in asks])
    for (p, c), g in zip(asks, got):
        assert_bits(g, twiddles(p, c), ("twiddles", p, c))
    # pitch wrote its table of period 2 n as cos(kPi * q / n), -sin(kPi * q / n), q <= n
    pitch = (2048, 4096, 8192)
    got = dump([f"tw {2 * n} {n + 1}" for n in pitch])
    for n, g in zip(pitch, got):
        want = [v for q in range(n + 1) for v in (math.cos(math.pi * q / n), -math.sin(math.pi * q / n))]
        assert_bits(g, want, ("pitch twiddles", n))


def np_window_formula(kind, M):
    """design.cpp's np_window per point, as every former site called it (and [1.0] for M = 1)."""
    a, b = {HANN: (0.5, 0.5), HAMMING: (0.54, 0.46)}[kind]
    return [1.0] if M == 1 else [a + b * math.cos(math.pi * float(1 - M + 2 * i) / (M - 1)) for i in range(M)]


@pytest.mark.parametrize("kind,numpys", [(HANN, np.hanning), (HAMMING, np.hamming)])
def test_windows_equal_numpys_and_the_former_formula(dump, kind, numpys):
    got = dump([f"win {kind} {M}" for M in WINDOW_LENGTHS])
    for M, g in zip(WINDOW_LENGTHS, got):
        assert_bits(g, np_window_formula(kind, M), ("np_window", kind, M))
        assert_bits(g, numpys(M), (numpys.__name__, M))


def test_savgol_cubic_21_equals_the_function_it_replaced(dump):
    want = load_golden("savgol_21_3")["W"]
    assert want.shape == (21, 21) and want.dtype == np.float64
    assert_bits(dump(["sg 21"])[0], want, "savgol_cubic(21)")


def test_savgol_cubic_rows_are_scipys(dump):
    """Every window the library asks for, against scipy's own solver. The weights are at most 1 in magnitude; both
    sides solve a four-parameter least-squares problem whose condition number stays below 1e3 for these windows
    (scipy's in unscaled sample positions by lstsq, the library's in positions scaled to [-1, 1] through the normal
    equations), so each is within about 1e3 * 2.2e-16 of the exact weight: 1e-12 covers the two together."""
    got = dump([f"sg {w}" for w in SAVGOL_WINDOWS])
    for w, g in zip(SAVGOL_WINDOWS, got):
        W = g.view(np.float64).reshape(w, w)
        # row p: the cubic fitted to the window, evaluated at window position p
        want = np.stack([signal.savgol_coeffs(w, 3, pos=p, use="dot") for p in range(w)])
        err = float(np.max(np.abs(W - want)))
        print(f"savgol_cubic({w}) against scipy: {err:.2e}")
        assert err <= 1e-12, (w, err)


# ---- the shared cache on the device ----

FS = 48000


def _engine():
    from omega_gpu.engine import utility_engine
    return utility_engine(FS)


def _host(eng, fn, *args):
    from omega_gpu import _lib as L
    eng._check(fn(eng._ctx, *args, L.MEM_HOST))


def _frames(m, seed):
    """two frames [2, m] float64 and their magnitude spectra [2, m / 2 + 1] float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(2 * m).reshape(2, m) / FS
    x = 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 3000.0 * t) + 0.05 * rng.standard_normal((2, m))
    x[1, m // 3:m // 3 + 8] += 0.5  # (something for the envelopes to find)
    spec = np.abs(np.fft.rfft(x * np.hanning(m), axis=1)).astype(np.float32)
    return np.ascontiguousarray(x), np.ascontiguousarray(spec)


def _phase(eng, m):
    from omega_gpu import _lib as L
    from omega_gpu import phase_correlation as P
    x, _ = _frames(m, 1)
    y = np.ascontiguousarray(0.7 * x + 0.3 * np.roll(x, 5, axis=1))
    edges = np.logspace(np.log10(20), np.log10(20000), P.N_BANDS + 1)
    cfg = L.PhaseConfig(FS, m)
    eng._check(L.lib().omega_phase_configure(eng._ctx, C.byref(cfg), edges.ctypes.data))
    out, pts = np.empty((2, len(P.COLUMNS))), np.empty((2, P.N_POINTS, 2))
    _host(eng, L.lib().omega_phase_correlation, x.ctypes.data, y.ctypes.data, 1, m, 2, out.ctypes.data, pts.ctypes.data)
    return out, pts


def _hiphop(eng, m):
    from omega_gpu import _lib as L
    from omega_gpu import hip_hop_detector as H
    x, spec = _frames(m, 2)
    freqs = np.ascontiguousarray(np.fft.rfftfreq(m, 1.0 / FS))
    cfg = L.HipHopConfig(FS, spec.shape[1])
    eng._check(L.lib().omega_hiphop_configure(eng._ctx, C.byref(cfg), freqs.ctypes.data))
    out, peaks = np.empty((2, len(H.COLUMNS))), np.empty((2, H.N_PEAKS), np.int32)
    _host(eng, L.lib().omega_hiphop_features, spec.ctypes.data, spec.shape[1], x.ctypes.data, 1, m, m, 2,
          out.ctypes.data, peaks.ctypes.data)
    return out, peaks


def _transients(eng, m):
    from omega_gpu import _lib as L
    from omega_gpu import transient as T
    x, _ = _frames(m, 3)
    out = np.empty((2, len(T.COLUMNS)))
    _host(eng, L.lib().omega_transients, x.ctypes.data, 1, 2, m, m, out.ctypes.data)
    return (out,)


def _tdetect(eng, m):
    from omega_gpu import _lib as L
    from omega_gpu import transient_detection as D
    x, spec = _frames(m, 4)
    cfg = L.TdetectConfig(float(FS), spec.shape[1], m)
    eng._check(L.lib().omega_tdetect_configure(eng._ctx, C.byref(cfg)))
    out, state = np.empty((2, len(D.COLUMNS))), np.empty(D.STATE_LEN)
    _host(eng, L.lib().omega_tdetect_features, spec.ctypes.data, spec.shape[1], x.ctypes.data, 1, 2, m, None,
          state.ctypes.data, out.ctypes.data)
    return out, state


def _pitch(eng, n):
    from omega_gpu import _lib as L
    from omega_gpu import pitch_detection as P
    x, _ = _frames(n, 5)
    cfg = L.PitchConfig()
    L.lib().omega_pitch_config_default(C.byref(cfg))
    eng._check(L.lib().omega_pitch_configure(eng._ctx, C.byref(cfg)))
    out = np.empty((2, len(P.COLUMNS)))
    _host(eng, L.lib().omega_pitch_detect, x.ctypes.data, 1, 2, n, n, out.ctypes.data)
    return (out,)


FAMILIES = (_phase, _hiphop, _transients, _tdetect)
TAIL = ((_pitch, 2048), (_transients, 4096))


@pytest.fixture(scope="module")
def alone():
    """every call's outputs from a context of its own (computed once)"""
    ref = {}
    for fn, m in [(fn, m) for m in (256, 512) for fn in FAMILIES] + list(TAIL):
        eng = _engine()
        ref[fn.__name__, m] = fn(eng, m)
        eng.close()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("families", [FAMILIES, FAMILIES[::-1]], ids=["forward", "reversed"])
def test_one_context_shares_tables_without_changing_a_bit(alone, families):
    eng = _engine()
    try:
        for fn, m in [(fn, m) for m in (256, 512) for fn in families] + list(TAIL):
            got, want = fn(eng, m), alone[fn.__name__, m]
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.tobytes() == w.tobytes(), (fn.__name__, m, "output", i)
    finally:
        eng.close()
