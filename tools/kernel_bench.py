#!/usr/bin/env python3
"""Run one stage of the cfg2 hot path in isolation (for rocprofv3 counter passes and A/B timing).

  python tools/kernel_bench.py {batch,tp,kw,mrfft,meters,all,host,spectra,drums,post,pitch,harmonic,genre,room,voice,waterfall,tonal,meterpanel} [--reps N]

spectra-bands / spectra-chroma / spectra-mag: the cfg3 kernel with one output set only (where its LDS
bank conflicts and time come from); spectra-rot: bench.py's cfg3 call, rotating over 4 distinct input
batches (537 MB: the frames come from HBM, not the Infinity Cache).
room: omega_room_modes over 512 resident spectra at K = 92 (16384-point) and K = 11 (2048-point) in-range bins
and omega_room_decay over 8 resident histories of 122880 samples; one event pair per call, median / min / max.
voice: omega_voice_features over 512 resident frames at the app's shape (K 1025, m 2048, float64 audio): the
golden's `app` frames (tests/golden/voice.npz) repeated.
waterfall: omega_waterfall_rows over 4096 resident frames (1025 bins, 853 cells; float32 and float64, with and without
the RGB output) and omega_waterfall_colors over a 200 x 853 history; with --lib, another build of the same ABI.
tonal: omega_tonal_features over 4096 resident chroma rows and omega_tonal_spectra over 4096 resident spectra of 4097
bins, rows only and with the four detail matrices; with --lib, a build with another OMEGA_TONAL_LANES.
meterpanel: omega_meterpanel_update on resident float64 frames at 2048, 16384, 256 and 1 samples (1, 256 and 4096
frames); --samples and --frames pick one shape; with --lib, a build of the measured alternatives (make alt).
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-analyzer-omega_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def room(reps):
    """RoomModeAnalyzer's two device calls on resident inputs: per-call event times after warm-up."""
    from omega_gpu import RoomModeAnalyzer
    from omega_gpu import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(12)

    def timed(label, unit, n, call):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            call()
            e.record()
            e.synchronize()
            us.append(s.elapsed_time(e) * 1e3)
        med = float(np.median(us))
        print(f"room {label}: median {med:.1f} us per call of {n} {unit} (min {min(us):.1f}, max {max(us):.1f}; "
              f"{med / n:.3f} us per {unit[:-1]})")

    t = np.arange(16384) / 48000.0
    for m in (16384, 2048):
        x = sum(np.sin(2 * np.pi * f * t[:m] + k) for k, f in enumerate((47.0, 94.0, 141.0, 230.0)))
        x = x[None, :] + 0.02 * rng.standard_normal((512, m))
        spec = torch.from_numpy(np.abs(np.fft.rfft(x * np.blackman(m), axis=1)).astype(np.float32)).cuda()
        rm = RoomModeAnalyzer(48000)
        freqs = np.linspace(0, 24000, m // 2 + 1)
        rows = rm.analyze_spectra(spec, freqs)  # (configures the table)
        K = int(np.sum((freqs >= 30) & (freqs <= 300)))
        print(f"room modes K = {K}: {int(rows[0, 0, 0])} modes in frame 0")
        rm._eng._bind_stream(spec)
        timed(f"modes K = {K}", "frames", 512, lambda: rm._eng._check(lib.omega_room_modes(
            rm._eng._ctx, spec.data_ptr(), 0, spec.shape[1], 512, rows.data_ptr(), L.MEM_DEVICE)))
    Ln = 60 * 2048
    h = rng.standard_normal((8, Ln)) * np.exp(-7.0 * np.arange(Ln) / Ln)[None, :]
    for dt in (torch.float32, torch.float64):
        hd = torch.from_numpy(h).to(dt).cuda()
        out, en = rm.analyze_histories(hd, 2048)
        timed(f"rt60 {str(dt).split('.')[1]}", "streams", 8, lambda: rm._eng._check(lib.omega_room_decay(
            rm._eng._ctx, hd.data_ptr(), int(dt == torch.float64), Ln, Ln, 2048, 8, out.data_ptr(), en.data_ptr(),
            L.MEM_DEVICE)))
    print("room rt60 row 0:", out[0].cpu().numpy())


def voice(reps):
    """VoiceDetectionPanel's device call on resident inputs: per-call event times after warm-up."""
    from omega_gpu import VoiceDetectionPanel
    from omega_gpu import _lib as L
    lib = L.lib()
    G = np.load(os.path.join(REPO, "tests", "golden", "voice.npz"))
    fr = G["app/frame"].astype(np.float64) * np.hanning(2048)
    pick = np.arange(512) % len(fr)
    spec = torch.from_numpy(G["app/spec"][pick]).cuda()
    audio = torch.from_numpy(fr[pick]).cuda()
    vp = VoiceDetectionPanel(48000)
    rows = vp.analyze_frames(spec, audio)  # (configures the shape)
    print("voice row 0:", rows[0].cpu().numpy())
    vp._eng._bind_stream(spec)
    call = lambda: vp._eng._check(lib.omega_voice_features(  # noqa: E731
        vp._eng._ctx, spec.data_ptr(), 1025, audio.data_ptr(), 1, 2048, 2048, 512, rows.data_ptr(), L.MEM_DEVICE))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        call()
        e.record()
        e.synchronize()
        us.append(s.elapsed_time(e) * 1e3)
    med = float(np.median(us))
    print(f"voice K = 1025, m = 2048: median {med:.1f} us per call of 512 frames (min {min(us):.1f}, max "
          f"{max(us):.1f}; {med / 512:.3f} us per frame)")


def waterfall(reps):
    """SpectrogramWaterfall's two device calls on resident inputs: omega_waterfall_rows over 4096 frames of 1025 bins
    (853 cells) in float32 and float64, with and without the RGB output, and omega_waterfall_colors over a 200 x 853
    history. Three passes of `reps` calls each between one event pair; the median pass, per call."""
    import ctypes as C
    from omega_gpu import SpectrogramWaterfall
    from omega_gpu import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(13)
    F, n, lo, K = 4096, 1025, 1, 853
    wf = SpectrogramWaterfall(48000)
    eng = wf._eng
    eng._check(lib.omega_waterfall_configure(eng._ctx, C.byref(L.WaterfallConfig(n, lo, K))))

    def timed(label, call, moved):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        passes = []
        for _ in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                call()
            e.record()
            e.synchronize()
            passes.append(s.elapsed_time(e) * 1e3 / reps)
        med = float(np.median(passes))
        print(f"waterfall {label}: median {med:.1f} us per call (passes {', '.join(f'{v:.1f}' for v in passes)}); "
              f"{moved / 1e6:.2f} MB moved = {moved / med / 1e3:.0f} GB/s")

    amp = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), (F, n)))
    for dt in (torch.float32, torch.float64):
        x = torch.from_numpy(amp).to(dt).cuda()
        el = x.element_size()
        stats = torch.empty(F, 7, dtype=torch.float64, device="cuda")
        rows = torch.empty(F, K, dtype=dt, device="cuda")
        rgb = torch.empty(F, K, 3, dtype=torch.uint8, device="cuda")
        state = torch.empty(45, dtype=torch.float64, device="cuda")
        eng._bind_stream(x)
        for img in (None, rgb):
            call = lambda: eng._check(lib.omega_waterfall_rows(  # noqa: E731
                eng._ctx, x.data_ptr(), n, int(dt == torch.float64), F, 1, 0.0, 3, None, state.data_ptr(),
                stats.data_ptr(), rows.data_ptr(), None if img is None else img.data_ptr(), L.MEM_DEVICE))
            # the spectrum once, the dB row out and back in, the row out, the stats, the pixels
            moved = F * (n * el + 3 * K * el + 7 * 8 + (3 * K if img is not None else 0))
            timed(f"rows {str(dt).split('.')[1]} {'with' if img is not None else 'without'} rgb, F = {F}, cells = {K}",
                  call, moved)
        hist = rows[:200].contiguous()
        out = torch.empty(200, K, 3, dtype=torch.uint8, device="cuda")
        timed(f"colors {str(dt).split('.')[1]} 200 x {K}", lambda: eng._check(lib.omega_waterfall_colors(
            eng._ctx, hist.data_ptr(), K, int(dt == torch.float64), 200, K, 3, out.data_ptr(), L.MEM_DEVICE)),
            200 * K * (el + 3))
    print("waterfall stats row 0:", stats[0].cpu().numpy())


def tonal(reps):
    """The two tonal entry points on resident inputs at 4096 frames, K = 4097 (metal: both chord matrices are live;
    the features call once more in pop).
    Three passes of `reps` calls each between one event pair; the median pass, per call."""
    import ctypes as C
    from omega_gpu import ChromagramAnalyzer
    from omega_gpu import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(14)
    F, K = 4096, 4097
    an = ChromagramAnalyzer(48000)
    eng = an._eng
    eng._check(lib.omega_tonal_configure(eng._ctx, C.byref(L.TonalConfig(3))))
    spec = torch.from_numpy(np.abs(rng.standard_normal((F, K))).astype(np.float32) ** 4).cuda()
    raw = torch.empty(F, 12, dtype=torch.float64, device="cuda")
    eng._bind_stream(spec)
    eng._check(lib.omega_chroma(eng._ctx, spec.data_ptr(), F, K, 24000.0 / (K - 1), raw.data_ptr(), L.MEM_DEVICE))
    rows = torch.empty(F, 52, dtype=torch.float64, device="cuda")
    det = [torch.empty(F, n, dtype=torch.float64, device="cuda") for n in (24, 24, 312, 84)]
    state = torch.empty(13, dtype=torch.float64, device="cuda")

    def timed(label, call):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        passes = []
        for _ in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                call()
            e.record()
            e.synchronize()
            passes.append(s.elapsed_time(e) * 1e3 / reps)
        med = float(np.median(passes))
        print(f"tonal {label}: median {med:.1f} us per call of {F} frames (passes {', '.join(f'{v:.1f}' for v in passes)}); "
              f"{med / F * 1e3:.1f} ns per frame")

    for name, d in (("rows only", [None] * 4), ("with details", [t.data_ptr() for t in det])):
        timed(f"features, {name}", lambda: eng._check(lib.omega_tonal_features(
            eng._ctx, raw.data_ptr(), F, None, None, None, state.data_ptr(), rows.data_ptr(), *d, L.MEM_DEVICE)))
        timed(f"spectra K = {K}, {name}", lambda: eng._check(lib.omega_tonal_spectra(
            eng._ctx, spec.data_ptr(), F, K, 24000.0 / (K - 1), None, None, None, state.data_ptr(), rows.data_ptr(), *d,
            L.MEM_DEVICE)))
    timed(f"omega_chroma K = {K} alone", lambda: eng._check(lib.omega_chroma(
        eng._ctx, spec.data_ptr(), F, K, 24000.0 / (K - 1), raw.data_ptr(), L.MEM_DEVICE)))
    # pop: the second chord matrix is not computed (stored as NaN), six chord types are scored
    eng._check(lib.omega_tonal_configure(eng._ctx, C.byref(L.TonalConfig(0))))
    timed("features, rows only, pop", lambda: eng._check(lib.omega_tonal_features(
        eng._ctx, raw.data_ptr(), F, None, None, None, state.data_ptr(), rows.data_ptr(), None, None, None, None,
        L.MEM_DEVICE)))
    print("tonal row 0:", rows[0, 12:28].cpu().numpy())


def meterpanel(reps, samples=None, frames=None):
    """omega_meterpanel_update (its kernels behind one another) on resident float64 frames and meters: the app's shape
    (2048 samples; 1 and 4096 frames), 16384 samples, 256 samples, and 1-sample frames, where the frame kernel has
    nothing to do. With --samples M --frames F that one shape alone, for a kernel-trace run that splits the call
    into its kernels; with --lib, a build of the measured alternatives (`make alt`). Three passes of `reps`
    calls each between one event pair; the median pass, per call."""
    import ctypes as C
    from omega_gpu import ProfessionalMetersPanel
    from omega_gpu import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(15)
    p = ProfessionalMetersPanel(48000)
    eng = p._eng
    Fmax = 4096
    meters = np.zeros((Fmax, 5))
    meters[:, 0] = rng.uniform(-70, 3, Fmax)
    meters[:, 3] = rng.uniform(0, 12, Fmax)
    meters[:, 4] = rng.uniform(-20, 0, Fmax)
    meters = torch.from_numpy(meters).cuda()
    rows = torch.empty(Fmax, 8, dtype=torch.float64, device="cuda")
    hist = torch.empty(Fmax, 60, dtype=torch.int32, device="cuda")
    state = torch.zeros(p._state_len, dtype=torch.float64, device="cuda")
    eng._bind_stream(meters)

    def timed(m, F):
        cfg = L.MeterPanelConfig.from_buffer_copy(p._cfg)
        cfg.frame_len = m
        eng._check(lib.omega_meterpanel_configure(eng._ctx, C.byref(cfg)))
        x = torch.from_numpy(0.3 * rng.standard_normal((F, m))).cuda()

        def call():
            eng._check(lib.omega_meterpanel_update(eng._ctx, x.data_ptr(), m, 1, meters.data_ptr(), F, 60, 0, None,
                                                   rows.data_ptr(), hist.data_ptr(), state.data_ptr(), L.MEM_DEVICE))
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        passes = []
        for _ in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                call()
            e.record()
            e.synchronize()
            passes.append(s.elapsed_time(e) * 1e3 / reps)
        med = float(np.median(passes))
        print(f"meterpanel {m} samples x {F} frames: median {med:.1f} us per call "
              f"(passes {', '.join(f'{v:.1f}' for v in passes)}); {med / F * 1e3:.1f} ns per frame")

    shapes = [(samples, frames)] if samples else ((2048, 1), (2048, 4096), (16384, 1), (16384, 256), (256, 4096),
                                                   (1, 1), (1, 4096))
    for m, F in shapes:
        timed(m, min(F, Fmax))
    print("meterpanel row 0:", rows[0].cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stage")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256, help="stereo frames per call (cfg2: 256, cfg4 shard: 4096)")
    ap.add_argument("--bins", type=int, default=512, help="genre: spectrum bins per frame (512, 4097)")
    ap.add_argument("--samples", type=int, default=None, help="meterpanel: this frame length with --frames alone")
    ap.add_argument("--lib", default=None, help="another build in lib/ (A/B of two builds on one box)")
    a = ap.parse_args()
    if a.lib:
        from omega_gpu import _lib as L0
        L0.use_development_library(a.lib)
    if a.stage == "room":
        return room(a.reps)
    if a.stage == "voice":
        return voice(a.reps)
    if a.stage == "waterfall":
        return waterfall(a.reps)
    if a.stage == "tonal":
        return tonal(a.reps)
    if a.stage == "meterpanel":
        return meterpanel(a.reps, a.samples, a.frames)
    import bench
    from omega_gpu import NORTHSTAR_RESOLUTIONS, Engine
    from omega_gpu import _lib as L
    F = a.frames
    x = torch.from_numpy(bench.cfg2_input(F)).cuda()
    eng = Engine(NORTHSTAR_RESOLUTIONS, 48000, 20000, target_bins=512, n_channels=2)
    ncf = 2 * F
    lib = L.lib()
    eng._bind_stream(x)
    out = {k: torch.empty(ncf, device="cuda") for k in ("tp", "li")}
    comb = torch.empty(ncf, 512, device="cuda")
    met = torch.empty(ncf, 5, dtype=torch.float64, device="cuda")

    xh = bench.cfg2_input()
    host_out = {}
    if a.stage.startswith("spectra"):
        from omega_gpu import Resolution
        from omega_gpu.engine import BandTable
        x3 = torch.from_numpy(bench.cfg3_input(4096, 8192)).cuda()
        e3 = Engine([Resolution((20, 20000), 8192, 2048, 1.0)], 48000, 20000, 512)
        st_, en_, comp_ = bench.band_table_512()
        bt = BandTable(e3, L.BANDS_MAX, st_, en_, 512, 4097, scale=comp_)
        so = {"bands": torch.empty(4096, 512, device="cuda"),
              "chroma": torch.empty(4096, 12, dtype=torch.float64, device="cuda")}
        so_mag = {"mag": torch.empty(4096, 4097, device="cuda")}
        x3s = [x3] + [x3 * (1.0 + 0.125 * k) for k in range(1, 4)] if a.stage == "spectra-rot" else [x3]
        rot = [0]

    if a.stage == "drums":  # bench.py drums_line's call: 4096 magnitude frames x 1025 bins of one stream
        rng = np.random.default_rng(5)
        dmag = torch.from_numpy(np.abs(rng.standard_normal((4096, 1025))).astype(np.float32)).cuda()
        deng = Engine(sample_rate=48000)
        dout = torch.empty(4096, 14, dtype=torch.float64, device="cuda")
    if a.stage == "post":  # bench.py post_line's call: 4096 combined spectra x 512 bins of one stream
        from omega_gpu.app_post import SpectrumPostProcessor
        rng = np.random.default_rng(6)
        px = torch.from_numpy(rng.random((4096, 512)).astype(np.float32)).cuda()
        pp = SpectrumPostProcessor(np.linspace(20, 20000, 512))

    if a.stage == "pitch":  # CepstralAnalyzer over 4096 resident frames x 4096 samples (balanced preset)
        from omega_gpu.pitch_detection import CepstralAnalyzer
        rng = np.random.default_rng(7)
        tt = np.arange(4096) / 48000.0
        f0 = rng.uniform(60.0, 1800.0, 4096)[:, None]
        px = sum((0.7 ** k) * np.sin(2 * np.pi * f0 * (k + 1) * tt[None, :]) for k in range(4))
        px = torch.from_numpy((0.2 * px + 0.01 * rng.standard_normal(px.shape)).astype(np.float32)).cuda()
        pan = CepstralAnalyzer(48000)
        pout = torch.empty(4096, 10, dtype=torch.float64, device="cuda")
        pan._eng._bind_stream(px)

    if a.stage == "harmonic":  # HarmonicAnalyzer over 4096 resident frames: 512-bin spectra, 2048-sample audio
        from omega_gpu.harmonic_analysis import HarmonicAnalyzer
        rng = np.random.default_rng(8)
        hfr = np.linspace(0, 24000, 512)
        tt = np.arange(2048) / 48000.0
        f0 = hfr[rng.integers(3, 40, 4096)][:, None]
        hx = sum((1.0 / (k + 1)) * np.sin(2 * np.pi * f0 * (k + 1) * tt[None, :]) for k in range(8))
        hx = (0.3 * hx + 0.002 * rng.standard_normal(hx.shape)) * np.hanning(2048)
        hs = np.abs(np.fft.rfft(hx[:, :1022] * np.hanning(1022), axis=1))
        hs = torch.from_numpy(np.minimum(1.6 * (hs / hs.max(axis=1, keepdims=True)) ** 0.7, 1.0).astype(np.float32)).cuda()
        hx = torch.from_numpy(hx).cuda()
        han = HarmonicAnalyzer(48000)
        han.analyze_frames(hs[:1], hfr, hx[:1])  # (configures the table)
        hout = torch.empty(4096, 16, dtype=torch.float64, device="cuda")
        hsb = torch.empty(4096, 16, 17, dtype=torch.int32, device="cuda")
        hss = torch.empty(4096, 16, dtype=torch.float64, device="cuda")
        han._eng._bind_stream(hs)

    if a.stage == "genre":  # GenreClassifier features over 4096 resident frames: 512-bin spectra, 2048-sample audio
        from omega_gpu.genre_classification import COLUMNS as GCOLS, GenreClassifier
        rng = np.random.default_rng(9)
        gfr = np.linspace(0, 24000, a.bins)
        tt = np.arange(2048) / 48000.0
        f0 = np.linspace(0, 24000, 512)[rng.integers(3, 40, 4096)][:, None]
        gx = sum((1.0 / (k + 1)) * np.sin(2 * np.pi * f0 * (k + 1) * tt[None, :]) for k in range(8))
        gx = ((0.3 * gx + 0.002 * rng.standard_normal(gx.shape)) * np.hanning(2048)).astype(np.float32)
        nfft = 2 * (a.bins - 1)
        gs = np.abs(np.fft.rfft(np.resize(gx, (4096, nfft)) * np.hanning(nfft), axis=1))
        gs = torch.from_numpy((gs / gs.max(axis=1, keepdims=True)).astype(np.float32)).cuda()
        gx = torch.from_numpy(gx).cuda()
        gen = GenreClassifier(48000)
        gen.extract_features_frames(gs[:1], gfr, gx[:1])  # (configures the table)
        gout = torch.empty(4096, len(GCOLS), dtype=torch.float64, device="cuda")
        gpb = torch.empty(4096, 5, dtype=torch.int32, device="cuda")
        gen._eng._bind_stream(gs)

    outs = L.Outputs()
    outs.combined, outs.lufs_inst, outs.true_peak_db = comb.data_ptr(), out["li"].data_ptr(), out["tp"].data_ptr()

    # the batch kernel without one role (its marginal cost inside the mixed grid)
    part = {}
    for nm, drop in (("batch-nores", "combined"), ("batch-notp", "true_peak_db"), ("batch-nokw", "lufs_inst")):
        o2 = L.Outputs()
        o2.combined, o2.lufs_inst, o2.true_peak_db = outs.combined, outs.lufs_inst, outs.true_peak_db
        setattr(o2, drop, None)
        part[nm] = o2

    def run():
        if a.stage == "batch":  # one batch_kernel launch: the step's per-channel-frame work, no meters
            import ctypes
            eng._check(lib.omega_process_frames(eng._ctx, x.data_ptr(), F, 2 * 16384, 16384, ctypes.byref(outs),
                                                L.MEM_DEVICE))
        if a.stage in part:
            import ctypes
            eng._check(lib.omega_process_frames(eng._ctx, x.data_ptr(), F, 2 * 16384, 16384,
                                                ctypes.byref(part[a.stage]), L.MEM_DEVICE))
        if a.stage == "spectra":
            e3.spectra(x3, "hann", bands=bt, chroma=True, out=so)
        if a.stage == "spectra-rot":
            e3.spectra(x3s[rot[0] % 4], "hann", bands=bt, chroma=True, out=so)
            rot[0] += 1
        if a.stage == "spectra-bands":
            e3.spectra(x3, "hann", bands=bt, chroma=False, out={"bands": so["bands"]})
        if a.stage == "spectra-chroma":
            e3.spectra(x3, "hann", chroma=True, out={"chroma": so["chroma"]})
        if a.stage == "spectra-mag":
            e3.spectra(x3, "hann", chroma=False, mags=True, out=so_mag)
        if a.stage == "drums":
            deng.drum_features(dmag, out=dout)
        if a.stage == "post":
            pp.process(px)
        if a.stage == "pitch":
            pan._eng._check(lib.omega_pitch_detect(pan._eng._ctx, px.data_ptr(), 0, 4096, 4096, 4096, pout.data_ptr(),
                                                   L.MEM_DEVICE))
        if a.stage == "harmonic":
            han._eng._check(lib.omega_harmonic_analyze(han._eng._ctx, hs.data_ptr(), 512, hx.data_ptr(), 1, 2048, 2048,
                                                       4096, hout.data_ptr(), hsb.data_ptr(), hss.data_ptr(), L.MEM_DEVICE))
        if a.stage == "genre":
            gen._eng._check(lib.omega_genre_features(gen._eng._ctx, gs.data_ptr(), a.bins, gx.data_ptr(), 0, 2048, 2048,
                                                     4096, gout.data_ptr(), gpb.data_ptr(), L.MEM_DEVICE))
        if a.stage == "host":  # host buffers in and out: PCIe-inclusive rate of the full path
            host_out.update(eng.process_frames(xh, 256, 2 * 16384, 16384, meters=True))
        if a.stage in ("tp", "all"):
            eng._check(lib.omega_true_peak(eng._ctx, x.data_ptr(), ncf, 16384, out["tp"].data_ptr(), L.MEM_DEVICE))
        if a.stage in ("kw", "all"):
            eng._check(lib.omega_k_weighting(eng._ctx, x.data_ptr(), ncf, 16384, None, out["li"].data_ptr(), L.MEM_DEVICE))
        if a.stage in ("mrfft", "all"):
            eng.process_frames(x, F, 2 * 16384, 16384, combined=True, lufs=False, true_peak=False,
                               out={"combined": comb})
        if a.stage in ("meters", "all"):
            eng._check(lib.omega_meter_update(eng._ctx, out["li"].data_ptr(), out["tp"].data_ptr(), F,
                                              met.data_ptr(), L.MEM_DEVICE))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_begin = time.time()
    s.record()
    for _ in range(a.reps):
        run()
    e.record()
    torch.cuda.synchronize()
    t_end = time.time()
    us = s.elapsed_time(e) / a.reps * 1e3
    print(f"window {t_begin:.3f} {t_end:.3f}")
    if a.stage == "pitch":
        print(f"pitch: {us:.1f} us per call of 4096 frames = {4096 / us * 1e6:.0f} frames/s ({us / 4096:.3f} us per frame)")
        return
    if a.stage == "harmonic":
        print(f"harmonic: {us:.1f} us per call of 4096 frames = {4096 / us * 1e6:.0f} frames/s ({us / 4096:.3f} us per frame)")
        return
    if a.stage == "genre":
        print(f"genre ({a.bins} bins): {us:.1f} us per call of 4096 frames = {4096 / us * 1e6:.0f} frames/s ({us / 4096:.3f} us per frame)")
        return
    print(f"{a.stage}: {us:.1f} us per call, {us * 1e3 / ncf:.1f} ns per channel-frame ({ncf} cf)" +
          (f" = {ncf / us * 1e6:.0f} channel-frames/s (host in/out)" if a.stage == "host" else ""))


if __name__ == "__main__":
    main()
