"""Overlapped pipelined batches (omega_set_meter_pipelining): consecutive pipelined calls
run on two batch streams of the context's, each joined into the caller's stream by the next call or a
flush. Every comparison is bitwise against an unpipelined Engine on the same inputs."""
import pytest

from oracle import signals as S

FS = 48000
W = 16384
SIZES = [8, 16, 4, 32, 8]
KEYS = ("combined", "lufs_inst", "true_peak_db", "meters")

pytestmark = pytest.mark.gpu


def _engine(pipe):
    from omega_gpu import Engine, NORTHSTAR_RESOLUTIONS
    eng = Engine(NORTHSTAR_RESOLUTIONS, FS, 20000, target_bins=512, n_channels=2)
    eng.set_meter_pipelining(pipe)
    return eng


def _batches(scale=1.0):
    import torch
    x = torch.from_numpy(S.cfg2_batch(sum(SIZES), seed_l=21, seed_r=22)).cuda() * scale
    out, f0 = [], 0
    for n in SIZES:
        out.append(x[f0:f0 + n].contiguous())
        f0 += n
    return out


_REF = {}


def _reference(scale=1.0):
    """The unpipelined context's outputs over SIZES (computed once per scale, never modified)."""
    import torch
    if scale not in _REF:
        eng = _engine(False)
        outs = [eng.process_frames(xb, n, 2 * W, W, meters=True) for xb, n in zip(_batches(scale), SIZES)]
        eng.synchronize()
        torch.cuda.synchronize()
        _REF[scale] = [{k: o[k].cpu() for k in KEYS} for o in outs]
        eng.close()
    return _REF[scale]


def _out_set(n):
    import torch
    return {"combined": torch.empty(2 * n, 512, device="cuda"), "lufs_inst": torch.empty(2 * n, device="cuda"),
            "true_peak_db": torch.empty(2 * n, device="cuda"),
            "meters": torch.empty(2 * n, 5, dtype=torch.float64, device="cuda")}


def test_overlapped_sequence_two_output_sets():
    import torch
    ref = _reference()
    xs = _batches()
    eng = _engine(True)
    sets = [_out_set(max(SIZES)), _out_set(max(SIZES))]
    got = []
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)
    for i, (xb, n) in enumerate(zip(xs, SIZES)):
        o = {k: v[:2 * n] for k, v in sets[i % 2].items()}
        eng.process_frames(xb, n, 2 * W, W, meters=True, out=o)
        # (each set is written again two calls later: keep a copy, ordered by the stream, once the next
        # call has joined this one)
        if i:
            got.append({k: sets[(i - 1) % 2][k][:2 * SIZES[i - 1]].clone() for k in KEYS})
    eng.synchronize()
    got.append({k: sets[(len(SIZES) - 1) % 2][k][:2 * SIZES[-1]].clone() for k in KEYS})
    torch.cuda.synchronize()
    for i, (g, r) in enumerate(zip(got, ref)):
        for k in KEYS:
            assert torch.equal(g[k].cpu(), r[k]), (i, k)


def test_stream_ordered_visibility_without_device_sync():
    import torch
    ref = _reference()
    eng = _engine(True)
    outs, clones = [], []
    for i, (xb, n) in enumerate(zip(_batches(), SIZES)):
        outs.append(eng.process_frames(xb, n, 2 * W, W, meters=True))
        if i:
            clones.append({k: outs[i - 1][k].clone() for k in KEYS})
    eng.flush_meters()
    clones.append({k: outs[-1][k].clone() for k in KEYS})
    torch.cuda.synchronize()
    for i, (g, r) in enumerate(zip(clones, ref)):
        for k in KEYS:
            assert torch.equal(g[k].cpu(), r[k]), (i, k)


def test_input_produced_on_the_callers_stream():
    import torch
    ref = _reference(0.5)
    base = _batches()
    eng = _engine(True)
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)
    outs = []
    for xb, n in zip(base, SIZES):
        x = xb * 0.5
        outs.append(eng.process_frames(x, n, 2 * W, W, meters=True))
    eng.synchronize()
    torch.cuda.synchronize()
    for i, (g, r) in enumerate(zip(outs, ref)):
        for k in KEYS:
            assert torch.equal(g[k].cpu(), r[k]), (i, k)


def test_input_lifetime_with_dropped_temporaries():
    import torch
    ref = _reference()
    xs = _batches()
    eng = _engine(True)
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)
    mets = []
    for xb, n in zip(xs, SIZES):
        mets.append(eng.process_frames(xb.clone(), n, 2 * W, W, meters=True)["meters"])
        junk = torch.empty_like(xb)
        junk.fill_(123.0)
        del junk
    eng.synchronize()
    torch.cuda.synchronize()
    for i, (m, r) in enumerate(zip(mets, ref)):
        assert torch.equal(m.cpu(), r["meters"]), i


def test_one_context_through_every_meter_path():
    """One context through every path of the meter ledger (csrc/meter_sync.hpp) in one sequence: a direct
    batch (its own segment in the grid), pipelining switched on, a pipelined batch (its segment left
    pending), omega_calculate_lufs over 4 frames of 2048 samples (another entry point: it flushes the
    pending segment, and its counted true peaks release its prep) and a pipelined batch again. Every
    output, the host-memory call's included, is bitwise the unpipelined context's over the same calls."""
    import torch
    sizes = (4, 8, 4)
    x = torch.cat(_batches())[:sum(sizes) + 4]
    short = x[sum(sizes):, :, :2048].reshape(8, 2048).cpu().numpy()
    res = []
    for pipe in (False, True):
        eng = _engine(False)
        outs = [eng.process_frames(x[:4].contiguous(), 4, 2 * W, W, meters=True)]
        eng.set_meter_pipelining(pipe)
        outs.append(eng.process_frames(x[4:12].contiguous(), 8, 2 * W, W, meters=True))
        li, tp, met = eng.calculate_lufs(short)
        outs.append({"lufs_inst": torch.from_numpy(li), "true_peak_db": torch.from_numpy(tp),
                     "meters": torch.from_numpy(met)})
        outs.append(eng.process_frames(x[12:16].contiguous(), 4, 2 * W, W, meters=True))
        eng.synchronize()
        torch.cuda.synchronize()
        res.append([{k: o[k].cpu() for k in KEYS if k in o} for o in outs])
        eng.close()
    for i, (a, b) in enumerate(zip(*res)):
        assert a.keys() == b.keys() and "meters" in a
        for k in a:
            assert torch.equal(a[k], b[k]), (i, k)  # (equal: no NaN either)


def test_fallback_output_over_previous_input():
    """The second call's `combined` is a view of the first call's input storage: the calls run serial."""
    import torch
    ref = _reference()
    xs = _batches()
    n0, n1 = SIZES[0], SIZES[1]
    assert xs[0].numel() >= 2 * n1 * 512
    eng = _engine(True)
    x0 = xs[0].clone()
    torch.cuda.synchronize()
    torch.cuda._sleep(20_000_000)
    a = eng.process_frames(x0, n0, 2 * W, W, meters=True)
    comb = x0.view(-1)[:2 * n1 * 512].view(2 * n1, 512)
    b = eng.process_frames(xs[1], n1, 2 * W, W, meters=True, out={"combined": comb})
    eng.synchronize()
    torch.cuda.synchronize()
    for i, g in enumerate((a, b)):
        for k in KEYS:
            assert torch.equal(g[k].cpu(), ref[i][k]), (i, k)
