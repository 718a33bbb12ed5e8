"""Model of the meter pipeline's ledger (csrc/meter_sync.hpp): the six device counters that order the meter
prep, the meter segment and the query kernels against the batch, the host's running counts of what it
launched to count into them, and what each kind of call does to both. Written from the rules (DESIGN.md §4,
"The meter counters"), not from the header, in 32-bit wrap-around arithmetic, so tests/test_meter_sync.py can
hold the header to it step by step over long mixed sequences, failed launches included.

A ledger is a dict: kw, query, tp, prep, seg, lufs_tp (issued counts), seg_par (two targets), cur (state
parity), pend / pend_nq / pend_par (the pipelined segment not yet launched), mirror_gen, tail, side (a meter
kernel is on the side stream that the caller's stream has not joined). Every step returns (targets, {outcome:
ledger}); `targets` always has the same keys, 0 / [] where a step has none.

The side rule: whatever may have put a meter prep or a LUFS query on the side stream leaves side = 1 -- a
chunked or direct batch and the back-to-back layout whether the batch launch succeeds or not (their preps go
first), a pipelined batch from its launch on (launched, waited, ok) but not when the launch fails (nothing was
enqueued). Only a join of the side stream into the caller's stream takes it back to 0, and a counted
omega_calculate_lufs needs that join first exactly when side is 1."""
M32 = 2 ** 32
METER_WGS_MAX = 64
WAVES = 8


def u32(v):
    return v % M32


def sdiff(a, b):
    """the device's comparison: a - b as a signed 32-bit number (a has reached b when >= 0)"""
    d = (a - b) % M32
    return d - M32 if d >= 2 ** 31 else d


def meter_segment_wgs(n_cf):
    return min(-(-n_cf // WAVES), METER_WGS_MAX)


def zero():
    return dict(kw=0, query=0, tp=0, prep=0, seg=0, lufs_tp=0, seg_par=[0, 0], cur=0, pend=0, pend_nq=0,
                pend_par=0, mirror_gen=0, tail=0, side=0)


def filled(v):
    """every count at v (a ledger late in a context's life)"""
    m = zero()
    for k in ("kw", "query", "tp", "prep", "seg", "lufs_tp", "mirror_gen", "tail"):
        m[k] = v
    m["seg_par"] = [v, v]
    return m


def copy(m):
    return dict(m, seg_par=list(m["seg_par"]))


def _targets(**kw):
    t = dict(wait=0, start=0, join=0, tail_target=0, gen=0, q_n=0, join_side=0, frames=[], par=[], seg_pre=[],
             seg_post=[])
    t.update(kw)
    return t


def _chunks(m, frames):
    """the parity rule: chunk i reads parity a and writes a ^ 1; its prep waits for the segments reading
    either (seg_par[a] before its scratch, seg_par[a ^ 1] before the next state); cur flips per chunk"""
    par, pre, post = [], [], []
    for _ in frames:
        a = m["cur"]
        par.append(a)
        pre.append(m["seg_par"][a])
        post.append(m["seg_par"][a ^ 1])
        m["cur"] = a ^ 1
    return dict(frames=list(frames), par=par, seg_pre=pre, seg_post=post)


def state_chunks(m, frames, on_side=False):
    """no counter: the back-to-back layout (on_side: its meter kernels run on the side stream), meters_enqueue
    and a graph replay (on the caller's stream)"""
    s = copy(m)
    ch = _chunks(s, frames)
    if on_side:
        s["side"] = 1
    return _targets(**ch), dict(ok=s, fail=copy(s))


def chunks(m, n_cf, C, frames):
    """meters by query kernels: the state is kept as advanced whatever the batch launch does"""
    s = copy(m)
    ch = _chunks(s, frames)
    s["kw"] = u32(s["kw"] + n_cf)
    for f in frames:
        s["query"] = u32(s["query"] + -(-f // 4) * C)
        s["side"] = 1   # every chunk's prep and LUFS query, before the batch launch
    return _targets(wait=s["kw"], join=s["query"], **ch), dict(ok=s, fail=copy(s))


def direct(m, n_cf, C):
    s = copy(m)
    ch = _chunks(s, [n_cf // C])
    a = ch["par"][0]
    n_mq = meter_segment_wgs(n_cf)
    t = _targets(wait=u32(m["kw"] + n_cf), start=u32(m["prep"] + C), join=u32(m["tp"] + n_cf), q_n=n_mq, **ch)
    # a failed batch launch: the prep is enqueued (it waits at kw, it will count in), the batch's work is not
    bad = copy(s)
    bad["kw"], bad["prep"], bad["side"] = t["wait"], t["start"], 1
    ok = copy(bad)
    ok["tp"] = t["join"]
    ok["seg"] = u32(m["seg"] + n_mq)
    ok["seg_par"][a] = ok["seg"]
    return t, dict(ok=ok, fail=bad)


def next_gen(g):
    return 2 if g == M32 - 1 else g + 1


def pipelined(m, n_cf, C, tail):
    """the launch runs the pending segment and leaves its own pending; `launched` and `waited` are what a
    failing tail wait resp. prep launch leave behind after a successful batch launch"""
    q_n = m["pend_nq"] if m["pend"] else 0
    s = copy(m)
    if m["pend"]:
        s["seg_par"][m["pend_par"]] = u32(m["seg"] + q_n)   # before the chunk's targets are read
    ch = _chunks(s, [n_cf // C])
    s["mirror_gen"] = next_gen(m["mirror_gen"])
    t = _targets(start=u32(m["prep"] + C), tail_target=u32(m["tail"] + 1), gen=s["mirror_gen"], q_n=q_n, **ch)
    s["side"] = 1   # the batch is launched: the tail wait and the prep follow on the side stream
    launched = copy(s)
    if tail:
        s["tail"] = t["tail_target"]
    waited = copy(s)
    s["prep"] = t["start"]
    s["seg"] = u32(m["seg"] + q_n)
    s["pend"], s["pend_nq"], s["pend_par"] = 1, meter_segment_wgs(n_cf), ch["par"][0]
    return t, dict(ok=s, fail=copy(m), launched=launched, waited=waited)


def flush(m):
    ok = copy(m)
    q_n = 0
    if m["pend"]:
        q_n = m["pend_nq"]
        ok["seg"] = u32(m["seg"] + q_n)
        ok["seg_par"][m["pend_par"]] = ok["seg"]
        ok["pend"] = 0
    return _targets(q_n=q_n), dict(ok=ok, fail=copy(m))


def lufs_tp(m, n_cf, counted):
    """omega_calculate_lufs' true peaks: counted, they count in -- after a join when a meter kernel is on the
    side stream; otherwise no counter moves"""
    ok = copy(m)
    if counted:
        ok["lufs_tp"] = u32(m["lufs_tp"] + n_cf)
    return _targets(wait=ok["lufs_tp"], join_side=int(bool(counted and m["side"]))), dict(ok=ok, fail=copy(m))


def join(m):
    """the caller's stream has joined the side stream"""
    return _targets(), dict(ok=dict(copy(m), side=0), fail=copy(m))


def step(m, line):
    """one line of tests/abi/meter_sync_dump.cpp's script -> (targets, ledger after the line's outcome)"""
    w = line.split()
    kind, a = w[0], w[1:]
    if kind == "Z":
        return _targets(), zero()
    if kind == "S":
        return _targets(), dict(copy(m), **{k: v for k, v in filled(int(a[0])).items()
                                            if k not in ("cur", "pend", "pend_nq", "pend_par", "side")})
    if kind == "B":
        t, after = state_chunks(m, [int(x) for x in a[1:1 + int(a[0])]])
    elif kind == "E":
        t, after = state_chunks(m, [int(x) for x in a[1:1 + int(a[0])]], on_side=True)
    elif kind == "K":
        t, after = chunks(m, int(a[0]), int(a[1]), [int(x) for x in a[3:3 + int(a[2])]])
    elif kind == "D":
        t, after = direct(m, int(a[0]), int(a[1]))
    elif kind == "P":
        t, after = pipelined(m, int(a[0]), int(a[1]), int(a[2]) != 0)
    elif kind == "F":
        t, after = flush(m)
    elif kind == "L":
        t, after = lufs_tp(m, int(a[0]), int(a[1]) != 0)
    elif kind == "J":
        t, after = join(m)
    else:
        raise ValueError(line)
    return t, after[w[-1]]
