"""Index model of the batch grid (csrc/batch_plan.hpp BatchPlan, plan_batch, decode_block): where every
workgroup of one batch_kernel launch sits, from the call's shape alone, and -- the other way round -- which
work a blockIdx decodes to. Plain integers (Python's: no overflow), so tests/test_batch_plan.py can hold
the header to it, the plan field by field and the kernel's decode block by block, and check what the kernel
relies on:
the ranges partition the grid, every small resolution has its workgroups, and the roles of a channel-frame
share blockIdx % 8 (one XCD).

Grid: segment 0 (K-weighting, role 0, and the 16384-point resolution, role 2) | segment 1 (the true peaks,
role 1) | [the meter segment, pipelined] | the small resolutions | [the meter segment, unpipelined]."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
WG_THREADS = 512        # one batch workgroup
WAVES = WG_THREADS // 64
METER_WGS_MAX = 64      # OMEGA_METER_WGS
SEGMENT_TOO_LARGE, GRID_TOO_LARGE = 1, 2


def ceil_div(a, b):
    return -(-a // b)


def meter_segment_wgs(n_cf):
    """one wave per output, capped"""
    return min(ceil_div(n_cf, WAVES), METER_WGS_MAX)


def frames_per_wg(fft_size):
    """a small resolution's frames per workgroup: groups of max(64, K / 16) threads, K = fft_size / 2"""
    return WG_THREADS // max(64, (fft_size // 2) // 16)


def plan(n_cf, res, mr, do_kw, do_tp, q_n, q_before_multi):
    """res: [(fft_size, wanted)]. Returns (code, fields, grid); fields and grid are None on a refusal."""
    groups = ceil_div(n_cf, 8)
    seg_roles = [[0] * do_kw + [2] * (mr >= 0), [1] * do_tp]
    seg_begin = [0]
    for roles in seg_roles:
        seg_begin.append(seg_begin[-1] + 8 * len(roles) * groups)
        if seg_begin[-1] > INT32_MAX:
            return SEGMENT_TOO_LARGE, None, None
    small = [r for r, (_, wanted) in enumerate(res) if wanted and r != mr]
    counts = [ceil_div(n_cf, frames_per_wg(res[r][0])) for r in small]
    multi_n = sum(counts)
    body = seg_begin[2] + multi_n
    if body + q_n > INT32_MAX:
        return GRID_TOO_LARGE, None, None
    pad4 = lambda v: list(v) + [0] * (4 - len(v))  # noqa: E731
    f = dict(
        seg_begin=seg_begin,
        n_roles=[max(len(r), 1) for r in seg_roles],
        roles=[x for r in seg_roles for x in (r + [0, 0, 0])[:3]],
        mr_res=max(mr, 0),
        multi_n_seg=len(small),
        multi_res=pad4(small),
        multi_wg_begin=pad4(np.cumsum([0] + counts)[:-1].tolist()),
        q_begin=seg_begin[2] if q_before_multi else body,
        q_n=q_n,
        tail_ctr=0,  # (the caller's: a device pointer)
        pat=1,
        seg_start=seg_begin[:2],
        multi_start=seg_begin[2],
        multi_n=multi_n,
    )
    return 0, f, body + q_n


def segment_only(nq):
    """nq meter workgroups and nothing else: the segments and the small resolutions are empty"""
    f = dict(seg_begin=[0, 0, 0], n_roles=[0, 0], roles=[0] * 6, mr_res=0, multi_n_seg=0, multi_res=[0] * 4,
             multi_wg_begin=[0] * 4, q_begin=0, q_n=nq, tail_ctr=0, pat=0, seg_start=[nq, nq], multi_start=nq,
             multi_n=0)
    return f, nq


# ---- blockIdx -> work (decode_block is held to these) ----

PERIOD8 = [0, 1, 0, 1, 1, 0, 1, 0]  # pat 1: the group order A B A B B A B A of a two-role segment


def segment_work(f, sg):
    """(role, channel-frame) of every workgroup of segment sg, in grid order, as two arrays"""
    j = np.arange(f["seg_begin"][sg + 1] - f["seg_begin"][sg], dtype=np.int64)
    nr = f["n_roles"][sg]
    roles = np.asarray(f["roles"][3 * sg:3 * sg + 3])
    g = j // 8  # the group of 8 workgroups
    if nr == 2 and f["pat"] == 1:
        which = np.asarray(PERIOD8)[g % 8]
        # a group's index among its role's groups: 4 per period and the same-role groups before it
        before = np.asarray([[PERIOD8[:k].count(w) for k in range(8)] for w in (0, 1)])
        idx = 4 * (g // 8) + before[which, g % 8]
    else:
        which = g % nr
        idx = g // nr
    return roles[which], idx * 8 + j % 8


def ranges(f, grid):
    """[(begin, end, what)] of the grid in order: ('seg', s), ('res', r), ('meter',). The small
    resolutions after the meter segment shift by q_n when it sits before or inside them."""
    out = []
    for sg in range(2):
        n = f["seg_begin"][sg + 1] - f["seg_begin"][sg]
        out.append((f["seg_start"][sg], f["seg_start"][sg] + n, ("seg", sg)))
    q0, q1 = f["q_begin"], f["q_begin"] + f["q_n"]
    out.append((q0, q1, ("meter",)))
    ends = f["multi_wg_begin"][1:f["multi_n_seg"]] + [f["multi_n"]]
    for s in range(f["multi_n_seg"]):
        a, b = f["multi_start"] + f["multi_wg_begin"][s], f["multi_start"] + ends[s]
        # (the segment sits at multi_start or at the grid's end: no resolution's range straddles it)
        shift = f["q_n"] if a >= q0 else 0
        out.append((a + shift, b + shift, ("res", f["multi_res"][s])))
    return [r for r in out if r[1] > r[0]]
