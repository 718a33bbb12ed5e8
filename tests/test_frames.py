"""The frame-batch layer (csrc/frames.hpp: Rows, Rows32, chain_step, chain_chunks) on the CPU:
tests/abi/frames_dump.cpp, a stand-alone host program, evaluates the header and
  1. its spans, offsets and loads must equal numpy's own view arithmetic -- np.lib.stride_tricks.as_strided over
     a byte buffer -- for 0, 1, 2 and 5 rows of 1 and 7 elements at the strides 1 (fully overlapping), width and
     width + 3, float32 and float64, from every first frame;
  2. the launches it plans for a chained call must keep the chain's invariants, for 1, per, per + 1, 2 per and
     2 per + 1 frames and a caller's state_out that is absent, a buffer of its own, or state_in's buffer. Only
     the invariants are asserted: there is no second implementation of the plan to compare with.
The program's sample buffer is exactly span_bytes long, so built with -fsanitize=address,undefined (it is a
stand-alone program; feed it lines() of this module) a load past the span is an error there."""
import subprocess

import numpy as np
import pytest

from conftest import REPO
from host_program import compile_host_program

SRC = f"{REPO}/tests/abi/frames_dump.cpp"
PER = 3
NONE, BLOB0, BLOB1, IN, OUT = -1, 0, 1, 2, 3  # frames.hpp ChainBuf


def rows_cases():
    return [(f64, n, w, s, f0) for f64 in (0, 1) for n in (0, 1, 2, 5) for w in (1, 7) for s in (1, w, w + 3)
            for f0 in range(max(n, 1))]


def chain_cases():
    return [(n, PER, out) for n in (1, PER, PER + 1, 2 * PER, 2 * PER + 1) for out in (0, 1, 2)]


def lines():
    return ([" ".join(map(str, ("r",) + c)) for c in rows_cases()] +
            [" ".join(map(str, ("c",) + c)) for c in chain_cases()])


def run(exe):
    r = subprocess.run([exe], input="\n".join(lines()) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines())
    return out[:len(rows_cases())], out[len(rows_cases()):]


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    return run(compile_host_program(SRC, str(tmp_path_factory.mktemp("frames") / "frames_dump")))


def test_spans_offsets_and_loads_are_numpys_view_arithmetic(dumped):
    cases = rows_cases()
    assert len(cases) == 2 * (1 + 1 + 2 + 5) * 2 * 3
    for (f64, n, w, s, f0), ln in zip(cases, dumped[0]):
        what = (f64, n, w, s, f0)
        assert not ln.endswith("mismatch"), what  # (at, row, row_as and Rows32 agree among themselves)
        v = ln.split()
        dt = np.dtype(np.float64 if f64 else np.float32)
        span, off, got = int(v[0]), int(v[1]), np.array(v[2:], np.float64)
        raw = np.zeros(span, np.uint8)  # the bytes the library says the batch touches
        raw.view(dt)[:] = np.arange(span // dt.itemsize)
        if n == 0:
            assert span == 0 and off == 0 and len(got) == 0, what
            continue
        # (as_strided would read out of bounds without complaint, so the extent is taken from the addresses of
        # the view's own first and last elements: it must be the buffer, to the byte)
        view = np.lib.stride_tricks.as_strided(raw.view(dt), (n, w), (s * dt.itemsize, dt.itemsize), writeable=False)
        addr = lambda a: a.__array_interface__["data"][0]  # noqa: E731
        assert addr(view[-1:, -1:]) + dt.itemsize - addr(raw) == span, what
        assert addr(view[f0:]) - addr(raw) == off, what
        np.testing.assert_array_equal(got, view[f0:].astype(np.float64).ravel(), err_msg=str(what))


def launches(ln):
    v = [int(s) for s in ln.split()]
    assert len(v) % 5 == 0
    return [tuple(v[i:i + 5]) for i in range(0, len(v), 5)]  # f0, count, read, write, copy_back


def test_chain_plan_keeps_its_invariants(dumped):
    cases = chain_cases()
    assert len(cases) == 15
    multi = 0
    for (n, per, out), ln in zip(cases, dumped[1]):
        what = (n, per, out)
        L = launches(ln)
        # the launches tile [0, n) in order, `per` frames each but the last
        assert [f0 for f0, *_ in L] == list(range(0, n, per)) and sum(c for _, c, *_ in L) == n, what
        assert all(c == per for _, c, *_ in L[:-1]) and 1 <= L[-1][1] <= per, what
        multi += len(L) > 1
        # the buffers as memory: with out == 2 the caller's out is the caller's in
        mem = lambda b: IN if (b == OUT and out == 2) else b  # noqa: E731
        for i, (_, _, read, write, copy) in enumerate(L):
            last = i == len(L) - 1
            # no launch reads and writes one buffer
            assert read != NONE and (write == NONE or mem(read) != mem(write)), what
            # the first reads the caller's in, every other what the one before wrote
            assert read == (IN if i == 0 else L[i - 1][3]), what
            if not last:
                # (a later launch reads it: a blob; nothing reaches the caller's buffers before the last launch)
                assert write in (BLOB0, BLOB1) and not copy, what
        _, _, _, write, copy = L[-1]
        if out == 0:
            assert write == NONE and not copy, what  # no state_out: nothing written for the caller
        else:
            # the final state reaches the caller's out: written there, or to a blob and copied
            assert (write == OUT and not copy) or (write in (BLOB0, BLOB1) and copy), what
            assert all(mem(w) != IN for *_, w, _ in L), what  # the caller's in is never a launch's target
    assert multi == 9  # (per + 1, 2 per and 2 per + 1 frames take several launches)

