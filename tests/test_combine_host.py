"""The flat combiner of concurrent synchronous calls (comorag_amd/csrc/combine.h) without a GPU: tools/combine_selftest.cpp
wraps it round a "run batch" callback that records what it is given, this file compiles that driver with the host compiler and calls it
from Python threads through ctypes (the interpreter lock is released for the call).

The window: a leader with a gather window waits until its batch is full or the window has passed (combine.h) — so no test here lets a
batch that can still grow stand under a long window; every long-window batch below is filled exactly.  A caller alone with a window of 0
runs at once; a caller that cannot share (as many queries as the batch holds) runs at once whatever the window."""
import ctypes as C
import os
import shutil
import subprocess
import threading
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_US = 60_000_000      # a window no test waits for: a batch under it ends by being full


@pytest.fixture(scope="module")
def cst(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host tier needs g++"
    so = str(tmp_path_factory.mktemp("combine") / "combine_selftest.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-shared", "-fPIC", os.path.join(ROOT, "tools", "combine_selftest.cpp"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.cst_create.restype = C.c_void_p
    lib.cst_destroy.argtypes = [C.c_void_p]
    lib.cst_submit.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.cst_submit.restype = C.c_int
    lib.cst_gate.argtypes = [C.c_void_p, C.c_int]
    for f in (lib.cst_running, lib.cst_waiting, lib.cst_n_batches):
        f.argtypes, f.restype = [C.c_void_p], C.c_int
    lib.cst_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    lib.cst_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    return lib


class Harness:
    def __init__(self, lib):
        self.lib, self.h = lib, lib.cst_create()

    def close(self):
        self.lib.cst_destroy(self.h)

    def submit(self, key, tag, nq=1, width=16, wait_us=0, want_rc=0, fail_batch=0):
        """-> (code, message, batch number)"""
        err = C.create_string_buffer(128)
        batch = C.c_int(-1)
        rc = self.lib.cst_submit(self.h, key, tag, nq, width, wait_us, want_rc, fail_batch, err, len(err), C.byref(batch))
        return rc, err.value.decode(), batch.value

    def batches(self):
        out = []
        for i in range(self.lib.cst_n_batches(self.h)):
            rec = (C.c_longlong * 20)()
            self.lib.cst_batch(self.h, i, rec)
            out.append({"key": rec[0], "leader": rec[1], "n": rec[2], "total": rec[3], "tags": [rec[4 + t] for t in range(rec[2])]})
        return out

    def counters(self):
        c = (C.c_longlong * 3)()
        self.lib.cst_counters(self.h, c)
        return {"batches": c[0], "queries": c[1], "max_width": c[2]}

    def run_threads(self, calls, barrier=True, timeout=60.0):
        """calls: list of submit kwargs; every call on a thread of its own, released together.  -> results in call order"""
        res = [None] * len(calls)
        bar = threading.Barrier(len(calls)) if barrier else None

        def work(i):
            if bar:
                bar.wait()
            res[i] = self.submit(**calls[i])
        ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(calls))]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout)
            assert not t.is_alive(), "a combined call did not return"
        return res

    def until(self, cond, timeout=30.0):
        t0 = time.monotonic()
        while not cond():
            assert time.monotonic() - t0 < timeout, "the combiner did not reach the expected state"
            time.sleep(0.0002)


@pytest.fixture()
def hs(cst):
    h = Harness(cst)
    yield h
    h.close()


def test_lone_caller_runs_at_once(hs):
    # nobody else, no window: a batch of one, served by its own thread
    t0 = time.monotonic()
    assert hs.submit(key=1, tag=7) == (0, "", 0)
    # a caller that cannot share a batch (as wide as the batch itself) does not wait for the longest window either
    assert hs.submit(key=1, tag=8, nq=4, width=4, wait_us=LONG_US) == (0, "", 1)
    assert time.monotonic() - t0 < 5.0
    b = hs.batches()
    assert [(x["n"], x["total"], x["leader"], x["tags"]) for x in b] == [(1, 1, 7, [7]), (1, 4, 8, [8])]
    assert hs.counters() == {"batches": 2, "queries": 5, "max_width": 4}


@pytest.mark.parametrize("W", [2, 5, 16])
def test_barrier_forms_batches_of_exactly_w(hs, W):
    # 2 W callers under a window nobody waits for: the first W fill one batch, the W + 1-th lands in the next, which the rest fill
    res = hs.run_threads([dict(key=3, tag=i, width=W, wait_us=LONG_US) for i in range(2 * W)])
    assert all(r[0] == 0 and r[1] == "" for r in res)
    b = hs.batches()
    assert [(x["n"], x["total"]) for x in b] == [(W, W), (W, W)]
    assert sorted(b[0]["tags"] + b[1]["tags"]) == list(range(2 * W))
    for i, r in enumerate(res):                       # every caller was told the batch that held it
        assert i in b[r[2]]["tags"]
    assert hs.counters() == {"batches": 2, "queries": 2 * W, "max_width": W}


def test_mixed_query_counts_fill_a_batch(hs):
    # 1 + 3 + 7 + 5 = 16 queries in four calls: one batch, the window ends when it is full
    res = hs.run_threads([dict(key=4, tag=i, nq=nq, width=16, wait_us=LONG_US) for i, nq in enumerate((1, 3, 7, 5))])
    assert all(r[0] == 0 for r in res)
    b = hs.batches()
    assert len(b) == 1 and b[0]["n"] == 4 and b[0]["total"] == 16
    assert hs.counters() == {"batches": 1, "queries": 16, "max_width": 16}


def test_keys_never_share_a_batch(hs):
    W = 4
    calls = [dict(key=10 + (i % 3), tag=i, width=W, wait_us=LONG_US) for i in range(3 * W)]
    res = hs.run_threads(calls)
    assert all(r[0] == 0 for r in res)
    b = hs.batches()
    assert len(b) == 3 and sorted(x["key"] for x in b) == [10, 11, 12]
    for x in b:
        assert x["total"] == W and all(calls[t]["key"] == x["key"] for t in x["tags"])


def test_leadership_is_handed_over(hs):
    """A leads and is held "on the device"; B, C, D queue behind it in that order; width 2, no window.  A serves only itself, hands over to
    B (the first queued), which takes C along and hands over to D: three batches, three leaders, nobody leads twice."""
    hs.lib.cst_gate(hs.h, 1)
    res = {}
    ts = []

    def start(tag):
        t = threading.Thread(target=lambda: res.__setitem__(tag, hs.submit(key=5, tag=tag, width=2)), daemon=True)
        t.start()
        ts.append(t)
    start(0)
    hs.until(lambda: hs.lib.cst_running(hs.h) == 1)
    for i, tag in enumerate((1, 2, 3)):
        start(tag)
        hs.until(lambda: hs.lib.cst_waiting(hs.h) == i + 1)
    hs.lib.cst_gate(hs.h, 0)
    for t in ts:
        t.join(60.0)
        assert not t.is_alive()
    b = hs.batches()
    assert [(x["leader"], x["tags"]) for x in b] == [(0, [0]), (1, [1, 2]), (3, [3])]
    assert [res[t][2] for t in range(4)] == [0, 1, 1, 2]
    assert hs.lib.cst_waiting(hs.h) == 0


def test_participant_error_reaches_its_thread_only(hs):
    W = 6
    res = hs.run_threads([dict(key=6, tag=i, width=W, wait_us=LONG_US, want_rc=(-1 if i == 4 else 0)) for i in range(W)])
    assert len(hs.batches()) == 1
    for i, (rc, msg, _) in enumerate(res):
        assert (rc, msg) == ((-1, "request 4 refused") if i == 4 else (0, ""))


def test_batch_failure_reaches_every_participant(hs):
    W = 6
    res = hs.run_threads([dict(key=7, tag=i, width=W, wait_us=LONG_US, fail_batch=int(i == 2)) for i in range(W)])
    assert len(hs.batches()) == 1
    assert all((rc, msg) == (-5, "batch failed by request 2") for rc, msg, _ in res)
    # the combiner is none the worse for it
    assert hs.submit(key=7, tag=99)[:2] == (0, "")


def test_sixteen_threads_thousand_calls(hs):
    T, N = 16, 1000
    served = [None] * T

    def work(t):
        mine = []
        for i in range(N):
            rc, msg, batch = hs.submit(key=8 + (i & 1), tag=t * N + i, width=16)
            assert rc == 0 and msg == ""
            mine.append(batch)
        served[t] = mine
    ts = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(T)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120.0)
        assert not t.is_alive(), "a combined call did not return"
    b = hs.batches()
    c = hs.counters()
    assert c["queries"] == T * N == sum(x["total"] for x in b)
    assert c["batches"] == len(b) and 1 <= c["max_width"] <= 16 and c["max_width"] == max(x["total"] for x in b)
    tags = sorted(t for x in b for t in x["tags"])
    assert tags == list(range(T * N))                 # every call served exactly once
    leaders = [x["leader"] for x in b]
    assert len(set(leaders)) == len(leaders)          # a call leads one batch at the most
    for x in b:
        assert x["leader"] == x["tags"][0] and len({t & 1 for t in x["tags"]}) == 1      # a leader serves its own batch; keys apart
    for t in range(T):
        for i, batch in enumerate(served[t]):
            assert t * N + i in b[batch]["tags"]
    assert hs.lib.cst_waiting(hs.h) == 0
