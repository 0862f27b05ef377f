"""The combining queue of concurrent one-question encodes without a GPU (comorag_amd/embedding_model/combine.py, config `embedding_combine`,
DESIGN 4.10c): the protocol with a fake forward, the config defaults, and the argument refusals of the two many-row linear entry points
(cmr_encoder_linear_rows / _rows_partials), which need no device because every check precedes the first device call.

Every wait on another thread has a timeout and the test fails when it passes.  The window: a leader with a gather window waits until its
batch is full or the window has passed — every long-window batch below is filled exactly, and the one test that lets a window pass uses
a window of 50 ms."""
import ctypes as C
import threading
import time

import pytest

from comorag_amd.embedding_model.combine import EncodeCombiner

TIMEOUT = 20.0
LONG_US = 60_000_000      # a window no test waits for: a batch under it ends by being full


def _until(pred, what):
    t0 = time.monotonic()
    while not pred():
        assert time.monotonic() - t0 < TIMEOUT, f"the combiner did not reach the expected state: {what}"
        time.sleep(0.0005)


class _Harness:
    """Callers on threads of their own; `run` and `solo` record what they are given (and on which thread) and can be held at a gate."""
    def __init__(self, width, wait_us=0):
        self.cmb = EncodeCombiner(width, wait_us)
        self.runs, self.solos, self.out, self.threads, self.lock = [], [], {}, [], threading.Lock()
        self.run_raises = {}          # first item of a batch -> exception

    def run(self, key, items):
        with self.lock:
            self.runs.append((key, list(items), threading.get_ident()))
        if items[0] in self.run_raises:
            raise self.run_raises[items[0]]
        return [("batch", key, it) for it in items]

    def call(self, key, item, gate=None, solo_raises=None):
        """Starts a caller; returns once it has been queued or has become a leader that stands at its gate."""
        def solo():
            with self.lock:
                self.solos.append((key, item, threading.get_ident()))
            if gate is not None:
                assert gate.wait(TIMEOUT), "a gate was never opened"
            if solo_raises is not None:
                raise solo_raises
            return ("solo", key, item)

        def body():
            try:
                self.out[item] = (self.cmb.submit(key, item, solo, self.run), threading.get_ident())
            except Exception as e:
                self.out[item] = (e, threading.get_ident())
        before = self.cmb.waiting() + len(self.solos) + len(self.runs) + len(self.out)
        t = threading.Thread(target=body, daemon=True)
        t.start()
        self.threads.append(t)
        _until(lambda: self.cmb.waiting() + len(self.solos) + len(self.runs) + len(self.out) > before, f"caller {item} arrived")
        return t

    def join(self):
        for t in self.threads:
            t.join(TIMEOUT)
            assert not t.is_alive(), "a combined call did not return"


def test_config_defaults_are_off():
    from comorag_amd.utils.config_utils import BaseConfig
    cfg = BaseConfig()
    assert cfg.embedding_combine == 0 and cfg.embedding_combine_wait_us == 0
    cfg = BaseConfig(embedding_combine=16, embedding_combine_wait_us=100)
    assert cfg.embedding_combine == 16 and cfg.embedding_combine_wait_us == 100
    for bad in (1, 17, -2):
        with pytest.raises(ValueError):
            EncodeCombiner(bad)
    with pytest.raises(ValueError):
        EncodeCombiner(4, -1)


def test_a_caller_alone_runs_its_own_solo_call():
    h = _Harness(16)
    seen = []
    got = h.cmb.submit(("k",), "mine", lambda: seen.append("mine") or "my result", h.run)
    assert got == "my result" and seen == ["mine"] and h.runs == []
    assert h.cmb.stats() == {"batches": 1, "queries": 1, "max_width": 1} and h.cmb.waiting() == 0 and not h.cmb._slots


def test_arrival_order_width_and_leadership_hand_over():
    h, key, gate = _Harness(4), (48, True), threading.Event()
    h.call(key, 0, gate)                                   # a batch of one, held "on the device"
    for i in range(1, 7):                                  # six more arrive meanwhile, one after the other
        h.call(key, i)
        assert h.cmb.waiting() == i
    gate.set()
    h.join()
    assert [(k, it) for k, it, _ in h.solos] == [(key, 0)]                                     # nobody else ran alone
    assert [(k, it) for k, it, _ in h.runs] == [(key, [1, 2, 3, 4]), (key, [5, 6])]            # arrival order, at most W, two leaders
    assert h.runs[0][2] == h.out[1][1] and h.runs[1][2] == h.out[5][1]                         # each batch ran on its first member's thread
    assert h.out[0][0] == ("solo", key, 0)
    for i in range(1, 7):
        assert h.out[i][0] == ("batch", key, i)                                                # every member got ITS row
    assert h.cmb.stats() == {"batches": 3, "queries": 7, "max_width": 4}
    assert h.cmb.waiting() == 0 and not h.cmb._slots


def test_keys_never_mix_and_every_key_has_a_leader_of_its_own():
    h, ka, kb, ga, gb = _Harness(8), (16, True), (32, True), threading.Event(), threading.Event()
    h.call(ka, "a0", ga)
    h.call(kb, "b0", gb)                                   # stands at ITS gate while a0 stands at a0's: two leaders at once
    _until(lambda: [it for _, it, _ in h.solos] == ["a0", "b0"], "both leaders stand at their gates")
    for i in range(1, 4):
        h.call(ka, f"a{i}")
        h.call(kb, f"b{i}")
    h.call((16, False), "c0")                              # the same width, not normalised: a key of its own, nobody in front: runs at once
    _until(lambda: "c0" in h.out, "c0 returned")
    assert h.out["c0"][0] == ("solo", (16, False), "c0")
    gb.set(); ga.set()
    h.join()
    assert sorted((k, it) for k, it, _ in h.runs) == [(ka, ["a1", "a2", "a3"]), (kb, ["b1", "b2", "b3"])]
    for name, key in (("a", ka), ("b", kb)):
        for i in range(1, 4):
            assert h.out[f"{name}{i}"][0] == ("batch", key, f"{name}{i}")
    assert h.cmb.stats() == {"batches": 5, "queries": 9, "max_width": 3}


def test_an_exception_reaches_every_member_of_its_batch_and_nobody_else():
    h, key, gate = _Harness(2), (16, True), threading.Event()
    boom = ValueError("the forward raised")
    h.run_raises[1] = boom
    h.call(key, 0, gate)
    for i in range(1, 5):
        h.call(key, i)
    gate.set()
    h.join()
    assert [(k, it) for k, it, _ in h.runs] == [(key, [1, 2]), (key, [3, 4])]
    assert h.out[1][0] is boom and h.out[2][0] is boom                                         # leader and member of the failed batch
    assert h.out[0][0] == ("solo", key, 0) and h.out[3][0] == ("batch", key, 3) and h.out[4][0] == ("batch", key, 4)
    assert h.cmb.stats() == {"batches": 3, "queries": 5, "max_width": 2} and not h.cmb._slots
    # a solo call that raises: its caller gets it, the key is free again, the next call works
    err = KeyError("alone")
    h.call(key, 5, solo_raises=err)
    h.join()
    assert h.out[5][0] is err and not h.cmb._slots
    assert h.cmb.submit(key, 6, lambda: "fine", h.run) == "fine"
    # a batch call that answers with the wrong number of rows is an error of that batch, never a missing row
    h2 = _Harness(2)
    h2.run = lambda key, items: ["one row"]
    g2 = threading.Event()
    h2.call(key, 0, g2); h2.call(key, 1); h2.call(key, 2)
    g2.set()
    h2.join()
    assert isinstance(h2.out[1][0], RuntimeError) and isinstance(h2.out[2][0], RuntimeError) and h2.out[0][0] == ("solo", key, 0)


def test_the_window_ends_when_the_batch_is_full():
    h, key = _Harness(3, LONG_US), (16, True)
    t0 = time.monotonic()
    h.call(key, 0)                                         # leader: nobody to share with yet, so it gathers
    assert h.solos == [] and h.runs == [] and h.cmb.waiting() == 1
    h.call(key, 1)
    assert h.runs == [] and h.cmb.waiting() == 2           # still gathering
    h.call(key, 2)                                         # full: the leader goes without waiting the window out
    h.join()
    assert time.monotonic() - t0 < LONG_US * 1e-6 / 2
    assert [(k, it) for k, it, _ in h.runs] == [(key, [0, 1, 2])] and h.solos == []
    assert h.runs[0][2] == h.out[0][1]
    assert h.cmb.stats() == {"batches": 1, "queries": 3, "max_width": 3}


def test_the_window_passes_and_the_leader_goes_with_what_has_gathered():
    window_us = 50_000
    h, key = _Harness(4, window_us), (16, True)
    t0 = time.monotonic()
    h.call(key, 0)
    h.call(key, 1)                                         # joins inside the window (or, on a slow host, becomes the next leader)
    h.join()
    assert time.monotonic() - t0 >= window_us * 1e-6 * 0.9                                     # the leader did wait for the window
    served = [it for _, items, _ in h.runs for it in items] + [it for _, it, _ in h.solos]
    assert sorted(served) == [0, 1] and h.cmb.stats()["queries"] == 2 and not h.cmb._slots


def test_a_window_of_zero_never_waits():
    h = _Harness(16, 0)
    for i in range(3):
        assert h.cmb.submit((16, True), i, lambda i=i: ("solo", i), h.run) == ("solo", i)
    assert h.runs == [] and h.cmb.stats() == {"batches": 3, "queries": 3, "max_width": 1}


def test_many_row_entry_points_are_bound_and_refuse_before_any_device_call():
    from comorag_amd import _lib as L
    lib = L.lib()
    for name in ("cmr_encoder_linear_rows", "cmr_encoder_linear_rows_partials"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.cmr_abi_version() == L.ABI_VERSION == 2                                         # functions added only
    assert L.CMR_ENCODER_ROWS_MAX == 2048
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    rows = lambda m=1280, n=64, k=64, dt=L.CMR_BF16, act=0, x=p, out=p: lib.cmr_encoder_linear_rows(0, x, p, p, m, n, k, dt, act, out, None)
    part = lambda m=1280, n=64, k=64, dt=L.CMR_BF16, x=p, out=p: lib.cmr_encoder_linear_rows_partials(0, x, p, m, n, k, dt, out, None)
    for call in (rows, part):
        assert call(x=None) == L.CMR_ERR_INVALID and call(out=None) == L.CMR_ERR_INVALID
        assert call(m=0) == L.CMR_ERR_INVALID and call(n=0) == L.CMR_ERR_INVALID and call(k=-32) == L.CMR_ERR_INVALID
        assert call(dt=7) == L.CMR_ERR_INVALID
        assert call(m=2049) == L.CMR_ERR_UNSUPPORTED and b"2048" in lib.cmr_last_error()
        assert call(n=40) == L.CMR_ERR_UNSUPPORTED and call(k=48) == L.CMR_ERR_UNSUPPORTED
        assert call(dt=L.CMR_F32) == L.CMR_ERR_UNSUPPORTED and b"16-bit" in lib.cmr_last_error()
        assert call(x=C.c_void_p(p.value + 8)) == L.CMR_ERR_UNSUPPORTED and b"aligned" in lib.cmr_last_error()
    assert rows(act=2) == L.CMR_ERR_INVALID
    if L.device_count() == 0:                              # past every check the call needs a device: the limit itself is accepted
        assert rows(m=2048) == L.CMR_ERR_NO_DEVICE and part(m=129) == L.CMR_ERR_NO_DEVICE
    # the one-query entry points keep their limit
    assert lib.cmr_encoder_linear_small(0, p, p, p, 129, 64, 64, L.CMR_BF16, 0, p, None) == L.CMR_ERR_UNSUPPORTED


def test_the_rows_route_is_explicit_and_refused_where_the_short_row_route_is_not_armed():
    import inspect
    import numpy as np
    import torch
    from comorag_amd.embedding_model import fused_bert
    from oracle import encode_torch as enc
    assert fused_bert.ROWS_MAX == 2048
    assert inspect.signature(fused_bert.FusedBertLayers.forward_ragged).parameters["rows_route"].default is False
    model, _ = enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=32)
    m16 = model.to(torch.bfloat16)
    packed = np.array([1, 1, 0, 1, 2, 5, 5], dtype=np.int32)
    with pytest.raises(ValueError, match="rows_route"):
        fused_bert.FusedBertLayers(m16).forward_ragged(packed, 2, 16, True, rows_route=True)          # not armed
    with pytest.raises(ValueError, match="rows_route"):
        fused_bert.FusedBertLayers(m16, small_m=True).forward_ragged(packed, 129, 16, True, rows_route=True)      # 2064 token rows
