"""Flat combining of concurrent one-question encodes (config `embedding_combine`): the protocol of csrc/combine.h restated
in Python for the encoder, whose batch is formed above the C-ABI.  No HIP and no torch call in here: the owner hands in the two
callables that run a batch, so the protocol is tested without a device (tests/test_encoder_combine_host.py).

  - a call that arrives while no batch of its key is being gathered or run becomes the LEADER;
  - the leader takes what is queued for the key in arrival order, itself first, up to `width` calls;
  - it runs ONE batch — `run(key, items)` returns one result per item — hands every member its result, or all of them the exception
    `run` raised, and wakes them;
  - if calls queued up meanwhile it hands leadership to the first of them: a leader serves one batch, never a stream.
A caller that finds nobody else forms a batch of one and runs its own `solo()` — the unchanged call with its own arguments; with the
gather window at 0 that costs one uncontended lock.  With a window (`wait_us` > 0) the leader waits until `width` calls have gathered
or the window has passed, whichever comes first.  A queued caller holds no lock of the owner; `run` / `solo` are called with the
combiner's lock released.  Calls of different keys never meet: every key has a queue and a leader of its own.
"""
from __future__ import annotations

import collections
import threading

MAX_WIDTH = 16


class _Request:
    __slots__ = ("item", "solo", "result", "error", "done", "lead", "cv")

    def __init__(self, item, solo, lock):
        self.item, self.solo, self.result, self.error = item, solo, None, None
        self.done = self.lead = False
        self.cv = threading.Condition(lock)


class _Slot:
    __slots__ = ("queue", "leader", "busy", "gathering")

    def __init__(self):
        self.queue = collections.deque()      # arrival order; the head is the leader while busy
        self.leader, self.busy, self.gathering = None, False, False


class EncodeCombiner:
    def __init__(self, width: int, wait_us: int = 0):
        width, wait_us = int(width), int(wait_us)
        if not 2 <= width <= MAX_WIDTH:
            raise ValueError(f"EncodeCombiner: width must be in 2..{MAX_WIDTH}")
        if wait_us < 0:
            raise ValueError("EncodeCombiner: wait_us must be >= 0")
        self.width, self.wait_us = width, wait_us
        self._mu = threading.Lock()
        self._slots = {}
        self._batches = self._queries = self._max_width = 0

    def submit(self, key, item, solo, run):
        """Serves `item` — as the leader of a batch or as a member of somebody else's — and returns its result (or raises what the
        batch's forward raised).  `solo()` is this caller's unchanged single call; `run(key, items)` runs a batch of 2 .. width items
        and returns their results in order, complete (a member reads its result as soon as it is woken)."""
        req = _Request(item, solo, self._mu)
        with self._mu:
            slot = self._slots.get(key)
            if slot is None:
                slot = self._slots[key] = _Slot()
            slot.queue.append(req)
            if slot.busy:
                if slot.gathering and len(slot.queue) >= self.width:
                    slot.leader.cv.notify()                      # the window ends with the batch full
                while not (req.done or req.lead):
                    req.cv.wait()
            else:
                slot.busy = True
            if not req.done:
                # leader of one batch: this request is the queue's head
                slot.leader = req
                if self.wait_us > 0 and len(slot.queue) < self.width:
                    slot.gathering = True
                    req.cv.wait_for(lambda: len(slot.queue) >= self.width, timeout=self.wait_us * 1e-6)
                    slot.gathering = False
                batch = [slot.queue.popleft() for _ in range(min(self.width, len(slot.queue)))]
        if req.done:
            if req.error is not None:
                raise req.error
            return req.result
        results, error = None, None
        try:
            if len(batch) == 1:
                results = [req.solo()]
            else:
                results = list(run(key, [r.item for r in batch]))
                if len(results) != len(batch):
                    raise RuntimeError(f"EncodeCombiner: the batch call returned {len(results)} results for {len(batch)} items")
        except BaseException as e:                               # every member of THIS batch gets it, nobody else
            results, error = None, e
        with self._mu:
            self._batches += 1
            self._queries += len(batch)
            self._max_width = max(self._max_width, len(batch))
            for i, r in enumerate(batch):
                r.result, r.error = (results[i] if results is not None else None), error
                if r is not req:
                    r.done = True
                    r.cv.notify()
            # the slot is still ours: busy kept every other caller of the key out of leadership
            if slot.queue:
                nxt = slot.queue[0]
                slot.leader, nxt.lead = nxt, True
                nxt.cv.notify()
            else:
                del self._slots[key]
        if error is not None:
            raise error
        return results[0]

    def stats(self) -> dict:
        with self._mu:
            return {"batches": self._batches, "queries": self._queries, "max_width": self._max_width}

    def waiting(self) -> int:
        """Calls queued and not yet taken into a batch (the leader of a running batch is not among them)."""
        with self._mu:
            return sum(len(s.queue) for s in self._slots.values())
