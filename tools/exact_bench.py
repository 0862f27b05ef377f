"""Exact search against the plain search at the headline size.

One process: a 10 M x 768 bf16 index with the fp32 shadow (keep_f32), B = 64, k = 20.  Plain pipelined and exact pipelined
alternate over the same four rotated query batches; each timed region is `--steps` batches, q/s is the median of 5 regions.
Also: the share of queries the pipelined exact call leaves uncertified, synchronous single-query latency (plain against exact)
at 1 M rows, and --cand sweeps the stage-1 candidate count (option exact_cand).  --trace: a few steps of each at k' = 128 and
the plain scan at k = 20 and k' only, for a `rocprofv3 --kernel-trace --stats` run.

    python tools/exact_bench.py [--rows 10000000] [--steps 50] [--cand 64,96,128] [--out profiles/exact_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_index(n, d, dev, keep_f32=True, blk=500_000):
    import torch
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(d, "bf16", capacity_hint=n, keep_f32=keep_f32)
    for bi, r0 in enumerate(range(0, n, blk)):
        g = torch.Generator(device=dev); g.manual_seed(4242 + bi)
        x = torch.randn((min(blk, n - r0), d), generator=g, device=dev)
        idx.append_dev((x / x.norm(dim=1, keepdim=True)).contiguous())
    torch.cuda.synchronize(dev)
    return idx


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--cand", default="128")
    ap.add_argument("--latency-rows", type=int, default=1_000_000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from comorag_amd.index import DenseIndex
    dev = torch.device("cuda", 0)
    d, B, k = a.dim, a.batch, a.k
    idx = build_index(a.rows, d, dev)
    g = torch.Generator(device=dev); g.manual_seed(7)
    qs = []
    for _ in range(4):
        q = torch.randn((B, d), generator=g, device=dev)
        qs.append((q / q.norm(dim=1, keepdim=True)).contiguous())
    ids = torch.empty((B, 128), dtype=torch.int64, device=dev)
    sc = torch.empty((B, 128), dtype=torch.float32, device=dev)
    ex = torch.empty((4, B), dtype=torch.int32, device=dev)

    def plain(steps, kk=k):
        done = None
        for s in range(steps):
            done = idx.search_pipelined(qs[s % 4], kk, ids, sc)
        DenseIndex.sync(done)

    unc = []

    def exact(steps):
        done = None
        for s in range(steps):
            done = idx.search_exact_pipelined(qs[s % 4], k, ids, sc, ex[s % 4])
        DenseIndex.sync(done)
        unc.append(float((ex == 0).float().mean()))

    if a.trace:
        for f in (lambda: plain(8), lambda: plain(8, 128), lambda: exact(8)):
            f()
        print(json.dumps({"trace": True, "rows": a.rows}))
        return

    def qps(fn, steps):
        t = []
        for _ in range(5):
            t0 = time.perf_counter(); fn(steps); t.append(B * steps / (time.perf_counter() - t0))
        return statistics.median(t)

    out = {"rows": a.rows, "dim": d, "dtype": "bf16+keep_f32", "batch": B, "k": k, "steps_per_region": a.steps, "by_cand": {}}
    plain(8)
    for kc in [int(c) for c in a.cand.split(",")]:
        idx.set_option("exact_cand", kc)
        exact(8)
        unc.clear()
        p_q, e_q = [], []
        for _ in range(2):             # alternate: plain, exact, plain, exact
            p_q.append(qps(plain, a.steps)); e_q.append(qps(exact, a.steps))
        out["by_cand"][kc] = {"plain_qps": statistics.median(p_q), "exact_qps": statistics.median(e_q),
                              "ratio": statistics.median(e_q) / statistics.median(p_q), "uncertified_share": max(unc)}
    idx.set_option("exact_cand", 128)
    idx.close()
    del idx
    torch.cuda.empty_cache()
    # synchronous single-query latency at 1 M rows
    small = build_index(a.latency_rows, d, dev)
    q1 = qs[0][:1].cpu().numpy()
    lat = {}
    for name, fn in (("plain_us", lambda: small.search(q1, k)), ("exact_us", lambda: small.search_exact(q1, k))):
        for _ in range(10):
            fn()
        t = []
        for _ in range(50):
            t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e6)
        lat[name] = statistics.median(t)
    out["sync_single_query_at_rows"] = a.latency_rows
    out.update(lat)
    small.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
