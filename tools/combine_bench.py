"""Sixteen threads of single-query calls on one index, with and without the combiner (option "combine").

    python tools/combine_bench.py [--only search_1M,search_5K,ppr_comorag,ppr_1M] [--baseline] [--out profiles/combine_bench.json]

A region is THREADS x CALLS distinct single-query calls (16 x 50) issued from a thread pool, as ComoRAG's question threads issue them; its
time is the wall time from the barrier that releases the threads to the last thread's return.  Within one process and on one index the
configurations alternate region by region — combine = 0, combine = 16 with the gather window at 0, combine = 16 with the window at WINDOW_US
— so box-to-box spread does not enter their ratios; each is reported as the median of REGIONS regions, in microseconds per call.
--baseline measures combine = 0 only and touches no option: the form that also runs on a library without the combiner (the parent commit's,
loaded through COMORAG_HIP_LIB).  Prints ONE JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

THREADS, CALLS, REGIONS = 16, 50, 5
WINDOW_US = 100      # about a third of a 1 M x 768 bf16 scan: long enough for sixteen racing threads to meet, short against what it saves
K = 20
CONFIGS = (("combine_0", 0, 0), ("combine_16", 16, 0), (f"combine_16_wait_{WINDOW_US}us", 16, WINDOW_US))


def _region(call):
    """THREADS x CALLS calls `call(thread, j)` -> seconds"""
    bar = threading.Barrier(THREADS + 1)
    err = []

    def work(t):
        bar.wait()
        try:
            for j in range(CALLS):
                call(t, j)
        except Exception as e:          # noqa: BLE001
            err.append(repr(e))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for t in ts:
        t.start()
    bar.wait()
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    if err:
        raise RuntimeError(err[0])
    return dt


def _measure(idx, call, baseline):
    configs = CONFIGS[:1] if baseline else CONFIGS
    times = {name: [] for name, _, _ in configs}
    stats = {}
    for r in range(REGIONS + 1):                      # region 0 warms every configuration up
        for name, width, wait in configs:
            if not baseline:
                idx.set_option("combine", width)
                idx.set_option("combine_wait_us", wait)
                before = idx.combine_stats()
            dt = _region(call)
            if r:
                times[name].append(dt)
                if not baseline and width:
                    now = idx.combine_stats()
                    stats.setdefault(name, []).append((now["queries"] - before["queries"]) / max(1, now["batches"] - before["batches"]))
    out = {}
    for name, _, _ in configs:
        t = np.array(times[name]) / (THREADS * CALLS) * 1e6
        out[name] = {"us_per_call": float(np.median(t)), "spread": float((t.max() - t.min()) / np.median(t))}
        if name in stats:
            out[name]["queries_per_batch"] = float(np.median(stats[name]))
    if not baseline:
        idx.set_option("combine", 0)
        idx.set_option("combine_wait_us", 0)
        for name, _, _ in configs[1:]:
            out[name]["over_combine_0"] = out[name]["us_per_call"] / out["combine_0"]["us_per_call"]
    return out


def _search_case(torch, device, rows, dim, dtype, seed, baseline):
    from comorag_amd.index import DenseIndex
    from tools.bench_extras import _unit_rows_dev
    idx = DenseIndex(dim, dtype, device=device.index or 0, capacity_hint=rows)
    for blk in _unit_rows_dev(torch, rows, dim, device, seed):
        idx.append_dev(blk)
    torch.cuda.synchronize(device)
    Q = np.random.default_rng(seed + 1).standard_normal((THREADS * CALLS, dim)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    res = {"rows": rows, "dim": dim, "dtype": dtype, "k": K}
    res.update(_measure(idx, lambda t, j: idx.search(Q[t * CALLS + j], K), baseline))
    idx.close()
    return res


def _ppr_case(torch, device, n_pass, n_ent, dim, dtype, seed, baseline):
    """the graphs of tools/ppr_batch_bench.py"""
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores
    from tools.bench_extras import _unit_rows_dev
    rng = np.random.default_rng(seed)
    idx = DenseIndex(dim, dtype, device=device.index or 0, capacity_hint=n_pass)
    for blk in _unit_rows_dev(torch, n_pass, dim, device, seed + 1):
        idx.append_dev(blk)
    torch.cuda.synchronize(device)
    nv = n_ent + n_pass
    passage_vertex = (n_ent + np.arange(n_pass)).astype(np.int32)
    src = np.concatenate([rng.integers(0, n_ent, 3 * n_pass), rng.integers(0, n_ent, 2 * n_ent)]).astype(np.int32)
    dst = np.concatenate([np.repeat(passage_vertex, 3), rng.integers(0, n_ent, 2 * n_ent)]).astype(np.int32)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    g = DeviceGraph(nv, src, dst, rng.uniform(0.5, 1.5, len(src)), device=device.index or 0)
    g.set_passage_vertices(passage_vertex)
    Q = rng.standard_normal((THREADS * CALLS, dim)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    seeds = [(np.unique(rng.integers(0, n_ent, 6)).astype(np.int32),) for _ in range(THREADS * CALLS)]
    seeds = [(sv[0], rng.uniform(0.2, 1.0, len(sv[0]))) for sv in seeds]
    res = {"passages": n_pass, "entities": n_ent, "edges": int(len(src)), "dim": dim, "dtype": dtype}
    res.update(_measure(idx, lambda t, j: ppr_passage_scores(idx, g, Q[t * CALLS + j], seeds[t * CALLS + j], 0.05), baseline))
    idx.close(); g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="search_1M,search_5K,ppr_comorag,ppr_1M")
    ap.add_argument("--baseline", action="store_true", help="combine = 0 only, no option is touched (runs on a library without the combiner)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    import torch
    device = torch.device("cuda", 0)
    cases = {
        "search_1M": lambda: _search_case(torch, device, 1_000_000, 768, "bf16", 8101, a.baseline),
        "search_5K": lambda: _search_case(torch, device, 5_000, 768, "f32", 8102, a.baseline),
        "ppr_comorag": lambda: _ppr_case(torch, device, 5_000, 1_500, 768, "f32", 7001, a.baseline),
        "ppr_1M": lambda: _ppr_case(torch, device, 1_000_000, 200_000, 768, "bf16", 7002, a.baseline),
    }
    out = {"tool": "tools/combine_bench.py", "device": torch.cuda.get_device_name(0), "threads": THREADS, "calls_per_thread": CALLS, "regions": REGIONS,
           "library": os.environ.get("COMORAG_HIP_LIB", "default")}
    for name in a.only.split(","):
        out[name] = cases[name]()
        print(f"# {name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
