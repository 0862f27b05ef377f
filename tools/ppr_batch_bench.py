"""Batched vs sequential DPR-seeded personalised PageRank (cmr_index_ppr_batch vs B x cmr_index_ppr).

    python tools/ppr_batch_bench.py [--small-only] [--out profiles/ppr_batch.json]

The two graphs of tools/bench_extras.py:_ppr_case (5 K passages / 1.5 K entities / 768-d f32; 1 M passages / 200 K entities / bf16).
For B in {1, 2, 4, 8, 16}: the median over REGIONS timed regions of CALLS calls each, after warm-up, of (a) B sequential
`ppr_passage_scores` calls and (b) one `ppr_passage_scores_batch`; both in the same process, interleaved per B, so box-to-box spread
does not enter their ratio.  The step time is the slope of `DeviceGraph.ppr_batch` over the iteration count (43 vs 3 steps: copies and
the one-off kernels cancel); its algorithmic bytes — col + wnorm + ELL records once, BW * 8 per gathered entry, r and y — over that time
is the fraction of HBM peak.  Prints ONE JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0
BATCHES = (1, 2, 4, 8, 16)
REGIONS, CALLS = 5, 20


def _region_us(fn, calls, regions=REGIONS, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        t.append((time.perf_counter() - t0) / calls)
    return float(np.median(t) * 1e6), float((max(t) - min(t)) / np.median(t))


def _case(torch, device, n_pass, n_ent, dim, dtype, seed, calls):
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores, ppr_passage_scores_batch
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
    w = rng.uniform(0.5, 1.5, len(src))
    g = DeviceGraph(nv, src, dst, w, device=device.index or 0); g.set_passage_vertices(passage_vertex)
    Q = rng.standard_normal((16, dim)).astype(np.float32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    phrases = []
    for _ in range(16):
        ph = np.zeros(nv); ph[rng.integers(0, n_ent, 6)] = rng.uniform(0.2, 1.0, 6)
        sv = np.flatnonzero(ph).astype(np.int32)
        phrases.append((sv, ph[sv]))                      # the sparse form on both sides: no dense [nv] scan on the host in either timing
    deg = np.bincount(np.concatenate([src, dst]), minlength=nv)
    n_one = int((deg <= 4).sum())
    csr_entries = int(deg[deg > 4].sum())
    entries = int(deg.sum())
    res = {"passages": n_pass, "entities": n_ent, "edges": int(len(src)), "dim": dim, "dtype": dtype, "iterations": 43,
           "regions": REGIONS, "calls_per_region": calls, "by_batch": {}}
    for B in BATCHES:
        seq = lambda: [ppr_passage_scores(idx, g, Q[b], phrases[b], 0.05) for b in range(B)]
        bat = lambda: ppr_passage_scores_batch(idx, g, Q[:B], phrases[:B], 0.05)
        equal = all(np.array_equal(a, b) for a, b in zip(seq(), bat()))
        seq_us, seq_spread = _region_us(seq, calls)
        bat_us, bat_spread = _region_us(bat, calls)
        row = {"sequential_us_per_query": seq_us / B, "batch_us_per_query": bat_us / B, "batch_over_sequential": bat_us / seq_us,
               "sequential_spread": seq_spread, "batch_spread": bat_spread, "bit_equal": bool(equal)}
        if B > 1:
            bw = 2 if B <= 2 else 4 if B <= 4 else 8 if B <= 8 else 16
            R = np.zeros((B, nv)); R[:, :n_ent] = rng.uniform(0, 1, (B, n_ent))
            t43, _ = _region_us(lambda: g.ppr_batch(R, max_iter=43), max(3, calls // 4), warm=2)
            t3, _ = _region_us(lambda: g.ppr_batch(R, max_iter=3), max(3, calls // 4), warm=2)
            step_us = (t43 - t3) / 40.0
            algo = csr_entries * 12 + n_one * 48 + entries * bw * 8 + 2 * nv * bw * 8
            row.update({"step_us": step_us, "step_algorithmic_bytes": algo, "step_frac_of_hbm": algo / (step_us * 1e-6) / 1e9 / HBM_PEAK_GBS})
        else:
            r1 = np.zeros(nv); r1[:n_ent] = rng.uniform(0, 1, n_ent)
            t43, _ = _region_us(lambda: g.ppr(r1, max_iter=43), max(3, calls // 4), warm=2)
            t3, _ = _region_us(lambda: g.ppr(r1, max_iter=3), max(3, calls // 4), warm=2)
            step_us = (t43 - t3) / 40.0
            algo = csr_entries * 12 + n_one * 48 + entries * 8 + 2 * nv * 8
            row.update({"step_us": step_us, "step_algorithmic_bytes": algo, "step_frac_of_hbm": algo / (step_us * 1e-6) / 1e9 / HBM_PEAK_GBS})
        res["by_batch"][str(B)] = row
    idx.close(); g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true", help="ComoRAG scale only (skips the 1 M-passage graph)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    import torch
    device = torch.device("cuda", 0)
    out = {"tool": "tools/ppr_batch_bench.py", "device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS,
           "comorag_scale": _case(torch, device, 5_000, 1_500, 768, "f32", 7001, CALLS)}
    if not a.small_only:
        out["at_1M_passages"] = _case(torch, device, 1_000_000, 200_000, 768, "bf16", 7002, CALLS)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
