"""Batched vs sequential DPR-seeded personalised PageRank (cmr_index_ppr_batch vs B x cmr_index_ppr).

    python tools/ppr_batch_bench.py [--small-only] [--out profiles/ppr_batch.json]

The two graphs of tools/bench_extras.py:_ppr_case (5 K passages / 1.5 K entities / 768-d f32; 1 M passages / 200 K entities / bf16).
For B in {1, 2, 4, 8, 16}: the median over REGIONS timed regions of CALLS calls each, after warm-up, of (a) B sequential
`ppr_passage_scores` calls and (b) one `ppr_passage_scores_batch`; both in the same process, interleaved per B, so box-to-box spread
does not enter their ratio.  The step time is the slope of `DeviceGraph.ppr_batch` over the iteration count (43 vs 3 steps: copies and
the one-off kernels cancel); its algorithmic bytes — col + wnorm + ELL records once, BW * 8 per gathered entry, r and y — over that time
is the fraction of HBM peak.  Prints ONE JSON object.

    python tools/ppr_batch_bench.py --rank [--small-only] [--out profiles/ppr_rank.json]

The ranking instead, per query, for both graphs and B in {1, 16}: (a) `ppr_passage_scores(_batch)` plus the reference's two
host lines (np.argsort(doc)[::-1], doc[ids.tolist()]: ComoRAG.py:1101-1105), (b) the ranked call `ppr_passage_ranked(_batch)`, (c) the unranked
device call alone — (b) - (c) is what the sort, its finish kernel and the 8 more bytes per row of copy cost.  Regions of (a), (b), (c) alternate
in one process; medians of REGIONS regions with their spread.  Then the same three at B = 1 for n_rows in RANK_SWEEP (128-d f32 rows, entities =
rows / 4): the smallest size from which (b) <= (a) holds at every larger one, rounded up to a multiple of 1024 and never below 8192, is
comorag_amd.ppr.DEVICE_RANK_MIN_ROWS.
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
RANK_SWEEP = (2048, 4096, 8192, 16384, 32768, 65536)


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


def _alternating_us(fns, calls, regions=REGIONS, warm=2):
    """[(median us per call, spread)] of several callables whose timed regions alternate: a, b, c, a, b, c, ..."""
    for fn in fns:
        for _ in range(warm):
            fn()
    t = [[] for _ in fns]
    for _ in range(regions):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[k].append((time.perf_counter() - t0) / calls)
    return [(float(np.median(x) * 1e6), float((max(x) - min(x)) / np.median(x))) for x in t]


def _host_lines(doc):
    ids = np.argsort(doc)[::-1]
    return ids, doc[ids.tolist()]


def _rank_rows(idx, g, Q, phrases, batches, calls):
    """{B: per-query times of (a) unranked call + host lines, (b) ranked call, (c) unranked call}"""
    from comorag_amd.ppr import ppr_passage_ranked, ppr_passage_ranked_batch, ppr_passage_scores, ppr_passage_scores_batch
    n = g.n_rows
    tiles = -(-n // 2048)
    out = {"rows": n, "sort_launches": 2 + 3 * 8, "workspace_bytes_per_row_and_query": 24 + 1024 * tiles / n,
           "extra_d2h_bytes_per_row_and_query": 8, "by_batch": {}}
    for B in batches:
        if B == 1:
            a = lambda: _host_lines(ppr_passage_scores(idx, g, Q[0], phrases[0], 0.05))
            b = lambda: ppr_passage_ranked(idx, g, Q[0], phrases[0], 0.05)
            c = lambda: ppr_passage_scores(idx, g, Q[0], phrases[0], 0.05)
            doc, (ids, sc) = c(), b()
            equal = np.array_equal(ids, np.argsort(-doc, kind="stable")) and np.array_equal(sc, doc[ids])
        else:
            a = lambda: [_host_lines(d) for d in ppr_passage_scores_batch(idx, g, Q[:B], phrases[:B], 0.05)]
            b = lambda: ppr_passage_ranked_batch(idx, g, Q[:B], phrases[:B], 0.05)
            c = lambda: ppr_passage_scores_batch(idx, g, Q[:B], phrases[:B], 0.05)
            doc, (ids, sc) = c(), b()
            equal = all(np.array_equal(ids[q], np.argsort(-doc[q], kind="stable")) and np.array_equal(sc[q], doc[q][ids[q]]) for q in range(B))
        (ta, sa), (tb, sb), (tc, sc_) = _alternating_us([a, b, c], calls)
        out["by_batch"][str(B)] = {"host_ranking_us_per_query": ta / B, "device_ranking_us_per_query": tb / B, "unranked_call_us_per_query": tc / B,
                                   "sort_cost_us_per_query": (tb - tc) / B, "device_over_host": tb / ta, "host_spread": sa, "device_spread": sb,
                                   "unranked_spread": sc_, "device_below_host_by_more_than_spread": bool(tb * (1 + sb) < ta * (1 - sa)),
                                   "equals_stable_argsort": bool(equal)}
    return out


def _rank_sweep(torch, device):
    """B = 1 over RANK_SWEEP; the crossover by the rule stated in the module docstring"""
    rows = {}
    for n in RANK_SWEEP:
        rows[str(n)] = _rank_case(torch, device, n, n // 4, 128, "f32", 7100 + n, 40, batches=(1,))["ranking"]["by_batch"]["1"]
    ok_from = None
    for n in reversed(RANK_SWEEP):
        if rows[str(n)]["device_ranking_us_per_query"] <= rows[str(n)]["host_ranking_us_per_query"]:
            ok_from = n
        else:
            break
    thr = None if ok_from is None else max(8192, -(-ok_from // 1024) * 1024)
    return {"by_rows": rows, "device_not_slower_from": ok_from, "DEVICE_RANK_MIN_ROWS": thr}


def _build(torch, device, n_pass, n_ent, dim, dtype, seed):
    """(rng, index, graph, Q [16, dim], 16 sparse phrase-weight pairs, src, dst) of one bench graph"""
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph
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
    return rng, idx, g, Q, phrases, src, dst


def _rank_case(torch, device, n_pass, n_ent, dim, dtype, seed, calls, batches=(1, 16)):
    _, idx, g, Q, phrases, src, _ = _build(torch, device, n_pass, n_ent, dim, dtype, seed)
    res = {"passages": n_pass, "entities": n_ent, "edges": int(len(src)), "dim": dim, "dtype": dtype, "iterations": 43,
           "regions": REGIONS, "calls_per_region": calls, "ranking": _rank_rows(idx, g, Q, phrases, batches, calls)}
    idx.close(); g.close()
    return res


def _case(torch, device, n_pass, n_ent, dim, dtype, seed, calls):
    from comorag_amd.ppr import ppr_passage_scores, ppr_passage_scores_batch
    rng, idx, g, Q, phrases, src, dst = _build(torch, device, n_pass, n_ent, dim, dtype, seed)
    nv = n_ent + n_pass
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
    ap.add_argument("--rank", action="store_true", help="the ranking's rows (host lines vs ranked call) and the crossover sweep instead")
    a = ap.parse_args()
    import torch
    device = torch.device("cuda", 0)
    if a.rank:
        out = {"tool": "tools/ppr_batch_bench.py --rank", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
               "comorag_scale": _rank_case(torch, device, 5_000, 1_500, 768, "f32", 7001, CALLS)}
        if not a.small_only:
            out["at_1M_passages"] = _rank_case(torch, device, 1_000_000, 200_000, 768, "bf16", 7002, 3)
        out["sweep_b1"] = _rank_sweep(torch, device)
    else:
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
