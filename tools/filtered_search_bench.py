"""Filtered top-k (cmr_index_search_masked) on one MI355X: 1 M x 768 bf16 rows, k = 20, B in {1, 8, 64}, four masks.

    python tools/filtered_search_bench.py [--rows 1000000] [--regions 7] [--out profiles/filtered_search.json]

Masks: all ones, random 50 %, random 1 %, one contiguous 10 % block.  Three rows per (B, mask), on the same index and queries:
 (1) `filtered`   DenseIndex.search_filtered with the packed words (the call uploads them: 122 KiB at 1 M rows);
 (2) `unfiltered_chain`   DenseIndex.search held to the same route (scan_fin = 0, scan_no_tiny = 1, scan_no_small = 1): an otherwise identical
     pack / sample / scan / merge chain over ALL rows — the price of the mask, recorded as a ratio, no bar;
 (3) `scores_numpy`   what a user writes without the feature: DenseIndex.scores (all N floats per query), numpy masking, argpartition and a
     sort into the exported order (score descending, row ascending), min and max over the allowed rows.
Timing: a host clock around calls that end with their results on the host; every row is warmed up, then the rows alternate region by region;
a region is as many back-to-back calls as fill ~0.15 s (at least one); a row is the median over --regions regions (>= 5) with min and max, in
ms per call.  Judging (the project's rule, tools/rerank_bench.py): a row wins when its median is below the other's by more than the two
min-to-max spreads added.  Rows (1) and (3) must return the same ids: checked per case.  Prints ONE JSON object."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIM, K, BATCHES = 768, 20, (1, 8, 64)


def _row(times_s):
    t = np.asarray(times_s) * 1e3
    return {"ms_per_call": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["ms_per_call"] < old["ms_per_call"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _compare(new, old):
    return {"ratio": new["ms_per_call"] / old["ms_per_call"], "wins": passes(new, old), "loses": passes(old, new)}


def _masks(n):
    rng = np.random.default_rng(7)
    block = np.zeros(n, bool)
    block[n // 3: n // 3 + n // 10] = True
    return {"all_ones": np.ones(n, bool), "random_50": rng.random(n) < 0.5, "random_1": rng.random(n) < 0.01, "block_10": block}


def scores_numpy(idx, q, k, rows):
    """the user's own filter on the parent commit: every score to the host, the allowed columns, the k best in the exported order"""
    s = idx.scores(q)[:, rows]
    kk = min(k, s.shape[1])
    part = np.argpartition(-s, kk - 1, axis=1)[:, :kk] if kk < s.shape[1] else np.tile(np.arange(s.shape[1]), (len(q), 1))
    ps = np.take_along_axis(s, part, axis=1)
    order = np.lexsort((rows[part], -ps), axis=1)
    return rows[np.take_along_axis(part, order, axis=1)], np.take_along_axis(ps, order, axis=1), s.min(axis=1), s.max(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of back-to-back calls per timed region")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filtered_search_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex, pack_row_mask
    n = a.rows
    dev = torch.device("cuda", 0)
    idx = DenseIndex(DIM, "bf16", capacity_hint=n, options={"scan_fin": 0, "scan_no_tiny": 1, "scan_no_small": 1})
    gen = torch.Generator(device=dev).manual_seed(1)
    for r0 in range(0, n, 100_000):
        x = torch.randn((min(100_000, n - r0), DIM), generator=gen, device=dev)
        idx.append_dev(torch.nn.functional.normalize(x, dim=1).contiguous())
    torch.cuda.synchronize(dev)
    q_all = torch.nn.functional.normalize(torch.randn((max(BATCHES), DIM), generator=gen, device=dev), dim=1).cpu().numpy()
    out = {"rows": n, "dim": DIM, "dtype": "bf16", "k": K, "regions": a.regions, "window_s": a.window, "unit": "ms per call (median, min, max)",
           "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev), "cases": {}}
    for name, keep in _masks(n).items():
        words, rows = pack_row_mask(n, allow=keep), np.flatnonzero(keep)
        for b in BATCHES:
            q = np.ascontiguousarray(q_all[:b])
            arms = {"filtered": lambda: idx.search_filtered(q, K, mask=words), "unfiltered_chain": lambda: idx.search(q, K),
                    "scores_numpy": lambda: scores_numpy(idx, q, K, rows)}
            res, calls = {}, {}
            for arm, call in arms.items():
                call()
                t0 = time.perf_counter()
                res[arm] = call()
                calls[arm] = max(1, min(500, math.ceil(a.window / max(time.perf_counter() - t0, 1e-6))))
            idx.search_filtered(q, K, mask=words)      # (last_route is the index's last call: ask right behind a filtered one)
            route = idx.get_option("last_route")
            times = {arm: [] for arm in arms}
            for _ in range(a.regions):
                for arm, call in arms.items():
                    t0 = time.perf_counter()
                    for _ in range(calls[arm]):
                        call()
                    times[arm].append((time.perf_counter() - t0) / calls[arm])
            case = {arm: dict(_row(t), calls_per_region=calls[arm]) for arm, t in times.items()}
            case["allowed_rows"] = int(len(rows))
            case["filtered_route"] = hex(route)
            case["same_ids_as_scores_numpy"] = bool(np.array_equal(res["filtered"][0], res["scores_numpy"][0]))
            case["filtered_vs_scores_numpy"] = _compare(case["filtered"], case["scores_numpy"])
            case["mask_price_filtered_over_unfiltered_chain"] = case["filtered"]["ms_per_call"] / case["unfiltered_chain"]["ms_per_call"]
            out["cases"][f"{name}_B{b}"] = case
            print(f"# {name} B={b}: {json.dumps(case)}", file=sys.stderr, flush=True)
    out["filtered_beats_scores_numpy_everywhere"] = all(c["filtered_vs_scores_numpy"]["wins"] for c in out["cases"].values())
    idx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
