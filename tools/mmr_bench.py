"""Diversified top-k (cmr_index_search_mmr) on one MI355X: 1 M x 768 bf16 rows, k = 10.

    python tools/mmr_bench.py [--rows 1000000] [--regions 7] [--out profiles/mmr.json]

Rows: B = 1 / 16 / 64 queries x fetch_k = 50 / 128.  Arms, all timed in the same run:
(a) `search_mmr`   DenseIndex.search_mmr: the candidate search, the pair scores and the selection on one stream, [B, k] to the host.
(b) `by_hand`      what a caller writes without it, from calls of the parent commit: search(q, fetch_k), get_rows of the candidates
                   (fetch_k x dim floats per query to the host), a numpy Gram matrix per query and the greedy loop in Python.
(c) `search`       plain search(q, fetch_k): the floor — what (a) adds on top of it is the pair scores and the selection.
(b) sums in the host BLAS's order, so its picks may differ from (a)'s where two values are a rounding apart; the share of equal rows is
reported, outside the clock, and is not a pass criterion.
Timing: a host clock around one call, buffers warmed by an uncounted region 0; a row is the median over --regions regions (>= 5) with min
and max; the arms alternate region by region.  Judging (the project's rule, tools/rerank_bench.py): a row wins when its median is below the
other's by more than the two min-to-max spreads added.  Every row is reported, also those that lose.  Prints ONE JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIM = 768
K = 10
LAM = 0.5


def _row(times_s):
    t = np.asarray(times_s) * 1e3
    return {"ms_per_call": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["ms_per_call"] < old["ms_per_call"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _versus(new, old):
    wins, loses = passes(new, old), passes(old, new)
    return {"ratio": new["ms_per_call"] / old["ms_per_call"], "wins": wins, "loses": loses, "verdict": "win" if wins else "loss" if loses else "tie"}


def by_hand(idx, q, k, fetch_k, lam):
    """search + get_rows + numpy Gram + Python greedy loop (the same rule: max-similarity penalty, first of equal values)"""
    ids, sc, _, _ = idx.search(q, fetch_k, with_minmax=False)
    rows = idx.get_rows(ids).reshape(ids.shape[0], ids.shape[1], -1)
    lam32, oml = np.float32(lam), np.float32(1.0) - np.float32(lam)
    out_i, out_s = np.full((len(ids), k), -1, np.int64), np.full((len(ids), k), -np.inf, np.float32)
    for i in range(len(ids)):
        G = rows[i] @ rows[i].T
        open_ = np.ones(ids.shape[1], bool)
        pen = np.full(ids.shape[1], -np.inf, np.float32)
        for n in range(min(k, ids.shape[1])):
            val = sc[i] if n == 0 else lam32 * sc[i] - oml * pen
            best = int(np.argmax(np.where(open_, val, -np.inf)))
            out_i[i, n], out_s[i, n] = ids[i, best], sc[i, best]
            open_[best] = False
            pen = np.maximum(pen, G[best])
    return out_i, out_s


def _time(arms, regions):
    t = {name: [] for name in arms}
    for region in range(regions + 1):      # region 0 warms every arm up and is not counted
        for name, call in arms.items():
            t0 = time.perf_counter(); call(); dt = time.perf_counter() - t0
            if region:
                t[name].append(dt)
    return {name: _row(v) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mmr_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex
    n = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.cat([torch.nn.functional.normalize(torch.randn((min(100_000, n - r0), DIM), generator=gen, device=dev), dim=1).cpu()
                   for r0 in range(0, n, 100_000)]).numpy()
    q_all = torch.nn.functional.normalize(torch.randn((64, DIM), generator=gen, device=dev), dim=1).cpu().numpy()
    idx = DenseIndex(DIM, "bf16", capacity_hint=n)
    idx.append(x)
    del x
    out = {"tool": "tools/mmr_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "k": K, "lambda": LAM, "regions": a.regions,
           "unit": "ms per call (median, min, max)", "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev), "rows_measured": {}}
    for B in (1, 16, 64):
        q = np.ascontiguousarray(q_all[:B])
        for F in (50, 128):
            got = idx.search_mmr(q, K, F, LAM)
            hand = by_hand(idx, q, K, F, LAM)
            case = {"queries": B, "fetch_k": F, "rows_equal_to_by_hand": float(np.mean([got[0][i].tolist() == hand[0][i].tolist() for i in range(B)])),
                    "route": int(idx.get_option("last_route"))}
            case.update(_time({"search_mmr": lambda: idx.search_mmr(q, K, F, LAM), "by_hand": lambda: by_hand(idx, q, K, F, LAM),
                               "search": lambda: idx.search(q, F, with_minmax=False)}, a.regions))
            case["search_mmr_vs_by_hand"] = _versus(case["search_mmr"], case["by_hand"])
            case["search_mmr_vs_search"] = _versus(case["search_mmr"], case["search"])
            case["added_ms_over_search"] = case["search_mmr"]["ms_per_call"] - case["search"]["ms_per_call"]
            out["rows_measured"][f"B{B}_F{F}"] = case
            print(f"# B{B}_F{F}: {json.dumps(case)}", file=sys.stderr, flush=True)
    idx.close()
    out["verdicts_vs_by_hand"] = {k: c["search_mmr_vs_by_hand"]["verdict"] for k, c in out["rows_measured"].items()}
    out["verdicts_vs_search"] = {k: c["search_mmr_vs_search"]["verdict"] for k, c in out["rows_measured"].items()}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
