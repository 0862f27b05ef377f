"""Filtered score-bound searches (cmr_index_range_search_masked / _ids, cmr_index_search_min_score_masked / _ids) on one
MI355X: 1 M x 768 bf16 rows.

    python tools/filtered_range_bench.py [--rows 1000000] [--regions 7] [--out profiles/filtered_range.json]

Rows: B = 1 / 16 / 64 queries x a bound that leaves about 100 and about 10 000 UNFILTERED hits per query (read off the sorted scores of the
first query) x a filter:
  `exclude_200_ids`  every query excludes 200 row ids of its own — its best 200, the ids an earlier search returned (id form);
  `shared_half`      one random 50 % allow bitmap for every query;
  `each_1_percent`   a random 1 % allow bitmap per query.
Range arms, all timed in the same run:
(a) `filtered`       DenseIndex.range_search_filtered / range_search_filtered_ids: the new call.
(b) `range_drop`     what a caller does without it: the unfiltered DenseIndex.range_search, then per list a numpy drop of the disallowed
                     entries (a lookup in the bool rows of the bitmap / np.isin against the excluded ids) — calls of the parent commit.
(c) `scores_numpy`   (the 1 % rows) DenseIndex.scores (4 * B * N bytes to the host), then per query the selection among the allowed rows and
                     np.lexsort — also the parent commit's.
Threshold arms: `filtered` = search_min_score_filtered(_ids)(k = 128) against `topk_cut` = search_filtered / _each / _ids (k = 128) and a cut of
the entries below the bound on the host.
The lists of the arms are compared bit for bit once per row, outside the clock.
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
K = 128


def _row(times_s):
    t = np.asarray(times_s) * 1e3
    return {"ms_per_call": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["ms_per_call"] < old["ms_per_call"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _versus(new, old):
    return {"ratio": new["ms_per_call"] / old["ms_per_call"], "wins": passes(new, old), "loses": passes(old, new)}


def _csr(lims, ids, sc):
    return (np.array(lims, np.int64), np.concatenate(ids).astype(np.int64) if ids else np.empty(0, np.int64),
            np.concatenate(sc).astype(np.float32) if sc else np.empty(0, np.float32))


def range_drop(idx, q, bound, keep_bool=None, exclude=None):
    """the unfiltered range search, then the disallowed entries dropped per list.  keep_bool: bool [n] (shared) or [nq, n]; exclude: int64
    [nq, m] row ids per query"""
    lims, ids, sc = idx.range_search(q, bound)
    o_l, o_i, o_s = [0], [], []
    for i in range(len(lims) - 1):
        seg_i, seg_s = ids[lims[i]:lims[i + 1]], sc[lims[i]:lims[i + 1]]
        keep = (keep_bool[seg_i] if keep_bool.ndim == 1 else keep_bool[i][seg_i]) if keep_bool is not None else np.isin(seg_i, exclude[i], invert=True)
        o_i.append(seg_i[keep]); o_s.append(seg_s[keep]); o_l.append(o_l[-1] + int(keep.sum()))
    return _csr(o_l, o_i, o_s)


def scores_numpy(idx, q, bound, keep_bool):
    S = idx.scores(q)
    b = np.float32(bound)
    o_l, o_i, o_s = [0], [], []
    for i in range(len(S)):
        keep = np.flatnonzero((S[i] >= b) & keep_bool[i])
        order = keep[np.lexsort((keep, -S[i][keep]))]
        o_i.append(order); o_s.append(S[i][order]); o_l.append(o_l[-1] + len(order))
    return _csr(o_l, o_i, o_s)


def cut(ids, sc, bound):
    """a filtered top-k's entries below the bound as padding"""
    ids, sc = ids.copy(), sc.copy()
    low = ~(sc >= np.float32(bound))
    ids[low] = -1
    sc[low] = -np.inf
    return ids, sc


def _pack(keep_bool):
    n = keep_bool.shape[-1]
    bits = np.zeros(keep_bool.shape[:-1] + ((n + 31) // 32 * 32,), np.uint8)
    bits[..., :n] = keep_bool
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little").view("<u4").astype(np.uint32))


def _same_csr(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def _same_rows(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


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
        raise SystemExit("filtered_range_bench.py needs an MI355X: a timing taken anywhere else says nothing")
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
    s0 = np.sort(idx.scores(q_all[:1])[0])[::-1]
    bounds = {"about_100_hits": float(s0[min(100, n - 1)]), "about_10000_hits": float(s0[min(10_000, n - 1)])}
    rng = np.random.default_rng(2)
    half = rng.random(n) < 0.5
    one = rng.random((64, n)) < 0.01
    best = idx.range_search(q_all, float(s0[min(1000, n - 1)]))
    ex_all = np.stack([best[1][best[0][i]:best[0][i] + 200] for i in range(64)]).astype(np.int64)      # every query's best 200 (lists hold ~1000)
    half_w, one_w = _pack(half), _pack(one)

    out = {"tool": "tools/filtered_range_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "regions": a.regions, "k_threshold": K,
           "unit": "ms per call (median, min, max)", "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev), "bounds": bounds, "range_rows": {}, "threshold_rows": {}}
    for B in (1, 16, 64):
        q = np.ascontiguousarray(q_all[:B])
        ex = np.ascontiguousarray(ex_all[:B])
        one_b, one_wb = one[:B], np.ascontiguousarray(one_w[:B])
        filters = {
            "exclude_200_ids": dict(new=lambda b: idx.range_search_filtered_ids(q, b, exclude=ex), old=lambda b: range_drop(idx, q, b, exclude=ex),
                                    thr=lambda b: idx.search_min_score_filtered_ids(q, K, b, exclude=ex),
                                    topk=lambda b: cut(*idx.search_filtered_ids(q, K, exclude=ex, with_minmax=False)[:2], b)),
            "shared_half": dict(new=lambda b: idx.range_search_filtered(q, b, half_w), old=lambda b: range_drop(idx, q, b, keep_bool=half),
                                thr=lambda b: idx.search_min_score_filtered(q, K, b, half_w),
                                topk=lambda b: cut(*idx.search_filtered(q, K, half_w, with_minmax=False)[:2], b)),
            "each_1_percent": dict(new=lambda b: idx.range_search_filtered(q, b, one_wb), old=lambda b: range_drop(idx, q, b, keep_bool=one_b),
                                   scores=lambda b: scores_numpy(idx, q, b, one_b), thr=lambda b: idx.search_min_score_filtered(q, K, b, one_wb),
                                   topk=lambda b: cut(*idx.search_filtered_each(q, K, one_wb, with_minmax=False)[:2], b)),
        }
        for bname, b in bounds.items():
            for fname, f in filters.items():
                got = f["new"](b)
                counts = np.diff(got[0])
                same = _same_csr(got, f["old"](b)) and ("scores" not in f or _same_csr(got, f["scores"](b)))
                arms = {"filtered": lambda: f["new"](b), "range_drop": lambda: f["old"](b)}
                if "scores" in f:
                    arms["scores_numpy"] = lambda: f["scores"](b)
                case = {"queries": B, "bound": b, "unfiltered_hits_per_query": float(np.diff(idx.range_search(q, b)[0]).mean()),
                        "hits_per_query": {"min": int(counts.min()), "mean": float(counts.mean()), "max": int(counts.max())}, "same_bits": same}
                case.update(_time(arms, a.regions))
                case["filtered_vs_range_drop"] = _versus(case["filtered"], case["range_drop"])
                if "scores" in f:
                    case["filtered_vs_scores_numpy"] = _versus(case["filtered"], case["scores_numpy"])
                out["range_rows"][f"B{B}_{bname}_{fname}"] = case
                print(f"# range B{B}_{bname}_{fname}: {json.dumps(case)}", file=sys.stderr, flush=True)
                tcase = {"queries": B, "bound": b, "same_bits": _same_rows(f["thr"](b), f["topk"](b))}
                tcase.update(_time({"filtered": lambda: f["thr"](b), "topk_cut": lambda: f["topk"](b)}, a.regions))
                tcase["filtered_vs_topk_cut"] = _versus(tcase["filtered"], tcase["topk_cut"])
                out["threshold_rows"][f"B{B}_{bname}_{fname}"] = tcase
                print(f"# threshold B{B}_{bname}_{fname}: {json.dumps(tcase)}", file=sys.stderr, flush=True)
    idx.close()
    out["losing_rows"] = [k for k, c in out["range_rows"].items() if c["filtered_vs_range_drop"]["loses"] or c.get("filtered_vs_scores_numpy", {}).get("loses")] + \
                         ["threshold_" + k for k, c in out["threshold_rows"].items() if c["filtered_vs_topk_cut"]["loses"]]
    out["winning_rows"] = [k for k, c in out["range_rows"].items() if c["filtered_vs_range_drop"]["wins"]] + \
                          ["threshold_" + k for k, c in out["threshold_rows"].items() if c["filtered_vs_topk_cut"]["wins"]]
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
