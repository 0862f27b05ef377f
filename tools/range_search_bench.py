"""Range search (cmr_index_range_search) on one MI355X: 1 M x 768 bf16 rows.

    python tools/range_search_bench.py [--rows 1000000] [--regions 7] [--join-rows 100000] [--out profiles/range_search.json]

Rows: B = 1 / 16 / 64 queries x a bound that leaves about 0, about 100 and about 10 000 hits per query (the bounds are read off the sorted
scores of the first query: random unit vectors score ~N(0, 1/768) against each other).  Arms, all timed in the same run:
(a) `range`        DenseIndex.range_search(q, bound): CSR lists, numpy copies.
(b) `scores_numpy` what a caller does without the feature for the same lists: DenseIndex.scores(q) (4 * B * N bytes to the host), then per
                   query the selection S >= bound and np.lexsort((rows, -S)) of the hits — calls that exist on the parent commit.
(c) `min_score`    DenseIndex.search_min_score(q, 128, bound), where every list fits in 128 entries (the threshold search cannot return
                   more and cannot say that it cut a list short) — also a call of the parent commit.
The lists of (a) and (b) are compared bit for bit once per row, outside the clock.
Join rows: retrieve_knn(min_score = 0.8, max_neighbours = 8) over --join-rows clustered unit rows (768-d, every row its own query: the
synonymy self-join), full_lists = "large_k" (the parent commit's re-run of the filled lists through the large-k path) against "range";
the two dicts are compared once.  The clock covers the whole call, index build included, in both arms.
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


def _row(times_s):
    t = np.asarray(times_s) * 1e3
    return {"ms_per_call": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["ms_per_call"] < old["ms_per_call"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _versus(new, old):
    return {"ratio": new["ms_per_call"] / old["ms_per_call"], "wins": passes(new, old), "loses": passes(old, new)}


def scores_numpy(idx, q, bound):
    S = idx.scores(q)
    lims, ids, sc = [0], [], []
    b = np.float32(bound)
    for i in range(len(S)):
        keep = np.flatnonzero(S[i] >= b)
        order = keep[np.lexsort((keep, -S[i][keep]))]
        ids.append(order.astype(np.int64)); sc.append(S[i][order]); lims.append(lims[-1] + len(order))
    return np.array(lims, np.int64), np.concatenate(ids), np.concatenate(sc)


def clustered(n, d, clusters, members, seed=3):
    """unit rows; `clusters` centres with `members` rows each at cosine ~0.86 .. 0.999 to their centre"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    pos = rng.permutation(n)[:clusters * (members + 1)].reshape(clusters, members + 1)
    for c in range(clusters):
        centre = X[pos[c, 0]]
        s = (0.05 + 0.5 * np.arange(members) / members).astype(np.float32)[:, None]
        v = centre[None, :] + s / np.float32(np.sqrt(d)) * rng.standard_normal((members, d), dtype=np.float32)
        X[pos[c, 1:]] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--join-rows", type=int, default=100_000)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("range_search_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex
    from comorag_amd.retrieval import retrieve_knn
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
    bounds = {"about_0_hits": float(s0[0]) + 0.1, "about_100_hits": float(s0[min(100, n - 1)]), "about_10000_hits": float(s0[min(10_000, n - 1)])}

    out = {"tool": "tools/range_search_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "regions": a.regions,
           "unit": "ms per call (median, min, max)", "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev), "bounds": bounds, "rows_by_case": {}}
    for B in (1, 16, 64):
        q = np.ascontiguousarray(q_all[:B])
        for name, b in bounds.items():
            counts = idx.range_count(q, b)
            fits = bool(counts.max() <= 128)
            got, want = idx.range_search(q, b), scores_numpy(idx, q, b)
            same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))
            t = {"range": [], "scores_numpy": [], "min_score": []}
            for region in range(a.regions + 1):      # region 0 warms every arm up and is not counted
                t0 = time.perf_counter(); idx.range_search(q, b); d_range = time.perf_counter() - t0
                t0 = time.perf_counter(); scores_numpy(idx, q, b); d_np = time.perf_counter() - t0
                t0 = time.perf_counter(); idx.search_min_score(q, 128, b); d_thr = time.perf_counter() - t0
                if region:
                    t["range"].append(d_range); t["scores_numpy"].append(d_np); t["min_score"].append(d_thr)
            case = {"queries": B, "bound": b, "hits_per_query": {"min": int(counts.min()), "mean": float(counts.mean()), "max": int(counts.max())},
                    "same_bits_as_scores_numpy": same, "range": _row(t["range"]), "scores_numpy": _row(t["scores_numpy"])}
            case["range_vs_scores_numpy"] = _versus(case["range"], case["scores_numpy"])
            if fits:
                case["min_score_k128"] = _row(t["min_score"])
                case["range_vs_min_score"] = _versus(case["range"], case["min_score_k128"])
            out["rows_by_case"][f"B{B}_{name}"] = case
            print(f"# B{B}_{name}: {json.dumps(case)}", file=sys.stderr, flush=True)
    idx.close()

    m = a.join_rows
    X = clustered(m, DIM, clusters=max(1, m // 2000), members=300)
    names = [f"e{i}" for i in range(m)]
    t = {"large_k": [], "range": []}
    res = {}
    for region in range(a.regions + 1):
        for arm in ("large_k", "range"):
            t0 = time.perf_counter()
            res[arm] = retrieve_knn(names, names, X, X, min_score=0.8, query_batch_size=1000, max_neighbours=8, full_lists=arm)
            dt = time.perf_counter() - t0
            if region:
                t[arm].append(dt)
    sizes = np.array([len(res["range"][k][0]) for k in names])
    join = {"rows": m, "dim": DIM, "index_dtype": "f32", "min_score": 0.8, "max_neighbours": 8, "queries_with_more": int((sizes > 8).sum()), "longest_list": int(sizes.max()),
            "same_dict": bool(res["large_k"] == res["range"]), "large_k": _row(t["large_k"]), "range": _row(t["range"])}
    join["range_vs_large_k"] = _versus(join["range"], join["large_k"])
    out["retrieve_knn_join"] = join
    print(f"# join: {json.dumps(join)}", file=sys.stderr, flush=True)
    out["losing_rows"] = [k for k, c in out["rows_by_case"].items() if c["range_vs_scores_numpy"]["loses"] or c.get("range_vs_min_score", {}).get("loses")] + \
                         (["retrieve_knn_join"] if join["range_vs_large_k"]["loses"] else [])
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
