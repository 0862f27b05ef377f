"""Per-query filtered top-k (cmr_index_search_masked_each) on one MI355X: 1 M x 768 bf16 rows, k = 20.

    python tools/filtered_each_bench.py [--rows 1000000] [--regions 7] [--only a,b,c] [--loop-only] [--parent-json FILE] [--out profiles/filtered_each.json]

(a) ONE call against B calls, B in {8, 16, 64}: `each` = DenseIndex.search_filtered_each with B masks against `loop` = B sequential one-query
    DenseIndex.search_filtered calls with the same masks (what a user writes without the feature).  Masks: every query excludes its own
    random 1 %; every query allows its own random 50 %; every query allows one of four disjoint 25 % blocks (namespaces).  Both arms return
    the same ids: checked per case.
    --loop-only measures the `loop` arm alone and touches nothing newer than search_filtered: the form that runs on the parent commit's tree
    (a copy of this file in its tools/).  --parent-json FILE takes that run's output and judges `each` against the PARENT's loop as well.
(b) the price of per-query words: `each` with one mask repeated B times against DenseIndex.search_filtered with that mask at the same B — a
    ratio, no bar; once through the host calls (which upload B x 122 KiB of words against 122 KiB) and once through the _dev forms with
    queries and words resident on the device (no upload: the kernel's in-place read alone).
(c) combining: 16 threads x 50 one-query search_filtered calls, a mask per thread, "combine" = 16 with "combine_filtered" 0 against 1, gather
    window 0 — us per call and queries per device call; and one thread alone, which must not lose.
Timing: a host clock around calls that end with their results on the host; every row is warmed up, then the rows alternate region by region;
a region is as many back-to-back calls as fill ~0.15 s (at least one; (c): 16 x 50 calls); a row is the median over --regions regions (>= 5)
with min and max.  Judging (the project's rule, tools/rerank_bench.py): a row wins when its median is below the other's by more than the two
min-to-max spreads added.  Prints ONE JSON object."""
import argparse
import json
import math
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIM, K, BATCHES = 768, 20, (8, 16, 64)
THREADS, CALLS = 16, 50


def _row(times_s, scale=1e3, unit="ms_per_call"):
    t = np.asarray(times_s) * scale
    return {unit: float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old, unit="ms_per_call") -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new[unit] < old[unit] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _compare(new, old, unit="ms_per_call"):
    return {"ratio": new[unit] / old[unit], "wins": passes(new, old, unit), "loses": passes(old, new, unit)}


def _keeps(n, kind, b):
    """bool [b, n]: query i's allowed rows"""
    rng = np.random.default_rng({"exclude_own_1": 11, "allow_own_50": 12, "namespace_25": 13}[kind])
    if kind == "exclude_own_1":
        return rng.random((b, n), dtype=np.float32) >= 0.01
    if kind == "allow_own_50":
        return rng.random((b, n), dtype=np.float32) < 0.5
    block = np.arange(n) * 4 // n                       # four disjoint quarters
    return np.stack([block == (i % 4) for i in range(b)])


def _alternate(arms, regions, window):
    """{arm: call} -> ({arm: [seconds per call per region]}, {arm: calls per region}, {arm: last result})"""
    res, calls = {}, {}
    for arm, call in arms.items():
        call()
        t0 = time.perf_counter()
        res[arm] = call()
        calls[arm] = max(1, min(500, math.ceil(window / max(time.perf_counter() - t0, 1e-6))))
    times = {arm: [] for arm in arms}
    for _ in range(regions):
        for arm, call in arms.items():
            t0 = time.perf_counter()
            for _ in range(calls[arm]):
                call()
            times[arm].append((time.perf_counter() - t0) / calls[arm])
    return times, calls, res


def _threads_region(call, threads):
    """threads x CALLS calls `call(thread, j)` from a barrier -> seconds"""
    bar = threading.Barrier(threads + 1)
    err = []

    def work(t):
        bar.wait()
        try:
            for j in range(CALLS):
                call(t, j)
        except Exception as e:          # noqa: BLE001
            err.append(repr(e))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of back-to-back calls per timed region")
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--loop-only", action="store_true", help="row (a)'s sequential loop alone: runs on a tree without the per-query call")
    ap.add_argument("--parent-json", default=None, help="output of a --loop-only run on the parent commit: `each` is judged against its loop too")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filtered_each_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex, pack_row_mask
    n = a.rows
    dev = torch.device("cuda", 0)
    idx = DenseIndex(DIM, "bf16", capacity_hint=n)
    gen = torch.Generator(device=dev).manual_seed(1)
    for r0 in range(0, n, 100_000):
        x = torch.randn((min(100_000, n - r0), DIM), generator=gen, device=dev)
        idx.append_dev(torch.nn.functional.normalize(x, dim=1).contiguous())
    torch.cuda.synchronize(dev)
    q_all = torch.nn.functional.normalize(torch.randn((THREADS * CALLS, DIM), generator=gen, device=dev), dim=1).cpu().numpy()
    parent = json.load(open(a.parent_json)) if a.parent_json else None
    out = {"tool": "tools/filtered_each_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "k": K, "regions": a.regions, "window_s": a.window,
           "unit": "ms per call (median, min, max); (c): us per call", "loop_only": bool(a.loop_only),
           "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev)}
    only = a.only.split(",")

    if "a" in only:
        out["a_one_call_against_B_calls"] = {}
        for kind in ("exclude_own_1", "allow_own_50", "namespace_25"):
            for b in BATCHES:
                q = np.ascontiguousarray(q_all[:b])
                words = np.stack([pack_row_mask(n, allow=keep) for keep in _keeps(n, kind, b)])

                def loop():
                    return np.concatenate([idx.search_filtered(q[i:i + 1], K, mask=words[i])[0] for i in range(b)])
                arms = {"loop": loop}
                if not a.loop_only:
                    arms["each"] = lambda: idx.search_filtered_each(q, K, masks=words)[0]
                times, calls, res = _alternate(arms, a.regions, a.window)
                case = {arm: dict(_row(t), calls_per_region=calls[arm]) for arm, t in times.items()}
                if not a.loop_only:
                    case["route"] = hex(idx.get_option("last_route"))
                    case["same_ids"] = bool(np.array_equal(res["each"], res["loop"]))
                    case["each_vs_loop"] = _compare(case["each"], case["loop"])
                    if parent:
                        case["loop_parent"] = parent["a_one_call_against_B_calls"][f"{kind}_B{b}"]["loop"]
                        case["each_vs_loop_parent"] = _compare(case["each"], case["loop_parent"])
                out["a_one_call_against_B_calls"][f"{kind}_B{b}"] = case
                print(f"# (a) {kind} B={b}: {json.dumps(case)}", file=sys.stderr, flush=True)
        if not a.loop_only:
            out["a_each_wins_every_row"] = all(c["each_vs_loop"]["wins"] and c.get("each_vs_loop_parent", {"wins": True})["wins"]
                                               for c in out["a_one_call_against_B_calls"].values())

    if "b" in only and not a.loop_only:
        out["b_price_of_per_query_words"] = {}
        shared = pack_row_mask(n, allow=_keeps(n, "allow_own_50", 1)[0])
        for b in BATCHES:
            q = np.ascontiguousarray(q_all[:b])
            words = np.ascontiguousarray(np.tile(shared, (b, 1)))
            arms = {"each_same_mask": lambda: idx.search_filtered_each(q, K, masks=words)[0], "shared": lambda: idx.search_filtered(q, K, mask=shared)[0]}
            times, calls, res = _alternate(arms, a.regions, a.window)
            case = {arm: dict(_row(t), calls_per_region=calls[arm]) for arm, t in times.items()}
            case["same_ids"] = bool(np.array_equal(res["each_same_mask"], res["shared"]))
            case["each_over_shared"] = _compare(case["each_same_mask"], case["shared"])
            # the same pair with queries and words resident on the device (the _dev forms read them in place): no upload of B x 122 KiB in
            # the timed call, so what is left of the ratio is the kernel's in-place read of a word per query and panel
            q_t, ids_t, sc_t = torch.from_numpy(q).to(dev), torch.empty((b, K), dtype=torch.int64, device=dev), torch.empty((b, K), dtype=torch.float32, device=dev)
            w_t, s_t = torch.from_numpy(words.view(np.int32)).to(dev), torch.from_numpy(shared.view(np.int32)).to(dev)

            def each_dev():
                idx.search_filtered_each_dev(q_t, K, w_t, ids_t, sc_t)
                torch.cuda.synchronize(dev)

            def shared_dev():
                idx.search_filtered_dev(q_t, K, s_t, ids_t, sc_t)
                torch.cuda.synchronize(dev)
            times, calls, _ = _alternate({"each_same_mask_dev": each_dev, "shared_dev": shared_dev}, a.regions, a.window)
            case.update({arm: dict(_row(t), calls_per_region=calls[arm]) for arm, t in times.items()})
            case["each_dev_over_shared_dev"] = _compare(case["each_same_mask_dev"], case["shared_dev"])
            out["b_price_of_per_query_words"][f"B{b}"] = case
            print(f"# (b) B={b}: {json.dumps(case)}", file=sys.stderr, flush=True)

    if "c" in only and not a.loop_only:
        words = np.stack([pack_row_mask(n, allow=keep) for keep in _keeps(n, "exclude_own_1", THREADS)])
        call = lambda t, j: idx.search_filtered(q_all[t * CALLS + j], K, mask=words[t])      # noqa: E731
        idx.set_option("combine", 16)
        idx.set_option("combine_wait_us", 0)
        res = {}
        for label, threads in (("sixteen_threads", THREADS), ("one_thread", 1)):
            times = {0: [], 1: []}
            per_batch = []
            for r in range(a.regions + 1):              # region 0 warms both settings up
                for cf in (0, 1):
                    idx.set_option("combine_filtered", cf)
                    before = idx.combine_stats()
                    dt = _threads_region(call, threads)
                    if r:
                        times[cf].append(dt / (threads * CALLS))
                        if cf:
                            now = idx.combine_stats()
                            per_batch.append((now["queries"] - before["queries"]) / max(1, now["batches"] - before["batches"]))
            off, on = _row(times[0], 1e6, "us_per_call"), _row(times[1], 1e6, "us_per_call")
            res[label] = {"combine_filtered_0": off, "combine_filtered_1": dict(on, queries_per_device_call=float(np.median(per_batch))),
                          "on_vs_off": _compare(on, off, "us_per_call")}
            print(f"# (c) {label}: {json.dumps(res[label])}", file=sys.stderr, flush=True)
        idx.set_option("combine_filtered", 0)
        idx.set_option("combine", 0)
        out["c_combining_filtered_calls"] = res

    idx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
