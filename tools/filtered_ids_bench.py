"""Filtered top-k from row-id lists (cmr_index_search_ids) on one MI355X: 1 M x 768 bf16 rows, k = 20.

    python tools/filtered_ids_bench.py [--rows 1000000] [--regions 7] [--parent-only] [--parent-json FILE] [--out profiles/filtered_ids.json]

Rows: B in {1, 16, 64}, each with two list shapes — every query excludes 200 random ids of its own (a memory pool); every query allows a
random 1 % of the rows.  Arms:
(a) `ids`      DenseIndex.search_filtered_ids with the lists: the device builds the words.
(b) `pack`     what a user writes without the feature: DenseIndex.search_filtered_each(exclude= / allow=lists), INCLUDING its numpy packing
               of one bool[n] per query and the upload of B x n / 8 bytes of words.  --parent-only measures this arm alone and touches nothing
               newer than search_filtered_each: the form that runs on the parent commit's tree, in a process of its own (a copy of this file
               in its tools/).  --parent-json FILE takes that run's output; (a) is judged against the PARENT's (b).  The same arm measured on
               this tree beside (a) and (c) is reported as `pack_here`.
(c) `prepacked` DenseIndex.search_filtered_each(masks=words packed before the clock starts): the device and upload cost alone.
All arms return the same ids: checked per row.
(d) rehearsal: MultiDeviceIndex(devices=[0] * 4) — four LOGICAL shards on this one GPU, so no speed-up is to be had — holding the same rows
    returns the one-index bits through search_filtered_ids; its time is recorded beside the one index's, not judged.
Timing: a host clock around calls that end with their results on the host; every arm is warmed up, then the arms alternate region by region;
a region is as many back-to-back calls as fill ~0.15 s (at least one); a row is the median over --regions regions (>= 5) with min and max.
Judging (the project's rule, tools/rerank_bench.py): a row wins when its median is below the other's by more than the two min-to-max spreads
added.  Every row is reported, also those that do not win.  Prints ONE JSON object."""
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

DIM, K, BATCHES = 768, 20, (1, 16, 64)
SHARDS = 4


def _row(times_s, scale=1e3, unit="ms_per_call"):
    t = np.asarray(times_s) * scale
    return {unit: float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old, unit="ms_per_call") -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new[unit] < old[unit] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _compare(new, old, unit="ms_per_call"):
    return {"ratio": new[unit] / old[unit], "wins": passes(new, old, unit), "loses": passes(old, new, unit)}


def _lists(n, kind, b):
    """(mode, one int64 id array per query)"""
    rng = np.random.default_rng({"exclude_pool_200": 21, "allow_own_1pct": 22}[kind] * 1000 + b)
    if kind == "exclude_pool_200":
        return "exclude", [rng.choice(n, 200, replace=False).astype(np.int64) for _ in range(b)]
    return "allow", [np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64) for _ in range(b)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of back-to-back calls per timed region")
    ap.add_argument("--parent-only", action="store_true", help="arm (b) alone: runs on a tree without the id-list calls")
    ap.add_argument("--parent-json", default=None, help="output of a --parent-only run on the parent commit: (a) is judged against its (b)")
    ap.add_argument("--no-multi", action="store_true", help="skip the MultiDeviceIndex rehearsal (d)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filtered_ids_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex, pack_row_masks
    n = a.rows
    dev = torch.device("cuda", 0)
    idx = DenseIndex(DIM, "bf16", capacity_hint=n)
    multi = None
    if not a.parent_only and not a.no_multi:
        from comorag_amd.multi_index import MultiDeviceIndex
        multi = MultiDeviceIndex(DIM, "bf16", devices=[0] * SHARDS)
    gen = torch.Generator(device=dev).manual_seed(1)
    for r0 in range(0, n, 100_000):
        x = torch.nn.functional.normalize(torch.randn((min(100_000, n - r0), DIM), generator=gen, device=dev), dim=1).contiguous()
        idx.append_dev(x)
        if multi is not None:
            multi.append_dev(x)
    torch.cuda.synchronize(dev)
    q_all = torch.nn.functional.normalize(torch.randn((max(BATCHES), DIM), generator=gen, device=dev), dim=1).cpu().numpy()
    parent = json.load(open(a.parent_json)) if a.parent_json else None
    out = {"tool": "tools/filtered_ids_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "k": K, "regions": a.regions, "window_s": a.window,
           "unit": "ms per call (median, min, max)", "parent_only": bool(a.parent_only),
           "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev), "rows_by_case": {}}

    for kind in ("exclude_pool_200", "allow_own_1pct"):
        for b in BATCHES:
            q = np.ascontiguousarray(q_all[:b])
            mode, lists = _lists(n, kind, b)
            arms = {"pack": lambda: idx.search_filtered_each(q, K, **{mode: lists})[0]}
            if not a.parent_only:
                words = pack_row_masks(n, **{mode: lists})
                arms = {"ids": lambda: idx.search_filtered_ids(q, K, **{mode: lists})[0], "pack_here": arms["pack"],
                        "prepacked": lambda: idx.search_filtered_each(q, K, masks=words)[0]}
            times, calls, res = _alternate(arms, a.regions, a.window)
            case = {arm: dict(_row(t), calls_per_region=calls[arm]) for arm, t in times.items()}
            case["list_bytes"] = int(sum(len(x) for x in lists) * 8 + (b + 1) * 8)
            case["word_bytes"] = int(b * ((n + 31) // 32) * 4)
            if not a.parent_only:
                case["route"] = hex(idx.get_option("last_route"))
                case["same_ids"] = bool(np.array_equal(res["ids"], res["pack_here"]) and np.array_equal(res["ids"], res["prepacked"]))
                case["ids_vs_pack_here"] = _compare(case["ids"], case["pack_here"])
                case["ids_vs_prepacked"] = _compare(case["ids"], case["prepacked"])
                if parent:
                    case["pack_parent"] = parent["rows_by_case"][f"{kind}_B{b}"]["pack"]
                    case["ids_vs_pack_parent"] = _compare(case["ids"], case["pack_parent"])
            out["rows_by_case"][f"{kind}_B{b}"] = case
            print(f"# {kind} B={b}: {json.dumps(case)}", file=sys.stderr, flush=True)
    if not a.parent_only:
        cases = out["rows_by_case"].values()
        out["ids_beats_pack_every_row"] = all(c["ids_vs_pack_here"]["wins"] and c.get("ids_vs_pack_parent", {"wins": True})["wins"] for c in cases)
        out["ids_loses_to_prepacked_rows"] = [name for name, c in out["rows_by_case"].items() if c["ids_vs_prepacked"]["loses"]]
        out["ids_beats_prepacked_rows"] = [name for name, c in out["rows_by_case"].items() if c["ids_vs_prepacked"]["wins"]]

    if multi is not None:
        reh = {"label": f"REHEARSAL: {SHARDS} logical shards on ONE GPU — the layout of a multi-device index, no speed-up to be had here",
               "shard_rows": multi.shard_rows()}
        for kind in ("exclude_pool_200", "allow_own_1pct"):
            for b in BATCHES:
                q = np.ascontiguousarray(q_all[:b])
                mode, lists = _lists(n, kind, b)
                one = idx.search_filtered_ids(q, K, **{mode: lists})
                got = multi.search_filtered_ids(q, K, **{mode: lists})
                same = bool(np.array_equal(one[0], got[0]) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(one[1:], got[1:])))
                times, calls, _ = _alternate({"multi_ids": lambda: multi.search_filtered_ids(q, K, **{mode: lists})[0],
                                              "one_ids": lambda: idx.search_filtered_ids(q, K, **{mode: lists})[0]}, a.regions, a.window)
                reh[f"{kind}_B{b}"] = dict({arm: dict(_row(t), calls_per_region=calls[arm]) for arm, t in times.items()}, same_bits_as_one_index=same)
                print(f"# (d) {kind} B={b}: {json.dumps(reh[f'{kind}_B{b}'])}", file=sys.stderr, flush=True)
        reh["same_bits_every_row"] = all(v["same_bits_as_one_index"] for v in reh.values() if isinstance(v, dict))
        out["d_multi_device_rehearsal"] = reh
        multi.close()

    idx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
