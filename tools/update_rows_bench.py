"""In-place row update (cmr_index_update_rows) on one MI355X: 1 M x 768 bf16 rows.

    python tools/update_rows_bench.py [--rows 1000000] [--regions 7] [--out profiles/update_rows.json]

Rows: one update pattern each — 1 row, 25 rows (one memory-pool cycle), a random 1 %, a contiguous 10 % block, all rows.  Arms:
(a) `update`   DenseIndex.update_rows(ids, rows) on a full index, new rows in a contiguous host array.  An update leaves the index's
               shape as it was, so one index serves every region; region 0 warms the call up (plan scratch, staging buffer, the pinned
               buffer of small calls) and is not counted.
(b) `rebuild`  what a user does without the feature for the same end state: a new DenseIndex and append() of ALL rows, final contents,
               from one contiguous host matrix prepared before the clock starts — calls that exist on the parent commit, so the arm is
               timed in the same run.  The clock covers create + append + close of the old index.
(c) `append`   all-rows case only: append() of the same rows into an index created (with capacity) outside the clock — what the scatter
               mapping and the check pass cost against the append's own kernel on the same commit.  No bar on the ratio.
Both arms end with the same index: the ids and score bits of one 8-query search are compared per row.
Up to 128 KiB of rows go through the pinned, device-mapped buffer; a larger call stages its rows in chunks of 256 MiB and, when it has
more than one chunk, uploads them twice (every row is checked before the first store).
Timing: a host clock around one call; a row is the median over --regions regions (>= 5) with min and max; the arms alternate region by
region.  Judging (the project's rule, tools/rerank_bench.py): a row wins when its median is below the other's by more than the two
min-to-max spreads added.  Every row is reported, also those that do not win.  Prints ONE JSON object."""
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


def _patterns(n):
    rng = np.random.default_rng(17)
    return {"one_row": np.array([n // 2], dtype=np.int64),
            "pool_cycle_25_rows": np.sort(rng.choice(n, 25, replace=False)).astype(np.int64),
            "random_1pct": np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64),
            "block_10pct": np.arange(n // 2 - n // 20, n // 2 + n // 20, dtype=np.int64),
            "all_rows": np.arange(n, dtype=np.int64)}


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
        raise SystemExit("update_rows_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex
    n = a.rows
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)

    def unit_rows():
        return torch.cat([torch.nn.functional.normalize(torch.randn((min(100_000, n - r0), DIM), generator=gen, device=dev), dim=1).cpu()
                          for r0 in range(0, n, 100_000)]).numpy()

    x_old, x_new = unit_rows(), unit_rows()
    q = torch.nn.functional.normalize(torch.randn((8, DIM), generator=gen, device=dev), dim=1).cpu().numpy()
    q[:4] = x_new[:4] + 0.05 * q[:4]      # the first new rows of every pattern are found: the comparison of the arms sees updated rows

    out = {"tool": "tools/update_rows_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "regions": a.regions,
           "unit": "ms per call (median, min, max)", "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "device": torch.cuda.get_device_name(dev), "rows_by_case": {}}
    for name, ids in _patterns(n).items():
        m = len(ids)
        new = x_new[:m]
        final = x_old.copy()
        final[ids] = new
        idx = DenseIndex(DIM, "bf16", capacity_hint=n)
        idx.append(x_old)
        old = DenseIndex(DIM, "bf16", capacity_hint=n)
        old.append(x_old)
        t_update, t_rebuild, t_append, same, chunks = [], [], [], True, 0
        for region in range(a.regions + 1):      # region 0 warms both arms up and is not counted
            t0 = time.perf_counter()
            done = idx.update_rows(ids, new)
            dt = time.perf_counter() - t0
            assert done == m
            chunks = idx.get_option("update_chunks_last")
            if region:
                t_update.append(dt)
            t0 = time.perf_counter()
            fresh = DenseIndex(DIM, "bf16", capacity_hint=n)
            fresh.append(final)
            old.close()
            dt = time.perf_counter() - t0
            if region:
                t_rebuild.append(dt)
            else:
                got, want = idx.search(q, 20, with_minmax=False), fresh.search(q, 20, with_minmax=False)
                same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and np.isin(got[0], ids).any())
            old = fresh
            if name == "all_rows":
                empty = DenseIndex(DIM, "bf16", capacity_hint=n)
                empty.append(x_old[:1])      # the kernels and the staging buffer of the timed append exist
                t0 = time.perf_counter()
                empty.append(new)
                dt = time.perf_counter() - t0
                if region:
                    t_append.append(dt)
                empty.close()
        idx.close(); old.close()
        case = {"updated_rows": int(m), "host_bytes": int(new.nbytes), "chunks": int(chunks), "same_bits_both_arms": same,
                "update": _row(t_update), "rebuild": _row(t_rebuild), "rebuild_host_bytes": int(final.nbytes)}
        case["update_vs_rebuild"] = {"ratio": case["update"]["ms_per_call"] / case["rebuild"]["ms_per_call"], "wins": passes(case["update"], case["rebuild"]),
                                     "loses": passes(case["rebuild"], case["update"])}
        if t_append:
            case["append_same_rows"] = _row(t_append)
            case["update_vs_append_ratio"] = case["update"]["ms_per_call"] / case["append_same_rows"]["ms_per_call"]
        out["rows_by_case"][name] = case
        print(f"# {name}: {json.dumps(case)}", file=sys.stderr, flush=True)
        del final
    out["update_wins_every_row"] = all(c["update_vs_rebuild"]["wins"] for c in out["rows_by_case"].values())
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
