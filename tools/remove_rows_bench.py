"""Row removal by in-place compaction (cmr_index_remove_ids) on one MI355X: 1 M x 768 bf16 rows.

    python tools/remove_rows_bench.py [--rows 1000000] [--regions 7] [--stage-mib 64,16,1024] [--out profiles/remove_rows.json]

Rows: one removal pattern each — one row at the front, a random 1 %, a random 50 %, a 10 % block at the front, a tail run of 10 %.  Arms:
(a) `remove`   DenseIndex.remove_ids(ids) on a full index, once per staging size of --stage-mib (option remove_stage_panels; the first
               size is the one judged, 64 MiB is the default of the library).  A removal changes the index, so every timed call gets a
               freshly built index (built from a device tensor, outside the clock).  That index is built with one extra row in front,
               and a warm-up removal of that row — with an id list padded to the timed list's length — runs before the clock: it
               compacts the whole index once, so the scratch and the staging buffer of the timed call are allocated already and the
               clock holds no hipMalloc.
(b) `rebuild`  what a user does without the feature: a new DenseIndex and append() of the surviving rows from the host matrix — calls
               that exist on the parent commit, so the arm is timed in the same run.  The surviving rows are gathered into one
               contiguous host array BEFORE the clock starts (a favour to this arm); the clock covers create + append + close of the old
               index.
Both arms end with the same index: the ids of one 8-query search are compared per row.
Model: a compaction reads the panels from the first removed row's on once and moves the rows it keeps there three more times (stage
write, stage read, destination write): bytes = affected panels + 3 x kept rows behind the first affected panel; 4 x the affected bytes
is its upper bound, reached when nearly everything is kept.  A tail run moves nothing.  `gbps` is model bytes / median call time —
the call also holds a device synchronise, the upload of the ids, the keep words, the prefix sum and one 16-byte read-back, so it is
not purely a rate.
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
PANEL_BYTES = 32 * DIM * 2


def _row(times_s):
    t = np.asarray(times_s) * 1e3
    return {"ms_per_call": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["ms_per_call"] < old["ms_per_call"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _patterns(n):
    rng = np.random.default_rng(16)
    return {"front_one_row": np.array([0], dtype=np.int64),
            "random_1pct": np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64),
            "random_50pct": np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64),
            "front_block_10pct": np.arange(0, n // 10, dtype=np.int64),
            "tail_run_10pct": np.arange(n - n // 10, n, dtype=np.int64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--stage-mib", default="64,16,1024", help="staging sizes in MiB; the first one is judged against the rebuild arm")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("remove_rows_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    from comorag_amd.index import DenseIndex
    n = a.rows
    stages = [int(x) for x in a.stage_mib.split(",")]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    chunks = [torch.nn.functional.normalize(torch.randn((min(100_000, n - r0), DIM), generator=gen, device=dev), dim=1).contiguous()
              for r0 in range(0, n, 100_000)]
    x_host = torch.cat([c.cpu() for c in chunks]).numpy()
    q = torch.nn.functional.normalize(torch.randn((8, DIM), generator=gen, device=dev), dim=1).cpu().numpy()

    def full_index(stage_mib, n_ids):
        idx = DenseIndex(DIM, "bf16", capacity_hint=n + 1)
        idx.append_dev(chunks[0][:1].contiguous())      # the row the warm-up removal takes out again
        for c in chunks:
            idx.append_dev(c)
        torch.cuda.synchronize(dev)
        idx.set_option("remove_stage_panels", max(2, (stage_mib << 20) // PANEL_BYTES))
        warm = np.full(n_ids + 1, -1, dtype=np.int64)
        warm[0] = 0
        assert idx.remove_ids(warm) == 1 and len(idx) == n and idx.get_option("remove_chunks_last") >= 1
        return idx

    out = {"tool": "tools/remove_rows_bench.py", "rows": n, "dim": DIM, "dtype": "bf16", "regions": a.regions, "stage_mib": stages,
           "unit": "ms per call (median, min, max)", "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added",
           "model": "bytes of the panels from the first removed row's on + 3 x the bytes of the rows kept there; a tail run moves nothing",
           "device": torch.cuda.get_device_name(dev), "rows_by_case": {}}
    for name, ids in _patterns(n).items():
        keep = np.ones(n, dtype=bool)
        keep[ids] = False
        survivors = np.ascontiguousarray(x_host[keep])
        tail_only = int(ids.min()) == n - len(ids)
        p0 = int(ids.min()) // 32
        affected_bytes = ((n + 31) // 32 - p0) * PANEL_BYTES
        model_bytes = 0 if tail_only else affected_bytes + 3 * (n - p0 * 32 - len(ids)) * DIM * 2
        t_remove = {s: [] for s in stages}
        t_rebuild, chunks_run, want, same = [], {}, None, True
        old = full_index(stages[0], 0)
        for region in range(a.regions + 1):      # region 0 warms both arms up and is not counted
            for s in stages:
                idx = full_index(s, len(ids))
                t0 = time.perf_counter()
                removed = idx.remove_ids(ids)
                dt = time.perf_counter() - t0
                assert removed == len(ids) and len(idx) == n - len(ids)
                chunks_run[s] = idx.get_option("remove_chunks_last")
                if region:
                    t_remove[s].append(dt)
                else:
                    got = idx.search(q, 20, with_minmax=False)[0]
                    want = got if want is None else want
                    same = same and bool(np.array_equal(got, want))
                idx.close()
            t0 = time.perf_counter()
            new = DenseIndex(DIM, "bf16", capacity_hint=len(survivors))
            new.append(survivors)
            old.close()
            dt = time.perf_counter() - t0
            if region:
                t_rebuild.append(dt)
            else:
                same = same and bool(np.array_equal(new.search(q, 20, with_minmax=False)[0], want))
            old = new
        old.close()
        case = {"removed_rows": int(len(ids)), "first_removed_row": int(ids.min()), "model_bytes": int(model_bytes), "model_bytes_upper_bound": 0 if tail_only else int(4 * affected_bytes), "same_ids_every_arm": same,
                "rebuild": _row(t_rebuild), "rebuild_host_bytes": int(survivors.nbytes)}
        for s in stages:
            r = _row(t_remove[s])
            r["chunks"] = int(chunks_run[s])
            r["gbps"] = model_bytes / (r["ms_per_call"] * 1e-3) / 1e9
            case[f"remove_stage_{s}mib"] = r
        first = case[f"remove_stage_{stages[0]}mib"]
        case["remove_vs_rebuild"] = {"ratio": first["ms_per_call"] / case["rebuild"]["ms_per_call"], "wins": passes(first, case["rebuild"]),
                                     "loses": passes(case["rebuild"], first)}
        out["rows_by_case"][name] = case
        print(f"# {name}: {json.dumps(case)}", file=sys.stderr, flush=True)
        del survivors
    out["remove_wins_every_row"] = all(c["remove_vs_rebuild"]["wins"] for c in out["rows_by_case"].values())
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
