"""Step time of the pipelined search over option sets of the pre-filter's sampling, one index per row count, the option
sets applied in turn on it: three 40-step regions each, the counters of the last batch and its comparison with the synchronous search.
    python tools/prefilter_sample_sweep.py ROWS BATCH "name=value,name=value;name=value;..." [label] >> sweep.jsonl
An empty option set ("") is the defaults; every set starts from the defaults."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from comorag_amd.index import DenseIndex

rows, B = int(sys.argv[1]), int(sys.argv[2])
sets = sys.argv[3].split(";")
label = sys.argv[4] if len(sys.argv) > 4 else "this commit"
dim, k, steps, regions = 768, 20, 40, 3
DEFAULTS = {"prefilter": -1, "prefilter_sample": -1, "prefilter_sample_panels": 0, "prefilter_sample_run": 0, "prefilter_sample_wave_cap": 0,
            "prefilter_sample_level0": 0, "pipe_reserve_cus": -1, "sample_maxmul": 0}
dev = torch.device("cuda", 0); g = torch.Generator(device=dev); g.manual_seed(7)
idx = DenseIndex(dim, "bf16", capacity_hint=rows)
for b in range(0, rows, 250_000):
    x = torch.randn((min(250_000, rows - b), dim), generator=g, device=dev); idx.append_dev((x / x.norm(dim=1, keepdim=True)).contiguous())
qs = []
for _ in range(4):
    q = torch.randn((B, dim), generator=g, device=dev); qs.append((q / q.norm(dim=1, keepdim=True)).contiguous())
outs = [(torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev)) for _ in range(4)]
torch.cuda.synchronize()


def get(name):
    try:
        return idx.get_option(name)
    except Exception:
        return None


for opts in sets:
    for n, v in DEFAULTS.items():
        try:
            idx.set_option(n, v)
        except Exception:
            pass                      # (a build without the option: its defaults are all it has)
    for nv in filter(None, opts.split(",")):
        n, v = nv.split("=")
        idx.set_option(n, int(v))
    for i in range(8): h = idx.search_pipelined(qs[i & 3], k, outs[i & 3][0], outs[i & 3][1])
    idx.sync(h); torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for i in range(steps): h = idx.search_pipelined(qs[i & 3], k, outs[i & 3][0], outs[i & 3][1])
        idx.sync(h); torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / steps * 1e3, 4))
    last = (steps - 1) & 3
    rec = {"build": label, "rows": rows, "batch": B, "opts": opts or "defaults", "ms_per_step": ms, "active": get("prefilter_active"),
           "sample_active": get("prefilter_sample_active"), "sample_pairs": get("prefilter_sample_pairs"), "sample_overflow": get("prefilter_sample_overflow"),
           "pairs": get("prefilter_pairs"), "pair_overflow": get("prefilter_pair_overflow"), "wave_overflow": get("prefilter_wave_overflow"),
           "candidates": get("prefilter_candidates")}
    si, ss = idx.search_dev(qs[last], k); torch.cuda.synchronize()
    rec["equals_sync"] = bool(torch.equal(si, outs[last][0]) and torch.equal(ss, outs[last][1]))
    print(json.dumps(rec), flush=True)
idx.close()
