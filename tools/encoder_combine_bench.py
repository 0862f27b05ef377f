"""Sixteen threads of one-question encodes, with and without the encode combiner (config `embedding_combine`).

    python tools/encoder_combine_bench.py [--only base_bf16,large_fp16] [--parent-tree DIR] [--out profiles/encoder_combine.json]
    python tools/encoder_combine_bench.py --baseline [--tree DIR]        # the parent arm: no combine field is touched

A region is THREADS x CALLS distinct 12-word questions (16 x 50), one `batch_encode(question)` per call from a pool of threads, as ComoRAG's
question threads issue them; its time is the wall time from the barrier that releases the threads to the last thread's return.  Models are
seed-initialised BGE-base (bf16) and BGE-large (fp16) shapes with a synthetic WordPiece vocabulary, `embedding_fused_small_m = True`, query
cache off.  Within one process the arms — combine = 0, combine = 16, combine = 16 with a gather window of WINDOW_US — are three model
objects over the same weights and alternate region by region; each is reported as the median of REGIONS regions with min and max, in
microseconds per question.  The lone caller is the same with one thread.  --parent-tree DIR first runs this file with --baseline in a
process of its own whose package is DIR's (the parent commit's tree with its own built library): the "parent" arm.
The stage row (information only): the four linear stages of a layer at M = 1280 token rows on the many-row kernels against F.linear
(+ F.gelu) at the same M, the model's layers taken in turn (one weight set each), HIP-event time per layer.
Judging (the project's rule): new median below the old one by more than the two rows' min-to-max spreads added.  Prints ONE JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS, CALLS, REGIONS, LONE_CALLS = 16, 50, 5, 200
WINDOW_US = 100
ARMS = (("combine_0", 0, 0), ("combine_16", 16, 0), (f"combine_16_wait_{WINDOW_US}us", 16, WINDOW_US))
MODELS = {"base_bf16": ("base", "bf16"), "large_fp16": ("large", "fp16")}


def _region(call, threads, calls):
    """threads x calls calls `call(thread, j)` -> seconds"""
    bar = threading.Barrier(threads + 1)
    err = []

    def work(t):
        bar.wait()
        try:
            for j in range(calls):
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


def _row(times_s, calls):
    t = np.array(times_s) / calls * 1e6
    return {"us_per_question": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["us_per_question"] < old["us_per_question"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _measure(ems, questions, threads, calls):
    """ems: name -> model; alternating regions; region 0 warms every arm up (graph captures included)"""
    times = {name: [] for name in ems}
    width = {}
    for r in range(REGIONS + 1):
        for name, em in ems.items():
            before = em.combine_stats() if hasattr(em, "combine_stats") else None
            dt = _region(lambda t, j: em.batch_encode(questions[t * calls + j]), threads, calls)
            if r:
                times[name].append(dt)
                if before is not None:
                    now = em.combine_stats()
                    if now["batches"] > before["batches"]:
                        width.setdefault(name, []).append((now["queries"] - before["queries"]) / (now["batches"] - before["batches"]))
    out = {name: _row(times[name], threads * calls) for name in ems}
    for name, w in width.items():
        out[name]["questions_per_forward"] = float(np.median(w))
    return out


def _stage_row(torch, em):
    """The four linear stages of a layer at M = 1280 rows: many-row kernels against F.linear (+ F.gelu); us per layer."""
    import torch.nn.functional as F
    fz = em._fused
    m = 1280
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((m, fz.hidden), generator=g, device="cuda").to(fz.dtype)
    inter = fz.layers[0][6].shape[0]
    h = torch.randn((m, inter), generator=g, device="cuda").to(fz.dtype)

    def rows(lyr):
        wqkv, bqkv, wo, _, _, _, w1, b1, w2 = lyr[:9]
        fz.linear_rows(x, wqkv, bqkv, False); fz.linear_rows_partials(x, wo); fz.linear_rows(x, w1, b1, True); fz.linear_rows_partials(h, w2)

    def lib(lyr):
        wqkv, bqkv, wo, _, _, _, w1, b1, w2 = lyr[:9]
        F.linear(x, wqkv, bqkv); F.linear(x, wo); F.gelu(F.linear(x, w1, b1)); F.linear(h, w2)
    out = {}
    for name, fn in (("rows_kernels", rows), ("f_linear", lib)):
        ts = []
        for rep in range(REGIONS + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for lyr in fz.layers:
                fn(lyr)
            b.record()
            b.synchronize()
            if rep:
                ts.append(a.elapsed_time(b) * 1e3 / len(fz.layers))
        out[name] = {"us_per_layer": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
    out["rows_over_f_linear"] = out["rows_kernels"]["us_per_layer"] / out["f_linear"]["us_per_layer"]
    out["m"] = m
    return out


def _model_case(torch, kind, dtype, baseline):
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.utils.config_utils import BaseConfig
    from tools.synthetic import random_bert, synthetic_chunks, synthetic_wordpiece_tokenizer
    tok, words = synthetic_wordpiece_tokenizer()
    model = random_bert(kind, vocab_size=len(tok))
    chunks = synthetic_chunks(words, THREADS * CALLS, tokens_per_chunk=12, seed=99)
    questions = [" ".join(c.split()[:12]) for c in chunks]
    arms = ARMS[:1] if baseline else ARMS
    ems = {}
    for name, width, wait in arms:
        kw = {} if baseline else dict(embedding_combine=width, embedding_combine_wait_us=wait)
        cfg = BaseConfig(embedding_model_name=f"bge-{kind}-random-init", embedding_batch_size=8, embedding_model_dtype=dtype, embedding_fused_small_m=True,
                         embedding_query_cache=0, **kw)
        ems["parent" if baseline else name] = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=model, tokenizer=tok)
    first = next(iter(ems.values()))
    ids = first._ragged([first.embedding_config.encode_params["passage_instruction"] + q for q in questions[:50]], 512)
    res = {"model": f"bge-{kind} ({dtype}, seed-initialised)", "small_m_rows": int(first.small_m_rows),
           "prompt_tokens_median": float(np.median([len(x) for x in ids]))}
    res["threads_16"] = _measure(ems, questions, THREADS, CALLS)
    res["lone_caller"] = _measure(ems, questions, 1, LONE_CALLS)
    if not baseline:
        res["linear_stages_m1280"] = _stage_row(torch, first)
    for em in ems.values():
        em.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="base_bf16,large_fp16")
    ap.add_argument("--baseline", action="store_true", help="one arm, no combine field is touched (runs on a tree without the option)")
    ap.add_argument("--tree", default=None, help="import comorag_amd and tools from this tree instead of this file's")
    ap.add_argument("--parent-tree", default=None, help="first run --baseline --tree DIR in a process of its own: the parent arm")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    out = {"tool": "tools/encoder_combine_bench.py", "threads": THREADS, "calls_per_thread": CALLS, "regions": REGIONS, "lone_calls": LONE_CALLS}
    parent = None
    if a.parent_tree:           # before this process opens the device: a fresh child, its own package and library
        env = dict(os.environ)
        env.pop("COMORAG_HIP_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline", "--tree", os.path.abspath(a.parent_tree), "--only", a.only],
                           stdout=subprocess.PIPE, env=env, cwd=os.path.abspath(a.parent_tree), check=True, timeout=900)
        parent = json.loads(p.stdout.decode().strip().splitlines()[-1])
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(HERE))
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    for name in a.only.split(","):
        kind, dtype = MODELS[name]
        res = _model_case(torch, kind, dtype, a.baseline)
        if parent is not None:
            for part in ("threads_16", "lone_caller"):
                res[part] = {"parent": parent[name][part]["parent"], **res[part]}
            old = res["threads_16"]["parent"]
            res["verdict"] = {
                "threads_16_combine_16_over_parent": res["threads_16"]["combine_16"]["us_per_question"] / old["us_per_question"],
                "threads_16_combine_16_faster_by_the_rule": passes(res["threads_16"]["combine_16"], old),
                "threads_16_combine_16_wait_faster_by_the_rule": passes(res["threads_16"][ARMS[2][0]], old),
                "lone_combine_16_slower_by_the_rule": passes(res["lone_caller"]["parent"], res["lone_caller"]["combine_16"]),
                "lone_combine_0_slower_by_the_rule": passes(res["lone_caller"]["parent"], res["lone_caller"]["combine_0"]),
            }
        out[name] = res
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
