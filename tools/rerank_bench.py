"""Cross-encoder reranker: one call = 100 (query, passage) pairs in mini-batches of 32, three arms on the same token ids.

    python tools/rerank_bench.py [--only base_bf16,...] [--regions 7] [--out profiles/rerank.json]

Models: seed-initialised XLMRobertaForSequenceClassification (one label) at the bge-reranker-base shape (768 hidden, 12 heads, 12 layers,
3072 intermediate) and the -large / -v2-m3 shape (1024, 16, 24, 4096), bf16 and f16, with a small synthetic vocabulary (the real 250 K-row
table only costs memory: the embedding kernel gathers rows).  No bge-reranker weights exist offline; timings do not depend on the values.
Workload: a 12-token query and a passage that fills 512 tokens (and, second row, 128 tokens), 100 pairs, token ids drawn from a seed — the
tokenizer is outside every arm.
Arms: (a) `transformers` — the model's own forward in the same dtype, mini-batches of 32 padded ids + attention mask, logits read back: what a
user runs today; (b) `fused` — CrossEncoderReranker.score_token_ids with rerank_cls_tail = False (the whole stack + cmr_encoder_cls_head);
(c) `fused_cls_tail` — the same with rerank_cls_tail = True (the last layer for the CLS rows alone).
Timing: a host clock around one call, which ends in the read-back of its logits (a device synchronise); every arm is warmed up twice, then the
arms alternate region by region; a region is --calls calls back to back (a window of 0.1 - 0.3 s: a single 15 ms call measures the scheduler as
much as the work); a row is the median of --regions regions with min and max, in ms per call.  Judging (the project's rule): a row wins when its
median is below the other's by more than the two rows' min-to-max spreads added.  The two new kernels' own durations at b = 100, l = 512 are
event-timed: the mean over 20 back-to-back launches per region, median of the regions.  Prints ONE JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"base": dict(hidden=768, heads=12, layers=12, inter=3072), "large": dict(hidden=1024, heads=16, layers=24, inter=4096)}
VOCAB, PAIRS, BATCH = 1000, 100, 32


def _row(times_s):
    t = np.asarray(times_s) * 1e3
    return {"ms_per_call": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def passes(new, old) -> bool:
    """new median below the old one by more than the two rows' min-to-max spreads added"""
    return new["ms_per_call"] < old["ms_per_call"] - ((new["max"] - new["min"]) + (old["max"] - old["min"]))


def _compare(new, old):
    return {"ratio": new["ms_per_call"] / old["ms_per_call"], "wins": passes(new, old), "loses": passes(old, new)}


def _model(torch, shape, dtype):
    from transformers import XLMRobertaConfig, XLMRobertaForSequenceClassification
    s = SHAPES[shape]
    torch.manual_seed(0)
    cfg = XLMRobertaConfig(vocab_size=VOCAB, hidden_size=s["hidden"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"],
                           intermediate_size=s["inter"], max_position_embeddings=514, type_vocab_size=1, pad_token_id=1, bos_token_id=0,
                           eos_token_id=2, layer_norm_eps=1e-5, num_labels=1)
    return XLMRobertaForSequenceClassification(cfg).eval().to("cuda", dtype=dtype)


def _ids(tokens):
    """<s> query(12) </s></s> passage </s> filling `tokens` positions"""
    rng = np.random.default_rng(tokens)
    rows = []
    for _ in range(PAIRS):
        q, p = rng.integers(5, VOCAB, size=12), rng.integers(5, VOCAB, size=tokens - 16)
        rows.append([0] + q.tolist() + [2, 2] + p.tolist() + [2])
    return rows


def _transformers_arm(torch, model, ids):
    def call():
        parts = []
        with torch.no_grad():
            for i in range(0, len(ids), BATCH):
                arr = torch.from_numpy(np.asarray(ids[i:i + BATCH], np.int64)).pin_memory().to("cuda", non_blocking=True)
                parts.append(model(input_ids=arr, attention_mask=torch.ones_like(arr)).logits[:, 0].float())
        return torch.cat(parts).cpu().numpy()
    return call


def _kernel_times(torch, fz, head, regions):
    """(attention_cls, cls_head) at b = 100, l = 512: us per launch."""
    b, l, d = PAIRS, 512, fz.hidden
    qkv = torch.randn((b * l, 3 * d), device="cuda").to(fz.dtype)
    lens = torch.full((b,), l, dtype=torch.int32, device="cuda")
    x = torch.randn((b, d), device="cuda").to(fz.dtype)
    out = {}
    for name, fn in (("attention_cls", lambda: fz.attention_cls(qkv, lens, b, l)), ("cls_head", lambda: fz.cls_head(x, d, head, b)),
                     ("attention_all_rows", lambda: fz.attention(qkv, lens, b, l))):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(regions):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / 20)
        out[name] = {"us_per_launch": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
    return out


def _case(torch, shape, dtype, regions, calls):
    from comorag_amd.rerank import CrossEncoderReranker
    from comorag_amd.utils.config_utils import BaseConfig
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    model = _model(torch, shape, tdt)
    rr = {tail: CrossEncoderReranker(BaseConfig(rerank_model_dtype=dtype, rerank_batch_size=BATCH, rerank_max_seq_len=512, rerank_cls_tail=tail),
                                     model=model, tokenizer=object()) for tail in (False, True)}
    assert all(r.reranker_path.startswith("hip-fused-layers") for r in rr.values())
    res = {}
    for tokens in (512, 128):
        ids = _ids(tokens)
        arms = {"transformers": _transformers_arm(torch, model, ids), "fused": lambda: rr[False].score_token_ids(ids),
                "fused_cls_tail": lambda: rr[True].score_token_ids(ids)}
        outs = {}
        for name, call in arms.items():
            call()
            outs[name] = call()
        times = {name: [] for name in arms}
        for _ in range(regions):
            for name, call in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    call()
                times[name].append((time.perf_counter() - t0) / calls)
        rows = {name: _row(t) for name, t in times.items()}
        rows["cls_tail_vs_transformers"] = _compare(rows["fused_cls_tail"], rows["transformers"])
        rows["cls_tail_vs_fused"] = _compare(rows["fused_cls_tail"], rows["fused"])
        rows["fused_vs_transformers"] = _compare(rows["fused"], rows["transformers"])
        rows["max_abs_logit_difference"] = {"fused_vs_transformers": float(np.abs(outs["fused"] - outs["transformers"]).max()),
                                            "cls_tail_vs_fused": float(np.abs(outs["fused_cls_tail"] - outs["fused"]).max()),
                                            "logit_std": float(outs["transformers"].std())}
        res[f"tokens_{tokens}"] = rows
    res["kernels_b100_l512"] = _kernel_times(torch, rr[True]._fused, rr[True]._head, regions)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="base_bf16,base_f16,large_bf16,large_f16")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=6, help="calls per timed region")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.regions < 5:
        raise SystemExit("--regions must be at least 5")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rerank_bench.py needs an MI355X: a timing taken anywhere else says nothing")
    out = {"pairs_per_call": PAIRS, "mini_batch": BATCH, "regions": a.regions, "calls_per_region": a.calls, "unit": "ms per call of 100 pairs (median, min, max)",
           "rule": "a row wins when its median is below the other's by more than the two min-to-max spreads added", "cases": {}}
    for name in a.only.split(","):
        shape, dtype = name.split("_")
        out["cases"][name] = _case(torch, shape, dtype, a.regions, max(1, a.calls))
        print(f"# {name}: {json.dumps(out['cases'][name])}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    at512 = [c["tokens_512"]["cls_tail_vs_fused"]["wins"] for c in out["cases"].values()]
    out["rerank_cls_tail_default"] = bool(at512) and all(at512)          # True only if the tail beats the whole stack by the rule in every 512-token row
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
