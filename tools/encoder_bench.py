"""Corpus-embed rate and per-stage breakdown of the encoder path (tools/bench_extras.encode_breakdown) for the BERT-base bf16 and
BERT-large fp16 shapes, fused layer stack against the transformers forward.  `python -m tools.encoder_bench [--quick]`.
`python -m tools.encoder_bench --fp32 [--out FILE]`: the fp32 rows (`embedding_model_dtype = "auto"`, `embedding_fused_fp32` on and off in the
same run) — one short query, the corpus forward at 512 tokens, and the fp32 attention kernel next to PyTorch's SDPA on the same tensors.
`python -m tools.encoder_bench --head32 [--out FILE]`: the 32-wide-head rows (the bge-small shape, `embedding_fused_head32` on and off in the same
run, bf16 / f16 / fp32) — one short query, the corpus forward at 512 tokens, and the HD = 32 attention kernel next to SDPA and next to the HD = 64
kernel on the same tensors zero-padded to 64 columns per head."""
import json
import sys

import torch

from tools import bench_extras as bx


def query_latency(kind, dtype, dev, reps=40):
    """Median wall time of batch_encode(one short query) — what get_query_embeddings (ComoRAG.py:909-935) waits for."""
    import time
    import numpy as np
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.utils.config_utils import BaseConfig
    from tools.synthetic import random_bert, synthetic_wordpiece_tokenizer
    tok, words = synthetic_wordpiece_tokenizer()
    out = {}
    for fused in (True, False):
        cfg = BaseConfig(embedding_model_name=f"bge-{kind}-random-init", embedding_model_dtype=dtype, device=dev.index or 0, embedding_fused_encoder=fused)
        em = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=random_bert(kind, vocab_size=len(tok)), tokenizer=tok)
        q = " ".join(words[:12])
        for _ in range(5):
            em.batch_encode(q)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); em.batch_encode(q); ts.append(time.perf_counter() - t0)
        out[em.encoder_path] = float(np.median(ts) * 1e6)
        em.close()
    return out


def _timed(fn, reps, warm=3):
    """Seconds per call: `reps` calls back to back between two device synchronisations (launches overlap the device work)."""
    import time
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def fp32_report(dev, reps=60):
    """The fp32 opt-in (`embedding_fused_fp32`) against the transformers fp32 forward of the same model, same process, same run."""
    import time
    import numpy as np
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.utils.config_utils import BaseConfig
    from tools.synthetic import random_bert, synthetic_chunks, synthetic_wordpiece_tokenizer
    tok, words = synthetic_wordpiece_tokenizer()
    q = " ".join(words[:12])
    out = {"what": "fp32 encoder (embedding_model_dtype auto = fp32 weights): fused fp32 stack (embedding_fused_fp32 = True) vs the transformers fp32 forward",
           "single_query_encode_us": {}, "corpus": {}, "attention": {}}
    for kind in ("base", "large"):
        row = {}
        for flag in (True, False):
            cfg = BaseConfig(embedding_model_name=f"bge-{kind}-random-init", embedding_model_dtype="auto", device=dev.index or 0,
                             embedding_fused_fp32=flag, embedding_query_cache=0)                       # (every call a forward)
            em = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=random_bert(kind, vocab_size=len(tok)), tokenizer=tok)
            assert em.encoder_path.startswith("hip-fused-layers" if flag else "transformers (")
            for _ in range(8):
                em.batch_encode(q)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter(); em.batch_encode(q); ts.append(time.perf_counter() - t0)
            row["fused_fp32" if flag else "transformers_fp32"] = {"median": float(np.median(ts) * 1e6), "min": float(np.min(ts) * 1e6)}
            if kind == "base":
                # corpus forward: 32 chunks of 512 tokens, inputs on the device; and batch_encode of 128 chunks end to end
                chunks = synthetic_chunks(words, 128, tokens_per_chunk=560)
                host = em._tokenize(chunks[:32], 512)
                inp = {k: v.to(dev) for k, v in host.items()}
                lens = host["attention_mask"].numpy().sum(1).astype(np.int32)
                with torch.no_grad():
                    if flag:
                        dt = _timed(lambda: em._fused(inp["input_ids"], lens, token_type_ids=inp.get("token_type_ids"), pool=True), 5, warm=2)
                    else:
                        dt = _timed(lambda: em.embedding_model(**inp).last_hidden_state, 5, warm=2)
                em.batch_encode(chunks[:64])
                torch.cuda.synchronize()
                t0 = time.perf_counter(); em.batch_encode(chunks); torch.cuda.synchronize(); dt_e2e = time.perf_counter() - t0
                out["corpus"]["fused_fp32" if flag else "transformers_fp32"] = {
                    "forward_only_chunks_per_s": 32 / dt, "end_to_end_chunks_per_s": len(chunks) / dt_e2e, "tokens_per_chunk": int(inp["input_ids"].shape[1])}
                if flag:
                    # the attention kernel alone at 32 x 512 x 12 heads, every sequence full, next to SDPA on the same tensors (its inputs
                    # already split and head-major, which the transformers forward pays for with three more copies)
                    fz, b, l = em._fused, 32, 512
                    qkv = torch.randn((b * l, 3 * fz.hidden), device=dev) * 1.5
                    lens_dev = torch.full((b,), l, dtype=torch.int32, device=dev)
                    x = qkv.view(b, l, 3, fz.n_heads, 64)
                    qh, kh, vh = (x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))
                    dt_k = _timed(lambda: fz.attention(qkv, lens_dev, b, l), 20)
                    dt_s = _timed(lambda: torch.nn.functional.scaled_dot_product_attention(qh, kh, vh), 20)
                    flops = 4.0 * b * l * l * fz.hidden
                    out["attention"] = {"shape": "32 x 512 tokens x 12 heads x 64, fp32, full sequences", "timing": "20 launches back to back between two synchronisations",
                                        "hip_fp32_kernel_us": dt_k * 1e6, "torch_sdpa_fp32_us": dt_s * 1e6, "hip_TFLOPs": flops / dt_k / 1e12,
                                        "frac_of_155TF_f32_mfma": flops / dt_k / 1e12 / 155.0}
            em.close()
        out["single_query_encode_us"][kind] = row
    return out


def _regions(fn, regions=7, reps=10, warm=3):
    """Microseconds per call over `regions` timed regions of `reps` calls each (a synchronisation on either side of a region):
    median, min and max of the regions."""
    import numpy as np
    _timed(fn, warm, warm=0)
    ts = [_timed(fn, reps, warm=0) * 1e6 for _ in range(regions)]
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "regions": regions, "calls_per_region": reps}


def head32_report(dev):
    """The 32-wide-head opt-in (`embedding_fused_head32`) on the bge-small shape (384 hidden, 12 layers, 12 heads, 1536 intermediate) against
    the transformers forward of the same model, same process, same run, in bf16, f16 and fp32 (the latter with `embedding_fused_fp32` too)."""
    import types
    import numpy as np
    from comorag_amd import _lib as L
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    from comorag_amd.utils.config_utils import BaseConfig
    from tools.synthetic import random_bert, synthetic_chunks, synthetic_wordpiece_tokenizer
    tok, words = synthetic_wordpiece_tokenizer()
    q = " ".join(words[:12])
    chunks = synthetic_chunks(words, 32, tokens_per_chunk=560)
    out = {"what": "32-wide heads (bge-small shape: 384 hidden, 12 layers, 12 heads, 1536 intermediate, random init): fused stack (embedding_fused_head32 = True) "
                   "vs the transformers forward of the same model; microseconds per call, median / min / max over timed regions",
           "single_query_encode_us": {}, "corpus_forward_32x512_us": {}, "attention_32x512x12_us": {}}
    for name, dtype in (("bf16", "bf16"), ("f16", "fp16"), ("fp32", "auto")):
        qrow, crow = {}, {}
        for flag in (True, False):
            cfg = BaseConfig(embedding_model_name="bge-small-random-init", embedding_model_dtype=dtype, device=dev.index or 0,
                             embedding_fused_head32=flag, embedding_fused_fp32=flag and dtype == "auto", embedding_query_cache=0)      # (every call a forward)
            em = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=random_bert("small", vocab_size=len(tok)), tokenizer=tok)
            assert em.encoder_path.startswith("hip-fused-layers" if flag else "transformers ("), em.encoder_path
            key = "fused" if flag else "transformers"
            for _ in range(8):
                em.batch_encode(q)
            qrow[key] = _regions(lambda: em.batch_encode(q), regions=7, reps=20, warm=2)
            host = em._tokenize(chunks, 512)
            inp = {k: v.to(dev) for k, v in host.items()}
            lens = host["attention_mask"].numpy().sum(1).astype(np.int32)
            with torch.no_grad():
                if flag:
                    crow[key] = _regions(lambda: em._fused(inp["input_ids"], lens, token_type_ids=inp.get("token_type_ids"), pool=True), regions=5, reps=3, warm=2)
                else:
                    crow[key] = _regions(lambda: em.embedding_model(**inp).last_hidden_state, regions=5, reps=3, warm=2)
            crow["tokens_per_chunk"] = int(inp["input_ids"].shape[1])
            if flag:
                # the attention call alone at 32 x 512 x 12 heads, every sequence full: the HD = 32 kernel; SDPA on the same tensors already split
                # and head-major; the HD = 64 kernel on the same tensors with every head zero-padded to 64 columns (a TIMING baseline: its scale
                # is 1/8, its values differ)
                fz, b, l, nh = em._fused, 32, 512, 12
                qkv = (torch.randn((b * l, 3 * fz.hidden), device=dev) * 1.5).to(fz.dtype)
                lens_dev = torch.full((b,), l, dtype=torch.int32, device=dev)
                x = qkv.view(b, l, 3, nh, 32)
                qh, kh, vh = (x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))
                padded = torch.zeros((b * l, 3, nh, 64), dtype=fz.dtype, device=dev)
                padded[..., :32] = qkv.view(b * l, 3, nh, 32)
                padded = padded.view(b * l, 3 * nh * 64)
                wide = types.SimpleNamespace(hidden=nh * 64, n_heads=nh, cmr_dtype=fz.cmr_dtype)
                out["attention_32x512x12_us"][name] = {
                    "hip_head32": _regions(lambda: fz.attention(qkv, lens_dev, b, l), regions=7, reps=20),
                    "torch_sdpa_head_major": _regions(lambda: torch.nn.functional.scaled_dot_product_attention(qh, kh, vh), regions=7, reps=20),
                    "hip_head64_zero_padded": _regions(lambda: FusedBertLayers.attention(wide, padded, lens_dev, b, l), regions=7, reps=20)}
            em.close()
        out["single_query_encode_us"][name] = qrow
        out["corpus_forward_32x512_us"][name] = crow
    # acceptance, row by row: fused median below the transformers median by more than the two rows' own min-to-max spread; native attention not slower than padded
    acc = {}
    for table in ("single_query_encode_us", "corpus_forward_32x512_us"):
        for name, row in out[table].items():
            f, t = row["fused"], row["transformers"]
            acc[f"{table}/{name}"] = bool(t["median"] - f["median"] > (f["max"] - f["min"]) + (t["max"] - t["min"]))
    for name, row in out["attention_32x512x12_us"].items():
        acc[f"attention_native_not_slower_than_padded/{name}"] = bool(row["hip_head32"]["median"] <= row["hip_head64_zero_padded"]["median"])
    out["acceptance"] = acc
    return out


def main():
    if "--head32" in sys.argv or "--fp32" in sys.argv:
        rep = head32_report(torch.device("cuda", 0)) if "--head32" in sys.argv else fp32_report(torch.device("cuda", 0))
        text = json.dumps(rep, indent=1)
        print(text)
        if "--out" in sys.argv:
            with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
                f.write(text + "\n")
        return
    quick = "--quick" in sys.argv
    dev = torch.device("cuda", 0)
    cases = [("base", "bf16", 256, 0), ("base", "bf16", 256, 4), ("large", "fp16", 256, 0)]
    if quick:
        cases = cases[:1]
    for kind, dtype, n, procs in cases:
        res, em = bx.encode_breakdown(torch, dev, kind, dtype, n_chunks=n, batch=32, tok_processes=procs)
        em.close()
        keep = ("model", "value", "forward_only_chunks_per_s", "transformers_forward_only_chunks_per_s", "tokenizer_only_chunks_per_s",
                "forward_TFLOPs", "frac", "attention_us_per_layer", "attention_TFLOPs", "add_layernorm_us", "add_layernorm_GBps",
                "pool_l2norm_us_per_batch", "end_to_end_over_forward_only", "tokenizer_processes", "encoder_path", "host_ms")
        line = {k: res[k] for k in keep if k in res}
        if procs == 0:
            line["single_query_encode_us"] = query_latency(kind, dtype, dev)
        print(json.dumps(line))


if __name__ == "__main__":
    main()
