"""Corpus-embed rate and per-stage breakdown of the encoder path (tools/bench_extras.encode_breakdown) for the BERT-base bf16 and
BERT-large fp16 shapes, fused layer stack against the transformers forward.  `python -m tools.encoder_bench [--quick]`.
`python -m tools.encoder_bench --fp32 [--out FILE]`: the fp32 rows (`embedding_model_dtype = "auto"`, `embedding_fused_fp32` on and off in the
same run) — one short query, the corpus forward at 512 tokens, and the fp32 attention kernel next to PyTorch's SDPA on the same tensors.
`python -m tools.encoder_bench --head32 [--out FILE]`: the 32-wide-head rows (the bge-small shape, `embedding_fused_head32` on and off in the same
run, bf16 / f16 / fp32) — one short query, the corpus forward at 512 tokens, and the HD = 32 attention kernel next to SDPA and next to the HD = 64
kernel on the same tensors zero-padded to 64 columns per head.
`python -m tools.encoder_bench --small-m [--out profiles/encoder_small_m.json]`: the short-row route (`embedding_fused_small_m`) — every small-M stage
next to what it replaces for 16 .. 128 token rows at the base / large / small layer shapes, and the one-query call with the flag on and off; both arms
in one process, alternating region by region."""
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


def _alternating(arms, regions=7, reps=20, graph=False):
    """{name: callable} -> {name: median / min / max microseconds per call}: `regions` rounds, each timing every arm once (`reps` calls
    between two synchronisations), so the arms see the same clocks and neighbours.  graph = True: an arm's `reps` calls are captured
    as ONE hipGraph and a region is one replay timed with device events — the device time of the stage, free of the interpreter."""
    import time
    import numpy as np
    runs = {}
    for name, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(reps):
                    fn()
            g.replay()
            runs[name] = g
        else:
            runs[name] = fn
    torch.cuda.synchronize()
    ts = {name: [] for name in arms}
    for _ in range(regions):
        for name, run in runs.items():
            if graph:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); run.replay(); e1.record(); e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3 / reps)
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    run()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e6 / reps)
    return {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "regions": regions, "calls_per_region": reps} for name, v in ts.items()}


def _passes(new, old):
    """The rule of DESIGN 4.10: the new median below the old one by more than the two rows' min-to-max spreads added together."""
    return bool(old["median"] - new["median"] > (new["max"] - new["min"]) + (old["max"] - old["min"]))


SMALL_M_SWEEP = (16, 32, 48, 64, 80, 96, 128)
SMALL_M_SHAPES = {"base": ("bf16", 768, 3072), "large": ("fp16", 1024, 4096), "small": ("bf16", 384, 1536)}
SMALL_M_LAYERS = {"base": 12, "large": 24, "small": 12}


def small_m_report(dev):
    """The short-row route (`embedding_fused_small_m`): device time of each small-M stage against the PyTorch stage it replaces (hipGraph replays of
    20 calls, device events), per layer shape and token-row count; then batch_encode(one 12-word query) with the flag on and off."""
    import types
    import torch.nn.functional as F
    from comorag_amd import _lib as L
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    from comorag_amd.utils.config_utils import BaseConfig
    from tools.synthetic import random_bert, synthetic_wordpiece_tokenizer
    out = {"what": "short-row route of the fused encoder stack: small-M HIP stages vs the PyTorch / hipBLASLt stages they replace; microseconds per call, "
                   "median / min / max of 7 regions x 20 calls, both arms in one process, alternating",
           "rule": "pass = new median below the old median by more than the two rows' (max - min) added together",
           "stages_us": {}, "per_layer_sum_us": {}, "single_query_encode_us": {}}
    for kind, (dname, hidden, inter) in SMALL_M_SHAPES.items():
        tdt = torch.bfloat16 if dname == "bf16" else torch.float16
        fz = types.SimpleNamespace(dtype=tdt, eps=1e-12, cmr_dtype=L.CMR_BF16 if dname == "bf16" else L.CMR_F16)
        for name in ("linear_small", "linear_small_partials", "add_layernorm_partials", "add_layernorm"):
            setattr(fz, name, getattr(FusedBertLayers, name).__get__(fz))
        rnd = lambda *sh: torch.randn(sh, device=dev)
        # one weight set per LAYER of the model, taken in turn by consecutive calls: a forward streams every layer's own weights once, so a stage
        # timed on ONE weight tensor over and over would be timed out of the caches instead
        nl = SMALL_M_LAYERS[kind]
        wqkv, wo, w1, w2 = ([(rnd(n, k) / k ** 0.5).to(tdt) for _ in range(nl)] for n, k in ((3 * hidden, hidden), (hidden, hidden), (inter, hidden), (hidden, inter)))
        bqkv, b1, bh, gamma, beta = rnd(3 * hidden).to(tdt), rnd(inter).to(tdt), rnd(hidden).to(tdt), rnd(hidden).to(tdt), rnd(hidden).to(tdt)
        out["stages_us"][kind], out["per_layer_sum_us"][kind] = {}, {}

        def turn(fn):
            state = [0]
            def call():
                i = state[0]
                state[0] = (i + 1) % nl
                return fn(i)
            return call

        for m in SMALL_M_SWEEP:
            x, h = rnd(m, hidden).to(tdt), rnd(m, inter).to(tdt)
            stages = {
                "qkv": {"small_m": lambda i: fz.linear_small(x, wqkv[i], bqkv), "torch": lambda i: F.linear(x, wqkv[i], bqkv)},
                "ffn_up_gelu": {"small_m": lambda i: fz.linear_small(x, w1[i], b1, True), "torch": lambda i: F.gelu(F.linear(x, w1[i], b1))},
                "o_proj_ln": {"small_m": lambda i: fz.add_layernorm_partials(fz.linear_small_partials(x, wo[i]), bh, x, gamma, beta),
                              "torch": lambda i: fz.add_layernorm(F.linear(x, wo[i]), bh, x, gamma, beta)},
                "ffn_down_ln": {"small_m": lambda i: fz.add_layernorm_partials(fz.linear_small_partials(h, w2[i]), bh, x, gamma, beta),
                                "torch": lambda i: fz.add_layernorm(F.linear(h, w2[i]), bh, x, gamma, beta)}}
            row = {name: _alternating({arm: turn(fn) for arm, fn in arms.items()}, graph=True) for name, arms in stages.items()}
            for name in row:
                row[name]["pass"] = _passes(row[name]["small_m"], row[name]["torch"])
            # a layer's four stages together, one graph per arm (the sum the crossover is read from)
            layer = _alternating({arm: turn(lambda i, arm=arm: [stages[name][arm](i) for name in stages]) for arm in ("small_m", "torch")}, graph=True)
            layer["pass"] = _passes(layer["small_m"], layer["torch"])
            out["stages_us"][kind][str(m)] = row
            out["per_layer_sum_us"][kind][str(m)] = layer
            print(kind, m, {k: (round(v["small_m"]["median"], 2), round(v["torch"]["median"], 2), v["pass"]) for k, v in {**row, "layer": layer}.items()}, flush=True)
    ok = [m for m in SMALL_M_SWEEP if all(out["per_layer_sum_us"][kind][str(m)]["pass"] for kind in ("base", "large"))]
    upto = 0
    for m in SMALL_M_SWEEP:                                 # the largest M up to which every row of the sweep passes at both gating shapes
        if m not in ok:
            break
        upto = m
    out["crossover_rows"] = upto
    tok, words = synthetic_wordpiece_tokenizer()
    q = " ".join(words[:12])
    for kind, dtype, head32 in (("base", "bf16", False), ("large", "fp16", False), ("small", "bf16", True), ("small", "fp16", True)):
        ems = {}
        for flag in (True, False):
            cfg = BaseConfig(embedding_model_name=f"bge-{kind}-random-init", embedding_model_dtype=dtype, device=dev.index or 0, embedding_fused_head32=head32,
                             embedding_fused_small_m=flag, embedding_query_cache=0)      # (every call a forward)
            em = ems["small_m" if flag else "flag_off"] = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=random_bert(kind, vocab_size=len(tok)), tokenizer=tok)
            assert em.encoder_path == "hip-fused-layers" and (em.small_m_rows > 0) == flag
            for _ in range(8):
                em.batch_encode(q)
        row = _alternating({name: (lambda em=em: em.batch_encode(q)) for name, em in ems.items()})
        row["pass"] = _passes(row["small_m"], row["flag_off"])
        row["token_rows"] = int(sum(k[0] * k[1] for k in list(ems["small_m"]._fused._graphs)[:1]))
        out["single_query_encode_us"][f"{kind}_{dtype}"] = row
        print(kind, dtype, row, flush=True)
        for em in ems.values():
            em.close()
    out["gating_rows_pass"] = bool(out["single_query_encode_us"]["base_bf16"]["pass"] and out["single_query_encode_us"]["large_fp16"]["pass"])
    return out


def main():
    if "--small-m" in sys.argv:
        rep = small_m_report(torch.device("cuda", 0))
        text = json.dumps(rep, indent=1)
        print(text)
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/encoder_small_m.json"
        with open(out, "w") as f:
            f.write(text + "\n")
        return
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
