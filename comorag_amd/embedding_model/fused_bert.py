"""The encoder stack behind `self.embedding_model(**inputs)` (embedding_model/BGEEmbedding.py:119) for 16-bit BERT encoders — and,
opt-in (`fp32=True`, config `embedding_fused_fp32`), for fp32 ones: the same stages with fp32 tensors, fp32 GEMMs and fp32 HIP kernels.
Heads are 64 wide (bge-base / -large, bge-m3) or, opt-in (`head32=True`, config `embedding_fused_head32`), 32 wide: the 384-hidden / 12-head
small tier (bge-small, e5-small, gte-small, MiniLM), whose attention runs the HD = 32 instantiation of the same kernels; both opt-ins combine.

transformers' BertLayer is ~20 kernels and as many Python module calls per layer: three projection GEMMs, SDPA with an additive
mask, the output GEMM, bias / residual adds, LayerNorm, the FFN GEMMs and GELU.  Here a layer is

    qkv  = x @ [Wq | Wk | Wv]^T + b          one hipBLASLt GEMM instead of three (PyTorch-ROCm, as north_star prescribes)
    ctx  = cmr_encoder_attention(qkv, lens)   HIP: masked softmax(QK^T/sqrt(head width))V straight off the packed projection, no head transposes
    x    = cmr_encoder_add_layernorm(ctx @ Wo^T, bo, x)       HIP: dense bias + residual + LayerNorm in one pass
    x    = cmr_encoder_add_layernorm(gelu(x @ W1^T + b1) @ W2^T, b2, x)      (bias in the up-projection GEMM's epilogue; GELU: the erf-form kernel)

seven host calls per layer — and ONE per forward once a mini-batch shape has been captured as a hipGraph (`graphs`) — so the
thread that launches the forward leaves the interpreter lock to the tokenizer threads.
The weights are the loaded model's own tensors (query / key / value concatenated once); the embedding gathers, their sum and
LayerNorm are one HIP kernel (cmr_encoder_embed_layernorm).  Results equal the transformers forward up to 16-bit rounding (the fused LayerNorm rounds once instead of
three times): tests/test_encoder_fused_gpu.py compares both with the fp32 oracle.

Used when `why_not(model)` is None: BERT / RoBERTa / XLM-R architecture (bge-base / -large, bge-m3), absolute positions, exact GELU,
64-wide heads (32-wide with `head32=True`), bf16 / fp16 weights (fp32 with `fp32=True`); any other model keeps the transformers forward (`HipBGEEmbeddingModel.encoder_path` says which one runs).

`forward_cls` is the same stack ending in a one-logit classification head instead of the pooling tail (cross-encoder rerankers, rerank.py):
cmr_encoder_cls_head over the CLS rows, and optionally the last layer for those rows alone (cmr_encoder_attention_cls).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .. import _lib as L


# Graph captures are exclusive in the process — against each other AND against every other thread's forward launches:
#   * `torch.cuda.graph.__enter__` synchronises the whole DEVICE, which HIP refuses while another stream of it is capturing (two encoder
#     replicas — bge._EncodeReplica: one FusedBertLayers each, own stream and worker thread — capturing their first shapes at the same
#     moment: hipErrorStreamCaptureUnsupported);
#   * a forward launched EAGERLY by another thread meanwhile may be hipBLASLt's first call for its shape, and that call touches the
#     legacy stream: "operation would make the legacy stream depend on a capturing blocking stream" (hipblaslt.cpp:172), the GEMM fails,
#     the process dies in Tensile's initialisation (seen in bench.py --single-process: four replicas behind an index's blocking streams).
# Forwards hold the gate shared while they ENQUEUE (host side only: the GPU work of other streams runs on during a capture).
import threading as _threading


class _Gate:
    def __init__(self):
        self._cv, self._readers, self._writer = _threading.Condition(), 0, False

    class _Hold:
        def __init__(self, gate, exclusive): self.g, self.x = gate, exclusive
        def __enter__(self):
            g = self.g
            with g._cv:
                if self.x:
                    while g._writer or g._readers: g._cv.wait()
                    g._writer = True
                else:
                    while g._writer: g._cv.wait()
                    g._readers += 1
        def __exit__(self, *exc):
            g = self.g
            with g._cv:
                if self.x: g._writer = False
                else: g._readers -= 1
                g._cv.notify_all()

    def shared(self): return _Gate._Hold(self, False)
    def exclusive(self): return _Gate._Hold(self, True)


_GATE = _Gate()


# BERT and its RoBERTa-family twins (same layer; position ids start at padding_idx + 1, one token type): XLM-R is bge-m3, the one
# BGE model whose 8192 positions are safe with the reference's default embedding_max_seq_len = 2048 (config_utils.py:140)
ENCODER_TYPES = ("bert", "roberta", "xlm-roberta")


def position_offset(model) -> int:
    """First position id of a sequence: 0 for BERT, padding_idx + 1 for the RoBERTa family
    (transformers' RobertaEmbeddings.create_position_ids_from_input_ids)."""
    if getattr(model.config, "model_type", "") == "bert":
        return 0
    pad = getattr(model.embeddings, "padding_idx", None)
    if pad is None:
        pad = getattr(model.config, "pad_token_id", 1)
    return int(pad) + 1


def why_not(model, fp32: bool = False, head32: bool = False) -> Optional[str]:
    """None if the fused layer stack can run this model, else the reason it cannot.  fp32 = True also accepts torch.float32 weights
    (the fp32 kernels, opt-in); head32 = True also accepts 32-wide heads (the HD = 32 attention kernels, opt-in); every other reason
    applies unchanged."""
    import torch
    cfg = getattr(model, "config", None)
    if cfg is None or getattr(cfg, "model_type", "") not in ENCODER_TYPES:
        return "not a BERT / RoBERTa / XLM-R encoder"
    if not (hasattr(model, "embeddings") and hasattr(model, "encoder") and hasattr(model.encoder, "layer")
            and all(hasattr(model.embeddings, n) for n in ("word_embeddings", "position_embeddings", "token_type_embeddings", "LayerNorm"))):
        return "unexpected module layout"
    if getattr(cfg, "position_embedding_type", None) not in (None, "absolute"):
        return "relative position embeddings"
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        return f"activation {cfg.hidden_act!r}"
    if getattr(cfg, "is_decoder", False) or getattr(cfg, "add_cross_attention", False) or getattr(cfg, "chunk_size_feed_forward", 0):
        return "decoder / cross-attention / chunked feed-forward configuration"
    if cfg.hidden_size % cfg.num_attention_heads or cfg.hidden_size // cfg.num_attention_heads not in ((64, 32) if head32 else (64,)):
        return "head width is not 64"
    if cfg.hidden_size % 4 or cfg.hidden_size > 2048 or cfg.intermediate_size % 4:
        return "hidden size not supported by the LayerNorm kernel"
    dt = next(model.parameters()).dtype
    if fp32 and dt == torch.float32:
        return None
    if dt not in (torch.bfloat16, torch.float16):
        return f"{dt} weights (the fused layers are 16-bit)"
    return None


def lens_of_mask(mask: np.ndarray) -> Optional[np.ndarray]:
    """Token counts of a right-padded attention mask [b, l] (ones then zeros in every row), or None if it is anything else."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.shape[1] == 0 or not np.all((m == 0) | (m == 1)):
        return None
    if m.shape[1] > 1 and np.any(m[:, 1:] > m[:, :-1]):
        return None
    lens = m.sum(axis=1).astype(np.int32)
    return lens if np.all(lens > 0) else None


def gelu_epilogue_available(device, dtype) -> bool:
    """Does this PyTorch-ROCm build run `torch._addmm_activation(bias, x, w.T, use_gelu=True)` as ONE hipBLASLt GEMM whose epilogue
    adds the bias and applies GELU in its tanh form?  Checked on the device, two ways: (i) the call agrees with tanh-GELU of the
    same linear map to within a 16-bit rounding step and NOT better with the erf form; (ii) torch's profiler sees ONE device kernel
    for the call — PyTorch's fallback (`addmm` + a separate tanh-GELU kernel) computes the same values in two launches: there the
    approximation would be paid for with no launch saved, and the exact path stays."""
    import torch
    import torch.nn.functional as F
    if not hasattr(torch, "_addmm_activation"):
        return False
    try:
        g = torch.Generator(device="cpu").manual_seed(5)
        x = (torch.randn((256, 256), generator=g) * 1.5).to(device=device, dtype=dtype)
        w = (torch.randn((512, 256), generator=g) / 16.0).to(device=device, dtype=dtype)
        b = torch.randn((512,), generator=g).to(device=device, dtype=dtype)
        got = torch._addmm_activation(b, x, w.t(), use_gelu=True).float()
        lin = F.linear(x.float(), w.float(), b.float())
        want_tanh, want_erf = F.gelu(lin, approximate="tanh"), F.gelu(lin)
        step = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
        tol = step * (1.0 + want_tanh.abs())
        ok = bool(((got - want_tanh).abs() <= tol).all())
        if not (ok and float((got - want_tanh).abs().mean()) <= float((got - want_erf).abs().mean())):
            return False
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize(device)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch._addmm_activation(b, x, w.t(), use_gelu=True)
            torch.cuda.synchronize(device)
        kernels = [e for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "DeviceType.CUDA" in str(e.device_type)
                   and "memcpy" not in e.key.lower() and "memset" not in e.key.lower()]
        return sum(e.count for e in kernels) == 1
    except Exception:
        return False


# The short-row route (small_m = True): token rows b*l up to which it is taken.  SMALL_M_MAX_ROWS is the kernels' limit; SMALL_M_ROWS the
# default, the measured crossover of tools/encoder_bench.py --small-m (profiles/encoder_small_m.json).
# Measured (profiles/encoder_small_m.json; us per layer, small-M / hipBLASLt stages, medians, one weight set per layer taken in turn):
#   BGE-base bf16   M = 16: 34.5 / 40.5   80: 41.0 / 48.9   96: 41.5 / 46.6   128: 45.4 / 48.2 (inside the spreads: fails the rule)
#   BGE-large fp16  M = 16: 40.5 / 48.8   80: 49.0 / 61.0   96: 49.9 / 61.6   128: 55.4 / 63.8
# The whole route passes the rule at both shapes up to 96 rows, so every stage is routed — also the O-projection + LayerNorm stage, which
# alone loses at the base shape (12.1 against 11.1 us at 80 rows).
SMALL_M_MAX_ROWS = 128
SMALL_M_ROWS = 96
# The many-row route (`forward_ragged(..., rows_route=True)`, taken only when the caller asks: bge's combining queue): the same kernels
# over up to ROWS_MAX token rows — 16 one-question forwards of at most 128 rows each (cmr_encoder_linear_rows*, CMR_ENCODER_ROWS_MAX).
ROWS_MAX = L.CMR_ENCODER_ROWS_MAX
_SPLITS = {}      # (n, k, cmr dtype) -> K slices of the partials form (cmr_encoder_linear_small_split)


class FusedBertLayers:
    def __init__(self, model, graphs: int = 0, gelu: str = "exact", fp32: bool = False, head32: bool = False, small_m: bool = False,
                 small_m_rows: Optional[int] = None):
        """gelu = "exact" (default): FFN-up GEMM + bias in hipBLASLt, then PyTorch's erf-form GELU kernel — the function the model
        was trained with and the reference runs (BGEEmbedding.py:119-120, `hidden_act = "gelu"`).
        gelu = "epilogue" (opt-in, `embedding_gelu`): projection, bias and GELU are ONE hipBLASLt GEMM (`torch._addmm_activation`) —
        one read + write of the [b*l, 4*hidden] activation less per layer (~7 % of a BERT-base forward), but hipBLASLt's epilogue is
        the TANH form: a different function, |tanh form - erf form| <= 4.8e-4 per activation (largest near |x| ~ 2-3, where the value
        itself is ~1e-2: for small outputs the difference exceeds the 16-bit rounding step — bf16 ulp at 0.009 is 6e-5, fp16's 8e-6).
        Measured inside north_star's 1e-3 cosine bar on seed-initialised BERT shapes and on heavy-tailed pre-activations
        (tests/test_encoder_fused_gpu.py), not on real BGE weights (absent from the image) — hence not the default.  Falls back to
        "exact" when the build does not fuse it into a single launch (`gelu_path` says which one runs).
        fp32 = True admits an fp32 model: fp32 tensors through every stage (cmr_dtype = CMR_F32: exact f32-input MFMA attention,
        LayerNorm written unrounded), F.linear in fp32 as the transformers forward calls it.  gelu = "epilogue" then runs the exact
        kernel too: the tanh epilogue was validated against 16-bit rounding steps only.
        head32 = True admits 32-wide heads (`head_dim` = 32: the attention call names the width, nothing else changes).
        small_m = True (opt-in, `embedding_fused_small_m`; 16-bit models, fp32 ones ignore it) arms the short-row route: a mini-batch of
        b*l <= small_m_rows token rows (default SMALL_M_ROWS = 96, at most 128 — one short query) runs its four linear layers on the library's
        weight-streaming small-M kernels instead of hipBLASLt (`_layers_small_m`); larger mini-batches keep the route above, bit for bit.
        `small_m_rows` is the armed limit (0: not armed).  The route computes the exact erf GELU: where gelu = "epilogue" is in effect
        (`gelu_path` says so) it is NOT armed, so that every mini-batch size gets the same function."""
        import torch
        reason = why_not(model, fp32=fp32, head32=head32)
        if reason is not None:
            raise ValueError("FusedBertLayers: " + reason)
        if gelu not in ("epilogue", "exact"):
            raise ValueError("FusedBertLayers: gelu must be 'epilogue' or 'exact'")
        self.model = model
        cfg = model.config
        self.hidden, self.n_heads, self.eps = int(cfg.hidden_size), int(cfg.num_attention_heads), float(cfg.layer_norm_eps)
        self.head_dim = self.hidden // self.n_heads
        self.dtype = next(model.parameters()).dtype
        self.cmr_dtype = {torch.bfloat16: L.CMR_BF16, torch.float16: L.CMR_F16, torch.float32: L.CMR_F32}[self.dtype]
        if self.dtype == torch.float32:
            gelu = "exact"
        self.device = next(model.parameters()).device
        emb = model.embeddings
        self.emb = tuple(t.detach().contiguous() for t in (emb.word_embeddings.weight, emb.position_embeddings.weight,
                                                           emb.token_type_embeddings.weight, emb.LayerNorm.weight, emb.LayerNorm.bias))
        self.pos_offset = position_offset(model)
        self.gelu_path = "hipblaslt-epilogue-tanh" if (gelu == "epilogue" and gelu_epilogue_available(self.device, self.dtype)) else "exact-erf-kernel"
        import threading
        self.fold_pool = True                        # the encoder tail (mean-pool + L2-norm) rides the last layer's LayerNorm kernel
        # (not with the tanh epilogue: the route's GELU is the erf form, and one model must not compute two functions depending on the batch size)
        armed = (bool(small_m) and self.dtype != torch.float32 and self.hidden % 32 == 0 and int(cfg.intermediate_size) % 32 == 0
                 and self.gelu_path == "exact-erf-kernel")
        rows = SMALL_M_ROWS if small_m_rows is None else int(small_m_rows)
        self.small_m_rows = max(0, min(rows, SMALL_M_MAX_ROWS)) if armed else 0
        self.graphs = int(graphs)                    # mini-batch shapes kept as captured hipGraphs (0: every forward is launched eagerly)
        self._graphs, self._seen, self._glock = {}, {}, threading.Lock()
        self.layers = []
        with torch.no_grad():
            for lyr in model.encoder.layer:
                att, so = lyr.attention.self, lyr.attention.output
                wqkv = torch.cat([att.query.weight, att.key.weight, att.value.weight], dim=0).contiguous()
                bqkv = torch.cat([att.query.bias, att.key.bias, att.value.bias], dim=0).contiguous()
                self.layers.append(tuple(t.detach().contiguous() for t in (
                    wqkv, bqkv, so.dense.weight, so.dense.bias, so.LayerNorm.weight, so.LayerNorm.bias,
                    lyr.intermediate.dense.weight, lyr.intermediate.dense.bias, lyr.output.dense.weight, lyr.output.dense.bias,
                    lyr.output.LayerNorm.weight, lyr.output.LayerNorm.bias)))

    # ------------------------------------------------------------------ the two HIP stages (also called by the tests)
    def attention(self, qkv, lens_dev, b: int, l: int, stream: Optional[int] = None):
        import torch
        out = torch.empty((b * l, self.hidden), dtype=qkv.dtype, device=qkv.device)
        if stream is None:
            stream = torch.cuda.current_stream(qkv.device).cuda_stream
        L.check(L.lib().cmr_encoder_attention(qkv.device.index or 0, C.c_void_p(qkv.data_ptr()), self.cmr_dtype, C.c_void_p(lens_dev.data_ptr()),
                                              b, l, self.n_heads, self.hidden // self.n_heads, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def embed(self, input_ids, token_type_ids=None, stream: Optional[int] = None):
        """BertEmbeddings of a [b, l] id tensor → [b*l, hidden]."""
        import torch
        b, l = input_ids.shape
        word, pos, typ, gamma, beta = self.emb
        ids = input_ids.contiguous()
        tt = token_type_ids.contiguous() if token_type_ids is not None else None
        out = torch.empty((b * l, self.hidden), dtype=word.dtype, device=ids.device)
        if stream is None:
            stream = torch.cuda.current_stream(ids.device).cuda_stream
        L.check(L.lib().cmr_encoder_embed_layernorm(ids.device.index or 0, C.c_void_p(ids.data_ptr()), C.c_void_p(tt.data_ptr() if tt is not None else 0),
                                                    C.c_void_p(word.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(typ.data_ptr()),
                                                    C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()), self.eps, b * l, l, self.hidden,
                                                    word.shape[0], pos.shape[0], typ.shape[0], int(getattr(self, "pos_offset", 0)), self.cmr_dtype,
                                                    C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def embed_ragged(self, ids32, offsets, b: int, l: int, stream: Optional[int] = None):
        """BertEmbeddings straight from ragged token ids (int32 CUDA tensors: the b sequences back to back + their b + 1 starts)
        → [b*l, hidden]; rows behind a sequence's end are padding."""
        import torch
        word, pos, typ, gamma, beta = self.emb
        out = torch.empty((b * l, self.hidden), dtype=word.dtype, device=ids32.device)
        if stream is None:
            stream = torch.cuda.current_stream(ids32.device).cuda_stream
        L.check(L.lib().cmr_encoder_embed_layernorm_ragged(ids32.device.index or 0, C.c_void_p(ids32.data_ptr()), C.c_void_p(offsets.data_ptr()),
                                                           C.c_void_p(word.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(typ.data_ptr()),
                                                           C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()), self.eps, b, l, self.hidden,
                                                           word.shape[0], pos.shape[0], int(getattr(self, "pos_offset", 0)), self.cmr_dtype,
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def add_layernorm(self, y, bias, residual, gamma, beta, stream: Optional[int] = None):
        import torch
        out = torch.empty_like(y)
        if stream is None:
            stream = torch.cuda.current_stream(y.device).cuda_stream
        L.check(L.lib().cmr_encoder_add_layernorm(y.device.index or 0, C.c_void_p(y.data_ptr()), C.c_void_p(bias.data_ptr() if bias is not None else 0),
                                                  C.c_void_p(residual.data_ptr() if residual is not None else 0), C.c_void_p(gamma.data_ptr()),
                                                  C.c_void_p(beta.data_ptr()), self.eps, y.shape[0], y.shape[1], self.cmr_dtype,
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def add_layernorm_pool(self, y, bias, residual, gamma, beta, lens_dev, b: int, l: int, normalize: bool = True, stream: Optional[int] = None):
        """The last layer's add_layernorm with mean_pooling + F.normalize folded in (cmr_encoder_add_layernorm_pool): [b, hidden]
        fp32; the [b, l, hidden] state is never written."""
        import torch
        out = torch.empty((b, self.hidden), dtype=torch.float32, device=y.device)
        partial = torch.empty((b * (l // 16), self.hidden), dtype=torch.float32, device=y.device)
        if stream is None:
            stream = torch.cuda.current_stream(y.device).cuda_stream
        L.check(L.lib().cmr_encoder_add_layernorm_pool(y.device.index or 0, C.c_void_p(y.data_ptr()), C.c_void_p(bias.data_ptr() if bias is not None else 0),
                                                       C.c_void_p(residual.data_ptr() if residual is not None else 0), C.c_void_p(gamma.data_ptr()),
                                                       C.c_void_p(beta.data_ptr()), self.eps, b, l, self.hidden, self.cmr_dtype, C.c_void_p(lens_dev.data_ptr()),
                                                       1 if normalize else 0, C.c_void_p(partial.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def linear_small(self, x, w, bias=None, gelu: bool = False, stream: Optional[int] = None):
        """F.linear(x, w, bias) — or F.gelu of it — for 1 .. 128 token rows in one launch (cmr_encoder_linear_small)."""
        import torch
        m, k = x.shape
        n = w.shape[0]
        assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == k, "linear_small reads row-major [m, k] and [n, k] tensors"
        out = torch.empty((m, n), dtype=x.dtype, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.lib().cmr_encoder_linear_small(x.device.index or 0, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                                                 C.c_void_p(bias.data_ptr() if bias is not None else 0), m, n, k, self.cmr_dtype, 1 if gelu else 0,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def linear_small_partials(self, x, w, stream: Optional[int] = None):
        """x @ w.T for 1 .. 128 token rows as fp32 slabs [n_split, m, n] (cmr_encoder_linear_small_partials): K is split over the grid,
        the slabs are summed by `add_layernorm_partials`.  The slab tensor is allocated here, so a graph capture owns it."""
        import torch
        m, k = x.shape
        n = w.shape[0]
        assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == k, "linear_small_partials reads row-major [m, k] and [n, k] tensors"
        n_split = _SPLITS.get((n, k, self.cmr_dtype))
        if n_split is None:                                         # a function of (n, k, dtype): asked once
            ns, nbytes = C.c_int32(0), C.c_int64(0)
            L.check(L.lib().cmr_encoder_linear_small_split(m, n, k, self.cmr_dtype, C.byref(ns), C.byref(nbytes)))
            n_split = _SPLITS[(n, k, self.cmr_dtype)] = int(ns.value)
        part = torch.empty((n_split, m, n), dtype=torch.float32, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.lib().cmr_encoder_linear_small_partials(x.device.index or 0, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), m, n, k, self.cmr_dtype,
                                                          C.c_void_p(part.data_ptr()), C.c_void_p(stream)))
        return part

    def linear_rows(self, x, w, bias=None, gelu: bool = False, stream: Optional[int] = None):
        """`linear_small` for 1 .. 2048 token rows (cmr_encoder_linear_rows): every row gets the bits `linear_small` gives it."""
        import torch
        m, k = x.shape
        n = w.shape[0]
        assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == k, "linear_rows reads row-major [m, k] and [n, k] tensors"
        out = torch.empty((m, n), dtype=x.dtype, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.lib().cmr_encoder_linear_rows(x.device.index or 0, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                                                C.c_void_p(bias.data_ptr() if bias is not None else 0), m, n, k, self.cmr_dtype, 1 if gelu else 0,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def linear_rows_partials(self, x, w, stream: Optional[int] = None):
        """`linear_small_partials` for 1 .. 2048 token rows (cmr_encoder_linear_rows_partials): fp32 slabs [n_split, m, n], n_split that of
        cmr_encoder_linear_small_split for (n, k, dtype) — it does not depend on m, so it is asked with one row."""
        import torch
        m, k = x.shape
        n = w.shape[0]
        assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == k, "linear_rows_partials reads row-major [m, k] and [n, k] tensors"
        n_split = _SPLITS.get((n, k, self.cmr_dtype))
        if n_split is None:
            ns, nbytes = C.c_int32(0), C.c_int64(0)
            L.check(L.lib().cmr_encoder_linear_small_split(1, n, k, self.cmr_dtype, C.byref(ns), C.byref(nbytes)))
            n_split = _SPLITS[(n, k, self.cmr_dtype)] = int(ns.value)
        part = torch.empty((n_split, m, n), dtype=torch.float32, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.lib().cmr_encoder_linear_rows_partials(x.device.index or 0, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), m, n, k, self.cmr_dtype,
                                                         C.c_void_p(part.data_ptr()), C.c_void_p(stream)))
        return part

    def add_layernorm_partials(self, part, bias, residual, gamma, beta, stream: Optional[int] = None):
        """LayerNorm(sum of the slabs + bias + residual) (cmr_encoder_add_layernorm_partials) -> [m, n] of the model's dtype."""
        import torch
        n_split, m, n = part.shape
        out = torch.empty((m, n), dtype=self.dtype, device=part.device)
        if stream is None:
            stream = torch.cuda.current_stream(part.device).cuda_stream
        L.check(L.lib().cmr_encoder_add_layernorm_partials(part.device.index or 0, C.c_void_p(part.data_ptr()), n_split, C.c_void_p(bias.data_ptr() if bias is not None else 0),
                                                           C.c_void_p(residual.data_ptr() if residual is not None else 0), C.c_void_p(gamma.data_ptr()),
                                                           C.c_void_p(beta.data_ptr()), self.eps, m, n, self.cmr_dtype, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def add_layernorm_partials_pool(self, part, bias, residual, gamma, beta, lens_dev, b: int, l: int, normalize: bool = True, stream: Optional[int] = None):
        """The last layer's add_layernorm_partials with mean_pooling + F.normalize folded in (cmr_encoder_add_layernorm_partials_pool: the
        add_layernorm_pool kernel reading the slabs): [b, hidden] fp32."""
        import torch
        out = torch.empty((b, self.hidden), dtype=torch.float32, device=part.device)
        scratch = torch.empty((b * (l // 16), self.hidden), dtype=torch.float32, device=part.device)
        if stream is None:
            stream = torch.cuda.current_stream(part.device).cuda_stream
        L.check(L.lib().cmr_encoder_add_layernorm_partials_pool(part.device.index or 0, C.c_void_p(part.data_ptr()), part.shape[0], C.c_void_p(bias.data_ptr() if bias is not None else 0),
                                                                C.c_void_p(residual.data_ptr() if residual is not None else 0), C.c_void_p(gamma.data_ptr()),
                                                                C.c_void_p(beta.data_ptr()), self.eps, b, l, self.hidden, self.cmr_dtype, C.c_void_p(lens_dev.data_ptr()),
                                                                1 if normalize else 0, C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def attention_cls(self, qkv, lens_dev, b: int, l: int, stream: Optional[int] = None):
        """The attention of token 0 of every sequence alone (cmr_encoder_attention_cls): [b, hidden] of qkv's dtype."""
        import torch
        out = torch.empty((b, self.hidden), dtype=qkv.dtype, device=qkv.device)
        if stream is None:
            stream = torch.cuda.current_stream(qkv.device).cuda_stream
        L.check(L.lib().cmr_encoder_attention_cls(qkv.device.index or 0, C.c_void_p(qkv.data_ptr()), self.cmr_dtype, C.c_void_p(lens_dev.data_ptr()),
                                                  b, l, self.n_heads, self.hidden // self.n_heads, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def cls_head(self, x, x_stride: int, head, b: int, stream: Optional[int] = None):
        """One logit per sequence (cmr_encoder_cls_head): head = (w1 [d, d], b1 [d] | None, w2 [d], b2 [1] | None) of the model's dtype, x the
        b rows of d elements that sit x_stride elements apart -> [b] fp32."""
        import torch
        w1, b1, w2, b2 = head
        out = torch.empty((b,), dtype=torch.float32, device=x.device)
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.lib().cmr_encoder_cls_head(x.device.index or 0, C.c_void_p(x.data_ptr()), int(x_stride), C.c_void_p(w1.data_ptr()),
                                             C.c_void_p(b1.data_ptr() if b1 is not None else 0), C.c_void_p(w2.data_ptr()),
                                             C.c_void_p(b2.data_ptr() if b2 is not None else 0), b, w1.shape[0], self.cmr_dtype,
                                             C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def _cls_tail(self, x, lens_dev, b: int, l: int, head, stream):
        """The LAST layer of a forward that ends in a classification head, x [b*l, hidden] the layer's input: the packed projection over
        every token row (the keys and values), then attention, O-projection + LayerNorm, FFN and LayerNorm for the b CLS rows alone, then the
        head.  The b-row linear layers take the route `_layers` picks for a mini-batch of b token rows."""
        import torch
        import torch.nn.functional as F
        wqkv, bqkv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2 = self.layers[-1]
        qkv = self.linear_small(x, wqkv, bqkv, False, stream) if 0 < b * l <= self.small_m_rows else F.linear(x, wqkv, bqkv)
        ctx = self.attention_cls(qkv, lens_dev, b, l, stream)
        res = x.view(b, l, self.hidden)[:, 0].contiguous()                # the residual rows: token 0 of the layer's input
        if 0 < b <= self.small_m_rows:
            y = self.add_layernorm_partials(self.linear_small_partials(ctx, wo, stream), bo, res, g1, be1, stream)
            h = self.linear_small(y, w1, b1, True, stream)
            y = self.add_layernorm_partials(self.linear_small_partials(h, w2, stream), b2, y, g2, be2, stream)
        else:
            y = self.add_layernorm(F.linear(ctx, wo), bo, res, g1, be1, stream)
            if self.gelu_path == "hipblaslt-epilogue-tanh":
                h = torch._addmm_activation(b1, y, w1.t(), use_gelu=True)
            else:
                h = F.gelu(F.linear(y, w1, b1))
            y = self.add_layernorm(F.linear(h, w2), b2, y, g2, be2, stream)
        return self.cls_head(y, self.hidden, head, b, stream)

    def forward_cls(self, input_ids, lens, token_type_ids=None, head=None, cls_tail: bool = True):
        """A cross-encoder's forward: input_ids [b, l] int64 on the GPU (right-padded pairs), lens[b] real token counts (host array or int32
        GPU tensor), token_type_ids [b, l] or None, head = the classification head's tensors (`cls_head`) -> [b] fp32 logits.
        cls_tail = True: layers 0 .. n-2 run as in `__call__`, the last one for the b CLS rows alone (`_cls_tail`); False: the unchanged
        stack writes the whole last hidden state and the head reads its CLS rows in place.  Launched eagerly (no captured graphs)."""
        import torch
        if head is None:
            raise ValueError("forward_cls needs the classification head's tensors")
        b, l = input_ids.shape
        with torch.no_grad():
            if isinstance(lens, torch.Tensor) and lens.is_cuda:
                lens_dev = lens.to(torch.int32)
            else:
                lens_dev = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).pin_memory().to(input_ids.device, non_blocking=True)
            with _GATE.shared():
                stream = torch.cuda.current_stream(input_ids.device).cuda_stream
                x = self.embed(input_ids, token_type_ids, stream)
                if not cls_tail:
                    x = self._layers(x, lens_dev, b, l, None, stream)
                    return self.cls_head(x, l * self.hidden, head, b, stream)
                x = self._layers(x, lens_dev, b, l, None, stream, layers=self.layers[:-1])
                return self._cls_tail(x.reshape(b * l, self.hidden), lens_dev, b, l, head, stream)

    def can_pool(self, l: int) -> bool:
        """Can the encoder tail be folded into the last layer's LayerNorm for mini-batches of l (padded) tokens?"""
        return self.fold_pool and l % 16 == 0 and self.hidden % 8 == 0

    # ------------------------------------------------------------------ forward
    def _stack(self, input_ids, lens_dev, token_type_ids, pool=None):
        """Embeddings + every layer on torch's current stream; all arguments on the GPU.  pool = None: the last hidden state
        [b, l, hidden]; pool = True / False: the pooled rows [b, hidden] fp32, L2-normalised or not (the tail rides the last
        layer's LayerNorm kernel)."""
        import torch
        import torch.nn.functional as F
        b, l = input_ids.shape
        stream = torch.cuda.current_stream(input_ids.device).cuda_stream
        return self._layers(self.embed(input_ids, token_type_ids, stream), lens_dev, b, l, pool, stream)

    def _stack_ragged(self, packed, b: int, l: int, pool, rows_route: bool = False):
        """The same from ONE int32 tensor lens[b] | offsets[b + 1] | token ids (ragged, back to back)."""
        import torch
        stream = torch.cuda.current_stream(packed.device).cuda_stream
        x = self.embed_ragged(packed[2 * b + 1:], packed[b:2 * b + 1], b, l, stream)
        return self._layers(x, packed[:b], b, l, pool, stream, rows_route)

    def _layers(self, x, lens_dev, b: int, l: int, pool, stream, rows_route: bool = False, layers=None):
        """layers = None: the whole stack; a prefix of `self.layers` (forward_cls: every layer but the last) runs those alone."""
        import torch
        import torch.nn.functional as F
        if rows_route:                                 # asked for by the caller, never chosen by size: an ordinary mini-batch keeps hipBLASLt
            return self._layers_rows(x, lens_dev, b, l, pool, stream)
        if 0 < b * l <= self.small_m_rows:
            return self._layers_small_m(x, lens_dev, b, l, pool, stream) if layers is None else self._layers_small_m(x, lens_dev, b, l, pool, stream, layers=layers)
        layers = self.layers if layers is None else layers
        last = len(layers) - 1
        for n, (wqkv, bqkv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2) in enumerate(layers):
            qkv = F.linear(x, wqkv, bqkv)
            ctx = self.attention(qkv, lens_dev, b, l, stream)
            x = self.add_layernorm(F.linear(ctx, wo), bo, x, g1, be1, stream)
            if self.gelu_path == "hipblaslt-epilogue-tanh":
                h = torch._addmm_activation(b1, x, w1.t(), use_gelu=True)       # one GEMM: + bias, GELU in the epilogue
            else:
                h = F.gelu(F.linear(x, w1, b1))
            if n == last and pool is not None:
                return self.add_layernorm_pool(F.linear(h, w2), b2, x, g2, be2, lens_dev, b, l, bool(pool), stream)
            x = self.add_layernorm(F.linear(h, w2), b2, x, g2, be2, stream)
        return x.view(b, l, self.hidden)

    def _layers_small_m(self, x, lens_dev, b: int, l: int, pool, stream, layers=None):
        """The short-row route: seven launches per layer, none of them a PyTorch GEMM or GELU kernel.  The two K-split projections hand
        fp32 slabs to the LayerNorm launch that follows them; nothing waits inside a launch.  The GELU is the exact erf form."""
        layers = self.layers if layers is None else layers
        last = len(layers) - 1
        for n, (wqkv, bqkv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2) in enumerate(layers):
            qkv = self.linear_small(x, wqkv, bqkv, False, stream)
            ctx = self.attention(qkv, lens_dev, b, l, stream)
            x = self.add_layernorm_partials(self.linear_small_partials(ctx, wo, stream), bo, x, g1, be1, stream)
            h = self.linear_small(x, w1, b1, True, stream)
            part = self.linear_small_partials(h, w2, stream)
            if n == last and pool is not None:
                return self.add_layernorm_partials_pool(part, b2, x, g2, be2, lens_dev, b, l, bool(pool), stream)
            x = self.add_layernorm_partials(part, b2, x, g2, be2, stream)
        return x.view(b, l, self.hidden)

    def _layers_rows(self, x, lens_dev, b: int, l: int, pool, stream):
        """The many-row route: `_layers_small_m` with the linear layers' many-row entry points — the same seven launches per layer, the same
        attention and partials-LayerNorm calls, the pooled last layer.  A sequence of b*l <= 2048 token rows gets, row for row, the bits of its
        own [1, l] forward on the short-row route: the linear kernels' contract, and every other stage works per sequence or per row."""
        last = len(self.layers) - 1
        for n, (wqkv, bqkv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2) in enumerate(self.layers):
            qkv = self.linear_rows(x, wqkv, bqkv, False, stream)
            ctx = self.attention(qkv, lens_dev, b, l, stream)
            x = self.add_layernorm_partials(self.linear_rows_partials(ctx, wo, stream), bo, x, g1, be1, stream)
            h = self.linear_rows(x, w1, b1, True, stream)
            part = self.linear_rows_partials(h, w2, stream)
            if n == last and pool is not None:
                return self.add_layernorm_partials_pool(part, b2, x, g2, be2, lens_dev, b, l, bool(pool), stream)
            x = self.add_layernorm_partials(part, b2, x, g2, be2, stream)
        return x.view(b, l, self.hidden)

    def __call__(self, input_ids, lens: np.ndarray, token_type_ids=None, consume=None, pool=None):
        """input_ids [b, l] int64 on the GPU (right-padded), lens[b] real token counts (host array, or an int32 tensor already
        on the GPU) → last hidden state [b, l, hidden];
        with `consume`, returns consume(hidden) instead; with pool = True / False (and `can_pool(l)`), the pooled rows [b, hidden]
        fp32 — masked mean over the tokens, L2-normalised or not — computed inside the last layer's LayerNorm kernel.

        A mini-batch shape seen before runs as ONE captured hipGraph (`graphs` > 0: up to that many shapes are kept, captured at
        a shape's second occurrence): ~100 launches and as many interpreter round trips become one, which is most of a short
        query's encode time and leaves the interpreter lock to the tokenizer threads during corpus encodes.  A graph's inputs and
        output are its own static buffers, so replays are serialised by a lock and `consume` (the pooling kernel's launch) runs
        under it: the next replay is stream-ordered behind the reader of this one's output."""
        import torch
        b, l = input_ids.shape
        with torch.no_grad():
            # (pinned: a copy from pageable memory makes the host wait for everything queued on the stream before it)
            if isinstance(lens, torch.Tensor) and lens.is_cuda:
                lens_src = lens.to(torch.int32)              # already uploaded by the caller (its own pinned staging ring)
            else:
                lens_src = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).pin_memory()
            if pool is not None and not self.can_pool(l):
                if consume is None:
                    raise ValueError("FusedBertLayers: pool needs l % 16 == 0 (pass consume= for other shapes)")
                pool = None
            key = (b, l, token_type_ids is not None, pool)
            if self.graphs > 0:
                with self._glock:
                    ent = self._graphs.get(key)
                    if ent is None:
                        if len(self._seen) > 4096:               # a corpus of ragged shapes: forget the counts, keep the graphs
                            self._seen.clear()
                        seen = self._seen[key] = self._seen.get(key, 0) + 1
                        if seen >= 2 and self._room_for_a_graph():
                            with _GATE.exclusive():
                                ent = self._graphs[key] = self._capture(b, l, token_type_ids is not None, pool)
                    if ent is not None:
                        with _GATE.shared():
                            cur = torch.cuda.current_stream(input_ids.device)
                            if ent.get("stream") is not None and ent["stream"] != cur:
                                cur.wait_stream(ent["stream"])          # a caller on another stream: order behind the last reader of the buffers
                            ent["stream"] = cur
                            self._touch(ent)
                            ent["ids"].copy_(input_ids, non_blocking=True)
                            ent["lens"].copy_(lens_src, non_blocking=True)
                            if token_type_ids is not None:
                                ent["tt"].copy_(token_type_ids, non_blocking=True)
                            ent["graph"].replay()
                            if pool is not None:
                                return ent["hidden"].clone()         # [b, hidden] fp32: the graph's static output, copied out under the lock
                            return consume(ent["hidden"]) if consume is not None else ent["hidden"].clone()
            with _GATE.shared():
                hidden = self._stack(input_ids, lens_src.to(input_ids.device, non_blocking=True), token_type_ids, pool)
                return hidden if pool is not None else (consume(hidden) if consume is not None else hidden)

    def forward_ragged(self, packed_host: np.ndarray, b: int, l: int, normalize: bool = True, rows_route: bool = False):
        """One mini-batch from the tokenizer's ragged output: packed_host = int32 [lens (b) | offsets (b + 1) | token ids back to
        back], l = the padded width (a multiple of 16, >= the longest sequence).  Returns the pooled rows [b, hidden] fp32
        (masked mean, L2-normalised unless normalize = False).  The host ships ONE pinned array per mini-batch — no padded id /
        mask / token-type tensors are built on either side of the link; a shape seen before replays its captured hipGraph.
        rows_route = True (the short-row route must be armed; b*l <= ROWS_MAX): the linear layers run on the many-row small-M kernels
        (`_layers_rows`) whatever b*l is — several one-question forwards in one, each sequence with the bits of its own [1, l] forward.
        The route is part of the captured graph's key."""
        import torch
        if l % 16 or not self.can_pool(l):
            raise ValueError("forward_ragged needs a padded width that is a multiple of 16")
        if rows_route and not (self.small_m_rows > 0 and 0 < b * l <= ROWS_MAX):
            raise ValueError(f"forward_ragged: rows_route needs the short-row route armed (small_m) and at most {ROWS_MAX} token rows")
        n = int(packed_host.shape[0])
        with torch.no_grad():
            src = torch.from_numpy(packed_host).pin_memory()        # pinned: a pageable source makes the host wait for the stream
            key = (b, l, "ragged-rows" if rows_route else "ragged", bool(normalize))
            if self.graphs > 0:
                with self._glock:
                    ent = self._graphs.get(key)
                    if ent is None:
                        if len(self._seen) > 4096:
                            self._seen.clear()
                        seen = self._seen[key] = self._seen.get(key, 0) + 1
                        if seen >= 2 and self._room_for_a_graph():
                            with _GATE.exclusive():
                                ent = self._graphs[key] = self._capture_ragged(b, l, bool(normalize), bool(rows_route))
                    if ent is not None:
                        with _GATE.shared():
                            cur = torch.cuda.current_stream(self.device)
                            if ent.get("stream") is not None and ent["stream"] != cur:
                                cur.wait_stream(ent["stream"])
                            ent["stream"] = cur
                            self._touch(ent)
                            ent["packed"][:n].copy_(src, non_blocking=True)
                            ent["graph"].replay()
                            return ent["hidden"].clone()
            with _GATE.shared():
                return self._stack_ragged(src.to(self.device, non_blocking=True), b, l, bool(normalize), bool(rows_route))

    def _capture_ragged(self, b: int, l: int, normalize: bool, rows_route: bool = False):
        import torch
        dev = self.device
        packed = torch.zeros((2 * b + 1 + b * l,), dtype=torch.int32, device=dev)
        packed[:b] = 1                                              # one token per sequence: a valid batch for the warm-up pass
        packed[b:2 * b + 1] = torch.arange(b + 1, dtype=torch.int32, device=dev)
        ent = {"packed": packed}
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._stack_ragged(packed, b, l, normalize, rows_route)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self._capture_stream(), capture_error_mode="thread_local"):
            ent["hidden"] = self._stack_ragged(packed, b, l, normalize, rows_route)
        ent["graph"] = graph
        return ent

    def _capture_stream(self):
        """The side stream this stack captures on (one per stack: torch.cuda.graph's default is a process-wide one, shared by every
        capturing thread)."""
        import torch
        st = getattr(self, "_cap_stream", None)
        if st is None:
            st = self._cap_stream = torch.cuda.Stream(self.device)
        return st

    def _room_for_a_graph(self) -> bool:
        """Called under the lock before a capture: with the table full, the graph that was replayed longest ago goes (its static
        buffers and private pool return to PyTorch's allocator once nothing references them) — the first `graphs` shapes of a
        process must not occupy the table forever while the shapes of today's corpus run eagerly."""
        if self.graphs <= 0:
            return False
        if len(self._graphs) >= self.graphs:
            victim = min(self._graphs, key=lambda k: self._graphs[k].get("used", 0))
            st = self._graphs[victim].get("stream")
            if st is not None:
                st.synchronize()              # its last replay (and the reader of its output) are done
            del self._graphs[victim]
        return True

    def _touch(self, ent) -> None:
        self._clock = getattr(self, "_clock", 0) + 1
        ent["used"] = self._clock

    def _capture(self, b: int, l: int, has_tt: bool, pool=None):
        """Static buffers + one eager pass on a side stream (allocator and GEMM-heuristic warm-up) + the captured pass."""
        import torch
        dev = self.device
        ent = {"ids": torch.zeros((b, l), dtype=torch.int64, device=dev), "lens": torch.ones((b,), dtype=torch.int32, device=dev),
               "tt": torch.zeros((b, l), dtype=torch.int64, device=dev) if has_tt else None}
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._stack(ent["ids"], ent["lens"], ent["tt"], pool)
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self._capture_stream(), capture_error_mode="thread_local"):
            ent["hidden"] = self._stack(ent["ids"], ent["lens"], ent["tt"], pool)
        ent["graph"] = graph
        return ent

    def release(self) -> None:
        """Drop the captured graphs (their private memory pools go back to PyTorch's allocator)."""
        with self._glock:
            self._graphs.clear()
            self._seen.clear()
