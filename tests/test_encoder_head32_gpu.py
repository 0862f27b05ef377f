"""32-wide heads through the fused encoder stack (the HD = 32 instantiations of attn_fwd_kernel / attn_fwd_f32_kernel in
comorag_amd/csrc/encoder_kernels.hip, `FusedBertLayers(head32=True)`, config `embedding_fused_head32`): the tier of bge-small, e5-small and
MiniLM (384 hidden, 12 heads).  The attention kernels against the softmax formula, the LayerNorm kernels at d = 384, and the whole encoder
against the CPU oracle and the transformers forward.

Inputs are the recipe of tests/test_encoder_fused_gpu.py / test_encoder_fp32_gpu.py (qkv = randn * 1.5: the same per-element variance, so
scores / sqrt(HD) spread as they do at 64) and so are the tolerances: TOL per 16-bit dtype, and for fp32 the protocol
e_got <= 4 e_ref + 4 ulp32(max|want|) with `want` the formula in fp64 and `ref` the same formula in torch fp32 ops."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"bfloat16": 2e-2, "float16": 2.5e-3}
HD = 32

# one 128-row query block and two; either side of the 64-key chunk edge; two chunks past 256 tokens; hidden 384 with the real head count
SHAPES = [(3, 100, 2), (5, 37, 4), (2, 129, 1), (1, 64, 3), (2, 65, 2), (2, 300, 3), (2, 48, 12)]


class _Stages:
    """FusedBertLayers' kernel wrappers without a model around them (the head width follows from hidden / heads)."""
    def __init__(self, hidden, heads, dtype, eps=1e-12):
        import torch
        from comorag_amd import _lib as L
        from comorag_amd.embedding_model.fused_bert import FusedBertLayers
        self.hidden, self.n_heads, self.eps = hidden, heads, eps
        self.cmr_dtype = {torch.bfloat16: L.CMR_BF16, torch.float16: L.CMR_F16, torch.float32: L.CMR_F32}[dtype]
        self.attention = FusedBertLayers.attention.__get__(self)
        self.add_layernorm = FusedBertLayers.add_layernorm.__get__(self)
        self.add_layernorm_pool = FusedBertLayers.add_layernorm_pool.__get__(self)


def _within_protocol(got, ref, want, what):
    """e_got <= 4 e_ref + 4 ulp32(max|want|); prints the figures first (pytest -s shows them)."""
    import torch
    assert got.dtype == torch.float32 and ref.dtype == torch.float32 and want.dtype == torch.float64
    assert torch.isfinite(got).all()
    e_got = float((got.double() - want).abs().max())
    e_ref = float((ref.double() - want).abs().max())
    ulp = float(np.spacing(np.float32(float(want.abs().max()))))
    print(f"{what}: e_got {e_got:.3e}  e_ref {e_ref:.3e}  ratio {e_got / max(e_ref, 1e-30):.2f}  ulp32(max|want|) {ulp:.3e}")
    assert e_got <= 4.0 * e_ref + 4.0 * ulp, (what, e_got, e_ref, ulp)


# ---------------------------------------------------------------------------------------------------------------- attention
def _attention_case(b, l, heads):
    """fp32 qkv [b*l, 3*heads*32] and the lengths: a full row, a one-token row (below 200 tokens) / a query block of padding only."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(b * 1000 + l)
    qkv = torch.randn((b * l, 3 * heads * HD), generator=g, device="cuda") * 1.5                  # peaked, non-symmetric scores
    lens = np.random.default_rng(l).integers(1, l + 1, size=b).astype(np.int32)
    lens[0] = l
    if b > 1:
        lens[1] = 1 if l < 200 else l - 130
    return qkv, lens


def _attention_formula(qkv, lens_dev, b, l, heads):
    """softmax(Q K^T / sqrt(32), keys >= lens masked) V in qkv's own precision: [b, l, heads, 32]."""
    import torch
    x = qkv.view(b, l, 3, heads, HD)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    scores = q @ k.transpose(-1, -2) / (HD ** 0.5)
    keymask = torch.arange(l, device=qkv.device)[None, :] >= lens_dev[:, None]
    scores = scores.masked_fill(keymask[:, None, None, :], float("-inf"))
    return (torch.softmax(scores, dim=-1) @ v).permute(0, 2, 1, 3)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_attention_head32_vs_fp32_softmax(dtype, shape):
    import torch
    b, l, heads = shape
    tdt = getattr(torch, dtype)
    qkv, lens = _attention_case(b, l, heads)
    qkv = qkv.to(tdt)
    lens_dev = torch.from_numpy(lens).cuda()
    got = _Stages(heads * HD, heads, tdt).attention(qkv, lens_dev, b, l).float().view(b, l, heads, HD)
    torch.cuda.synchronize()
    want = _attention_formula(qkv.float(), lens_dev, b, l, heads)                                 # fp32 softmax on the rounded inputs
    assert torch.isfinite(got).all()                                                              # padding rows included
    for s in range(b):
        err = float((got[s, :lens[s]] - want[s, :lens[s]]).abs().max())
        print(f"attention {dtype} {shape} sequence {s} ({lens[s]} tokens): max abs error {err:.3e}")
        np.testing.assert_allclose(got[s, :lens[s]].cpu().numpy(), want[s, :lens[s]].cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_head32_fp32_vs_fp64(shape):
    import torch
    b, l, heads = shape
    qkv, lens = _attention_case(b, l, heads)
    lens_dev = torch.from_numpy(lens).cuda()
    fz = _Stages(heads * HD, heads, torch.float32)
    got = fz.attention(qkv, lens_dev, b, l)
    again = fz.attention(qkv, lens_dev, b, l)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.isfinite(got).all()                                # padding rows included
    assert torch.equal(got, again)                                                                 # two runs, identical bits
    got = got.view(b, l, heads, HD)
    ref = _attention_formula(qkv, lens_dev, b, l, heads)
    want = _attention_formula(qkv.double(), lens_dev, b, l, heads)
    live = (torch.arange(l, device="cuda")[None, :] < lens_dev[:, None])                           # every row < lens[s]
    _within_protocol(got[live], ref[live].contiguous(), want[live].contiguous(), f"attention fp32 {shape}")


def test_attention_head32_fp32_a_sequence_alone_gives_the_same_bits():
    import torch
    b, l, heads = 3, 100, 2
    qkv, lens = _attention_case(b, l, heads)
    fz = _Stages(heads * HD, heads, torch.float32)
    whole = fz.attention(qkv, torch.from_numpy(lens).cuda(), b, l).view(b, l, -1)
    for s in range(b):
        alone = fz.attention(qkv[s * l:(s + 1) * l].contiguous(), torch.from_numpy(lens[s:s + 1].copy()).cuda(), 1, l).view(l, -1)
        assert torch.equal(alone, whole[s])


@pytest.mark.parametrize("head_dim", [16, 48, 128])
def test_other_head_widths_are_refused(head_dim):
    import torch
    from comorag_amd import _lib as L
    x = torch.zeros((16, 3 * 128), device="cuda", dtype=torch.bfloat16)
    lens = torch.ones((1,), dtype=torch.int32, device="cuda")
    out = torch.zeros((16, 128), device="cuda", dtype=torch.bfloat16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dt in (L.CMR_BF16, L.CMR_F16, L.CMR_F32):
        rc = L.lib().cmr_encoder_attention(0, C.c_void_p(x.data_ptr()), dt, C.c_void_p(lens.data_ptr()), 1, 16, 1, head_dim, C.c_void_p(out.data_ptr()), st)
        msg = L.lib().cmr_last_error().decode()
        assert rc == L.CMR_ERR_INVALID and "64" in msg and "32" in msg, (rc, msg)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm at d = 384
@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float32"])
@pytest.mark.parametrize("rows", [5, 300])                                                        # the few-rows kernel and the many-rows one
def test_add_layernorm_at_the_hidden_size_of_this_tier(dtype, rows):
    import torch
    import torch.nn.functional as F
    d, tdt = 384, getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(d + rows)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")
    y, res = (rnd(rows, d) * 2 + 0.3).to(tdt), rnd(rows, d).to(tdt)
    bias, gamma, beta = rnd(d).to(tdt), (1 + 0.2 * rnd(d)).to(tdt), (0.1 * rnd(d)).to(tdt)
    got = _Stages(d, 12, tdt).add_layernorm(y, bias, res, gamma, beta)
    if dtype == "float32":
        ref = F.layer_norm(y + bias + res, (d,), gamma, beta, 1e-12)
        want = F.layer_norm(y.double() + bias.double() + res.double(), (d,), gamma.double(), beta.double(), 1e-12)
        _within_protocol(got, ref, want, f"add_layernorm d={d} rows={rows}")
    else:
        want = F.layer_norm(y.float() + bias.float() + res.float(), (d,), gamma.float(), beta.float(), 1e-12)
        np.testing.assert_allclose(got.float().cpu().numpy(), want.cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])


@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float32"])
@pytest.mark.parametrize("normalize", [True, False])
def test_add_layernorm_pool_at_the_hidden_size_of_this_tier(dtype, normalize):
    """(b, l, d) = (3, 48, 384): a one-token row, a full one, one that ends inside a 16-token block.  16-bit: the fp32 formula on the
    16-bit-rounded LayerNorm output, tolerances of test_last_layer_layernorm_with_the_encoder_tail_folded_in (b * l <= 256: the
    wave-per-row LayerNorm sums in another order than the folded kernel, 1.5 units in the last place of the 16-bit type on top); fp32: the protocol."""
    import torch
    import torch.nn.functional as F
    from oracle import encode_torch as enc
    b, l, d, tdt = 3, 48, 384, getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(b * 1000 + l + d)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")
    y, res = rnd(b * l, d).to(tdt), rnd(b * l, d).to(tdt)
    bias, gamma, beta = rnd(d).to(tdt), rnd(d).to(tdt), rnd(d).to(tdt)
    lens = torch.tensor([1, l, l - 5], dtype=torch.int32)
    mask = (torch.arange(l)[None, :] < lens[:, None]).to(torch.int64).cuda()
    fz = _Stages(d, 12, tdt)
    got = fz.add_layernorm_pool(y, bias, res, gamma, beta, lens.cuda(), b, l, normalize)
    assert got.dtype == torch.float32 and got.shape == (b, d)
    if dtype == "float32":
        def formula(dt):
            h = F.layer_norm(y.to(dt) + bias.to(dt) + res.to(dt), (d,), gamma.to(dt), beta.to(dt), 1e-12).view(b, l, d)
            e = enc.mean_pooling(h, mask)
            return F.normalize(e, p=2, dim=1) if normalize else e
        _within_protocol(got, formula(torch.float32), formula(torch.float64), f"add_layernorm_pool {(b, l, d)} normalize={normalize}")
        return
    hidden = fz.add_layernorm(y, bias, res, gamma, beta).view(b, l, d)
    want = (hidden.float() * mask[..., None]).sum(1) / lens.cuda()[:, None].float()
    if normalize:
        want = F.normalize(want, p=2, dim=1)
    ulp = 2.0 ** -8 if dtype == "bfloat16" else 2.0 ** -11
    tol = max(3e-6 if normalize else 3e-5, 1.5 * ulp * float(want.abs().max()))
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=tol, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- the whole stack
_TEXTS = [f"the prince and the golden slipper number {i} " + "and the bird in the tree " * (i % 7) for i in range(23)]
_TEXTS += ["she was good and pious " * 40, "midnight"]


def _peaked_head32_bert(dtype=None):
    """32-wide heads at the row length of the existing toy test (hidden 256): its bars apply."""
    import torch
    from oracle import encode_torch as enc
    model, tok = enc.tiny_bert(hidden=256, layers=3, heads=8, inter=512, max_pos=128)
    with torch.no_grad():                              # random-init scores are ~0 (uniform attention): make the softmax matter
        for lyr in model.encoder.layer:
            lyr.attention.self.query.weight.mul_(12.0)
            lyr.attention.self.key.weight.mul_(12.0)
        if dtype is not None:
            model.to(dtype).float()                    # the oracle runs fp32 arithmetic on the SAME 16-bit-representable weights
    return model, tok


def _make(model, tok, **kw):
    from comorag_amd.embedding_model import _get_embedding_model_class
    from comorag_amd.utils.config_utils import BaseConfig
    cfg = BaseConfig(embedding_model_name="bge-tiny-random", embedding_batch_size=8, embedding_max_seq_len=128, **kw)
    return _get_embedding_model_class("bge-tiny-random")(global_config=cfg, embedding_model_name=cfg.embedding_model_name, model=copy.deepcopy(model), tokenizer=tok)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_head32_stack_vs_transformers_forward_and_oracle(dtype):
    import torch
    from oracle import encode_torch as enc
    model, tok = _peaked_head32_bert(getattr(torch, dtype))
    want = enc.batch_encode(model, tok, _TEXTS, batch_size=8, max_length=128)
    fused = _make(model, tok, embedding_model_dtype=dtype, embedding_fused_head32=True)
    plain = _make(model, tok, embedding_model_dtype=dtype)
    assert fused.encoder_path == "hip-fused-layers" and fused._fused.head_dim == 32
    assert plain.encoder_path.startswith("transformers (") and "head width" in plain.encoder_path and plain._fused is None
    got, ref = fused.batch_encode(_TEXTS), plain.batch_encode(_TEXTS)
    e_got, e_ref, cos = float(np.abs(got - want).max()), float(np.abs(ref - want).max()), float(np.min((got * want).sum(1)))
    print(f"{dtype}: max abs error vs the CPU oracle: fused {e_got:.3e}, transformers forward {e_ref:.3e}; min row cosine {cos:.6f}")
    tol = {"bfloat16": 6e-3, "float16": 1e-3}[dtype]                     # unit-norm rows of 256: components ~0.06
    np.testing.assert_allclose(got, want, atol=tol)
    np.testing.assert_allclose(ref, want, atol=tol)
    assert e_got <= 2.0 * e_ref + 2e-4                                   # no worse than the transformers forward in the same dtype
    assert cos > 0.9995
    np.testing.assert_allclose(fused.batch_encode("midnight"), want[-1:], atol=tol)      # one string alone
    fused.close(); plain.close()


def test_head32_fp32_stack_needs_both_flags_and_meets_the_fp32_bar():
    import torch
    from oracle import encode_torch as enc
    model, tok = _peaked_head32_bert()
    assert next(model.parameters()).dtype == torch.float32
    want = enc.batch_encode(model, tok, _TEXTS, batch_size=8, max_length=128)
    want_one = enc.batch_encode(model, tok, "midnight", batch_size=8, max_length=128)
    only32, only_fp32 = _make(model, tok, embedding_fused_head32=True), _make(model, tok, embedding_fused_fp32=True)
    assert only32.encoder_path.startswith("transformers (") and "16-bit" in only32.encoder_path
    assert only_fp32.encoder_path.startswith("transformers (") and "head width" in only_fp32.encoder_path
    fused = _make(model, tok, embedding_fused_head32=True, embedding_fused_fp32=True)
    assert fused.encoder_path == "hip-fused-layers" and fused._fused.dtype == torch.float32 and fused._fused.head_dim == 32
    err = {}
    for name, em in (("transformers", only32), ("fused", fused)):
        got, one = em.batch_encode(_TEXTS), em.batch_encode("midnight")
        assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
        err[name] = max(float(np.abs(got - want).max()), float(np.abs(one - want_one).max()))
    print(f"fp32: max abs error vs the CPU oracle: fused {err['fused']:.3e}, transformers forward {err['transformers']:.3e}")
    assert err["fused"] <= 2.0 * err["transformers"] + 1e-6
    assert err["fused"] <= 2e-5
    for em in (only32, only_fp32, fused):
        em.close()


def test_head32_captured_graphs_equal_eager_forwards():
    import torch
    model, tok = _peaked_head32_bert(torch.bfloat16)
    kw = dict(embedding_model_dtype="bf16", embedding_fused_head32=True, embedding_query_cache=0)      # (every call a forward)
    em, eager = _make(model, tok, **kw), _make(model, tok, embedding_hip_graphs=0, **kw)
    assert em.encoder_path == eager.encoder_path == "hip-fused-layers"
    queries = ["midnight", "she was good and pious " * 5, "she was good and pious " * 12]              # three query lengths
    want = [eager.batch_encode(q) for q in queries]
    assert not eager._fused._graphs
    for rep in range(3):                                   # rep 0 eager, rep 1 captures, rep 2 replays
        for q, w in zip(queries, want):
            np.testing.assert_allclose(em.batch_encode(q), w, atol=2e-6)
    shapes = set(em._fused._graphs)
    assert 1 <= len(shapes) <= len(queries) and all(key[1] % 16 == 0 for key in shapes)
    em.close(); eager.close()


def test_bge_small_shape_ragged_chunks_vs_fp32_oracle():
    """The shape of bge-small / e5-small / MiniLM-L12 (12 x 384, 12 heads of 32, bf16) through the product path on 12 ragged chunks, against
    the oracle's fp32 restatement on the same bf16-representable weights: the three assertions of
    test_bge_base_and_large_shapes_ragged_512_tokens_vs_fp32_oracle."""
    import torch
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.utils.config_utils import BaseConfig
    from tools.bench_extras import encoder_parity
    from tools.synthetic import random_bert, synthetic_chunks, synthetic_wordpiece_tokenizer
    tok, words = synthetic_wordpiece_tokenizer()
    model = random_bert("small", vocab_size=len(tok))
    assert model.config.hidden_size == 384 and model.config.num_attention_heads == 12 and model.config.intermediate_size == 1536
    with torch.no_grad():
        for lyr in model.encoder.layer:
            lyr.attention.self.query.weight.mul_(2.0)
            lyr.attention.self.key.weight.mul_(2.0)
    cfg = BaseConfig(embedding_model_name="bge-small-random-init", embedding_batch_size=8, embedding_model_dtype="bf16", embedding_fused_head32=True)
    em = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=model, tokenizer=tok)
    assert em.encoder_path == "hip-fused-layers" and em._fused.hidden == 384 and em._fused.can_pool(48)
    chunks = synthetic_chunks(words, 12, tokens_per_chunk=560)
    r = encoder_parity(torch, em, chunks, n=12)
    print(r)
    assert r["min_row_cosine_vs_fp32_oracle"] >= 1.0 - 1e-3, r
    assert r["max_abs_pairwise_score_diff"] <= 1e-3, r
    assert 1.0 - r["min_row_cosine_vs_fp32_oracle"] <= 2.0 * (1.0 - r["transformers_same_dtype_min_row_cosine"]) + 1e-5, r
    em.close()
