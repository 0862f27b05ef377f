"""The short-row route of the fused encoder stack: small_linear_kernel (direct and partials form) and add_ln_partials_kernel of
comorag_amd/csrc/encoder_kernels.hip, their C-ABI entries, and `FusedBertLayers(small_m=True)` (config `embedding_fused_small_m`).

Kernel parity is the project's protocol e_got <= 4 e_ref + 4 ulp(max|want|): `want` the function in fp64 on the same 16-bit inputs, `ref`
PyTorch's own 16-bit path on the same device (F.linear, F.gelu(F.linear), the existing add_layernorm kernel behind F.linear), ulp that of
the OUTPUT type.  Shapes are the kernel's edge cases: M either side of a 16-row token tile and of its 32 / 64 / 96-row instantiations, one
k-step, a K slice that leaves waves idle, every split the BERT shapes take."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS = [1, 15, 16, 17, 80, 128]
DIRECT_NK = [(48, 96), (1152, 384), (2304, 768), (3072, 768), (4096, 1024)]
PARTIAL_NK = [(96, 64), (384, 1536), (768, 768), (768, 3072), (1024, 4096)]


class _Stages:
    """FusedBertLayers' kernel wrappers without a model around them."""
    def __init__(self, dtype, eps=1e-12):
        import torch
        from comorag_amd import _lib as L
        from comorag_amd.embedding_model.fused_bert import FusedBertLayers
        self.dtype, self.eps = dtype, eps
        self.cmr_dtype = {torch.bfloat16: L.CMR_BF16, torch.float16: L.CMR_F16}[dtype]
        for name in ("linear_small", "linear_small_partials", "add_layernorm_partials", "add_layernorm"):
            setattr(self, name, getattr(FusedBertLayers, name).__get__(self))


def _ulp16(v: float, dtype: str) -> float:
    """Spacing of the 16-bit type at |v| (8 / 11 significand bits)."""
    return float(2.0 ** (np.floor(np.log2(max(abs(v), 1e-30))) - (7 if dtype == "bfloat16" else 10)))


def _within_protocol(got, ref, want, dtype, what):
    import torch
    assert torch.isfinite(got.float()).all(), what
    e_got = float((got.double() - want).abs().max())
    e_ref = float((ref.double() - want).abs().max())
    ulp = _ulp16(float(want.abs().max()), dtype)
    print(f"{what}: e_got {e_got:.3e}  e_ref {e_ref:.3e}  ratio {e_got / max(e_ref, 1e-30):.2f}  ulp16(max|want|) {ulp:.3e}")
    assert e_got <= 4.0 * e_ref + 4.0 * ulp, (what, e_got, e_ref, ulp)


def _inputs(n, k, dtype, scale=1.0, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(n * 7 + k + seed)
    tdt = getattr(torch, dtype)
    x = (torch.randn((128, k), generator=g, device="cuda") * scale).to(tdt)
    w = (torch.randn((n, k), generator=g, device="cuda") / k ** 0.5).to(tdt)
    bias = torch.randn((n,), generator=g, device="cuda").to(tdt)
    return x, w, bias


# ---------------------------------------------------------------------------------------------------------------- 1. direct form
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("nk", DIRECT_NK)
def test_direct_form_vs_fp64_linear_and_gelu(nk, act, dtype):
    import torch
    import torch.nn.functional as F
    n, k = nk
    x, w, bias = _inputs(n, k, dtype, scale=1.5 if act else 1.0)         # GELU: pre-activations reach |3|
    fz = _Stages(getattr(torch, dtype))
    want_all = F.linear(x.double(), w.double(), bias.double())
    if act:
        want_all = F.gelu(want_all)
    for m in MS:
        xm = x[:m].contiguous()
        got = fz.linear_small(xm, w, bias, bool(act))
        ref = F.gelu(F.linear(xm, w, bias)) if act else F.linear(xm, w, bias)
        assert got.dtype == xm.dtype and got.shape == (m, n)
        _within_protocol(got, ref, want_all[:m], dtype, f"linear_small {dtype} act={act} M={m} N={n} K={k}")
    nb = fz.linear_small(x[:17].contiguous(), w, None, bool(act))        # no bias
    want = F.linear(x[:17].double(), w.double())
    _within_protocol(nb, F.gelu(F.linear(x[:17], w)) if act else F.linear(x[:17], w), F.gelu(want) if act else want, dtype, f"linear_small {dtype} act={act} no bias")


# ---------------------------------------------------------------------------------------------------------------- 2. partials + LayerNorm
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("nk", PARTIAL_NK)
def test_partials_then_add_layernorm_partials_vs_fp64(nk, dtype):
    import torch
    import torch.nn.functional as F
    n, k = nk
    tdt = getattr(torch, dtype)
    x, w, bias = _inputs(n, k, dtype, seed=1)
    g = torch.Generator(device="cuda").manual_seed(n + k)
    res = torch.randn((128, n), generator=g, device="cuda").to(tdt)
    gamma = (1 + 0.2 * torch.randn((n,), generator=g, device="cuda")).to(tdt)
    beta = (0.1 * torch.randn((n,), generator=g, device="cuda")).to(tdt)
    fz = _Stages(tdt)

    def want_of(m, b, r):
        y = F.linear(x[:m].double(), w.double())
        if b is not None: y = y + b.double()
        if r is not None: y = y + r.double()
        return F.layer_norm(y, (n,), gamma.double(), beta.double(), 1e-12)

    def both(m, b, r, what):
        xm = x[:m].contiguous()
        part = fz.linear_small_partials(xm, w)
        assert part.dtype == torch.float32 and part.shape[1:] == (m, n)
        got = fz.add_layernorm_partials(part, b, r, gamma, beta)
        ref = fz.add_layernorm(F.linear(xm, w), b, r, gamma, beta)
        assert got.dtype == tdt and got.shape == (m, n)
        _within_protocol(got, ref, want_of(m, b, r), dtype, what)
        return part

    for m in MS:
        part = both(m, bias, res[:m].contiguous(), f"partials + LN {dtype} M={m} N={n} K={k}")
    # the slabs ARE the product: their fp64 sum against the fp64 product (fp32 accumulation of K terms of magnitude ~1 / sqrt(K) each)
    e = float((part.double().sum(0) - F.linear(x.double(), w.double())).abs().max())
    # bound: a k-ordered fp32 chain is within ~3.5e-7 * sum|a b| of fp64 at K = 4096 (less below); sum|a b| ~ 0.64 sqrt(K) <= 41 here: 1.4e-5,
    # taken four times = 64 spacings of fp32 at the product's largest magnitude (8)
    print(f"slab sum vs fp64 product, N={n} K={k} split {part.shape[0]}: {e:.3e}")
    assert e <= 64 * float(np.spacing(np.float32(8.0)))
    both(17, None, res[:17].contiguous(), f"partials + LN {dtype} N={n} K={k} no bias")
    both(17, bias, None, f"partials + LN {dtype} N={n} K={k} no residual")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("normalize", [True, False])
def test_last_layer_partials_with_the_encoder_tail_folded_in(dtype, normalize):
    """cmr_encoder_add_layernorm_partials_pool == cmr_encoder_add_layernorm_partials followed by the masked mean (and F.normalize) of its
    16-bit output: (b, l) = (3, 32) — a one-token row, a full one, one that ends inside a 16-token block; tolerance of
    test_add_layernorm_pool_at_the_hidden_size_of_this_tier (the folded kernel sums a row in another order than the wave-per-row one:
    1.5 units in the last place of the 16-bit type on top of the fp32 pooling error)."""
    import torch
    import torch.nn.functional as F
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    b, l, n, k, tdt = 3, 32, 384, 1536, getattr(torch, dtype)
    x, w, bias = _inputs(n, k, dtype, seed=3)
    x = x[:b * l].contiguous()
    g = torch.Generator(device="cuda").manual_seed(n + k + 3)
    res = torch.randn((b * l, n), generator=g, device="cuda").to(tdt)
    gamma, beta = torch.randn((n,), generator=g, device="cuda").to(tdt), torch.randn((n,), generator=g, device="cuda").to(tdt)
    lens = torch.tensor([1, l, l - 5], dtype=torch.int32, device="cuda")
    fz = _Stages(tdt)
    fz.hidden = n
    part = fz.linear_small_partials(x, w)
    got = FusedBertLayers.add_layernorm_partials_pool(fz, part, bias, res, gamma, beta, lens, b, l, normalize)
    assert got.dtype == torch.float32 and got.shape == (b, n)
    hidden = fz.add_layernorm_partials(part, bias, res, gamma, beta).view(b, l, n)
    mask = (torch.arange(l, device="cuda")[None, :] < lens[:, None])
    want = (hidden.float() * mask[..., None]).sum(1) / lens[:, None].float()
    if normalize:
        want = F.normalize(want, p=2, dim=1)
    ulp = 2.0 ** -8 if dtype == "bfloat16" else 2.0 ** -11
    tol = max(3e-6 if normalize else 3e-5, 1.5 * ulp * float(want.abs().max()))
    print(f"partials pool {dtype} normalize={normalize}: max abs diff {float((got - want).abs().max()):.3e} (tol {tol:.3e})")
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=tol, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_a_rows_bits_do_not_depend_on_the_run_the_other_rows_or_m(dtype):
    import torch
    tdt = getattr(torch, dtype)
    fz = _Stages(tdt)
    for (n, k), partial in [((2304, 768), False), ((768, 3072), True), ((48, 96), False), ((384, 1536), True)]:
        x, w, bias = _inputs(n, k, dtype, seed=2)
        run = (lambda xm: fz.linear_small_partials(xm, w).transpose(0, 1)) if partial else (lambda xm: fz.linear_small(xm, w, bias, True))
        a80 = run(x[:80].contiguous())
        assert torch.equal(a80, run(x[:80].contiguous()))                                # two runs
        a17 = run(x[:17].contiguous())
        assert torch.equal(a17, a80[:17])                                                # M = 17 against 80: other instantiation, same bits
        other = x[:80].clone()
        other[1:] = torch.flip(other[1:], dims=[0]) * 3.0                                # row 0 kept, every other row other data
        assert torch.equal(run(other)[0], a80[0])
        if partial:
            g, b = torch.ones((n,), device="cuda", dtype=tdt), torch.zeros((n,), device="cuda", dtype=tdt)
            p80, p17 = fz.linear_small_partials(x[:80].contiguous(), w), fz.linear_small_partials(x[:17].contiguous(), w)
            assert torch.equal(fz.add_layernorm_partials(p80, bias, None, g, b)[:17], fz.add_layernorm_partials(p17, bias, None, g, b))


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_return_the_documented_error_and_launch_nothing():
    import torch
    from comorag_amd import _lib as L
    lib = L.lib()
    x = torch.ones((136, 64), device="cuda", dtype=torch.bfloat16)
    w = torch.ones((64, 64), device="cuda", dtype=torch.bfloat16)
    bias = torch.ones((64,), device="cuda", dtype=torch.bfloat16)
    out = torch.full((136, 64), 7.0, device="cuda", dtype=torch.bfloat16)
    part = torch.full((136 * 64,), 7.0, device="cuda", dtype=torch.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def direct(m=16, n=64, k=64, dt=L.CMR_BF16, xp=None, act=0):
        return lib.cmr_encoder_linear_small(0, P(x) if xp is None else xp, P(w), P(bias), m, n, k, dt, act, P(out), st)

    def partials(m=16, n=64, k=64, dt=L.CMR_BF16, xp=None):
        return lib.cmr_encoder_linear_small_partials(0, P(x) if xp is None else xp, P(w), m, n, k, dt, P(part), st)

    for call in (direct, partials):
        assert call(m=0) == L.CMR_ERR_INVALID
        assert call(m=129) == L.CMR_ERR_UNSUPPORTED and b"128" in lib.cmr_last_error()
        assert call(k=48) == L.CMR_ERR_UNSUPPORTED
        assert call(n=40) == L.CMR_ERR_UNSUPPORTED
        assert call(dt=L.CMR_F32) == L.CMR_ERR_UNSUPPORTED and b"16-bit" in lib.cmr_last_error()
        assert call(dt=7) == L.CMR_ERR_INVALID
        assert call(xp=P(x, 8)) == L.CMR_ERR_UNSUPPORTED and b"aligned" in lib.cmr_last_error()
        assert call(xp=C.c_void_p(0)) == L.CMR_ERR_INVALID
    assert direct(act=2) == L.CMR_ERR_INVALID
    g = torch.ones((64,), device="cuda", dtype=torch.bfloat16)
    ln = lambda **kw: lib.cmr_encoder_add_layernorm_partials(0, kw.get("p", P(part)), kw.get("s", 2), P(bias), None, P(g), P(g), 1e-12, kw.get("rows", 16), kw.get("d", 64),
                                                             kw.get("dt", L.CMR_BF16), P(out), st)
    assert ln(s=0) == L.CMR_ERR_INVALID and ln(rows=0) == L.CMR_ERR_INVALID and ln(d=66) == L.CMR_ERR_INVALID
    assert ln(dt=L.CMR_F32) == L.CMR_ERR_UNSUPPORTED and ln(p=P(part, 4)) == L.CMR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((part == 7.0).all())                       # nothing was launched
    assert direct() == L.CMR_OK and partials() == L.CMR_OK and ln(s=1) == L.CMR_OK      # and the same buffers are fine when the arguments are


# ---------------------------------------------------------------------------------------------------------------- 5. the stack
_SHORT = ["midnight", "the prince and the golden slipper", "she was good and pious and the bird sang"]
_LONG = [f"she was good and pious number {i} " + "and the bird in the tree " * 9 for i in range(16)]


def _peaked_tiny_bert(dtype, heads):
    """tests/test_encoder_fused_gpu.py's toy model (hidden 256: 4 heads of 64) and test_encoder_head32_gpu.py's (8 heads of 32)."""
    import torch
    from oracle import encode_torch as enc
    model, tok = enc.tiny_bert(hidden=256, layers=3, heads=heads, inter=512, max_pos=128)
    with torch.no_grad():                              # random-init scores are ~0 (uniform attention): make the softmax matter
        for lyr in model.encoder.layer:
            lyr.attention.self.query.weight.mul_(12.0)
            lyr.attention.self.key.weight.mul_(12.0)
        model.to(dtype).float()                        # the oracle runs fp32 arithmetic on the SAME 16-bit-representable weights
    return model, tok


def _make(model, tok, **kw):
    from comorag_amd.embedding_model import _get_embedding_model_class
    from comorag_amd.utils.config_utils import BaseConfig
    cfg = BaseConfig(embedding_model_name="bge-tiny-random", embedding_batch_size=8, embedding_max_seq_len=128, **kw)
    return _get_embedding_model_class("bge-tiny-random")(global_config=cfg, embedding_model_name=cfg.embedding_model_name, model=copy.deepcopy(model), tokenizer=tok)


def _count_route(em):
    """Calls of the short-row route of em's layer stack from here on: a list the wrapper appends the row counts to."""
    seen, inner = [], em._fused._layers_small_m
    def spy(x, lens_dev, b, l, pool, stream):
        seen.append(b * l)
        return inner(x, lens_dev, b, l, pool, stream)
    em._fused._layers_small_m = spy
    return seen


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("heads", [4, 8])
def test_small_m_stack_vs_oracle_and_the_flag_off_stack(heads, dtype):
    import torch
    from oracle import encode_torch as enc
    model, tok = _peaked_tiny_bert(getattr(torch, dtype), heads)
    kw = dict(embedding_model_dtype=dtype, embedding_fused_head32=heads == 8, embedding_query_cache=0, embedding_hip_graphs=0)
    on, off = _make(model, tok, embedding_fused_small_m=True, **kw), _make(model, tok, **kw)
    assert on.encoder_path == off.encoder_path == "hip-fused-layers" and on._fused.head_dim == 256 // heads
    assert on.small_m_rows == on._fused.small_m_rows == 96 and off.small_m_rows == off._fused.small_m_rows == 0
    seen = _count_route(on)
    tol = {"bfloat16": 6e-3, "float16": 1e-3}[dtype]                     # unit-norm rows of 256: components ~0.06
    for texts in ("midnight", _SHORT):                                   # one string alone; a ragged batch of three short strings
        want = enc.batch_encode(model, tok, texts, batch_size=8, max_length=128)
        n_before = len(seen)
        got, ref = on.batch_encode(texts), off.batch_encode(texts)
        assert len(seen) == n_before + 1 and seen[-1] <= 96, seen       # the route was taken, once, under the row limit
        e_got, e_ref, cos = float(np.abs(got - want).max()), float(np.abs(ref - want).max()), float(np.min((got * want).sum(1)))
        print(f"{dtype} heads {heads} rows {seen[-1]}: max abs error vs the CPU oracle: small-M {e_got:.3e}, flag off {e_ref:.3e}; min row cosine {cos:.6f}")
        np.testing.assert_allclose(got, want, atol=tol)
        np.testing.assert_allclose(got, ref, atol=tol)
        assert cos > 0.9995
    n_before = len(seen)                                                 # over the row limit: the route is not taken, the bits are the flag-off stack's
    big_on, big_off = on.batch_encode(_LONG), off.batch_encode(_LONG)
    assert len(seen) == n_before and np.array_equal(big_on, big_off)
    on.close(); off.close()


# ---------------------------------------------------------------------------------------------------------------- 6. BGE shapes
@pytest.mark.parametrize("kind,dtype", [("base", "bf16"), ("large", "fp16")])
def test_bge_base_and_large_shapes_one_short_query_vs_fp32_oracle(kind, dtype):
    import torch
    from comorag_amd.embedding_model.bge import HipBGEEmbeddingModel
    from comorag_amd.utils.config_utils import BaseConfig
    from oracle import encode_torch as enc_o
    from tools.synthetic import random_bert, synthetic_chunks, synthetic_wordpiece_tokenizer
    tok, words = synthetic_wordpiece_tokenizer()
    model = random_bert(kind, vocab_size=len(tok))
    with torch.no_grad():
        for lyr in model.encoder.layer:
            lyr.attention.self.query.weight.mul_(2.0)
            lyr.attention.self.key.weight.mul_(2.0)
    cfg = BaseConfig(embedding_model_name=f"bge-{kind}-random-init", embedding_batch_size=8, embedding_model_dtype=dtype, embedding_fused_small_m=True,
                     embedding_query_cache=0)
    em = HipBGEEmbeddingModel(cfg, cfg.embedding_model_name, model=model, tokenizer=tok)
    assert em.encoder_path == "hip-fused-layers" and em.small_m_rows == 96
    seen = _count_route(em)
    query = " ".join(synthetic_chunks(words, 1, tokens_per_chunk=560)[0].split()[:12])          # one 12-word query
    # tools.bench_extras.encoder_parity's three encodes of it: the fp32 oracle on the host, the product path, the transformers forward in the same
    # 16-bit dtype.  With ONE row the cosines are computed as cosines (a 16-bit forward's row is unit-norm only to 16-bit rounding: its plain dot
    # product with the oracle's row can exceed 1, and 1 - cos would turn negative)
    maxlen = int(model.config.max_position_embeddings)
    want = enc_o.batch_encode(copy.deepcopy(em.embedding_model).float().cpu().eval(), tok, [query], batch_size=8, max_length=maxlen).astype(np.float64)
    got = em.batch_encode([query]).astype(np.float64)
    plain = enc_o.encode(em.embedding_model, tok, [query], instruction=enc_o.BGE_PREFIX, max_length=maxlen).float().cpu().numpy().astype(np.float64)
    cosine = lambda a, b: float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)))
    cos, cos_tf = cosine(got, want), cosine(plain, want)
    print(f"bge-{kind} {dtype}: token rows {seen}; 1 - cos vs the fp32 oracle: small-M route {1 - cos:.3e}, transformers forward in {dtype} {1 - cos_tf:.3e}")
    assert seen and all(rows <= 96 for rows in seen)
    assert abs(float(np.linalg.norm(got)) - 1.0) <= 1e-5
    assert cos >= 1.0 - 1e-3
    assert 1.0 - cos <= 2.0 * (1.0 - cos_tf) + 1e-5
    em.close()


# ---------------------------------------------------------------------------------------------------------------- 7. captured graphs
def test_small_m_captured_graphs_equal_eager_forwards():
    import torch
    model, tok = _peaked_tiny_bert(torch.bfloat16, 4)
    kw = dict(embedding_model_dtype="bf16", embedding_fused_small_m=True, embedding_query_cache=0)      # (every call a forward)
    em, eager = _make(model, tok, **kw), _make(model, tok, embedding_hip_graphs=0, **kw)
    assert em.encoder_path == eager.encoder_path == "hip-fused-layers" and em.small_m_rows == 96
    queries = ["midnight", "she was good and pious " * 5, "she was good and pious " * 12]              # three query lengths
    seen = _count_route(eager)
    want = [eager.batch_encode(q) for q in queries]
    assert len(seen) == 3 and not eager._fused._graphs
    for rep in range(3):                                   # rep 0 eager, rep 1 captures, rep 2 replays
        for q, w in zip(queries, want):
            np.testing.assert_allclose(em.batch_encode(q), w, atol=2e-6)
    shapes = set(em._fused._graphs)
    assert 1 <= len(shapes) <= len(queries) and all(key[1] % 16 == 0 for key in shapes)
    em.close(); eager.close()


# ---------------------------------------------------------------------------------------------------------------- 8. no GEMM, no GELU kernel
def test_small_m_forward_launches_no_library_gemm_and_no_gelu_kernel():
    """The kernel list of one forward under the row limit, taken with torch's profiler (as test_fused_forward_launches_no_gelu_kernel does):
    the flag-off list names hipBLASLt / Tensile GEMMs (Cijk_...) and PyTorch's GELU kernel, the flag-on list names neither."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    model, _ = _peaked_tiny_bert(torch.bfloat16, 4)
    model = model.to("cuda", dtype=torch.bfloat16).eval()
    ids = torch.randint(0, model.config.vocab_size, (2, 48), device="cuda")                            # 96 token rows
    lens = np.array([48, 17], np.int32)
    names = {}
    for flag in (False, True):
        fz = FusedBertLayers(model, small_m=flag)
        fz(ids, lens, pool=True); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fz(ids, lens, pool=True); torch.cuda.synchronize()
        names[flag] = [e.key for e in prof.key_averages()]
        print(flag, names[flag])
    is_gemm = lambda n: "Cijk" in n or "gemm" in n.lower()
    is_gelu = lambda n: "gelu" in n.lower()
    assert any(is_gemm(n) for n in names[False]) and any(is_gelu(n) for n in names[False]), names[False]
    assert not any(is_gemm(n) or is_gelu(n) for n in names[True]), names[True]
    assert any("small_linear_kernel" in n for n in names[True]) and any("add_ln_partials_kernel" in n for n in names[True]), names[True]
