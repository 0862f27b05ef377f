"""Concurrent one-question encodes combined into one forward (config `embedding_combine`) on the device: the many-row linear
entry points (cmr_encoder_linear_rows / _rows_partials: small_linear_kernel over row tiles of 128), the explicit many-row route of the
layer stack (`forward_ragged(..., rows_route=True)`) and the combining queue of HipBGEEmbeddingModel.

The acceptance property is EQUALITY: a row of a many-row call has the bits cmr_encoder_linear_small(_partials) gives it in any call that
contains it, a sequence of a many-row forward the bits of its own [1, l] forward, a combined caller the bits of its solo call — every
comparison below is torch.equal / np.array_equal.  The one tolerance (a row against the fp32 oracle) is the small-M stack test's.

Every wait on another thread has a timeout and the test fails when it passes.  Batches that form under a long gather window are filled
exactly, so nobody waits a window out.  Not reachable, hence not tested: a prompt that is empty after tokenisation (the tokenizer adds
[CLS] / [SEP] and batch_encode the BGE prefix); such a call would take the padded path as it does with the option off."""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIMEOUT = 120.0
LONG_US = 2_000_000      # a gather window long enough that a batch of 16 forms by construction, not by a race
MS = [129, 256, 272, 1000]


class _Stages:
    """FusedBertLayers' kernel wrappers without a model around them."""
    def __init__(self, dtype, eps=1e-12):
        import torch
        from comorag_amd import _lib as L
        from comorag_amd.embedding_model.fused_bert import FusedBertLayers
        self.dtype, self.eps = dtype, eps
        self.cmr_dtype = {torch.bfloat16: L.CMR_BF16, torch.float16: L.CMR_F16}[dtype]
        for name in ("linear_small", "linear_small_partials", "linear_rows", "linear_rows_partials", "add_layernorm_partials"):
            setattr(self, name, getattr(FusedBertLayers, name).__get__(self))


def _inputs(n, k, dtype, rows=1000, scale=1.0, seed=0):
    import torch
    g = torch.Generator(device="cuda").manual_seed(n * 7 + k + seed)
    tdt = getattr(torch, dtype)
    x = (torch.randn((rows, k), generator=g, device="cuda") * scale).to(tdt)
    w = (torch.randn((n, k), generator=g, device="cuda") / k ** 0.5).to(tdt)
    bias = torch.randn((n,), generator=g, device="cuda").to(tdt)
    return x, w, bias


def _slices(m):
    """[r0, r0 + mq), mq <= 128: the first tile, one that straddles a 128-row boundary, the last (partial) tile, the tail row, and a short
    slice that ends at m from inside the tile before."""
    last0 = (m - 1) // 128 * 128
    out = {(0, 128), (120, 80) if m >= 200 else (120, m - 120), (last0, m - last0), (m - 1, 1), (max(0, m - 17), min(17, m))}
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- 1. kernel bits
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("nk,act", [((48, 96), 0), ((48, 96), 1), ((2304, 768), 0), ((2304, 768), 1)])
def test_direct_form_rows_have_the_bits_of_the_one_query_kernel(nk, act, dtype):
    import torch
    n, k = nk
    x, w, bias = _inputs(n, k, dtype, scale=1.5 if act else 1.0)
    fz = _Stages(getattr(torch, dtype))
    solo = {}                                                          # (r0, mq) -> linear_small of that slice: computed once
    for m in MS:
        got = fz.linear_rows(x[:m].contiguous(), w, bias, bool(act))
        assert got.dtype == x.dtype and got.shape == (m, n)
        assert torch.isfinite(got.float()).all()
        for r0, mq in _slices(m):
            if (r0, mq) not in solo:
                solo[(r0, mq)] = fz.linear_small(x[r0:r0 + mq].contiguous(), w, bias, bool(act))
            assert torch.equal(got[r0:r0 + mq], solo[(r0, mq)]), (m, r0, mq)
        assert torch.equal(got, fz.linear_rows(x[:m].contiguous(), w, bias, bool(act)))                 # two runs
        other = x[:m].clone()
        other[1:] = torch.flip(other[1:], dims=[0]) * 3.0                                              # row 0 kept, every other row other data
        assert torch.equal(fz.linear_rows(other, w, bias, bool(act))[0], got[0])
    nb = fz.linear_rows(x[:272].contiguous(), w, None, bool(act))                                       # no bias
    assert torch.equal(nb[120:200], fz.linear_small(x[120:200].contiguous(), w, None, bool(act)))
    small = fz.linear_rows(x[:80].contiguous(), w, bias, bool(act))                                     # m <= 128: the one-query instantiations
    assert torch.equal(small, fz.linear_small(x[:80].contiguous(), w, bias, bool(act)))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("nk", [(384, 1536), (768, 3072)])
def test_partials_form_rows_have_the_bits_of_the_one_query_kernel(nk, dtype):
    import torch
    n, k = nk
    tdt = getattr(torch, dtype)
    x, w, bias = _inputs(n, k, dtype, seed=1)
    g = torch.Generator(device="cuda").manual_seed(n + k)
    res = torch.randn((1000, n), generator=g, device="cuda").to(tdt)
    gamma = (1 + 0.2 * torch.randn((n,), generator=g, device="cuda")).to(tdt)
    beta = (0.1 * torch.randn((n,), generator=g, device="cuda")).to(tdt)
    fz = _Stages(tdt)
    solo = {}
    for m in MS:
        part = fz.linear_rows_partials(x[:m].contiguous(), w)
        assert part.dtype == torch.float32 and part.shape[1:] == (m, n) and torch.isfinite(part).all()
        ln = fz.add_layernorm_partials(part, bias, res[:m].contiguous(), gamma, beta)
        for r0, mq in _slices(m):
            if (r0, mq) not in solo:
                p = fz.linear_small_partials(x[r0:r0 + mq].contiguous(), w)
                solo[(r0, mq)] = (p, fz.add_layernorm_partials(p, bias, res[r0:r0 + mq].contiguous(), gamma, beta))
            p, want_ln = solo[(r0, mq)]
            assert p.shape[0] == part.shape[0]                                                         # the same K split
            assert torch.equal(part[:, r0:r0 + mq], p), (m, r0, mq)                                    # slab for slab
            assert torch.equal(ln[r0:r0 + mq], want_ln), (m, r0, mq)                                   # and what the LayerNorm launch makes of them
        assert torch.equal(part, fz.linear_rows_partials(x[:m].contiguous(), w))
        other = x[:m].clone()
        other[1:] = torch.flip(other[1:], dims=[0]) * 3.0
        assert torch.equal(fz.linear_rows_partials(other, w)[:, 0], part[:, 0])


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_return_the_documented_error_and_launch_nothing():
    import torch
    from comorag_amd import _lib as L
    lib = L.lib()
    rows_max = L.CMR_ENCODER_ROWS_MAX
    x = torch.ones((rows_max + 8, 64), device="cuda", dtype=torch.bfloat16)
    w = torch.ones((64, 64), device="cuda", dtype=torch.bfloat16)
    bias = torch.ones((64,), device="cuda", dtype=torch.bfloat16)
    out = torch.full((rows_max + 8, 64), 7.0, device="cuda", dtype=torch.bfloat16)
    part = torch.full(((rows_max + 8) * 64,), 7.0, device="cuda", dtype=torch.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def direct(m=272, n=64, k=64, dt=L.CMR_BF16, xp=None, act=0):
        return lib.cmr_encoder_linear_rows(0, P(x) if xp is None else xp, P(w), P(bias), m, n, k, dt, act, P(out), st)

    def partials(m=272, n=64, k=64, dt=L.CMR_BF16, xp=None):
        return lib.cmr_encoder_linear_rows_partials(0, P(x) if xp is None else xp, P(w), m, n, k, dt, P(part), st)

    for call in (direct, partials):
        assert call(m=0) == L.CMR_ERR_INVALID and call(n=-16) == L.CMR_ERR_INVALID and call(k=0) == L.CMR_ERR_INVALID
        assert call(m=rows_max + 1) == L.CMR_ERR_UNSUPPORTED and b"2048" in lib.cmr_last_error()
        assert call(k=48) == L.CMR_ERR_UNSUPPORTED
        assert call(n=40) == L.CMR_ERR_UNSUPPORTED
        assert call(dt=L.CMR_F32) == L.CMR_ERR_UNSUPPORTED and b"16-bit" in lib.cmr_last_error()
        assert call(dt=7) == L.CMR_ERR_INVALID
        assert call(xp=P(x, 8)) == L.CMR_ERR_UNSUPPORTED and b"aligned" in lib.cmr_last_error()
        assert call(xp=C.c_void_p(0)) == L.CMR_ERR_INVALID
    assert direct(act=2) == L.CMR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((part == 7.0).all())                       # nothing was launched
    assert direct() == L.CMR_OK and partials() == L.CMR_OK                              # and the same buffers are fine when the arguments are
    assert direct(m=rows_max) == L.CMR_OK                                               # the limit itself
    torch.cuda.synchronize()
    assert bool((out[:rows_max] == 65.0).all()) and bool((out[rows_max:] == 7.0).all())  # 64 ones + bias; no row behind m was written
    assert bool((part[:272 * 64] == 64.0).all()) and bool((part[272 * 64:] == 7.0).all())
    # the one-query entry points keep their limit
    assert lib.cmr_encoder_linear_small(0, P(x), P(w), P(bias), 129, 64, 64, L.CMR_BF16, 0, P(out), st) == L.CMR_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- 3. the stack
def _peaked_tiny_bert(dtype, heads):
    """tests/test_encoder_small_m_gpu.py's toy model: hidden 256, 3 layers, 4 heads of 64 or 8 heads of 32, peaked attention."""
    import torch
    from oracle import encode_torch as enc
    model, tok = enc.tiny_bert(hidden=256, layers=3, heads=heads, inter=512, max_pos=128)
    with torch.no_grad():
        for lyr in model.encoder.layer:
            lyr.attention.self.query.weight.mul_(12.0)
            lyr.attention.self.key.weight.mul_(12.0)
        model.to(dtype).float()
    return model, tok


def _packed(seqs):
    b = len(seqs)
    head = np.empty(2 * b + 1, dtype=np.int32)
    head[:b] = [len(s) for s in seqs]
    head[b] = 0
    np.cumsum(head[:b], out=head[b + 1:])
    return np.concatenate([head, *seqs])


def _count(fz, name):
    seen, inner = [], getattr(fz, name)
    def spy(x, lens_dev, b, l, pool, stream):
        seen.append(b * l)
        return inner(x, lens_dev, b, l, pool, stream)
    setattr(fz, name, spy)
    return seen


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("heads", [4, 8])
def test_rows_route_gives_every_sequence_the_bits_of_its_solo_forward(heads, dtype):
    import torch
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    tdt = getattr(torch, dtype)
    model, _ = _peaked_tiny_bert(tdt, heads)
    model = copy.deepcopy(model).to("cuda", dtype=tdt).eval()
    fz = FusedBertLayers(model, graphs=0, head32=heads == 8, small_m=True)
    assert fz.small_m_rows == 96 and fz.head_dim == 256 // heads
    rows_calls, small_calls = _count(fz, "_layers_rows"), _count(fz, "_layers_small_m")
    rng = np.random.default_rng(heads * 100 + len(dtype))
    vocab = int(model.config.vocab_size)
    for l in (16, 48, 96):
        # sixteen sequences of mixed true lengths that share the padded width l: a full one, the shortest the width admits, a one-token one
        # (what a filler sequence is) where the width is 16
        lens = [l, l - 15] + [int(v) for v in rng.integers(l - 15, l + 1, size=14)]
        if l == 16:
            lens[2] = 1
        seqs = [rng.integers(5, vocab, size=n).astype(np.int32) for n in lens]
        for normalize in (True, False):
            solo = [fz.forward_ragged(_packed([s]), 1, l, normalize) for s in seqs]
            assert all(r.shape == (1, 256) and r.dtype == torch.float32 for r in solo)
            for b in (2, 5, 16):
                n_rows, n_small = len(rows_calls), len(small_calls)
                got = fz.forward_ragged(_packed(seqs[:b]), b, l, normalize, rows_route=True)
                assert len(rows_calls) == n_rows + 1 and rows_calls[-1] == b * l and len(small_calls) == n_small
                assert got.shape == (b, 256) and bool(torch.isfinite(got).all())
                for i in range(b):
                    assert torch.equal(got[i], solo[i][0]), (l, normalize, b, i)
    assert len(small_calls) == 3 * 2 * 16                          # every solo forward ran the short-row route
    # an ordinary mini-batch over the row limit never takes the many-row route by itself
    n_rows = len(rows_calls)
    fz.forward_ragged(_packed(seqs[:5]), 5, 96, True)
    assert len(rows_calls) == n_rows
    with pytest.raises(ValueError, match="rows_route"):
        fz.forward_ragged(_packed(seqs * 2), 32, 96, True, rows_route=True)                            # 3072 token rows


def test_rows_route_graphs_replay_the_eager_bits_and_share_no_graph_with_the_library_route():
    import torch
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    model, _ = _peaked_tiny_bert(torch.bfloat16, 4)
    model = copy.deepcopy(model).to("cuda", dtype=torch.bfloat16).eval()
    eager, graphed = FusedBertLayers(model, graphs=0, small_m=True), FusedBertLayers(model, graphs=4, small_m=True)
    rng = np.random.default_rng(7)
    b, l = 5, 48
    batches = [[rng.integers(5, int(model.config.vocab_size), size=int(n)).astype(np.int32) for n in rng.integers(l - 15, l + 1, size=b)] for _ in range(3)]
    for rep, seqs in enumerate(batches):                   # rep 0 eager, rep 1 captures, rep 2 replays — other data every time
        want = eager.forward_ragged(_packed(seqs), b, l, True, rows_route=True)
        got = graphed.forward_ragged(_packed(seqs), b, l, True, rows_route=True)
        assert torch.equal(got, want), rep
        lib_got = graphed.forward_ragged(_packed(seqs), b, l, True)      # the same shape without the flag: hipBLASLt, a graph of its own
        assert lib_got.shape == want.shape and bool(torch.isfinite(lib_got).all())
    assert set(graphed._graphs) == {(b, l, "ragged-rows", True), (b, l, "ragged", True)}
    graphed.release()


# ---------------------------------------------------------------------------------------------------------------- 4. end to end
_WORDS = "the a an and of to in she he it her his was were had be good pious mother grave snow spring prince".split()


def _make(model, tok, **kw):
    from comorag_amd.embedding_model import _get_embedding_model_class
    from comorag_amd.utils.config_utils import BaseConfig
    cfg = BaseConfig(embedding_model_name="bge-tiny-random", embedding_batch_size=8, embedding_max_seq_len=128, embedding_query_cache=0, **kw)
    return _get_embedding_model_class("bge-tiny-random")(global_config=cfg, embedding_model_name=cfg.embedding_model_name, model=copy.deepcopy(model), tokenizer=tok)


def _prompts_of_one_width(em, count, extra_words=0):
    """`count` distinct short questions whose prompts (BGE prefix + text) share one padded width under the short-row limit: two words
    that differ from question to question and `extra_words` more (every word is one token of the toy vocabulary)."""
    from comorag_amd.embedding_model.bge import BGE_PREFIX
    tail = "".join(" " + _WORDS[i % len(_WORDS)] for i in range(extra_words))
    texts = [f"{a} {b}{tail}" for a in _WORDS for b in _WORDS][:count]
    widths = {-(-len(ids) // 16) * 16 for ids in em._ragged([BGE_PREFIX + t for t in texts], 128)}
    assert len(texts) == count and len(set(texts)) == count and len(widths) == 1, widths
    assert widths.pop() <= em.small_m_rows
    return texts


def _threads(fns):
    """Every fn on a thread of its own, released by one barrier; results or exceptions in call order."""
    out, bar = [None] * len(fns), threading.Barrier(len(fns))
    def body(i):
        try:
            bar.wait(TIMEOUT)
            out[i] = fns[i]()
        except Exception as e:
            out[i] = e
    ts = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(fns))]
    for t in ts: t.start()
    for t in ts:
        t.join(TIMEOUT)
        assert not t.is_alive(), "deadlock: a combined encode did not return"
    return out


@pytest.mark.parametrize("dtype,heads,extra_words,width", [("bfloat16", 4, 58, 80), ("float16", 8, 20, 48)])
def test_sixteen_threads_get_the_bits_of_their_solo_encodes(dtype, heads, extra_words, width):
    import torch
    from oracle import encode_torch as enc
    model, tok = _peaked_tiny_bert(getattr(torch, dtype), heads)
    kw = dict(embedding_model_dtype=dtype, embedding_fused_head32=heads == 8, embedding_fused_small_m=True)
    em, solo = _make(model, tok, embedding_combine=16, embedding_combine_wait_us=LONG_US, **kw), _make(model, tok, **kw)
    assert em.encoder_path == solo.encoder_path == "hip-fused-layers" and em.small_m_rows == solo.small_m_rows == 96
    assert em._combiner is not None and solo._combiner is None
    assert em.combine_stats() == solo.combine_stats() == {"batches": 0, "queries": 0, "max_width": 0}
    texts = _prompts_of_one_width(em, 96, extra_words)     # 16 x 80 = 1280 token rows a batch: ten row tiles; 16 x 48 = 768: six
    want = [solo.batch_encode(t) for t in texts]           # graphs: the width's solo shape runs eagerly, is captured, then replays
    rows_calls = _count(em._fused, "_layers_rows")
    # every thread encodes its six questions one after the other: a round's sixteen calls fill a batch exactly (nobody joins the next
    # round before this one's forward has completed and its members are awake), so six batches of sixteen form by construction
    got = _threads([lambda i=i: [em.batch_encode(texts[6 * i + j]) for j in range(6)] for i in range(16)])
    for i, rows in enumerate(got):
        assert not isinstance(rows, Exception), rows
        for j, row in enumerate(rows):
            assert row.shape == (1, 256) and row.dtype == np.float32
            assert np.array_equal(row, want[6 * i + j]), (i, j, float(np.abs(row - want[6 * i + j]).max()))
    assert em.combine_stats() == {"batches": 6, "queries": 96, "max_width": 16}
    assert rows_calls and all(r == 16 * width for r in rows_calls), rows_calls
    assert any(key[2] == "ragged-rows" and key[0] == 16 for key in em._fused._graphs)                  # rounds 2.. replayed a captured forward
    oracle_row = enc.batch_encode(model, tok, [texts[17]], batch_size=8, max_length=128)
    e = float(np.abs(got[2][5] - oracle_row).max())
    print(f"{dtype} heads {heads}: combined row vs the CPU oracle: max abs error {e:.3e}")
    np.testing.assert_allclose(got[2][5], oracle_row, atol={"bfloat16": 6e-3, "float16": 1e-3}[dtype])
    em.close(); solo.close()


def test_narrow_batches_pad_with_filler_sequences_and_keys_keep_their_widths_apart():
    """Three callers of one width (b is rounded up to 4: one filler sequence) and, at the same moment, two of another width."""
    import torch
    from comorag_amd.embedding_model.bge import BGE_PREFIX
    model, tok = _peaked_tiny_bert(torch.bfloat16, 4)
    kw = dict(embedding_model_dtype="bf16", embedding_fused_small_m=True, embedding_hip_graphs=0)
    solo = _make(model, tok, **kw)
    short = _prompts_of_one_width(solo, 3)
    longer = [" ".join(_WORDS[i:i + 18]) for i in range(2)]
    w_short, w_long = ({-(-len(x) // 16) * 16 for x in solo._ragged([BGE_PREFIX + t for t in ts], 128)} for ts in (short, longer))
    assert len(w_short) == len(w_long) == 1 and w_short != w_long and max(w_long) <= 96, (w_short, w_long)
    want = [solo.batch_encode(t) for t in short + longer]
    em3 = _make(model, tok, embedding_combine=3, embedding_combine_wait_us=LONG_US, **kw)
    rows_calls = _count(em3._fused, "_layers_rows")
    got = _threads([lambda t=t: em3.batch_encode(t) for t in short])
    for g, w in zip(got, want[:3]):
        assert np.array_equal(g, w)
    assert rows_calls == [4 * max(w_short)] and em3.combine_stats() == {"batches": 1, "queries": 3, "max_width": 3}
    em3.close()
    em2 = _make(model, tok, embedding_combine=2, embedding_combine_wait_us=LONG_US, **kw)
    got = _threads([lambda t=t: em2.batch_encode(t) for t in short[:2] + longer])                       # two keys, each filled exactly
    for g, w in zip(got, want[:2] + want[3:]):
        assert np.array_equal(g, w)
    assert em2.combine_stats() == {"batches": 2, "queries": 4, "max_width": 2}
    em2.close(); solo.close()


# ---------------------------------------------------------------------------------------------------------------- 5. not combined
def test_lists_wide_prompts_and_an_unarmed_model_take_todays_path():
    import torch
    model, tok = _peaked_tiny_bert(torch.bfloat16, 4)
    kw = dict(embedding_model_dtype="bf16")
    off = _make(model, tok, embedding_fused_small_m=True, **kw)
    on = _make(model, tok, embedding_fused_small_m=True, embedding_combine=16, embedding_combine_wait_us=LONG_US, **kw)
    unarmed = _make(model, tok, embedding_combine=16, embedding_combine_wait_us=LONG_US, **kw)          # embedding_fused_small_m = False
    off_flagless = _make(model, tok, **kw)
    assert on._combiner is not None and unarmed._combiner is None and unarmed.small_m_rows == 0
    zero = {"batches": 0, "queries": 0, "max_width": 0}
    three = ["midnight", "the prince and the golden slipper", "she was good and pious"]
    wide = "she was good and pious and the bird sang " * 8                                             # 109 tokens with the prefix: wider than the 96-row limit
    assert np.array_equal(on.batch_encode(three), off.batch_encode(three))                              # a list never queues
    assert np.array_equal(on.batch_encode(wide), off.batch_encode(wide))                                # nor a prompt over the short-row limit
    dev = on.batch_encode_dev("midnight")                                                              # nor rows that stay on the device
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), off.batch_encode("midnight"))
    assert on.combine_stats() == zero                                                                  # (none of them waited the window out either)
    assert np.array_equal(unarmed.batch_encode("midnight"), off_flagless.batch_encode("midnight"))
    assert np.array_equal(unarmed.batch_encode(three), off_flagless.batch_encode(three))
    assert unarmed.combine_stats() == zero
    for bad in (1, 17):
        with pytest.raises(ValueError, match="embedding_combine"):
            _make(model, tok, embedding_fused_small_m=True, embedding_combine=bad, **kw)
    for em in (off, on, unarmed, off_flagless):
        em.close()


# ---------------------------------------------------------------------------------------------------------------- 6. error paths
def test_a_raising_forward_reaches_its_own_batch_and_the_next_call_works():
    import torch
    model, tok = _peaked_tiny_bert(torch.bfloat16, 4)
    kw = dict(embedding_model_dtype="bf16", embedding_fused_small_m=True)
    em, solo = _make(model, tok, embedding_combine=2, embedding_combine_wait_us=LONG_US, **kw), _make(model, tok, **kw)
    texts = _prompts_of_one_width(em, 4)
    want = [solo.batch_encode(t) for t in texts]
    inner, fail = em._fused.forward_ragged, {"next": True}
    def raising(packed, b, l, normalize=True, rows_route=False):
        if rows_route and fail["next"]:
            fail["next"] = False
            raise RuntimeError("injected: the combined forward failed")
        return inner(packed, b, l, normalize, rows_route=rows_route)
    em._fused.forward_ragged = raising
    got = _threads([lambda t=t: em.batch_encode(t) for t in texts[:2]])
    assert all(isinstance(g, RuntimeError) and "injected" in str(g) for g in got), got                  # leader and member alike
    assert em._combiner.waiting() == 0 and not em._combiner._slots
    got = _threads([lambda t=t: em.batch_encode(t) for t in texts[2:]])                                 # the next batch of the same key works
    for g, w in zip(got, want[2:]):
        assert np.array_equal(g, w)
    got = _threads([lambda t=t: em.batch_encode(t) for t in texts[:2]])                                 # and so do the callers that failed
    for g, w in zip(got, want[:2]):
        assert np.array_equal(g, w)
    assert em.combine_stats() == {"batches": 3, "queries": 6, "max_width": 2}
    em.close(); solo.close()
