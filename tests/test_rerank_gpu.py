"""CrossEncoderReranker (comorag_amd/rerank.py) on the GPU: logits of the fused forward — whole stack + head, and the CLS-only last layer —
against the fp32 oracle and the transformers forward of the same model in the same dtype; ranking, the rerank call shape, determinism,
fallbacks and the config-5 flow.  Models and pairs: tests/reranker_probes.py (seed-initialised; no bge-reranker weights exist offline)."""
import copy
import functools

import numpy as np
import pytest

from tests import reranker_probes as rp

pytestmark = pytest.mark.gpu

MAX_LEN = 128
STEP = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}             # one 16-bit rounding step, relative: the CLS row that feeds the head


def _cfg(dtype, **kw):
    from comorag_amd.utils.config_utils import BaseConfig
    return BaseConfig(rerank_model_dtype={"bfloat16": "bf16", "float16": "f16", "float32": "auto"}[dtype], rerank_batch_size=8, rerank_max_seq_len=MAX_LEN,
                      embedding_fused_fp32=dtype == "float32", **kw)


def _reranker(kind, dtype, **kw):
    from comorag_amd.rerank import CrossEncoderReranker
    model, tok = _model(kind, dtype)
    return CrossEncoderReranker(_cfg(dtype, **kw), model=copy.deepcopy(model), tokenizer=tok)


@functools.lru_cache(maxsize=None)
def _model(kind, dtype):
    import torch
    return rp.make_cross_encoder(kind, None if dtype == "float32" else getattr(torch, dtype))


@functools.lru_cache(maxsize=None)
def _oracle(kind, dtype, single_query=False):
    """(pairs, want, plain): `want` the forward one precision up on the CPU — fp32 arithmetic on the 16-bit-representable weights, fp64 for the
    fp32 model — and `plain` the transformers forward in the model's own dtype on the GPU; float64 arrays, computed once per module."""
    import torch
    model, tok = _model(kind, dtype)
    pairs = rp.make_pairs()
    if single_query:
        pairs = [(pairs[0][0], p) for _, p in pairs]
    ids, types = rp.tokenize(tok, pairs, MAX_LEN)
    assert len({tuple(r) for r in ids}) == len(ids) and min(len(r) for r in ids) < 16 and max(len(r) for r in ids) == MAX_LEN
    pad = int(model.config.pad_token_id or 0)
    if dtype == "float32":
        want = rp.reference_logits(copy.deepcopy(model).double(), ids, types, pad)
        plain = rp.reference_logits(copy.deepcopy(model).cuda(), ids, types, pad)
    else:
        want = rp.reference_logits(model, ids, types, pad)
        plain = rp.reference_logits(copy.deepcopy(model).to("cuda", dtype=getattr(torch, dtype)), ids, types, pad)
    return pairs, want, plain


def _bound(dtype, want, plain):
    """The logit bar: 2 max|plain - want| + one 16-bit step of the largest logit (the bar of test_fused_layer_stack_vs_transformers_forward_and_oracle
    plus the rounding of the CLS row); fp32: 4 e_ref + 4 ulp32(max|want|), the protocol of tests/test_encoder_fp32_gpu.py."""
    e_ref = float(np.abs(plain - want).max())
    if dtype == "float32":
        return 4.0 * e_ref + 4.0 * float(np.spacing(np.float32(np.abs(want).max())))
    return 2.0 * e_ref + STEP[dtype] * float(np.abs(want).max())


def _assert_logits(got, kind, dtype, what, single_query=False):
    _, want, plain = _oracle(kind, dtype, single_query)
    bound, e_got = _bound(dtype, want, plain), float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: max|got - want| {e_got:.3e}  max|plain - want| {float(np.abs(plain - want).max()):.3e}  bound {bound:.3e}  std(want) {want.std():.3f}")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert e_got <= bound, (what, e_got, bound)
    return bound


@pytest.mark.parametrize("cls_tail", [True, False])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float32"])
@pytest.mark.parametrize("kind", ["bert", "xlmr"])
def test_logits_vs_oracle_and_transformers_forward(kind, dtype, cls_tail):
    r = _reranker(kind, dtype, rerank_cls_tail=cls_tail)
    assert r.reranker_path == ("hip-fused-layers (cls tail)" if cls_tail else "hip-fused-layers")
    pairs, _, _ = _oracle(kind, dtype)
    got = r.score_pairs([q for q, _ in pairs], [p for _, p in pairs])
    _assert_logits(got, kind, dtype, f"{kind} {dtype} cls_tail {cls_tail}")
    assert np.array_equal(got, r.score_pairs([q for q, _ in pairs], [p for _, p in pairs]))           # the same call twice: identical bits


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("kind", ["bert", "xlmr"])
def test_cls_tail_on_the_small_m_route(kind, dtype):
    """embedding_fused_small_m armed: the tail's b CLS rows (8 <= 96) run the small-M linear kernels, as `_layers` would route 8 token rows."""
    r = _reranker(kind, dtype, rerank_cls_tail=True, embedding_fused_small_m=True)
    assert r._fused.small_m_rows > 0
    pairs, _, _ = _oracle(kind, dtype)
    _, want, plain = _oracle(kind, dtype)
    bound = _assert_logits(r.score_pairs([q for q, _ in pairs], [p for _, p in pairs]), kind, dtype, f"{kind} {dtype} cls_tail small-M")
    alone = r.score_pairs([pairs[0][0]], [pairs[0][1]])                   # 16 token rows: the layers in front of the tail take the short-row route too
    print(f"pair 0 alone, short-row route: |got - want| {abs(float(alone[0]) - want[0]):.3e}  bound {bound:.3e}")
    assert abs(float(alone[0]) - want[0]) <= bound


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("kind", ["bert", "xlmr"])
def test_rerank_order_and_call_shape(kind, dtype):
    """One query against the 25 passages.  rerank() may invert two candidates only if their oracle logits differ by less than twice the logit
    bound; at least half of all candidate pairs are decided by that criterion (bf16 deviates too much against this spread to decide most)."""
    r = _reranker(kind, dtype, rerank_cls_tail=True)
    pairs, want, plain = _oracle(kind, dtype, True)
    query, passages = pairs[0][0], [p for _, p in pairs]
    scores = r.score_pairs(query, passages)
    bound = _assert_logits(scores, kind, dtype, f"{kind} {dtype} one query", True)
    gap = np.abs(want[:, None] - want[None, :])[np.triu_indices(len(want), 1)]
    decided = float((gap >= 2.0 * bound).mean())
    print(f"decided candidate pairs: {decided:.2f}")
    assert decided >= 0.5
    cand = list(range(100, 100 + len(passages)))
    idx, items, info = r.rerank(query, passages, cand)
    assert sorted(idx) == cand and items == [passages[i - 100] for i in idx]
    conf = np.asarray(info["confidence"], np.float32)
    assert np.array_equal(conf, scores[[i - 100 for i in idx]]) and np.all(conf[:-1] >= conf[1:])
    order = [i - 100 for i in idx]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            assert want[order[b]] - want[order[a]] < 2.0 * bound, (order[a], order[b])                # an inversion only inside the bound
    # the call shape
    assert r.rerank(query, [], []) == ([], [], {"confidence": []})
    top = r.rerank(query, passages, cand, len_after_rerank=5)
    assert top[0] == idx[:5] and top[1] == items[:5] and top[2]["confidence"] == info["confidence"][:5]
    tup = [(f"key{i}", p) for i, p in enumerate(passages)]
    t_idx, t_items, t_info = r(query, tup, cand)
    assert t_idx == idx and t_items == [tup[i - 100] for i in idx] and t_info == info                # tuple items: their last element is the passage
    rep = r.rerank(query, passages[:3] + passages[:2], [7, 8, 9, 8, 7])
    assert sorted(rep[0]) == [7, 8, 9] and len(rep[1]) == 3                                           # a repeated index keeps its first position
    sig = r.score_pairs(query, passages, normalize=True)
    assert sig.dtype == np.float32 and np.array_equal(sig, (np.float32(1) / (np.float32(1) + np.exp(-scores, dtype=np.float32))).astype(np.float32))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_a_pair_alone_in_the_batch_and_without_bucketing(dtype):
    """Every way of batching a pair stays inside the logit bound (no bit equality across mini-batch shapes: hipBLASLt picks kernels by M)."""
    kind = "xlmr"
    pairs, want, plain = _oracle(kind, dtype)
    bound = _bound(dtype, want, plain)
    r = _reranker(kind, dtype, rerank_cls_tail=True)
    for i in (0, 1, 7):
        alone = r.score_pairs([pairs[i][0]], [pairs[i][1]])
        print(f"pair {i} alone: |got - want| {abs(float(alone[0]) - want[i]):.3e}  bound {bound:.3e}")
        assert alone.shape == (1,) and abs(float(alone[0]) - want[i]) <= bound
    flat = _reranker(kind, dtype, rerank_cls_tail=True, embedding_length_bucketing=False)
    _assert_logits(flat.score_pairs([q for q, _ in pairs], [p for _, p in pairs]), kind, dtype, f"{kind} {dtype} bucketing off")


def test_models_the_stack_declines_score_through_transformers():
    import torch
    from comorag_amd.rerank import CrossEncoderReranker
    from comorag_amd.utils.config_utils import BaseConfig
    pairs = rp.make_pairs(9)
    for kind, over, reason, col in (("xlmr", {"num_labels": 2}, "num_labels = 2", 1), ("bert", {"position_embedding_type": "relative_key"}, "relative position", 0)):
        model, tok = rp.make_cross_encoder(kind, None, **over)
        r = CrossEncoderReranker(BaseConfig(rerank_model_dtype="auto", rerank_batch_size=4, rerank_max_seq_len=MAX_LEN, embedding_fused_fp32=True),
                                 model=copy.deepcopy(model), tokenizer=tok)
        assert r.reranker_path.startswith("transformers (") and reason in r.reranker_path
        got = r.score_pairs([q for q, _ in pairs], [p for _, p in pairs])
        ids, types = rp.tokenize(tok, pairs, MAX_LEN)
        with torch.no_grad():                               # pair by pair, unpadded, fp32 on the CPU
            want = np.asarray([float(model(input_ids=torch.tensor([ids[i]]), **({"token_type_ids": torch.tensor([types[i]])} if types else {})).logits[0, col])
                               for i in range(len(ids))])
        np.testing.assert_allclose(got, want, atol=2e-5)    # two fp32 evaluations of one forward (logits of size ~1)


def test_search_then_cross_score_on_a_dense_index():
    from comorag_amd.index import DenseIndex
    from comorag_amd.rerank import search_then_cross_score
    r = _reranker("xlmr", "float16", rerank_cls_tail=True)
    rng = np.random.default_rng(5)
    texts = [" ".join(rng.choice(rp.WORDS, size=int(rng.integers(2, 40)))) for _ in range(40)]
    rows = rng.standard_normal((40, 64)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rows[3] + 0.3 * rng.standard_normal(64).astype(np.float32)
    idx = DenseIndex(64, "bf16")
    idx.append(rows)
    query = "who was the prince"
    ids, sc = search_then_cross_score(idx, texts, r, query, q, k_candidates=10, k=4)
    cand = [int(c) for c in idx.search(q.reshape(1, -1), 10, with_minmax=False)[0][0]]
    idx.close()
    assert ids.shape == (4,) and sc.shape == (4,) and sc.dtype == np.float32 and set(ids.tolist()) <= set(cand) and len(set(ids.tolist())) == 4
    full = r.score_pairs(query, [texts[c] for c in cand])                                             # the same call: the same bits
    order = sorted(range(10), key=lambda p: (-float(full[p]), p))[:4]
    assert ids.tolist() == [cand[p] for p in order] and np.array_equal(sc, full[order])
