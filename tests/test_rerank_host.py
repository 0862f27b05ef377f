"""Host tier of the cross-encoder reranker (comorag_amd/rerank.py): model surgery and its refusals, pair packing and truncation, the length
buckets and the scatter back, the rerank triple and its tie rule (with a fake scorer in place of the forward), and the two new entry
points' argument checks — none of it needs a device."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd import rerank as rr
from tests import reranker_probes as rp


def test_head_extraction_for_both_architectures():
    import torch
    for kind in ("bert", "xlmr"):
        model, _ = rp.make_cross_encoder(kind, torch.bfloat16, layers=1)
        model.to(torch.bfloat16)
        base, head, reason = rr.cross_encoder_parts(model)
        assert reason is None
        dense, out = head
        if kind == "bert":
            assert base is model.bert and dense is model.bert.pooler.dense and out is model.classifier
        else:
            assert base is model.roberta and dense is model.classifier.dense and out is model.classifier.out_proj
        assert tuple(dense.weight.shape) == (256, 256) and tuple(out.weight.shape) == (1, 256)
        # the head IS the model's own map from the CLS row to the logit
        x = torch.randn(3, 5, 256)
        with torch.no_grad():
            m32 = model.float()
            want = (m32.classifier(m32.bert.pooler(x)) if kind == "bert" else m32.classifier(x))[:, 0]
            got = torch.tanh(x[:, 0] @ dense.weight.t() + dense.bias) @ out.weight[0] + out.bias[0]
        np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-6)


def test_refusal_reasons():
    import torch
    two, _ = rp.make_cross_encoder("xlmr", torch.bfloat16, num_labels=2, layers=1)
    assert "num_labels = 2" in rr.cross_encoder_parts(two.to(torch.bfloat16))[2]
    rel, _ = rp.make_cross_encoder("bert", torch.bfloat16, layers=1, position_embedding_type="relative_key")
    assert rr.cross_encoder_parts(rel.to(torch.bfloat16))[2] == "relative position embeddings"
    f32, _ = rp.make_cross_encoder("bert", None, layers=1)
    assert "float32" in rr.cross_encoder_parts(f32)[2]
    assert rr.cross_encoder_parts(f32, fp32=True)[2] is None                                        # the opt-in of embedding_fused_fp32
    assert rr.cross_encoder_parts(f32.bert, fp32=True)[2] == "unexpected classification head layout"      # a bare encoder: no head to take
    assert rr.cross_encoder_parts(object())[2] == "not a BERT / RoBERTa / XLM-R sequence classifier"


def test_max_length_is_clamped_to_the_models_positions():
    import torch
    bert, _ = rp.make_cross_encoder("bert", torch.bfloat16, layers=1)
    xlmr, _ = rp.make_cross_encoder("xlmr", torch.bfloat16, layers=1)
    assert rr.pair_max_length(bert.config, 512) == 128 and rr.pair_max_length(bert.config, 64) == 64
    assert rr.pair_max_length(xlmr.config, 512) == 512 and rr.pair_max_length(xlmr.config, 8192) == 514 - 1 - 1      # max_position_embeddings - padding_idx - 1


def _bare(tok, config, max_length, batch_size=4, bucket=True):
    """A CrossEncoderReranker without a device: its host half around a fake forward."""
    r = object.__new__(rr.CrossEncoderReranker)
    r.tokenizer, r.max_length, r.batch_size, r._bucket = tok, max_length, batch_size, bucket
    r.pad_id, r._has_types = int(config.pad_token_id or 0), int(config.type_vocab_size) > 1
    r.batches = []

    def fake(ids, types):                                   # score = a function of the pair's own tokens: checks the scatter back
        r.batches.append([len(x) for x in ids])
        arr, tt, lens = rr.pad_pairs(ids, types, r.pad_id)
        assert arr.shape[1] % 16 == 0 and (tt is None) == (types is None)
        return np.asarray([float(sum(x) % 977) + len(x) / 1000.0 for x in ids], np.float32)
    r._score_batch = fake
    return r


@pytest.mark.parametrize("kind", ["bert", "xlmr"])
def test_pair_packing_truncation_buckets_and_scatter(kind):
    import torch
    model, tok = rp.make_cross_encoder(kind, torch.bfloat16, layers=1)
    pairs = rp.make_pairs(13)
    r = _bare(tok, model.config, rr.pair_max_length(model.config, 96))
    ids, types = r.tokenize_pairs([q for q, _ in pairs], [p for _, p in pairs])
    lens = [len(x) for x in ids]
    assert max(lens) == 96 and min(lens) < 16 and len({tuple(x) for x in ids}) == len(ids)          # the long passage was truncated
    if kind == "bert":
        assert ids[0][0] == 2 and ids[0][-1] == 3 and ids[0].count(3) == 2                            # [CLS] A [SEP] B [SEP]
        assert types is not None and types[0][0] == 0 and types[0][-1] == 1 and all(len(t) == len(x) for t, x in zip(types, ids))
        first_sep = ids[0].index(3)
        assert set(types[0][:first_sep + 1]) == {0} and set(types[0][first_sep + 1:]) == {1}
    else:
        assert types is None and ids[0][0] == 0 and ids[0][-1] == 2 and ids[0].count(2) == 3          # <s> A </s></s> B </s>
    arr, tt, l32 = rr.pad_pairs(ids[:3], types[:3] if types else None, r.pad_id)
    assert arr.shape == (3, 96) and list(l32) == lens[:3] and (arr[0, lens[0]:] == r.pad_id).all() and list(arr[0, :lens[0]]) == ids[0]
    want = np.asarray([float(sum(x) % 977) + len(x) / 1000.0 for x in ids], np.float32)
    got = r.score_pairs([q for q, _ in pairs], [p for _, p in pairs])
    assert got.dtype == np.float32 and np.array_equal(got, want)                                      # scattered back to arrival order
    flat = [n for bt in r.batches for n in bt]
    assert flat == sorted(lens) and [len(bt) for bt in r.batches] == [4, 4, 4, 1]                     # sorted by token count, mini-batches of 4
    r2 = _bare(tok, model.config, r.max_length, bucket=False)
    assert np.array_equal(r2.score_pairs([q for q, _ in pairs], [p for _, p in pairs]), want)
    assert [n for bt in r2.batches for n in bt] == lens                                               # arrival order
    one = r.score_pairs(pairs[5][0], [p for _, p in pairs[:2]])                                       # one query string against several passages
    assert one.shape == (2,)
    np.testing.assert_allclose(r.score_pairs(pairs[5][0], [p for _, p in pairs[:2]], normalize=True), 1.0 / (1.0 + np.exp(-one.astype(np.float64))), rtol=1e-6)
    assert r.score_pairs("x", []).shape == (0,)
    with pytest.raises(ValueError):
        r.score_pairs(["a", "b"], ["c"])


def test_length_buckets():
    b = rr.length_buckets([5, 3, 9, 3, 1], 2)
    assert [list(x) for x in b] == [[4, 1], [3, 0], [2]]                                               # stable: equal lengths keep arrival order
    assert [list(x) for x in rr.length_buckets([5, 3, 9], 2, bucketing=False)] == [[0, 1], [2]]


def test_rerank_triple_and_tie_rule_with_a_fake_scorer():
    r = object.__new__(rr.CrossEncoderReranker)
    table = {"a": 0.5, "b": 2.0, "c": 0.5, "d": -1.0, "e": 2.0}
    seen = []

    def fake(query, passages, normalize=False):
        seen.append((query, list(passages)))
        return np.asarray([table[p] for p in passages], np.float32)
    r.score_pairs = fake
    assert r.rerank("q", [], []) == ([], [], {"confidence": []}) and not seen
    items, idx = ["a", "b", "c", "d", "e"], [10, 11, 12, 13, 14]
    got = r.rerank("q", items, idx)
    assert got == ([11, 14, 10, 12, 13], ["b", "e", "a", "c", "d"], {"confidence": [2.0, 2.0, 0.5, 0.5, -1.0]})       # ties: candidate position ascending
    assert r("q", items, idx, 2) == ([11, 14], ["b", "e"], {"confidence": [2.0, 2.0]})                                  # len_after_rerank cuts
    tup = [("k1", "a"), ("k2", "b"), ("k3", "d")]
    assert r.rerank("q", tup, [7, 8, 9])[:2] == ([8, 7, 9], [("k2", "b"), ("k1", "a"), ("k3", "d")]) and seen[-1] == ("q", ["a", "b", "d"])
    assert r.rerank("q", ["a", "b", "e", "d"], [3, 4, 4, 3]) == ([4, 3], ["b", "a"], {"confidence": [2.0, 0.5]})        # a repeated index keeps its first position


def test_search_then_cross_score_with_fakes(numpy_index_cls):
    idx = numpy_index_cls(4)
    rows = np.eye(4, dtype=np.float32)[[0, 1, 2, 3, 0, 1]] * np.asarray([1, 2, 3, 4, 5, 6], np.float32)[:, None]
    idx.append(rows)
    texts = ["a", "b", "c", "d", "e", "f"]
    r = object.__new__(rr.CrossEncoderReranker)
    r.score_pairs = lambda q, ps, normalize=False: np.asarray([{"a": 1, "b": 9, "c": 3, "d": 4, "e": 5, "f": 9}[p] for p in ps], np.float32)
    ids, sc = rr.search_then_cross_score(idx, texts, r, "q", np.asarray([1, 1, 0, 0], np.float32), k_candidates=3, k=2)
    assert ids.tolist() == [5, 1] and sc.tolist() == [9.0, 9.0]            # the scan's candidates are rows 5, 4, 1; the tie keeps scan order


def test_new_entry_points_reject_bad_arguments_without_a_device():
    """NULL, shape, head_dim, dtype and alignment are checked before any device call (as tests/test_cabi.py has it for its symbols)."""
    lib = L.lib()
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 8)
    a = lib.cmr_encoder_attention_cls
    assert a(0, None, L.CMR_BF16, p, 1, 16, 1, 64, p, None) == L.CMR_ERR_INVALID and b"NULL" in lib.cmr_last_error()
    assert a(0, p, L.CMR_BF16, None, 1, 16, 1, 64, p, None) == L.CMR_ERR_INVALID
    assert a(0, p, L.CMR_BF16, p, 1, 16, 1, 64, None, None) == L.CMR_ERR_INVALID
    assert a(0, p, L.CMR_BF16, p, 1, 0, 1, 64, p, None) == L.CMR_ERR_INVALID
    assert a(0, p, L.CMR_BF16, p, 1, 16, 1, 128, p, None) == L.CMR_ERR_INVALID and b"head_dim" in lib.cmr_last_error()
    assert a(0, p, 9, p, 1, 16, 1, 64, p, None) == L.CMR_ERR_INVALID
    assert a(0, odd, L.CMR_F16, p, 1, 16, 1, 64, p, None) == L.CMR_ERR_INVALID and b"aligned" in lib.cmr_last_error()
    h = lib.cmr_encoder_cls_head
    assert h(0, None, 256, p, p, p, p, 1, 256, L.CMR_BF16, p, None) == L.CMR_ERR_INVALID
    assert h(0, p, 256, p, None, None, None, 1, 256, L.CMR_BF16, p, None) == L.CMR_ERR_INVALID          # w2 is not optional, the biases are
    assert h(0, p, 256, p, p, p, p, 0, 256, L.CMR_BF16, p, None) == L.CMR_ERR_INVALID
    assert h(0, p, 255, p, p, p, p, 1, 256, L.CMR_BF16, p, None) == L.CMR_ERR_INVALID
    assert h(0, p, 256, p, p, p, p, 1, 256, 9, p, None) == L.CMR_ERR_INVALID
    for d in (2050, 260, 4096):
        assert h(0, p, d, p, p, p, p, 1, d, L.CMR_BF16, p, None) == L.CMR_ERR_UNSUPPORTED
    assert h(0, odd, 256, p, p, p, p, 1, 256, L.CMR_F16, p, None) == L.CMR_ERR_UNSUPPORTED
    assert h(0, p, 260, p, p, p, p, 1, 256, L.CMR_F16, p, None) == L.CMR_ERR_UNSUPPORTED
    if L.device_count() == 0:                                                                           # valid arguments: only then the device is asked for
        assert a(0, p, L.CMR_BF16, p, 1, 16, 1, 64, p, None) == L.CMR_ERR_NO_DEVICE
        assert h(0, p, 256, p, None, p, None, 1, 256, L.CMR_BF16, p, None) == L.CMR_ERR_NO_DEVICE


def test_config_fields_are_inert_defaults():
    from comorag_amd.utils.config_utils import BaseConfig
    c = BaseConfig()
    assert c.rerank_model_name is None and c.rerank_model_dtype == "bf16" and c.rerank_batch_size == 32 and c.rerank_max_seq_len == 512
    assert isinstance(c.rerank_cls_tail, bool)
