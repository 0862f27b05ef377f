"""Numeric re-score stage behind the reference's rerank call shape.

src/comorag/rerank.py:97-123 (`DSPyFilter.rerank`) is an LLM filter: it returns
`(sorted_indices[:n], sorted_items[:n], {'confidence': None})` and contains no numeric scoring.
BASELINE config 5 asks for "cross-scores on top-100 candidates"; this module supplies that as an
exact fp32 re-score of low-precision candidates (cmr_index_rescore) with the same return triple,
`confidence` carrying the scores.  The LLM filter itself stays the reference's (out of scope).

`CrossEncoderReranker` puts a model behind the same call shape: a one-logit sequence classifier of the BGE reranker family
(bge-reranker-base / -large / -v2-m3: XLM-R + classification head) on the fused encoder stack, `confidence` carrying its logits
(DESIGN.md 4.10d).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .index import DenseIndex


class ExactRescorer:
    def __init__(self, index: DenseIndex):
        self.index = index

    def __call__(self, *args, **kwargs):
        return self.rerank(*args, **kwargs)

    def rerank(self, query_embedding, candidate_items: Sequence, candidate_indices: Sequence[int],
               len_after_rerank: int = None) -> Tuple[List[int], List, dict]:
        """query_embedding [D] fp32 (the reference passes the query *string* to its LLM; the numeric
        stage needs the vector), candidate_items / candidate_indices as in rerank.py:100-104."""
        n = len(candidate_indices)
        if n == 0:
            return [], [], {"confidence": []}
        k = n if len_after_rerank is None else min(len_after_rerank, n)
        ids, sc = self.index.rescore(np.asarray(query_embedding, np.float32), np.asarray(candidate_indices, np.int64), k)
        pos = {int(r): i for i, r in reversed(list(enumerate(candidate_indices)))}
        keep = [int(r) for r in ids[0] if r >= 0]
        return keep, [candidate_items[pos[r]] for r in keep], {"confidence": sc[0][:len(keep)].tolist()}


def search_then_rescore(index: DenseIndex, queries, k_candidates: int = 100, k: int = 20):
    """BASELINE config 5 flow: low-precision top-`k_candidates` → exact fp32 top-`k`."""
    q = np.asarray(queries, np.float32)
    cand, _, _, _ = index.search(q, k_candidates, with_minmax=False)
    return index.rescore(q, cand, k)


# ---------------------------------------------------------------------------------------------------------------- cross-encoder
# A cross-score reads query and passage TOGETHER: the bge-reranker-base / -large / -v2-m3 models are XLM-R encoders with a one-logit
# classification head (BertForSequenceClassification is the same map with the pooler as the head's dense layer).  The encoder runs on the
# fused layer stack (embedding_model/fused_bert.py: `forward_cls`), the head on cmr_encoder_cls_head; with `rerank_cls_tail` the last
# layer is computed for the CLS rows alone (cmr_encoder_attention_cls).

def cross_encoder_parts(model, fp32: bool = False, head32: bool = False):
    """(base encoder, head modules (dense, out), None) of a *ForSequenceClassification model the fused stack can run, or
    (None, None, reason).  RoBERTa / XLM-R: model.roberta, classifier.dense -> tanh -> classifier.out_proj; BERT: model.bert,
    bert.pooler.dense -> tanh -> classifier.  Accepted: whatever fused_bert.why_not accepts, with one label."""
    from .embedding_model import fused_bert
    cfg = getattr(model, "config", None)
    kind = getattr(cfg, "model_type", "")
    if cfg is None or kind not in fused_bert.ENCODER_TYPES:
        return None, None, "not a BERT / RoBERTa / XLM-R sequence classifier"
    if int(getattr(cfg, "num_labels", 0)) != 1:
        return None, None, f"num_labels = {getattr(cfg, 'num_labels', None)} (one-logit heads only)"
    if kind == "bert":
        base, cls = getattr(model, "bert", None), getattr(model, "classifier", None)
        dense = getattr(getattr(base, "pooler", None), "dense", None)
        out = cls
    else:
        base, cls = getattr(model, "roberta", None), getattr(model, "classifier", None)
        dense, out = getattr(cls, "dense", None), getattr(cls, "out_proj", None)
    if base is None or dense is None or out is None or not hasattr(dense, "weight") or not hasattr(out, "weight"):
        return None, None, "unexpected classification head layout"
    d = int(cfg.hidden_size)
    if tuple(dense.weight.shape) != (d, d) or tuple(out.weight.shape) != (1, d):
        return None, None, "unexpected classification head shape"
    if d % 8:
        return None, None, "hidden size not supported by the head kernel"
    reason = fused_bert.why_not(base, fp32=fp32, head32=head32)
    if reason is not None:
        return None, None, reason
    return base, (dense, out), None


def pair_max_length(model_config, rerank_max_seq_len: int) -> int:
    """min(rerank_max_seq_len, the positions the model has): max_position_embeddings, less padding_idx + 1 for the RoBERTa family,
    whose position ids start there."""
    mp = int(getattr(model_config, "max_position_embeddings", 1 << 30))
    if getattr(model_config, "model_type", "") in ("roberta", "xlm-roberta", "camembert"):
        pad = getattr(model_config, "pad_token_id", 1)
        mp = max(1, mp - int(1 if pad is None else pad) - 1)
    return max(1, min(int(rerank_max_seq_len), mp))


def length_buckets(lens: Sequence[int], batch_size: int, bucketing: bool = True) -> List[np.ndarray]:
    """Mini-batches of at most batch_size pairs as index arrays into the call: sorted by token count (stable), so that a mini-batch is
    padded to the width of pairs like its own; arrival order with bucketing = False."""
    n = len(lens)
    order = np.argsort(np.asarray(lens, np.int64), kind="stable") if bucketing else np.arange(n)
    bs = max(1, int(batch_size))
    return [order[i:i + bs] for i in range(0, n, bs)]


def pad_pairs(ids: Sequence[Sequence[int]], types, pad_id: int, multiple: int = 16):
    """Right-pad one mini-batch to a multiple of `multiple`: (input_ids [b, l] int64, token types [b, l] int64 or None, lens [b] int32)."""
    lens = np.asarray([len(r) for r in ids], np.int32)
    l = int(-(-int(lens.max()) // multiple) * multiple)
    out = np.full((len(ids), l), int(pad_id), np.int64)
    tt = np.zeros((len(ids), l), np.int64) if types is not None else None
    for i, r in enumerate(ids):
        out[i, :len(r)] = r
        if tt is not None:
            tt[i, :len(r)] = types[i]
    return out, tt, lens


def rank_by_score(scores, candidate_items: Sequence, candidate_indices: Sequence[int], len_after_rerank: int = None):
    """The reference's return triple from one score per candidate: score descending, then candidate position ascending; an index that
    occurs twice keeps its first position."""
    seen, keep = set(), []
    for p, r in enumerate(candidate_indices):
        if int(r) not in seen:
            seen.add(int(r))
            keep.append(p)
    keep.sort(key=lambda p: (-float(scores[p]), p))
    if len_after_rerank is not None:
        keep = keep[:max(0, int(len_after_rerank))]
    return [int(candidate_indices[p]) for p in keep], [candidate_items[p] for p in keep], {"confidence": [float(scores[p]) for p in keep]}


class CrossEncoderReranker:
    """Cross-scores (query, passage) pairs with a one-logit sequence classifier behind the reference's rerank call shape.
    `reranker_path` names the route: "hip-fused-layers" (+ " (cls tail)") or "transformers (<reason>)"."""

    def __init__(self, global_config=None, model=None, tokenizer=None) -> None:
        import torch
        from .utils.config_utils import cfg_get
        if not torch.cuda.is_available():
            raise RuntimeError("CrossEncoderReranker needs an MI355X (no CPU fallback)")
        cfg = self.global_config = global_config
        name = cfg_get(cfg, "rerank_model_name", None)
        if model is None or tokenizer is None:
            if not name:
                raise ValueError("CrossEncoderReranker: set rerank_model_name or pass model= and tokenizer=")
            from transformers import AutoModelForSequenceClassification, AutoTokenizer
            tokenizer = tokenizer or AutoTokenizer.from_pretrained(name)
            model = model or AutoModelForSequenceClassification.from_pretrained(name)
        self.device = torch.device("cuda", int(cfg_get(cfg, "device", 0)))
        dt = str(cfg_get(cfg, "rerank_model_dtype", "bf16")).lower()
        tdt = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "float16": torch.float16, "f16": torch.float16}.get(dt)
        self.tokenizer = tokenizer
        self.model = (model.to(self.device) if tdt is None else model.to(self.device, dtype=tdt)).eval()
        self.batch_size = max(1, int(cfg_get(cfg, "rerank_batch_size", 32)))
        self.max_length = pair_max_length(self.model.config, int(cfg_get(cfg, "rerank_max_seq_len", 512)))
        self.cls_tail = bool(cfg_get(cfg, "rerank_cls_tail", False))
        self._bucket = bool(cfg_get(cfg, "embedding_length_bucketing", True))
        pad = getattr(self.model.config, "pad_token_id", None)
        if pad is None:
            pad = getattr(tokenizer, "pad_token_id", None)
        self.pad_id = int(pad or 0)
        self._has_types = int(getattr(self.model.config, "type_vocab_size", 1) or 1) > 1
        self._fused, self._head = None, None
        fp32, head32 = bool(cfg_get(cfg, "embedding_fused_fp32", False)), bool(cfg_get(cfg, "embedding_fused_head32", False))
        base, head, reason = cross_encoder_parts(self.model, fp32=fp32, head32=head32)
        if reason is None and getattr(tokenizer, "padding_side", "right") != "right":
            reason = "left-padding tokenizer"
        if reason is None:
            from .embedding_model import fused_bert
            self._fused = fused_bert.FusedBertLayers(base, graphs=0, gelu=str(cfg_get(cfg, "embedding_gelu", "exact")), fp32=fp32, head32=head32,
                                                     small_m=bool(cfg_get(cfg, "embedding_fused_small_m", False)),
                                                     small_m_rows=int(cfg_get(cfg, "embedding_small_m_rows", fused_bert.SMALL_M_ROWS)))
            dense, out = head
            self._head = (dense.weight.detach().contiguous(), dense.bias.detach().contiguous() if dense.bias is not None else None,
                          out.weight.detach().reshape(-1).contiguous(), out.bias.detach().contiguous() if out.bias is not None else None)
            self.reranker_path = "hip-fused-layers (cls tail)" if self.cls_tail else "hip-fused-layers"
        else:
            self.reranker_path = f"transformers ({reason})"

    def __call__(self, *args, **kwargs):
        return self.rerank(*args, **kwargs)

    # ------------------------------------------------------------------ scoring
    def tokenize_pairs(self, queries, passages: Sequence[str]):
        """(token ids, token types or None) per pair: ONE tokenizer call, truncated to the model's positions."""
        passages = list(passages)
        if isinstance(queries, str):
            queries = [queries] * len(passages)
        queries = list(queries)
        if len(queries) != len(passages):
            raise ValueError("score_pairs: queries and passages differ in length")
        # (a model with two token types asks for them by name: a generic PreTrainedTokenizerFast lists no token_type_ids among its model inputs)
        kw = {"return_token_type_ids": True} if self._has_types else {}
        enc = self.tokenizer(queries, passages, truncation=True, max_length=self.max_length, **kw)
        ids = [list(r) for r in enc["input_ids"]]
        types = None
        if self._has_types:
            try:
                types = [list(r) for r in enc["token_type_ids"]]
            except (KeyError, TypeError):
                types = None
        return ids, types

    def _score_batch(self, ids, types):
        """One mini-batch -> [b] fp32 logits on the GPU."""
        import torch
        arr, tt, lens = pad_pairs(ids, types, self.pad_id)
        dev = self.device
        ids_dev = torch.from_numpy(arr).pin_memory().to(dev, non_blocking=True)
        tt_dev = torch.from_numpy(tt).pin_memory().to(dev, non_blocking=True) if tt is not None else None
        if self._fused is not None:
            with torch.cuda.device(dev):
                return self._fused.forward_cls(ids_dev, lens, tt_dev, self._head, cls_tail=self.cls_tail)
        with torch.no_grad():                              # the transformers forward, on the GPU, for models the stack declines
            mask = torch.from_numpy((np.arange(arr.shape[1])[None, :] < lens[:, None]).astype(np.int64)).to(dev)
            kw = {"token_type_ids": tt_dev} if tt_dev is not None else {}
            logits = self.model(input_ids=ids_dev, attention_mask=mask, **kw).logits
            return logits[:, -1].float()                      # one label: its logit; several: the last class

    def score_pairs(self, queries, passages: Sequence[str], normalize: bool = False) -> np.ndarray:
        """Raw logits, fp32 [n] (normalize = True: their sigmoid, computed on the host in fp32).  Pairs are sorted by token count inside the
        call, run in mini-batches of `rerank_batch_size` padded to a multiple of 16 tokens, and the scores scattered back."""
        if len(passages) == 0:
            return np.zeros((0,), np.float32)
        ids, types = self.tokenize_pairs(queries, passages)
        return self.score_token_ids(ids, types, normalize)

    def score_token_ids(self, ids: Sequence[Sequence[int]], types=None, normalize: bool = False) -> np.ndarray:
        """`score_pairs` behind the tokenizer: one token-id row per pair (and its token types, or None)."""
        out = np.empty((len(ids),), np.float32)
        parts = []                                            # every mini-batch is enqueued before the first result is read back
        for sel in length_buckets([len(r) for r in ids], self.batch_size, self._bucket):
            parts.append((sel, self._score_batch([ids[i] for i in sel], [types[i] for i in sel] if types is not None else None)))
        for sel, t in parts:
            out[sel] = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t, np.float32)
        if normalize:
            out = (np.float32(1.0) / (np.float32(1.0) + np.exp(-out, dtype=np.float32))).astype(np.float32)
        return out

    def rerank(self, query: str, candidate_items: Sequence, candidate_indices: Sequence[int], len_after_rerank: int = None) -> Tuple[List[int], List, dict]:
        """The reference's call shape (rerank.py:100-104): passages are the items, or an item's last element where items are tuples."""
        if len(candidate_indices) == 0:
            return [], [], {"confidence": []}
        passages = [it[-1] if isinstance(it, (tuple, list)) else it for it in candidate_items]
        return rank_by_score(self.score_pairs(query, passages), candidate_items, candidate_indices, len_after_rerank)


def search_then_cross_score(index: DenseIndex, texts: Sequence[str], reranker, query: str, query_embedding, k_candidates: int = 100, k: int = 20):
    """BASELINE config 5 with a model behind its cross-scores: low-precision top-`k_candidates` of one query → the candidates' texts (by
    row id) → cross scores → (ids [k], scores [k]), cross-score descending, ties in scan order."""
    q = np.asarray(query_embedding, np.float32).reshape(1, -1)
    cand, _, _, _ = index.search(q, k_candidates, with_minmax=False)
    rows = [int(r) for r in cand[0] if r >= 0]
    ids, _, info = reranker.rerank(query, [texts[r] for r in rows], rows, k)
    return np.asarray(ids, np.int64), np.asarray(info["confidence"], np.float32)
