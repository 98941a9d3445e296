"""``model_memory`` — the Model of the hot path (reference: MemVul/model_memory.py:39-224), with the
tensor work done by libmemvul_hip.so through the C ABI.

Same constructor arguments, method names and output-dict keys as the reference:
  * ``__init__(vocab, text_field_embedder, PTM, dropout, label_namespace, device, use_header, temperature,
    initializer, regularizer)`` (l.41-51);
  * ``forward(sample1, sample2, label, metadata)`` (l.118-167): ``metadata[0]["type"] == "golden"`` ->
    ``forward_gold_instances`` and ``{}`` (l.126-128); ``"test"``/``"unlabel"`` -> ``{"meta", "probs"}``
    with ``probs`` the full ``[B,G,2]`` softmax (an ndarray instead of ``p.tolist()``, l.143), metric
    updates on the best-anchor row (l.144-147,162-166);
  * ``forward_gold_instances`` (l.105-115), ``forward_on_instances`` (AllenNLP ``Model`` API used at
    predict_memory.py:81-83), ``make_output_human_readable`` (l.169-191), ``get_metrics`` (l.194-217),
    ``get_output_dim`` (l.220-224);
  * ``_golden_instances_embeddings`` / ``_golden_instances_labels`` stay assignable from outside
    (callbacks.py:48-49 resets them to ``None`` before rebuilding the bank).
Out of scope: the training branch (l.149-160: pair loss with temperature) — it raises.

There is no CPU implementation here: without the HIP library / a GPU, constructing the engine raises.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Any, Dict, List, Optional

import numpy as np

from .binding import Engine, compute_dtype_of, wanted_form, tokenize_policy
from .custom_metric import SiameseMeasureV1
from .data import Instance, collate
from .kept_sweep import KEY_MATCH_W, KeptSweepState
from .registry import HAVE_ALLENNLP, Model, TextFieldEmbedder, TokenEmbedder, Vocabulary, register_builtin

logger = logging.getLogger(__name__)

PFX_BERT = "_text_field_embedder.token_embedder_tokens.transformer_model."


class _LoadResult(tuple):
    """``(missing_keys, unexpected_keys)`` of ``torch.nn.Module.load_state_dict``."""

    def __new__(cls, missing, unexpected):
        return super().__new__(cls, (list(missing), list(unexpected)))

    missing_keys = property(lambda self: self[0])
    unexpected_keys = property(lambda self: self[1])


def _np(x):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


@TokenEmbedder.register("custom_pretrained_transformer")
class CustomPretrainedTransformerEmbedder(TokenEmbedder):
    """Configuration holder for the reference's embedder (custom_PTM_embedder.py:22-147): the BERT
    weights arrive with the archive's ``weights.th`` (keys ``..transformer_model.*``); the directory
    ``pretrained_model_path`` (l.99) is only consulted for ``config.json`` when present."""

    def __init__(self, model_name: str = None, *, max_length: int = None, sub_module: str = None, train_parameters: bool = True,
                 eval_mode: bool = False, last_layer_only: bool = True, override_weights_file: Optional[str] = None,
                 override_weights_strip_prefix: Optional[str] = None, gradient_checkpointing: Optional[bool] = None,
                 tokenizer_kwargs: Optional[Dict[str, Any]] = None, transformer_kwargs: Optional[Dict[str, Any]] = None,
                 pretrained_model_path: str = "out_wwm/") -> None:
        super().__init__()  # AllenNLP's TokenEmbedder is a torch.nn.Module (BasicTextFieldEmbedder registers it as a sub-module)
        if max_length is not None:
            raise NotImplementedError("segment folding (custom_PTM_embedder.py:244-381) is dead code in every reference config")
        if not last_layer_only:
            raise NotImplementedError("ScalarMix over hidden states is not used by the reference configs")
        self.model_name, self.pretrained_model_path = model_name, pretrained_model_path
        self.output_dim = 768

    def get_output_dim(self):
        return self.output_dim


@register_builtin(TokenEmbedder, "pretrained_transformer")
class _PlainPretrainedTransformerEmbedder(CustomPretrainedTransformerEmbedder):
    """config_no_pretrain.json uses the stock embedder type; same inference path."""

    def __init__(self, model_name: str = None, **kw) -> None:
        kw.pop("pretrained_model_path", None)
        super().__init__(model_name, **kw)


@register_builtin(TextFieldEmbedder, "basic")
class BasicTextFieldEmbedder(TextFieldEmbedder):
    def __init__(self, token_embedders: Dict[str, TokenEmbedder]) -> None:
        super().__init__()
        self.token_embedders = token_embedders

    def get_output_dim(self):
        return sum(e.get_output_dim() for e in self.token_embedders.values())


class _ClassificationCounts:
    """CategoricalAccuracy + FBetaMeasure(beta=1, average in {"weighted", None}) of model_memory.py:80-84,
    from one running confusion matrix."""

    def __init__(self, num_class: int) -> None:
        self.n = num_class
        self.reset()

    def reset(self):
        self.cm = np.zeros((self.n, self.n), np.int64)  # [gold, pred]

    def __call__(self, predictions: np.ndarray, gold_labels: np.ndarray):
        pred = np.argmax(predictions, axis=-1)
        np.add.at(self.cm, (gold_labels.astype(np.int64), pred), 1)

    def accuracy(self) -> float:
        t = self.cm.sum()
        return float(np.trace(self.cm) / t) if t else 0.0

    def prf(self):
        tp = np.diag(self.cm).astype(np.float64)
        pred_sum, true_sum = self.cm.sum(0).astype(np.float64), self.cm.sum(1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(pred_sum > 0, tp / pred_sum, 0.0)
            r = np.where(true_sum > 0, tp / true_sum, 0.0)
            f = np.where(p + r > 0, 2 * p * r / (p + r), 0.0)
        return p, r, f, true_sum

    def weighted(self):
        p, r, f, w = self.prf()
        tot = w.sum()
        if tot == 0:
            return 0.0, 0.0, 0.0
        return float((p * w).sum() / tot), float((r * w).sum() / tot), float((f * w).sum() / tot)


@Model.register("model_memory")
class ModelMemory(Model):
    def __init__(self,
                 vocab: Vocabulary,
                 text_field_embedder: TextFieldEmbedder,
                 PTM: str = "bert-base-uncased",
                 dropout: float = 0.1,
                 label_namespace: str = "labels",
                 device: str = "cpu",
                 use_header: bool = True,
                 temperature: float = 1,
                 initializer: Any = None,
                 regularizer: Any = None,
                 engine_options: Optional[Dict[str, Any]] = None) -> None:
        super().__init__(vocab, regularizer)
        self.device = device
        self._device_index = int(str(device).split(":")[1]) if ":" in str(device) else 0
        self._use_header = use_header
        self._label_namespace = label_namespace
        self._idx2token_label = self.vocab.get_index_to_token_vocabulary(namespace=label_namespace)
        self._same_idx = vocab.get_token_index("same", namespace=label_namespace)
        self._text_field_embedder = text_field_embedder
        self._num_class = self.vocab.get_vocab_size(self._label_namespace)
        self._temperature = temperature
        self._golden_labels: Optional[List[str]] = None
        self._counts = _ClassificationCounts(self._num_class)
        self._siamese_metric = SiameseMeasureV1(self._same_idx)
        self._engine_options = dict(engine_options or {})
        self._engine: Optional[Engine] = None
        self._kept = KeptSweepState()  # (the last keeping sweep_arrays and the indexes over it)

    # ---- weights --------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, Any], strict: bool = True):
        """``model.load_state_dict(torch.load(weights.th))`` of AllenNLP's ``load_archive``: creates the
        engine on ``self.device`` sized from the tensors and uploads them (mv_load_tensor /
        mv_finalize_weights)."""
        sd = {k: _np(v) for k, v in state_dict.items()}
        layers = 0
        while (PFX_BERT + f"encoder.layer.{layers}.attention.self.query.weight") in sd:
            layers += 1
        vocab_size = sd[PFX_BERT + "embeddings.word_embeddings.weight"].shape[0]
        max_pos = min(512, sd[PFX_BERT + "embeddings.position_embeddings.weight"].shape[0])
        type_vocab = sd[PFX_BERT + "embeddings.token_type_embeddings.weight"].shape[0]
        opts = dict(max_tokens=128 * 512, max_batch=512, max_anchors=1024)
        opts.update(self._engine_options)
        # use_header (model_memory.py:69-73): with the header the matcher runs on its 512-d output; without it the model has
        # no _projector_single and `_projector` is Linear(3 * 768, 2) on the pooler output -> mv_config.proj_dim = 768
        has_header = "_projector_single._linear_layers.0.weight" in sd
        if has_header != bool(self._use_header):
            raise ValueError(f"use_header={self._use_header} but the state dict {'has' if has_header else 'lacks'} "
                             "_projector_single (model_memory.py:69-71)")
        opts["proj_dim"] = 512 if self._use_header else 768
        # compute dtype: MV_F16X8 ("precise", the DEFAULT: fp16 sweep + one fp8 correction sweep per GEMM — the mode that holds the
        # reference's 1e-3 on trained-like logits; include/memvul_hip.h) or MV_F16 ("fast": explicit opt-in, 3.0-5.6e-3 there);
        # engine_options["compute_dtype"] or $MEMVUL_COMPUTE = precise | f16x8 | f16 | fast | safe | guarded.  An unknown name raises here
        # (ValueError), not inside ctypes.
        # "safe" / "guarded" = MV_F16X8 in that form (include/memvul_hip.h mv_set_form): the name itself goes to Engine.load_state_dict, which sets the form.
        # engine_options["sink_tokens"] = [id, ...] (or $MEMVUL_SINK_TOKENS): the sink-token list of the guarded form — Engine.load_state_dict applies it after
        # finalize and raises unless the form is "guarded" (binding.sink_tokens_policy).
        cd = opts.pop("compute_dtype", None)
        cd = wanted_form(cd) or compute_dtype_of(cd)
        # engine_options["tokenize"] = host | gpu (or $MEMVUL_TOKENIZE) is the drivers' switch (predict_memory.attach_tokenizer), not an engine argument; it is
        # checked here too, so that a typo raises wherever the options arrive first
        tokenize_policy(opts.pop("tokenize", None))
        if self._engine is not None:
            self._engine.close()
        self._engine = Engine(self._device_index, vocab_size=vocab_size, layers=layers, max_pos=max_pos, type_vocab=type_vocab,
                              same_idx=self._same_idx, **opts)
        self._engine.load_state_dict(sd, cd)
        self._kept.drop()  # (a kept sweep was the old engine's)
        self._kept.matcher_weight = np.ascontiguousarray(sd[KEY_MATCH_W], np.float32) if KEY_MATCH_W in sd else None  # (the indexes over a kept sweep take it)
        # torch's contract (AllenNLP's Model._load unpacks it): every tensor the engine needs was found by mv_load_tensor /
        # mv_finalize_weights (they fail otherwise); keys it has no use for — the BertModel's own pooler copy, position_ids — are
        # not "unexpected" to a model that declares no parameters of its own
        return _LoadResult([], [])

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            raise RuntimeError("ModelMemory has no weights yet: call load_state_dict (or load_archive) first")
        return self._engine

    # ---- anchor memory attributes the callers poke (callbacks.py:48-49) --------------------------
    @property
    def _golden_instances_embeddings(self):
        if self._engine is None or self._engine.n_anchors == 0:
            return None
        return self._engine.anchor_get()

    @_golden_instances_embeddings.setter
    def _golden_instances_embeddings(self, value):
        if value is None:
            if self._engine is not None:
                self._engine.anchor_reset()
        else:
            self.engine.anchor_set(_np(value))

    @property
    def _golden_instances_labels(self):
        return self._golden_labels

    @_golden_instances_labels.setter
    def _golden_instances_labels(self, value):
        self._golden_labels = None if value is None else list(value)

    # ---- the reference's methods ------------------------------------------------------------------
    @staticmethod
    def _ids_lens(sample: Dict[str, Dict[str, Any]]):
        t = sample["tokens"]
        known = t.get("_collated")
        if known is not None:  # memvul_amd.data.collate: lengths, prefix mask, zero padding and the segment check by construction
            ids32, lens, single = known
            if not single:
                raise ValueError("non-zero token-type ids: the hot path is single-segment (custom_PTM_embedder.py:199-202)")
            return ids32, lens
        ids = _np(t["token_ids"]).astype(np.int32)
        mask = np.asarray(_np(t["mask"]), bool)
        tid = t.get("type_ids")
        if tid is not None and _np(tid).any():
            raise ValueError("non-zero token-type ids: the hot path is single-segment (custom_PTM_embedder.py:199-202)")
        lens = mask.sum(1).astype(np.int32)
        # a prefix mask: the LAST set position of a row is its count - 1 (then every position before it is set too)
        last = mask.shape[1] - 1 - np.argmax(mask[:, ::-1], axis=1) if mask.shape[1] else np.zeros(len(lens), np.int64)
        if not np.array_equal(np.where(lens > 0, last, -1), lens.astype(np.int64) - 1):
            raise ValueError("mask must be a prefix mask (pad-to-longest collation)")
        np.multiply(ids, mask, out=ids)
        return ids, lens

    def _instance_forward(self, sample, use_header: bool = False) -> np.ndarray:
        # (the reference passes self._use_header at every call site, l.112, 133; the engine was created for that choice)
        assert bool(use_header) == bool(self._use_header), "the engine was built for use_header=%s" % self._use_header
        ids, lens = self._ids_lens(sample)
        return self.engine.encode(ids, lens)

    def forward_gold_instances(self, sample, metadata):
        ids, lens = self._ids_lens(sample)
        self.engine.anchor_append(ids, lens)
        labels = [_["instance"][0]["label"] for _ in metadata]
        if self._golden_labels is None:
            self._golden_labels = labels
        else:
            self._golden_labels.extend(labels)

    def forward(self, sample1=None, sample2=None, label=None, metadata: List[Dict[str, Any]] = None) -> Dict[str, Any]:
        output_dict: Dict[str, Any] = dict()
        if metadata and metadata[0]["type"] == "golden":
            self.forward_gold_instances(sample1, metadata)
            return output_dict
        if metadata:
            output_dict["meta"] = metadata
        if not (metadata and metadata[0]["type"] in ["test", "unlabel"]):
            raise NotImplementedError("the pair-training branch (model_memory.py:149-160) is outside the inference hot path")
        ids, lens = self._ids_lens(sample1)
        # (rows grouped by their own padded length: a pad-to-longest batch of unsorted reports is mostly padding — Engine.forward_by_length)
        out = self.engine.forward_by_length(ids, lens, want_logits=False, want_probs=True)
        output_dict["probs"] = out["probs"]           # [B,G,2]; the reference stores p.tolist()
        output_dict["best_anchor"] = out["best_idx"]  # extra (not in the reference): g* per issue report
        probs = out["best"]                           # [B,2] = p[b, g*]
        if label is not None:
            self._counts(probs, _np(label))
        self._siamese_metric(probs, metadata)
        return output_dict

    __call__ = forward

    def forward_begin(self, sample1=None, sample2=None, label=None, metadata: List[Dict[str, Any]] = None):
        """``forward`` in two halves for a caller that overlaps batches (predict_memory.evaluate): the engine takes the batch here without waiting for it
        (Engine.forward_by_length_begin) ..."""
        if not (metadata and metadata[0]["type"] in ["test", "unlabel"]) or not hasattr(self.engine, "forward_by_length_begin"):
            return ("done", self.forward(sample1, sample2, label, metadata))
        ids, lens = self._ids_lens(sample1)
        return ("pending", self.engine.forward_by_length_begin(ids, lens, want_logits=False, want_probs=True), label, metadata)

    def forward_end(self, pending) -> Dict[str, Any]:
        """... and is collected here, where the metric accumulators are updated: ``forward_end(forward_begin(**batch))`` is ``forward(**batch)`` (model_memory.py:118-167),
        and batches collected in the order they were begun update the metrics in the reference's order.  Collecting consumes the ticket, also when this call raises."""
        if pending[0] == "done":
            return pending[1]
        _, ticket, label, metadata = pending
        out = self.engine.forward_by_length_end(ticket)
        output_dict: Dict[str, Any] = {"meta": metadata, "probs": out["probs"], "best_anchor": out["best_idx"]}
        probs = out["best"]
        if label is not None:
            self._counts(probs, _np(label))
        self._siamese_metric(probs, metadata)
        return output_dict

    def forward_on_instances(self, instances: List[Instance]) -> List[Dict[str, Any]]:
        """AllenNLP ``Model.forward_on_instances``: collate (pad to the longest of the chunk) + forward."""
        batch = collate(instances, self.vocab)
        out = self.make_output_human_readable(self.forward(**batch))
        return out if isinstance(out, list) else [dict() for _ in instances]

    def sweep(self, instances: List[Instance], batch_size: int = 512) -> List[List[Dict[str, Any]]]:
        """The whole evaluation set in one resident, length-bucketed sweep (Engine.bucketed_sweep) instead of one
        ``forward`` per pad-to-longest batch (predict_memory.py:97-110): same per-IR arithmetic, same metric updates,
        same human-readable records in the same order and the same per-batch grouping — but every batch runs at its
        own longest member's length, two batches are in flight on the GPU, and token ids / results cross PCIe once."""
        if not instances:
            return []
        metadata, p_same = self.sweep_scores(instances, batch_size)
        out = []
        for s0 in range(0, len(instances), batch_size):
            out.append(self.make_output_human_readable({"meta": metadata[s0:s0 + batch_size], "p_same": p_same[s0:s0 + batch_size]}))
        return out

    def sweep_scores(self, instances: List[Instance], batch_size: int = 512):
        """``sweep`` up to the records: ``(metadata, P(same) [n, G])`` with the metric accumulators updated — what a caller that writes the records itself
        (predict_memory.evaluate_sweep, through records.RecordWriter: the same bytes without one dict per issue report) needs."""
        batch = collate(instances, self.vocab)
        metadata = batch["metadata"]
        if metadata[0]["type"] not in ["test", "unlabel"]:
            raise NotImplementedError("sweep() serves the test / unlabel branch (model_memory.py:133-147)")
        ids, lens = self._ids_lens(batch["sample1"])
        best, best_idx, p_same = self.engine.bucketed_sweep(ids, lens, batch_size, with_probs=True)
        if batch.get("label") is not None:
            self._counts(best, _np(batch["label"]))
        self._siamese_metric(best, metadata)
        return metadata, p_same

    def sweep_arrays(self, arrays: Dict[str, Any], first: int = 0, last: Optional[int] = None, batch_size: int = 512,
                     with_probs: bool = False, keep: bool = False, topk: int = 0):
        """``sweep`` on the array form of the evaluation set (ReaderMemory.read_arrays): rows ``first:last`` in one resident
        length-bucketed sweep, metric accumulators updated exactly as ``forward`` / ``sweep`` do (model_memory.py:133-147,
        162-167).  Returns ``(best [n, 2], best_idx [n], p_same [n, G] or None)``; no Instances, no per-IR Python objects.
        keep: the corpus keeps its embeddings, so that ``rematch_arrays`` can score the same rows against a changed anchor bank without encoding them again;
        topk: it keeps the k best anchors of every row (``engine.sweep_topk()``)."""
        if arrays["type"] not in ["test", "unlabel"]:
            raise NotImplementedError("sweep_arrays() serves the test / unlabel branch (model_memory.py:133-147)")
        last = len(arrays["lens"]) if last is None else last
        lens = np.ascontiguousarray(arrays["lens"][first:last], np.int32)
        self._kept.drop()  # (the sweep this one replaces, and what indexed it)
        if len(lens) == 0:
            return np.zeros((0, 2), np.float32), np.zeros((0,), np.int32), None
        ids = arrays["ids"][first:last, :int(lens.max())]
        if keep or topk:  # (an engine that is never asked to keep anything is called exactly as before)
            best, best_idx, p_same = self.engine.bucketed_sweep(ids, lens, batch_size, with_probs=with_probs, keep=keep, topk=topk)
            self._kept.rows = (first, last) if keep else None
        else:
            best, best_idx, p_same = self.engine.bucketed_sweep(ids, lens, batch_size, with_probs=with_probs)
        self._score_arrays(arrays, first, last, best)
        return best, best_idx, p_same

    def _score_arrays(self, arrays: Dict[str, Any], first: int, last: int, best: np.ndarray):
        same = np.asarray(arrays["same"][first:last], bool)
        diff_idx = self.vocab.get_token_index("diff", namespace=self._label_namespace)
        self._counts(best, np.where(same, self._same_idx, diff_idx).astype(np.int64))
        self._siamese_metric.add_arrays(same.astype(np.uint8), best[:, self._same_idx])

    def rematch_arrays(self, arrays: Dict[str, Any], first: int = 0, last: Optional[int] = None, with_probs: bool = False):
        """The rows of the last ``sweep_arrays(..., keep=True)`` scored against the anchor bank as it is NOW (forward_gold_instances, model_memory.py:105-115,
        appended to or rebuilt it since) by the matcher alone (l.135-147) — the encoder does not run.  Returns what ``sweep_arrays`` returns and updates the
        metric accumulators the same way."""
        last = self._kept_last("rematch_arrays", arrays, first, last)
        best, best_idx, p_same = self.engine.rematch_sweep(with_probs=with_probs)
        self._score_arrays(arrays, first, last, best)
        return best, best_idx, p_same

    def _kept_last(self, who: str, arrays: Dict[str, Any], first: int, last: Optional[int]) -> int:
        """``last`` resolved, after the refusal unless rows ``first:last`` are the last keeping sweep's."""
        last = len(arrays["lens"]) if last is None else last
        self._kept.require(who, first, last)
        return last

    def _kept_index(self, who: str, kind: str, index_class, index_factory, classes=None):
        return self._kept.index(who, kind, index_class, self.engine, self._same_idx, index_factory, classes)

    def _vectors_and_labels(self, who: str, vectors, labels):
        """The query vectors and their names: by default the bank as it is now under the golden labels; given vectors without labels are numbered."""
        if vectors is None:
            vectors = self.engine.anchor_get()
            if labels is None:
                labels = self._golden_labels
        vectors = np.ascontiguousarray(vectors, np.float32)
        if labels is None:
            labels = [str(g) for g in range(len(vectors))]
        if len(labels) != len(vectors):
            raise ValueError(f"{who}(): {len(labels)} labels for {len(vectors)} vectors")
        return vectors, list(labels)

    def anchor_reports(self, arrays: Dict[str, Any], k: int, first: int = 0, last: Optional[int] = None, vectors=None, labels: Optional[List[str]] = None,
                       index_factory=None) -> List[Dict[str, Any]]:
        """The other direction of the match, over the rows of the last ``sweep_arrays(..., keep=True)``: for every anchor of the bank as it is NOW — or for every
        row of ``vectors`` (fp32 [Q, P], e.g. ``engine.encode(...)`` of a fresh CVE description), named by ``labels`` — the k issue reports with the highest
        P(same): ``[{"anchor": label, "reports": [{"Issue_Url", "row", "prob"}, ...]}, ...]``, ``row`` numbered as in ``arrays``.  The ranking runs on the GPU
        (retrieve.ReportIndex; ``index_factory(device, proj_dim, matcher_weight, same_idx)`` builds it) over an index that is filled once per kept sweep and
        dropped when another sweep replaces it; P(same) is bit for bit the matcher's."""
        from . import retrieve

        self._kept_last("anchor_reports", arrays, first, last)
        vectors, labels = self._vectors_and_labels("anchor_reports", vectors, labels)
        p, rows = self._kept_index("anchor_reports", "reports", retrieve.ReportIndex, index_factory).query(vectors, k)
        return retrieve.format_reports(labels, arrays["urls"], p, rows, first)

    def anchor_claims(self, arrays: Dict[str, Any], thres=0.5, first: int = 0, last: Optional[int] = None, vectors=None, labels: Optional[List[str]] = None,
                      grid=None, index_factory=None) -> List[Dict[str, Any]]:
        """The reference's decision rule (predict_memory.py:170-177: ``prob >= thres``) per anchor, over the rows of the last ``sweep_arrays(..., keep=True)``: for
        every anchor of the bank as it is NOW — or for every row of ``vectors`` (fp32 [Q, P]), named by ``labels`` — EVERY issue report with P(same) >= ``thres``
        (a number, or one per vector): ``[{"anchor", "thres", "claimed", "positives", "reports": [{"Issue_Url", "row", "prob"}, ...]}, ...]``, reports ranked
        (P descending, row ascending), ``positives`` counted from ``arrays["same"]``.  grid (a list of thresholds, or "reference" = np.arange(0.5, 0.9, 0.01)): also
        ``"grid": [{"thres", "claimed", "positives"}, ...]`` and ``"best_thres"``, the per-anchor find_best_thres (custom_metric.py:35-52: best F1, ``>=``, the
        last threshold wins a tie).  Runs on the GPU (claims.ClaimIndex; ``index_factory(device, proj_dim, matcher_weight, same_idx)`` builds it) over an index
        that is filled once per kept sweep — a further device copy of the embeddings, 2 KB per row — and dropped when another sweep replaces it."""
        from . import claims

        last = self._kept_last("anchor_claims", arrays, first, last)
        vectors, labels = self._vectors_and_labels("anchor_claims", vectors, labels)
        positive = np.ascontiguousarray(np.asarray(arrays["same"][first:last], bool))
        index = self._kept_index("anchor_claims", "claims", claims.ClaimIndex, index_factory, positive)
        return claims.claims_of(index, labels, arrays["urls"], vectors, thres, positive, first, grid)

    def anchor_bank_audit(self, arrays: Dict[str, Any], thres=0.5, first: int = 0, last: Optional[int] = None, candidates=None,
                          candidate_labels: Optional[List[str]] = None, w_pos: int = 1, w_neg: int = 1, max_rounds: Optional[int] = None, candidate_thres=None,
                          top: int = 20, index_factory=None) -> Dict[str, Any]:
        """The bank as a whole, over the rows of the last ``sweep_arrays(..., keep=True)`` and the anchors as they are NOW, each at its own threshold (``thres``: a
        number, or one per anchor — e.g. the ``best_thres`` of ``anchor_claims``): one dict (bank.audit_of) with the union decision ("claimed by at least one
        anchor") and its confusion matrix, per anchor what it claims, what ONLY it claims and the union's F1 without it, the ``top`` overlapping pairs by Jaccard,
        and the greedy order (gain = w_pos * new positives - w_neg * new negatives) in which the bank would be rebuilt.  candidates (fp32 [K, P], e.g.
        ``engine.encode(...)`` of CVE descriptions; thresholds ``candidate_thres``, default the first anchor's): the bank's anchors are fixed and "greedy" ranks the
        candidates by what each adds beyond the bank.  Runs on the GPU (bank.BankAudit; ``index_factory(device, proj_dim, matcher_weight, same_idx)`` builds it)
        over an index that is filled once per kept sweep — from the same download as the other two indexes while that is still held — and dropped with them."""
        from . import bank

        last = self._kept_last("anchor_bank_audit", arrays, first, last)
        vectors = np.ascontiguousarray(self.engine.anchor_get(), np.float32)
        labels = list(self._golden_labels)
        if len(labels) != len(vectors):
            raise ValueError(f"anchor_bank_audit(): {len(labels)} labels for {len(vectors)} anchors")
        if np.ndim(thres) != 0 and np.shape(thres) != (len(vectors),):
            raise ValueError(f"anchor_bank_audit(): thres: a number, or one per anchor ({len(vectors)}), not shape {list(np.shape(thres))}")
        if not np.isfinite(np.asarray(thres, np.float64)).all():
            raise ValueError("anchor_bank_audit(): a threshold is not finite")
        positive = np.ascontiguousarray(np.asarray(arrays["same"][first:last], bool))
        index = self._kept_index("anchor_bank_audit", "bank", bank.BankAudit, index_factory, positive)
        return bank.run_audit(index, labels, vectors, thres, positive, candidates, candidate_labels, candidate_thres, w_pos, w_neg, max_rounds, top)

    def anchor_ranking(self, arrays: Dict[str, Any], first: int = 0, last: Optional[int] = None, vectors=None, labels: Optional[List[str]] = None, bank: bool = True,
                       index_factory=None) -> List[Dict[str, Any]]:
        """How well every anchor RANKS the rows of the last ``sweep_arrays(..., keep=True)`` against ``arrays["same"]`` — the three numbers the reference judges
        the matcher by (custom_metric.py:86-90), per anchor: for every anchor of the bank as it is NOW — or for every row of ``vectors`` (fp32 [Q, P]), named by
        ``labels`` — ``{"anchor", "n_pos", "n_neg", "n_nan", "auc", "ap", "best_thres", "best_f1", "best_claimed", "best_positives"}``: the exact ROC-AUC (ties
        at one half), sklearn's average precision, and the threshold that maximises F1 over EVERY distinct score (a tie to the highest).  bank: one more entry,
        ``"anchor": "bank"``, for a report's maximum over the vectors — what the reference's own auc / ap measure.  Runs on the GPU (rank.RankIndex;
        ``index_factory(device, proj_dim, matcher_weight, same_idx)`` builds it) over an index that is filled once per kept sweep and dropped with the others."""
        from . import rank

        last = self._kept_last("anchor_ranking", arrays, first, last)
        vectors, labels = self._vectors_and_labels("anchor_ranking", vectors, labels)
        positive = np.ascontiguousarray(np.asarray(arrays["same"][first:last], bool))
        index = self._kept_index("anchor_ranking", "ranking", rank.RankIndex, index_factory, positive)
        return rank.ranking_of(index, labels, vectors, bank=bank)

    def format_records_json(self, labels: List[str], urls: List[str], p_same: np.ndarray) -> str:
        """``json.dumps(make_output_human_readable(...))`` of one batch, byte for byte, built from arrays: the line
        predict_memory.py:111 writes per batch ({"Issue_Url", "label", "predict": {cwe: P(same)}} per issue report)."""
        from .records import format_batch, record_layout

        cols, fmt, names = record_layout(self._golden_labels)
        return format_batch(fmt, names, urls, labels, np.asarray(p_same)[:, cols].astype(np.float64))

    def make_output_human_readable(self, output_dict: Dict[str, Any]):
        if "meta" not in output_dict or output_dict["meta"][0]["type"] not in ["test", "unlabel"]:
            return output_dict
        labels = self._golden_labels
        ps = (np.asarray(output_dict["p_same"]) if "p_same" in output_dict                  # [B,G] (resident sweep)
              else np.asarray(output_dict["probs"])[:, :, self._same_idx])
        # vote_num[golden_name] = p[idx_same] in anchor order: a later duplicate label overwrites (l.181-183)
        order = {name: i for i, name in enumerate(labels)}  # last occurrence wins
        names = list(order.keys())
        cols = np.fromiter(order.values(), dtype=np.int64, count=len(order))
        sel = ps[:, cols].astype(np.float64)
        out2file = []
        for i, meta in enumerate(output_dict["meta"]):
            out2file.append({"Issue_Url": meta["instance"][0]["Issue_Url"], "label": meta["instance"][0]["label"],
                             "predict": dict(zip(names, sel[i].tolist()))})
        return out2file

    def get_metrics(self, reset: bool = False) -> Dict[str, float]:
        metrics = dict()
        metrics["accuracy"] = self._counts.accuracy()
        metrics["precision"], metrics["recall"], metrics["f1-score"] = self._counts.weighted()
        p, r, f, _ = self._counts.prf()
        for i in range(self._num_class):
            metrics[f"{self._idx2token_label[i]}_precision"] = float(p[i])
            metrics[f"{self._idx2token_label[i]}_recall"] = float(r[i])
            metrics[f"{self._idx2token_label[i]}_f1-score"] = float(f[i])
        if reset:
            s = self._siamese_metric.get_metric(reset)
            metrics["s_precision"], metrics["s_recall"], metrics["s_f1-score"] = s["precision"], s["recall"], s["f1"]
            metrics["s_thres"], metrics["s_auc"], metrics["s_ave_precision_score"] = s["thres"], s["auc"], s["ave_precision_score"]
            self._counts.reset()
        return metrics

    def get_output_dim(self, use_header=False):
        return 512 if use_header else self._text_field_embedder.get_output_dim()
