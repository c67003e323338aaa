"""The evaluation pass: batches -> model -> decode -> metrics (reference: ``PEneoTrainer.prediction_loop``
pipeline/trainer.py:57-211 and the ``compute_metrics`` closure of start/run_rfund.py:242-301).

The reference runs this inside a HuggingFace ``Trainer`` subclass; the model-facing part of it is small and is what
BASELINE config 1 exercises end to end (RFUND json -> ``RFUNDDataset`` -> ``DataCollatorForPEneo`` -> ``PEneoModel`` ->
``decode_peneo`` -> ``calculate_KVPE_metric``), so it is restated here without the Trainer: the same per-batch reads of the
model output (``orig_bbox.tolist()``, the five score maps split along the batch dimension, ``<x>_loss.mean().item()`` of
the LAST batch), the same arguments to ``decode_peneo`` and the same metric keys.  The score maps stay on the device: the
decode front end (``peneo_spots_compact``) reduces each ``[P, C]`` map to its few spots there.  ``compact_spots=True`` does that
reduction batch by batch (``peneo_spots_compact_batch``) and keeps only the spot lists, so the loop's device memory does not grow
with the number of documents."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional

import torch

from ..model.peneo_decoder import HandshakingTaggingScheme
from .decode import decode_peneo
from .evaluation import calculate_detail_KVPE_metric, calculate_KVPE_metric

_OUTPUTS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
_TAGS = ("line_extraction", "ent_linking_head_rel", "ent_linking_tail_rel", "line_grouping_head_rel", "line_grouping_tail_rel")


def _to_device(batch: Dict[str, object], device) -> Dict[str, object]:
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}


def make_compute_metrics(detail_eval: bool = False, start_eval_epoch: int = 0,
                         on_detail: Optional[Callable[[dict], None]] = None) -> Callable:
    """The ``compute_metrics(p, epoch)`` of start/run_rfund.py:242-301: decode predictions and ground truth, score the
    key/value pairs (``detail_eval``: all six tasks); before ``start_eval_epoch`` the metric is all zeros.  ``on_detail``
    receives the detail dictionary (the reference dumps it to ``detail.json`` on the main process)."""
    tagger = HandshakingTaggingScheme()

    def compute_metrics(p, epoch: int = 0) -> Dict[str, float]:
        predictions, label_ids, file_ids = p
        if epoch < start_eval_epoch:
            return {"precision": 0.0, "recall": 0.0, "f1": 0.0}
        tags, (gt_relations, orig_bboxes, texts) = label_ids[:5], label_ids[5:]
        all_pred, all_gt, all_fname = decode_peneo(
            handshaking_tagger=tagger, texts=texts,
            line_extraction_shaking_outputs=predictions[0], ent_linking_h2h_shaking_outputs=predictions[1],
            ent_linking_t2t_shaking_outputs=predictions[2], line_grouping_h2h_shaking_outputs=predictions[3],
            line_grouping_t2t_shaking_outputs=predictions[4],
            line_extraction_shaking_tags=tags[0], ent_linking_h2h_shaking_tags=tags[1], ent_linking_t2t_shaking_tags=tags[2],
            line_grouping_h2h_shaking_tags=tags[3], line_grouping_t2t_shaking_tags=tags[4],
            orig_bboxes=orig_bboxes, file_ids=file_ids)
        score = calculate_detail_KVPE_metric if detail_eval else calculate_KVPE_metric
        metric, detail = score(all_pred=all_pred, all_gt=all_gt, all_fname=all_fname)
        if on_detail is not None:
            on_detail(detail)
        return metric

    return compute_metrics


@torch.no_grad()
def prediction_loop(model, dataloader: Iterable[Dict[str, object]], compute_metrics: Optional[Callable] = None,
                    epoch: int = 0, metric_key_prefix: str = "eval", device=None, compact_spots: bool = False) -> Dict[str, float]:
    """One pass over ``dataloader`` (batches of ``DataCollatorForPEneo``) in eval mode; returns the metric dict with every
    key prefixed ``<prefix>_`` (pipeline/trainer.py:57-211).  As in the reference the reported losses are those of the last
    batch, and ``<prefix>_line_grouping_h2h_loss`` ends up holding the tail->tail loss (:196-201 assigns that key twice);
    callers that want the separate values read them from the model output.

    ``compact_spots=False`` (default) hands ``compute_metrics`` the score maps and label maps of every document as tensors, as
    the reference does.  ``compact_spots=True`` compacts the five score maps of each batch right after its forward, and the
    five label maps the same way (sparse labels through ``ops.spots_to_tags`` first, which keeps "last spot wins"), drops the
    tensors and hands ``compute_metrics`` spot lists ``[(i, j, tag, score)]`` in their place; ``decode_peneo`` /
    ``sample_decode_peneo`` take either, and the metrics are the same.

    A model with ``set_skip_padded_pairs(True)`` needs no argument here: its maps hold the background row at every pair that
    touches the padding, so predicted spots in the padding disappear (with either ``compact_spots`` setting), and the reported
    eval losses are the live-pair losses of ``PEneoOutput``, not the reference's means over all pairs."""
    if device is None:
        device = next(model.parameters()).device
    compute_metrics = compute_metrics or make_compute_metrics()
    was_training = model.training
    model.eval()
    file_ids: List[str] = []
    orig_bboxes: List[list] = []
    text: List[list] = []
    relations: List[list] = []
    maps: List[List[torch.Tensor]] = [[] for _ in _OUTPUTS]
    tags: List[List[torch.Tensor]] = [[] for _ in _TAGS]
    losses = None
    for batch in dataloader:
        if "text" not in batch:
            raise ValueError("No text given in evaluation")
        inputs = _to_device(batch, device)
        outputs = model(**inputs)
        orig_bboxes += outputs.orig_bbox.tolist()
        text += batch["text"]
        file_ids += batch.get("fname", [])
        relations += batch["relations"]
        N = outputs.orig_bbox.shape[1]
        batch_maps = [getattr(outputs, name + "_shaking_outputs") for name in _OUTPUTS]
        batch_tags = []
        for name in _TAGS:
            key = name + "_shaking_tag"
            if key in batch:
                batch_tags.append(inputs[key] if compact_spots else batch[key])
            else:  # sparse labels: rebuild the per-document maps on the device for the ground-truth side of the decode
                from .. import ops
                batch_tags.append(ops.spots_to_tags(inputs[name + "_matrix_spots"], N, device, B=inputs["input_ids"].shape[0]))
        if compact_spots:   # tensors -> spot lists now
            batch_maps = HandshakingTaggingScheme.get_spots_from_shaking_tags_batch(batch_maps, N)
            batch_tags = HandshakingTaggingScheme.get_spots_from_shaking_tags_batch(batch_tags, N)
        for k in range(len(_OUTPUTS)):
            maps[k] += list(batch_maps[k])
            tags[k] += list(batch_tags[k])
        # the reported losses are the last batch's; the output object (it holds the five score maps) and this batch's tensors go
        # before the next forward runs, so with compact_spots no map outlives its iteration
        losses = (outputs.loss, outputs.line_extraction_loss, outputs.ent_linking_h2h_loss, outputs.ent_linking_t2t_loss,
                  outputs.line_grouping_t2t_loss)
        del outputs, inputs, batch_maps, batch_tags
    model.train(was_training)
    if losses is None:
        return {}
    metrics = dict(compute_metrics((tuple(maps), (*tags, relations, orig_bboxes, text), file_ids), epoch))
    pre = metric_key_prefix + "_"
    for key, loss in zip(("loss", "line_extraction_loss", "ent_linking_h2h_loss", "ent_linking_t2t_loss", "line_grouping_h2h_loss"),
                         losses):
        metrics[pre + key] = loss.mean().item()
    return {(k if k.startswith(pre) else pre + k): v for k, v in metrics.items()}
