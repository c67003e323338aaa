"""PEneo decoder on libpeneo_hip kernels (reference: model/peneo_decoder.py).

``HandshakingTaggingScheme`` (label map <-> spots, :12-115), ``HandshakingKernel`` (:118-177),
``PEneoOutput`` (:180-198) and ``PEneoDecoder`` (:201-443) keep the reference's names, parameter
layout (``shrink_projection.{0,3}``, ``handshaking_kernel.combine_fc``, ``<head>_fc.{0,3}``,
``link_loss.weight`` / ``le_loss.weight`` buffers) and outputs.  The forward never materialises the
[B, P, D] pair tensor: K10 runs as two GEMMs with fused bias+SiLU(+dropout), K11+K12+K13 as the fused
pair-heads kernel; the backward re-creates the pair activations chunk by chunk (rows of the
triangle) so that its three GEMMs per chunk stay Infinity-Cache resident.
"""
from __future__ import annotations

import os

from dataclasses import dataclass, replace
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from transformers.modeling_outputs import ModelOutput

from .. import ops
from ..hip import ACT_NONE, ACT_SILU, PeneoHipError, deterministic_mode
from .engine import DropoutSeeds, WeightCache, big_acquire, big_clear, big_release, can_defer, defer_join, join_pending, mark_late

HEAD_NAMES = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
TAG_KWARGS = ("line_extraction_shaking_tag", "ent_linking_head_rel_shaking_tag", "ent_linking_tail_rel_shaking_tag",
              "line_grouping_head_rel_shaking_tag", "line_grouping_tail_rel_shaking_tag")
HEAD_CLASSES = (2, 3, 3, 3, 3)
_HEAD_OF_CLASS_SLOT: dict = {}   # device -> int64 [sum(HEAD_CLASSES)]: head index of every class slot


class HandshakingTaggingScheme:
    """Label-map <-> spot conversion (reference :12-115).  The packed index of pair (i, j), i <= j, of a
    length-n sequence is p = i*n - i*(i-1)/2 + (j - i)."""

    @staticmethod
    def spots2shaking_tag(spots: List[Tuple], seq_len: int) -> torch.Tensor:
        """NOTE: the reference builds an all-zero index map here, so every spot lands on p = 0
        (:26-31); only ``spots2shaking_tag4batch`` is used by its collator.  Reproduced as is."""
        tag = torch.zeros(seq_len * (seq_len + 1) // 2).long()
        for sp in spots:
            tag[0] = sp[2]
        return tag

    @staticmethod
    def spots2shaking_tag4batch(batch_spots, shaking_ind2matrix_ind=None, matrix_ind2shaking_ind=None,
                                seq_len: int = None) -> torch.Tensor:
        if shaking_ind2matrix_ind is not None and matrix_ind2shaking_ind is not None:
            seq_len = len(matrix_ind2shaking_ind)
        elif seq_len is None:
            raise ValueError("If shaking_ind2matrix_ind and matrix_ind2shaking_ind are not provided,seq_len must be given")
        n = seq_len
        out = torch.zeros(len(batch_spots), n * (n + 1) // 2).long()
        for b, spots in enumerate(batch_spots):
            for sp in spots:
                i, j = sp[0], sp[1]
                if matrix_ind2shaking_ind is not None:
                    p = matrix_ind2shaking_ind[i][j]
                else:
                    p = i * n - i * (i - 1) // 2 + (j - i) if i <= j else 0  # reference's table is 0 below the diagonal
                out[b][p] = sp[2]
        return out

    @staticmethod
    def spots2shaking_tag4batch_device(batch_spots, seq_len: int, device) -> torch.Tensor:
        """Same result as ``spots2shaking_tag4batch(batch_spots, seq_len=seq_len)`` but built by one device kernel from the
        sparse spots: no O(N^2) host table, no 5.2 MB/document label copy."""
        return ops.spots_to_tags(batch_spots, seq_len, device)

    @staticmethod
    def get_spots_from_shaking_tag(shaking_tag: torch.Tensor, shaking_ind2matrix_ind=None, seq_len: int = None):
        """[P, C] logits (or [P] tags) -> [(i, j, tag, score)] in increasing p order (reference :76-115).
        Device tensors go through the fused softmax/argmax/compaction kernel (K14) — one launch and one
        copy instead of a Python loop with three ``.item()`` syncs per spot."""
        if isinstance(shaking_tag, list):   # already compacted (get_spots_from_shaking_tags_batch): the spot list itself
            return shaking_tag
        if shaking_ind2matrix_ind is None and seq_len is None:
            raise ValueError("If shaking_ind2matrix_ind and matrix_ind2shaking_ind are not provided,seq_len must be given")
        P = shaking_tag.shape[0]
        if seq_len is None:
            seq_len = int(((8 * P + 1) ** 0.5 - 1) // 2)
        n = seq_len
        if shaking_tag.dim() > 1 and shaking_tag.shape[-1] > 1 and shaking_tag.is_cuda:
            spots, scores = ops.spots_compact(shaking_tag.float().contiguous(), n)
            sp, sc = spots.cpu().tolist(), scores.cpu().tolist()
            return [(a, b, t, s) for (a, b, t), s in zip(sp, sc)]
        if shaking_tag.dim() > 1 and shaking_tag.shape[-1] > 1:
            prob = shaking_tag.softmax(-1)
            pred, score = prob.argmax(-1), prob.max(-1)[0]
        else:
            pred, score = shaking_tag.view(-1), torch.ones_like(shaking_tag.view(-1), dtype=torch.float32)
        out = []
        for p in torch.nonzero(pred)[:, 0].tolist():
            if shaking_ind2matrix_ind is not None:
                i, j = shaking_ind2matrix_ind[p]
            else:
                i = int((2 * n + 1 - ((2 * n + 1) ** 2 - 8 * p) ** 0.5) // 2)
                while i > 0 and i * n - i * (i - 1) // 2 > p:
                    i -= 1
                while i < n - 1 and (i + 1) * n - (i + 1) * i // 2 <= p:
                    i += 1
                j = i + p - (i * n - i * (i - 1) // 2)
            out.append((i, j, int(pred[p]), float(score[p])))
        return out

    @staticmethod
    def get_spots_from_shaking_tags_batch(maps: Sequence[torch.Tensor], seq_len: int):
        """Every map of a batch at once: ``maps[m]`` is [B, P, C] logits or a [B, P] label map; returns ``out[m][b]`` =
        ``get_spots_from_shaking_tag(maps[m][b], seq_len=seq_len)``.  Device maps that are floating [B, P, C >= 2] logits or
        integer [B, P] / [B, P, 1] labels take one batched compaction call (``ops.spots_compact_batch``: two launches and two
        device-to-host copies for the whole batch, up to 8 maps a call) instead of one launch and three copies per document
        and map; every other map (host tensors, floating label maps) takes the per-document call itself."""
        get = HandshakingTaggingScheme.get_spots_from_shaking_tag
        out: List[Optional[list]] = [None] * len(maps)
        dev_maps, dev_at = [], []
        for k, m in enumerate(maps):
            logits = torch.is_tensor(m) and m.is_cuda and m.dim() == 3 and m.shape[-1] > 1 and m.is_floating_point()
            labels = torch.is_tensor(m) and m.is_cuda and not m.is_floating_point() and not m.is_complex() and \
                (m.dim() == 2 or (m.dim() == 3 and m.shape[-1] == 1))
            if logits or labels:
                dev_maps.append(m.float().contiguous() if logits else m.reshape(m.shape[0], m.shape[1]).long().contiguous())
                dev_at.append(k)
            else:
                out[k] = [get(m[b], seq_len=seq_len) for b in range(len(m))]
        for m0 in range(0, len(dev_maps), ops.hip.MAX_HEADS):
            records, counts = ops.spots_compact_batch(dev_maps[m0:m0 + ops.hip.MAX_HEADS], seq_len)
            # column by column: a [n, 3] tolist() makes n short lists at once, and the collector walks them again and again
            spots = list(zip(records[:, 0].tolist(), records[:, 1].tolist(), records[:, 2].tolist(),
                             records.view(torch.float32)[:, 3].tolist()))
            at = 0
            for k, per_doc in zip(dev_at[m0:], counts.tolist()):
                out[k] = []
                for n in per_doc:
                    out[k].append(spots[at:at + n])
                    at += n
        return out


@dataclass
class PEneoOutput(ModelOutput):
    """The reference's output record.  Of a forward that ran with ``skip_padded_pairs`` (PEneoDecoder.set_skip_padded_pairs: no
    gradients, an attention mask given) the six losses are LIVE-PAIR losses - class-weighted means over the pairs of real tokens,
    not over all P pairs as the reference's - and the ``*_shaking_outputs`` hold (0, -1e30, ...) at every pair that touches the
    padding."""
    loss: Optional[torch.Tensor] = None

    line_extraction_loss: Optional[torch.Tensor] = None
    ent_linking_h2h_loss: Optional[torch.Tensor] = None
    ent_linking_t2t_loss: Optional[torch.Tensor] = None
    line_grouping_h2h_loss: Optional[torch.Tensor] = None
    line_grouping_t2t_loss: Optional[torch.Tensor] = None

    line_extraction_shaking_outputs: Optional[torch.Tensor] = None
    ent_linking_h2h_shaking_outputs: Optional[torch.Tensor] = None
    ent_linking_t2t_shaking_outputs: Optional[torch.Tensor] = None
    line_grouping_h2h_shaking_outputs: Optional[torch.Tensor] = None
    line_grouping_t2t_shaking_outputs: Optional[torch.Tensor] = None

    attentions: Optional[Tuple[torch.FloatTensor]] = None
    hidden_states: Optional[Tuple[torch.FloatTensor]] = None
    orig_bbox: Optional[torch.Tensor] = None


class HandshakingKernel(nn.Module):
    """Parameter holder for ``combine_fc`` (Linear(2D -> D)); the pair expansion itself is fused into the
    pair-heads kernel via combine_fc(cat(h_i, h_j)) = W[:, :D] h_i + (W[:, D:] h_j + b)."""

    def __init__(self, hidden_size: int) -> None:
        super().__init__()
        self.combine_fc = nn.Linear(hidden_size * 2, hidden_size)
        self.activation = nn.SiLU()


class _ClassWeightedCE(nn.Module):
    """Holds the ``weight`` buffer of the reference's CrossEntropyLossOHEM (model/custom_loss.py:104-202)."""

    def __init__(self, weight: torch.Tensor, num_hard_positive: int, num_hard_negative: int):
        super().__init__()
        self.register_buffer("weight", weight)
        # -1 / -1: plain class-weighted mean (custom_loss.py:189-202, fused into the pair-heads kernel); anything else runs
        # the OHEM branch (:204-288) through peneo_ohem_ce on the logit maps
        self.num_hard_positive, self.num_hard_negative = int(num_hard_positive), int(num_hard_negative)

    @property
    def ohem(self) -> bool:
        return self.num_hard_positive != -1 or self.num_hard_negative != -1


def _row_chunks(n: int, max_pairs: int) -> List[Tuple[int, int]]:
    """Split rows 0..n of the pair triangle into [i0, i1) ranges of at most ~max_pairs pairs."""
    out, i0, acc = [], 0, 0
    for i in range(n):
        row = n - i
        if acc > 0 and acc + row > max_pairs:
            out.append((i0, i))
            i0, acc = i, 0
        acc += row
    out.append((i0, n))
    return out


@dataclass(frozen=True)
class PairRoute:
    """Which kernels one step of the decoder stage runs for the pair heads (DESIGN 5 has the table).  ``pair_route`` decides it
    once, in the forward; the backward dispatches on the route the forward stored and reads no switch of the decoder again, so a
    switch changed between the forward and the backward of one step does not affect that step."""
    forward: str                     # "generic" | "mxfp8_eval" | "mxfp8_save" | "bf16" (the compute dtype's kernel, fp32 included)
    save: bool = False               # the forward leaves the classifiers' pre-activations and x for the "saved" backward ...
    save_format: str = "f16"         # ... as "f16" or "e4m3" records
    backward: Optional[str] = None   # "generic" | "saved" | "fused" | "chunked"; None: nothing to run (no gradients or no labels)
    dz: Optional[str] = None         # "chunked" only, its dz producer: "fused" | "wide" | "epilogue" | "standalone"
    writes_x: bool = False           # "wide" only: that kernel also stores x / a_i + b_j (no peneo_pair_x_fwd launch)
    lens: bool = False               # "bf16" without gradients only: the length-aware launch (peneo_pair_heads_fwd_lens)


def pair_route(dec: "PEneoDecoder", dt: torch.dtype, D: int, need_grad: bool, has_tags: bool, p_hidden: float,
               has_mask: bool = False) -> PairRoute:
    """The route of a step at compute dtype `dt` and decoder width `D` from the decoder's switches and formats and the
    library's host-side queries (no GPU).  p_hidden: the classifier dropout in force (DropoutSeeds.p_hidden).  has_mask: the
    forward received an attention mask (what skip_padded_pairs takes the lengths from)."""
    nh = len(HEAD_NAMES)
    train = need_grad and has_tags
    # (above 512 the "mxfp8" format - set_pair_heads_format("mxfp8", wide=True) - has a kernel of its own and does not consult
    # pair_wide, the bf16 A/B arm inside fused_pair_heads; up to 512 the order of the questions is what it always was)
    mx_wide = dec.pair_heads_format == "mxfp8" and D > 512
    if not mx_wide and not dec.fused_pair_heads(dt, D):
        # (classifier depths other than the shipped 2, widths without a fused pair-heads kernel: the materialising per-document path)
        return PairRoute("generic", backward="generic" if train else None)
    if dec.pair_heads_format == "mxfp8":
        return PairRoute("mxfp8_eval")   # (PEneoDecoder.forward has refused a forward with gradients)
    if not train:
        # skip_padded_pairs: forwards without gradients only (a forward with gradients and no labels stays today's too); OHEM picks
        # its pairs from the finished maps, padding included, and keeps the plain launch
        lens = dec.skip_padded_pairs and has_mask and not need_grad and not (has_tags and dec.le_loss.ohem)
        return PairRoute("bf16", lens=True) if lens else PairRoute("bf16")
    if dec.fused_bwd and ops.pair_bwd_supported(dt, D, nh):   # (LDS: the head count enters, D = 512 holds 5 heads)
        # the forward of such a step leaves the classifiers' pre-activations (dropout applied) and x in the backward's block order, 2
        # bytes per pair and hidden unit (4.2 GB at 8 x 511 tokens): the backward repeats neither the first-layer product nor the mask
        if not (dec.save_pair_act and ops.pair_save_supported(dt, D, nh)):
            return PairRoute("bf16", backward="fused")
        if dec.pair_heads_train_format == "mxfp8":   # (the same mask, the same saved buffers, the same backward: straight-through)
            return PairRoute("mxfp8_save", save=True, backward="saved")
        # (pair_save_e4m3_supported is pair_save_supported: whatever saves at all can save in either format)
        return PairRoute("bf16", save=True, save_format="e4m3" if dec.pair_act_format == "e4m3" else "f16", backward="saved")
    # the chunked backward: dz straight from ab by peneo_pair_dz_fused (the four-wave kernel above 512 only on request), else by the
    # z GEMM's pair-dz epilogue - which does not regenerate the dropout mask: with it active, a plain GEMM and peneo_pair_dz
    dz_kernel = dec.fused_dz and ops.pair_dz_fused_supported(dt, D, nh)
    if dz_kernel and D <= 512:
        return PairRoute("bf16", backward="chunked", dz="fused")
    if dz_kernel and dec.fused_dz_wide:
        return PairRoute("bf16", backward="chunked", dz="wide", writes_x=dec.dz_wide_writes_x)
    return PairRoute("bf16", backward="chunked", dz="standalone" if p_hidden > 0.0 else "epilogue")


def strict_refusal(dec: "PEneoDecoder", route: PairRoute, dt: torch.dtype, D: int) -> Optional[str]:
    """The piece of a step on `route` that has no order-independent backward (deterministic mode 2 refuses it), or None."""
    if dt != torch.bfloat16:
        return "fp32 compute (the chunked decoder backward adds into d_ab and the pair_dz workspace with float atomics)"
    if dec.num_cls_layers != 2:
        return f"a {dec.num_cls_layers}-layer classifier (only the 2-layer heads have the fused backward; peneo_weighted_ce uses float atomics)"
    if dec.le_loss.ohem:
        return "OHEM (peneo_ohem_ce sums the kept pairs with float atomics)"
    if not (route.backward in ("saved", "fused") or route.dz == "fused"):
        return (f"the decoder backward at D = {D} without peneo_pair_bwd_fused and peneo_pair_dz_fused (the pair_dz GEMM epilogue "
                "adds with float atomics)")


class _StageParams(NamedTuple):
    """`stage_params()` by name"""
    shrink: Optional[tuple]          # (w0, b0, w3, b3) of the shrink MLP, None with the shrink off
    wc_w: torch.Tensor
    wc_b: torch.Tensor
    heads: List[tuple]               # per head (w, b) x num_cls_layers, flat


def _stage_params(dec: "PEneoDecoder", params: Sequence[torch.Tensor]) -> _StageParams:
    at = 4 if dec.decoder_shrink else 0
    k = 2 * dec.num_cls_layers
    heads = [tuple(params[at + 2 + h * k:at + 2 + (h + 1) * k]) for h in range(len(HEAD_NAMES))]
    return _StageParams(tuple(params[:4]) if dec.decoder_shrink else None, params[at], params[at + 1], heads)


class _DecoderStage(torch.autograd.Function):
    """shrink MLP -> [a | b] projection -> fused pair heads (+ CE).  Inputs: cropped sequence output
    [B*N, Hin]; outputs: total loss, 5 per-head losses, 5 logit maps.  The pair heads run on one PairRoute, decided by the
    forward and kept in ``saved["route"]`` (as run: without the saved form where its buffers did not fit)."""

    @staticmethod
    def forward(ctx, dec, seq, B, N, tags, want_logits, need_grad, mask, *params):
        wc, dt, dev = dec.weight_cache, seq.dtype, seq.device
        sp = _stage_params(dec, params)
        D = sp.wc_w.shape[0]
        # (DropoutSeeds.p_hidden, before the seeds are drawn: a refused step does not advance them)
        route = pair_route(dec, dt, D, need_grad, tags is not None, float(dec.dropout_p) if dec.training else 0.0,
                           has_mask=mask is not None)
        # strict deterministic mode: say which piece of this step has no order-independent backward, before any of it runs
        what = strict_refusal(dec, route, dt, D) if need_grad and tags is not None and deterministic_mode() == 2 else None
        if what:
            raise ValueError(f"deterministic mode 2 does not cover {what}; use mode 1 to run it and count it")
        seeds = DropoutSeeds(dec.training, dec.dropout_p, 0.0)
        saved = dict(seeds=seeds, seq=seq, B=B, N=N, D=D, route=route)
        ctx.dec, ctx.saved, ctx.params, ctx.has_loss = dec, saved, params, tags is not None
        h = seq
        if dec.decoder_shrink:
            w0, b0, w3, b3 = sp.shrink
            W0, W3 = wc.cast("dec.s0", w0, dt), wc.cast("dec.s3", w3, dt)
            z1 = torch.empty((h.shape[0], w0.shape[0]), dtype=dt, device=dev)
            s1 = ops.gemm(h, W0, bias=b0, act=ACT_SILU, preact=z1, drop_p=seeds.p_hidden, drop_seed=seeds.seed(901))
            z2 = torch.empty((h.shape[0], w3.shape[0]), dtype=dt, device=dev)
            s2 = ops.gemm(s1, W3, bias=b3, act=ACT_SILU, preact=z2, drop_p=seeds.p_hidden, drop_seed=seeds.seed(902))
            saved.update(z1=z1, s1=s1, z2=z2)
            h = s2
        saved["s2"] = h
        # [a | b] = h [Wc[:, :D]; Wc[:, D:]]^T + [0 | bc]
        Wab = dec.stacked_combine_weight(sp.wc_w, dt)
        bab = wc.cat_vec("dec.bab", [None, sp.wc_b], [sp.wc_b.numel(), sp.wc_b.numel()])      # (zeros | bias)
        ab = saved["ab"] = ops.gemm(h, Wab, bias=bab).view(B, N, 2 * D)
        cws = [dec.le_loss.weight] + [dec.link_loss.weight] * 4 if tags is not None else None
        if route.forward == "generic":
            if dec.num_cls_layers == 2 and tags is not None and dec.le_loss.ohem:
                raise ValueError(f"OHEM runs behind the fused pair-heads kernel only, and there is none for {dt} at D = {D}")
            logits, outs, extra = _generic_heads_forward(dec, ab, sp.heads, tags, cws, seeds, need_grad, want_logits)
            saved.update(extra)
            return _DecoderStage._outputs(ctx, outs, logits)
        w1s, b1s = [hd[0] for hd in sp.heads], [hd[1] for hd in sp.heads]
        w2s, b2s = [hd[2] for hd in sp.heads], [hd[3] for hd in sp.heads]
        b1cat = wc.cat_vec("dec.b1", b1s, [b.numel() for b in b1s])
        b2cat = wc.cat_vec("dec.b2", b2s, [b.numel() for b in b2s])
        pack_mxfp8 = lambda: wc.get(("dec.pack_mxfp8",), w1s + w2s, lambda: ops.pair_heads_pack_mxfp8(   # (its own pack and cache key)
            [w.detach() for w in w1s], [w.detach() for w in w2s]))
        if route.forward == "mxfp8_eval":
            assert not need_grad
            if D > 512:
                # (set_pair_heads_format("mxfp8", wide=True): the four-wave kernel, its own pack and cache key; the width picks
                # the op as it does on the "bf16" route, and pair_wide - the bf16 A/B arm - is not consulted)
                wpw = wc.get(("dec.pack_mxfp8_wide",), w1s + w2s, lambda: ops.pair_heads_pack_mxfp8_wide(
                    [w.detach() for w in w1s], [w.detach() for w in w2s]))
                res = ops.pair_heads_fwd_mxfp8_wide(ab, wpw, b1cat, b2cat, HEAD_CLASSES, want_logits=want_logits, tags=tags,
                                                    class_weights=cws)
                return _DecoderStage._finish(ctx, res, tags, cws)
            res = ops.pair_heads_fwd_mxfp8(ab, pack_mxfp8(), b1cat, b2cat, HEAD_CLASSES, want_logits=want_logits, tags=tags,
                                           class_weights=cws)
            return _DecoderStage._finish(ctx, res, tags, cws)
        # the Dropout between the two layers of every classifier (reference :261) acts on the [B, P, 5D] hidden inside the
        # kernel; the backward regenerates the mask from (p, seed)
        saved["k12_drop"] = (seeds.p_hidden, seeds.seed(903))
        bufs = None
        if route.save:
            # (step-sized buffers are kept between steps: engine.big_acquire.)  The saved form is an optimisation that costs memory:
            # when its buffers do not fit, the step continues on the recomputing backward, which needs none of them
            try:
                act_bytes = (ops.pair_save_e4m3_bytes if route.save_format == "e4m3" else ops.pair_save_bytes)(B, N, len(HEAD_NAMES), D)
                act, act_h = big_acquire("pair_act", (act_bytes,), torch.uint8, dev)
                try:
                    xr, xr_h = big_acquire("pair_x", (B * ops.pair_bwd_rows(N), D), dt, dev)
                except torch.cuda.OutOfMemoryError:
                    big_release("pair_act", act_h)
                    raise
                bufs = (act, xr)
                saved["pair_act"], saved["pair_x"] = (act, act_h), (xr, xr_h)
            except torch.cuda.OutOfMemoryError:
                big_clear(dev)
                route = saved["route"] = replace(route, forward="bf16", save=False, save_format="f16", backward="fused")
        if route.forward == "mxfp8_save":
            res = ops.pair_heads_fwd_mxfp8_save(ab, pack_mxfp8(), b1cat, b2cat, HEAD_CLASSES, want_logits=want_logits, tags=tags,
                                                class_weights=cws, want_dlogits=True, drop_p=seeds.p_hidden,
                                                drop_seed=seeds.seed(903), save_buffers=bufs)
            return _DecoderStage._finish(ctx, res, tags, cws)
        wp = wc.get(("dec.pack", dt), w1s + w2s, lambda: ops.pair_heads_pack(dt, [w.detach() for w in w1s],
                                                                             [w.detach() for w in w2s]))
        if route.lens:
            # skip_padded_pairs: the lengths from the cropped mask, on the device (no synchronisation); pairs that touch the padding
            # get the background row, the losses are those of the live pairs
            assert not need_grad and seeds.p_hidden == 0.0
            res = ops.pair_heads_fwd_lens(ab, ops.pair_lens_from_mask(mask, N), wp, b1cat, b2cat, HEAD_CLASSES,
                                          want_logits=want_logits, tags=tags, class_weights=cws)
            return _DecoderStage._finish(ctx, res, tags, cws)
        res = ops.pair_heads_fwd(ab, wp, b1cat, b2cat, HEAD_CLASSES, want_logits=want_logits,
                                 tags=tags, class_weights=cws, want_dlogits=need_grad and tags is not None,
                                 drop_p=seeds.p_hidden, drop_seed=seeds.seed(903), save=route.save, save_buffers=bufs,
                                 save_format=route.save_format)
        return _DecoderStage._finish(ctx, res, tags, cws)

    @staticmethod
    def _finish(ctx, res, tags, cws):
        """losses from the pair kernel's logits / partial rows (both formats)"""
        dec, saved = ctx.dec, ctx.saved
        dev = saved["ab"].device
        logits, partials, dlog = res[:3]
        outs = [None] * 6
        if tags is not None and dec.le_loss.ohem:
            # OHEM: the kept pairs of each head are chosen from its finished logit map; the un-normalised dlogits of the
            # dropped pairs are zeroed in place, so the backward below runs unchanged with scale_h = ratio_h / (k_pos + k_neg)
            ratio = dec.loss_ratio_tensor(dev)
            out8 = torch.empty((len(HEAD_NAMES), 8), dtype=torch.float32, device=dev)
            dls = torch.zeros(sum(HEAD_CLASSES), dtype=torch.float32, device=dev)
            ws, off = None, 0
            for h, c in enumerate(HEAD_CLASSES):
                lossmod = dec.le_loss if h == 0 else dec.link_loss
                _, ws = ops.ohem_ce(logits[h], tags[h], cws[h], lossmod.num_hard_positive, lossmod.num_hard_negative,
                                    dlogits=dlog[h] if dlog is not None else None, out8=out8[h], dl_sum=dls[off:off + c],
                                    workspace=ws)
                off += c
            losses, scale = ops.ohem_finish(out8, ratio)
        elif tags is not None:
            losses, scale, dls = ops.loss_finish(partials, dec.loss_ratio_tensor(dev), sum(HEAD_CLASSES))
        if tags is not None:
            outs = [losses[5]] + [losses[i] for i in range(5)]
            saved.update(scale=scale[0], inv_den=scale[1], dlog=dlog, dls=dls)
        return _DecoderStage._outputs(ctx, outs, logits if logits is not None else [None] * 5)

    @staticmethod
    def _outputs(ctx, outs, logits):
        """the stage's return value and what autograd has to know about it"""
        # ONE call: each call replaces ctx.non_differentiable.  The logits carry no gradient (the CE is fused into the
        # kernel that produces them), so a loss built on them outside the model raises instead of training on zeros.
        ctx.mark_non_differentiable(*[lg for lg in logits if lg is not None])
        ctx.set_materialize_grads(False)             # unused loss outputs arrive as None in backward, not as zero tensors
        return tuple(outs) + tuple(logits)

    @staticmethod
    def backward(ctx, d_loss, d_le=None, d_elh=None, d_elt=None, d_lgh=None, d_lgt=None, *unused):
        dec, sv = ctx.dec, ctx.saved
        if not ctx.has_loss:
            raise PeneoHipError("backward through the PEneo decoder needs the five *_shaking_tag label maps")
        dev = sv["ab"].device
        # dlogits are un-normalised: scale_h = ratio_h / den_h, times the incoming d(loss); the five per-head losses are
        # ordinary differentiable outputs as in the reference (peneo_decoder.py:375-428): their own incoming gradients
        # enter head by head as d(head loss) / den_h = d_head * scale_h / ratio_h
        scale = sv["scale"] * (d_loss.to(torch.float32) if d_loss is not None else 0.0)
        d_heads = [d_le, d_elh, d_elt, d_lgh, d_lgt]
        if any(d is not None for d in d_heads):
            extra = torch.stack([d.to(torch.float32).reshape(()) if d is not None else torch.zeros((), device=dev)
                                 for d in d_heads])
            scale = scale + extra * sv["inv_den"]
        route = sv["route"]                          # (what the forward ran: the decoder's switches may have changed since)
        if route.backward == "generic":
            d_ab, head_grads = _generic_heads_backward(dec, sv, _stage_params(dec, ctx.params).heads, scale)
            return _DecoderStage._front_backward(ctx, d_ab, head_grads)
        if route.backward == "chunked":
            return _DecoderStage._backward_chunked(ctx, scale)
        return _DecoderStage._backward_fused(ctx, scale)

    @staticmethod
    def _head_operands(ctx):
        """What both forms of the two-layer backward start from: (w1s, W1cat [nh*D, D], b1cat, zeroed dW1cat, contiguous w2s)."""
        dec, sv = ctx.dec, ctx.saved
        heads = _stage_params(dec, ctx.params).heads
        wc, D, ab = dec.weight_cache, sv["D"], sv["ab"]
        w1s, b1s = [hd[0] for hd in heads], [hd[1] for hd in heads]
        W1cat = wc.cat_rows("dec.w1cat", w1s, ab.dtype)                      # [nh*D, D]
        b1cat = wc.cat_vec("dec.b1", b1s, [b.numel() for b in b1s])
        dW1cat = torch.zeros((len(heads) * D, D), dtype=torch.float32, device=ab.device)
        return w1s, W1cat, b1cat, dW1cat, [hd[2].detach().contiguous() for hd in heads]

    @staticmethod
    def _backward_fused(ctx, scale):
        """Routes "saved" and "fused".  ONE kernel for the whole batch: x, z, dz, du = dz W1 and the sums into d_a / d_b never leave
        the chip except dz and x themselves (block order), which the one remaining GEMM dW1 = dz^T x reads back once."""
        dec, sv, params = ctx.dec, ctx.saved, ctx.params
        # (W1cat is not read here; looking it up keeps it among the working copies an emitting optimizer writes)
        w1s, _, b1cat, dW1cat, w2d = _DecoderStage._head_operands(ctx)
        B, N, D, ab = sv["B"], sv["N"], sv["D"], sv["ab"]
        dt, dev = ab.dtype, ab.device
        nh = len(HEAD_NAMES)
        drop_p, drop_seed = sv["k12_drop"]
        # (under the deterministic mode: one workspace row per workgroup of the launch, ops.pair_bwd_workspace asks the library)
        dz_ws = ops.pair_bwd_workspace(B, N, nh, D, dev)
        d_ab = torch.empty((B, N, 2 * D), dtype=torch.float32, device=dev)   # the fused kernel overwrites d_ab
        wp2 = dec.weight_cache.get(("dec.pack2", dt), w1s, lambda: ops.pair_bwd_pack([w.detach() for w in w1s]))
        rows = ops.pair_bwd_rows(N)
        # (a kept buffer may still be read by an earlier decoder backward of THIS autograd run - two forwards summed into one loss -
        # whose side-stream join is deferred to the end of the backward: join first; nothing is pending in the usual step)
        join_pending()
        dzbuf, dz_h = big_acquire("pair_dz", (B * rows, nh * D), dt, dev)
        dza = ops.pair_dz_args(D, HEAD_CLASSES, sv["dlog"], w2d, scale, drop_p=drop_p, drop_seed=drop_seed)
        if sv["route"].backward == "saved":
            xbuf1, x_h = sv.pop("pair_x")
            act, act_h = sv.pop("pair_act")
            ops.pair_bwd_saved(ab, wp2, dza, act, dzbuf, d_ab, dz_ws, act_format=sv["route"].save_format)   # (what the forward wrote)
            big_release("pair_act", act_h)           # (read by that launch only: the next forward's stores are ordered behind it)
        else:
            xbuf1, x_h = big_acquire("pair_x", (B * rows, D), dt, dev)
            ops.pair_bwd_fused(ab, wp2, b1cat, dza, dzbuf, xbuf1, d_ab, dz_ws)
        # dz and x are read by the dW1 GEMM below, on the side stream or here: whoever takes them next (the next step's forward /
        # backward, on the main stream) is issued after this backward has ended, i.e. behind the join of that side stream
        big_release("pair_dz", dz_h)
        big_release("pair_x", x_h)
        # dW1 = dz^T x (2 ms of pure MFMA work, needed by nobody until the optimizer) runs on the side stream beside the
        # shrink-MLP backward and the first encoder layers, whose short kernels leave CUs idle; joined one stage later
        if dec.dw1_on_side:
            main = torch.cuda.current_stream()
            side = dec.side_stream(dev)
            ev = torch.cuda.Event()
            ev.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ev)
                # few, long workgroups: the split a GEMM gets when it runs alone fills all 512 resident slots, and the
                # main stream's kernels then find no CU to be dispatched to until it ends (measured: the stage after the
                # decoder stood still for 1.8 ms).  About one workgroup on every second CU runs ~7 ms beside the whole
                # encoder backward instead and is joined when the backward ends (split 11 / 7 / 5 / 4 / 3: 18.56 /
                # 18.79 / 18.34 / 18.16 / 18.10 ms per step on one box).
                # Only when the join can wait for the end of the backward (fresh .grad tensors, no DDP hooks reading them).
                can_hold = dec.dw1_hold and can_defer(params)
                # (D = 512: 80 tiles, i.e. ONE workgroup per tile from that target, would run 23 ms - longer than the 24-layer
                # encoder backward it hides behind; no workgroup gets more than dw1_side_rows rows of K: split 2 / 3 / 4 / 6 at
                # config 4: 30.5 / 31.1 / 32.8 / 32.7 ms per step)
                # (where peneo_gemm runs this product on 384 x 192 one-per-CU tiles -- nh D = 1920 x D = 384: 10 tiles --
                # the count is 10 x split workgroups, dw1_side_big_wgs of them: DESIGN 23 has the sweep)
                if ops.gemm_nn384_takes(nh * D, D, B * rows, dt):
                    tiles, wgs = (nh * D // 384) * (D // 192), dec.dw1_side_big_wgs
                else:
                    tiles, wgs = -(-nh * D // 128) * -(-D // 128), dec.dw1_side_wgs
                # (not held, or on the main stream below: the step pays the launch's alone-time, and ops.gemm picks the split of
                # a launch that has the chip to itself - one round of CUs on the 384 x 192 tiles, choose_split_k_nn384)
                split = None if not can_hold else \
                    dec.dw1_side_split or max(1, wgs // tiles, -(-B * rows // dec.dw1_side_rows))
                with ops.kernel_timer("dw1_gemm"):
                    ops.gemm(dzbuf, xbuf1, a_kmajor=False, b_kmajor=False, out=dW1cat, split_k=split)
            ctx.side_work = (side, (dzbuf, xbuf1, dW1cat, ab), can_hold)
        else:
            with ops.kernel_timer("dw1_gemm"):
                ops.gemm(dzbuf, xbuf1, a_kmajor=False, b_kmajor=False, out=dW1cat)
        return _DecoderStage._finish_backward(ctx, scale, dW1cat, dz_ws, d_ab)

    @staticmethod
    def _backward_chunked(ctx, scale):
        """Route "chunked": the pair activations re-created chunk by chunk (rows of the triangle), dz by the route's producer."""
        dec, sv = ctx.dec, ctx.saved
        w1s, W1cat, b1cat, dW1cat, w2d = _DecoderStage._head_operands(ctx)
        B, N, D, ab, route = sv["B"], sv["N"], sv["D"], sv["ab"], sv["route"]
        dt, dev = ab.dtype, ab.device
        nh = len(HEAD_NAMES)
        drop_p, drop_seed = sv["k12_drop"]
        # rows the dz producers spread their partial sums over: 256 for the fused kernels / the GEMM epilogue, the full
        # 1024 for the stand-alone peneo_pair_dz (the classifier dropout active)
        dz_ws = ops.pair_dz_workspace(nh, D, dev, slots=256 if drop_p == 0.0 else None)
        d_ab = torch.zeros((B, N, 2 * D), dtype=torch.float32, device=dev)   # the chunked path accumulates into d_ab
        chunks = _row_chunks(N, dec.bwd_chunk_pairs)
        maxp = max((i1 * N - i1 * (i1 - 1) // 2) - (i0 * N - i0 * (i0 - 1) // 2) for i0, i1 in chunks)
        # Two-stage pipeline over the pair chunks on two HIP streams: stage 1 (x, z GEMM whose epilogue turns z into dz:
        # VALU-bound) runs one chunk ahead of stage 2 (dW1 and dx GEMMs + the scatter into d_ab: MFMA-bound), so the two
        # kinds of work share the CUs instead of alternating.  Buffers are double-buffered; events order the hand-offs.
        xbuf = [torch.empty((maxp, D), dtype=dt, device=dev) for _ in range(2)]
        prebuf = [torch.empty((maxp, D), dtype=dt, device=dev) for _ in range(2)]   # a_i + b_j: SiLU' source of the dx GEMM
        zbuf = [torch.empty((maxp, nh * D), dtype=dt, device=dev) for _ in range(2)]
        dxbuf = torch.empty((maxp, D), dtype=dt, device=dev)
        dz_from_ab = route.dz in ("fused", "wide")     # peneo_pair_dz_fused, eight-wave or four-wave
        if dz_from_ab and dz_ws.shape[0] < ops.pair_dz_fused_workspace_rows(maxp):
            # (deterministic mode: peneo_pair_dz_fused gives every workgroup of a launch a workspace row of its own)
            dz_ws = torch.zeros((ops.pair_dz_fused_workspace_rows(maxp), 4 * nh * D), dtype=torch.float32, device=dev)
        if dz_from_ab:
            w2s = [hd[2] for hd in _stage_params(dec, ctx.params).heads]
            wp = dec.weight_cache.get(("dec.pack", dt), w1s + w2s, lambda: ops.pair_heads_pack(dt, [w.detach() for w in w1s],
                                                                                               [w.detach() for w in w2s]))
        main = torch.cuda.current_stream()
        side = main if os.environ.get("PENEO_DEC_STREAMS", "2") == "1" else dec.side_stream(dev)   # "1": strictly serial
        ready = [torch.cuda.Event() for _ in range(2)]
        done = [torch.cuda.Event() for _ in range(2)]
        side.wait_stream(main)                       # d_ab / dW1cat zero fills, ab, weights
        idx = 0
        for b in range(B):
            for (i0, i1) in chunks:
                k = idx & 1
                p0 = i0 * N - i0 * (i0 - 1) // 2
                p1 = i1 * N - i1 * (i1 - 1) // 2
                npairs = p1 - p0
                x, z, dx, pre = xbuf[k][:npairs], zbuf[k][:npairs], dxbuf[:npairs], prebuf[k][:npairs]
                if idx >= 2:
                    main.wait_event(done[k])         # stage 2 of chunk idx-2 has released x[k] / z[k]
                dza = ops.pair_dz_args(D, HEAD_CLASSES, [sv["dlog"][h][b, p0:p1] for h in range(nh)], w2d, scale,
                                       drop_p=drop_p, drop_seed=drop_seed, drop_doc=b, drop_pair0=p0)
                if dz_from_ab:
                    # dz straight from ab: x lives in registers, z in the MFMA accumulators; x / pre are only needed by
                    # the dW1 / dx GEMMs (measured best split of the two queues: x and dW1 on the main stream)
                    if route.writes_x:
                        ops.pair_dz_fused(ab[b], i0, i1, wp, b1cat, dza, z, dz_ws, x, pre)
                    else:
                        ops.pair_x_fwd(ab[b], i0, i1, x, pre)
                        ops.pair_dz_fused(ab[b], i0, i1, wp, b1cat, dza, z, dz_ws)
                    ops.gemm(z, x, a_kmajor=False, b_kmajor=False, out=dW1cat, accumulate=True)
                else:
                    ops.pair_x_fwd(ab[b], i0, i1, x, pre)
                    if route.dz == "standalone":
                        ops.gemm(x, W1cat, bias=b1cat, out=z)
                        ops.pair_dz(z, npairs, D, HEAD_CLASSES, None, None, dz_ws, None, args=dza)
                    else:
                        # z = x W1^T + b1 and, in the same kernel's epilogue, z -> dz plus the dW2 / db1 partial sums
                        ops.gemm(x, W1cat, bias=b1cat, out=z, pair_dz=dza, pair_dz_ws=dz_ws)
                ready[k].record(main)
                with torch.cuda.stream(side):
                    side.wait_event(ready[k])
                    if idx > 0:
                        side.wait_event(done_x)      # dxbuf is single-buffered: the previous chunk's scatter has read it
                    if not dz_from_ab:
                        ops.gemm(z, x, a_kmajor=False, b_kmajor=False, out=dW1cat, accumulate=True)
                    # du = (dz W1) * SiLU'(a_i + b_j) in the GEMM epilogue, then plain segmented sums into d_a / d_b
                    ops.gemm(z, W1cat, b_kmajor=False, out=dx, grad_src=pre, grad_act=ACT_SILU)
                    ops.pair_x_bwd(ab[b], i0, i1, dx, d_ab[b], premultiplied=True)
                    done[k].record(side)
                    done_x = done[k]
                idx += 1
        main.wait_stream(side)
        return _DecoderStage._finish_backward(ctx, scale, dW1cat, dz_ws, d_ab)

    @staticmethod
    def _finish_backward(ctx, scale, dW1cat, dz_ws, d_ab):
        """Second half of the two-layer backward: parameter gradients of the heads from the accumulated sums."""
        sv = ctx.saved
        D = sv["D"]
        nh = len(HEAD_NAMES)
        dw2, db1cat = ops.pair_dz_finish(dz_ws, nh, D, HEAD_CLASSES)
        # db2 of head h = its dlogit sums x scale_h: one multiply for all heads (was one tiny kernel per head on the main stream)
        hidx = _HEAD_OF_CLASS_SLOT.get(scale.device)
        if hidx is None:
            hidx = _HEAD_OF_CLASS_SLOT[scale.device] = torch.tensor([h for h, c in enumerate(HEAD_CLASSES) for _ in range(c)],
                                                                    device=scale.device)
        db2cat = sv["dls"] * scale[hidx]
        head_grads = []
        off = 0
        for h in range(nh):
            c = HEAD_CLASSES[h]
            head_grads += [dW1cat[h * D:(h + 1) * D], db1cat[h * D:(h + 1) * D], dw2[h], db2cat[off:off + c]]
            off += c
        return _DecoderStage._front_backward(ctx, d_ab, head_grads)

    @staticmethod
    def _front_backward(ctx, d_ab, head_grads):
        """Back through the [a | b] projection and the shrink MLP; `head_grads`: the heads' parameter gradients in
        stage_params() order."""
        dec, sv, params = ctx.dec, ctx.saved, ctx.params
        wc = dec.weight_cache
        B, N, D = sv["B"], sv["N"], sv["D"]
        ab, seeds = sv["ab"], sv["seeds"]
        dt = ab.dtype
        sp = _stage_params(dec, params)
        d_ab2 = ops.cast(d_ab.view(B * N, 2 * D), dt) if dt != torch.float32 else d_ab.view(B * N, 2 * D)
        s2 = sv["s2"]
        Wab = dec.stacked_combine_weight(sp.wc_w, dt)
        dWab = ops.gemm(d_ab2, s2, a_kmajor=False, b_kmajor=False, out_dtype=torch.float32)     # [2D, D]
        d_wc = torch.cat([dWab[:D], dWab[D:]], dim=1)
        d_bc = ops.colsum(d_ab2[:, D:])
        grads = []
        if dec.decoder_shrink:
            w0, b0, w3, b3 = sp.shrink
            W0, W3 = wc.cast("dec.s0", w0, dt), wc.cast("dec.s3", w3, dt)
            d_z2 = ops.gemm(d_ab2, Wab, b_kmajor=False, grad_src=sv["z2"], grad_act=ACT_SILU,
                            drop_p=seeds.p_hidden, drop_seed=seeds.seed(902))
            dw3 = ops.gemm(d_z2, sv["s1"], a_kmajor=False, b_kmajor=False, out_dtype=torch.float32)
            db3 = ops.colsum(d_z2)
            d_z1 = ops.gemm(d_z2, W3, b_kmajor=False, grad_src=sv["z1"], grad_act=ACT_SILU,
                            drop_p=seeds.p_hidden, drop_seed=seeds.seed(901))
            dw0 = ops.gemm(d_z1, sv["seq"], a_kmajor=False, b_kmajor=False, out_dtype=torch.float32)
            db0 = ops.colsum(d_z1)
            d_seq = ops.gemm(d_z1, W0, b_kmajor=False)
            grads += [dw0, db0, dw3, db3]
        else:
            d_seq = ops.gemm(d_ab2, Wab, b_kmajor=False)
        grads += [d_wc, d_bc]
        grads += list(head_grads)
        grads = tuple(g if p.requires_grad else None for g, p in zip(grads, params))
        side_work = getattr(ctx, "side_work", None)
        if side_work is not None:                    # (the dW1 GEMM of _backward_fused)
            side, keep, can_hold = side_work
            ctx.side_work = None
            if can_defer(params):
                if can_hold:   # the data-parallel wrapper lays these out last: their data is complete only at the end of the backward
                    mark_late([hd[0] for hd in sp.heads])
                defer_join(side, keep=keep, hold=can_hold)
            else:
                torch.cuda.current_stream().wait_stream(side)
        return (None, d_seq, None, None, None, None, None, None) + grads


def _generic_heads_forward(dec, ab, heads, tags, cws, seeds, need_grad, want_logits):
    """Classifier heads of any depth over the materialised pair activations, one document at a time: x = SiLU(a_i + b_j)
    [P, D] (peneo_pair_x_fwd), per head (Linear + SiLU + Dropout) x (k - 1) as GEMMs with fused epilogues, the D -> C layer as
    a GEMM into fp32 logits, class-weighted CE by peneo_weighted_ce (reference model/peneo_decoder.py:253-271,315-336).
    Nothing but the un-normalised dlogits is kept for the backward (it recomputes the activations document by document)."""
    B, N, D2 = ab.shape
    D = D2 // 2
    dt, dev = ab.dtype, ab.device
    wc = dec.weight_cache
    nh, k = len(HEAD_NAMES), dec.num_cls_layers
    P = N * (N + 1) // 2
    logits = [torch.empty((B, P, c), dtype=torch.float32, device=dev) for c in HEAD_CLASSES]
    num = torch.zeros(nh, dtype=torch.float32, device=dev)
    den = torch.zeros(nh, dtype=torch.float32, device=dev)
    dlog = [torch.empty((B, P, c), dtype=torch.float32, device=dev) for c in HEAD_CLASSES] if (need_grad and tags is not None) else None
    x = torch.empty((P, D), dtype=dt, device=dev)
    for b in range(B):
        ops.pair_x_fwd(ab[b], 0, N, x)
        for h in range(nh):
            cur = x
            for l in range(k - 1):
                W = wc.cast(f"dec.h{h}.{l}", heads[h][2 * l], dt)
                cur = ops.gemm(cur, W, bias=heads[h][2 * l + 1], act=ACT_SILU, drop_p=seeds.p_hidden,
                               drop_seed=seeds.seed(1000 + ((b * nh + h) * 8 + l)))
            Wl = wc.cast(f"dec.h{h}.{k - 1}", heads[h][2 * (k - 1)], dt)
            ops.gemm(cur, Wl, bias=heads[h][2 * (k - 1) + 1], out=logits[h][b])
            if tags is not None:
                n_, d_, dl_ = ops.weighted_ce(logits[h][b], tags[h][b], cws[h], want_dlogits=dlog is not None)
                num[h] += n_[0]
                den[h] += d_[0]
                if dlog is not None:
                    dlog[h][b].copy_(dl_)
    outs = [None] * 6
    extra = {}
    if tags is not None:
        ratio = dec.loss_ratio_tensor(dev)
        losses = num / den
        outs = [(losses * ratio).sum()] + [losses[i] for i in range(nh)]
        extra = dict(scale=ratio / den, inv_den=1.0 / den, dlog=dlog)
    return logits, outs, extra


def _generic_heads_backward(dec, sv, heads, scale):
    """Backward of _generic_heads_forward: per document and head the hidden activations are recomputed, then
    dlogits -> (dW, db) of every layer and dx, summed over the heads; d_ab = pair_x_bwd(dx).  -> (d_ab, head gradients in
    stage_params() order)."""
    ab, seeds = sv["ab"], sv["seeds"]
    B, N, D2 = ab.shape
    D = D2 // 2
    dt, dev = ab.dtype, ab.device
    wc = dec.weight_cache
    nh, k = len(HEAD_NAMES), dec.num_cls_layers
    P = N * (N + 1) // 2
    dlog = sv["dlog"]
    gW = [[torch.zeros(heads[h][2 * l].shape, dtype=torch.float32, device=dev) for l in range(k)] for h in range(nh)]
    gb = [[torch.zeros(heads[h][2 * l + 1].shape, dtype=torch.float32, device=dev) for l in range(k)] for h in range(nh)]
    d_ab = torch.zeros((B, N, D2), dtype=torch.float32, device=dev)
    x = torch.empty((P, D), dtype=dt, device=dev)
    dx32 = torch.empty((P, D), dtype=torch.float32, device=dev)
    for b in range(B):
        ops.pair_x_fwd(ab[b], 0, N, x)
        dx32.zero_()
        for h in range(nh):
            Ws = [wc.cast(f"dec.h{h}.{l}", heads[h][2 * l], dt) for l in range(k)]
            acts, pres = [x], []
            for l in range(k - 1):
                z = torch.empty((P, D), dtype=dt, device=dev)
                acts.append(ops.gemm(acts[-1], Ws[l], bias=heads[h][2 * l + 1], act=ACT_SILU, preact=z, drop_p=seeds.p_hidden,
                                     drop_seed=seeds.seed(1000 + ((b * nh + h) * 8 + l))))
                pres.append(z)
            g = (dlog[h][b] * scale[h]).to(dt)                                   # [P, C]: d loss / d logits of this document
            ops.gemm(g, acts[k - 1], a_kmajor=False, b_kmajor=False, out=gW[h][k - 1], accumulate=True)
            ops.colsum(g, out=gb[h][k - 1], accumulate=True)
            for l in range(k - 2, -1, -1):
                up = g if l == k - 2 else dz
                dz = ops.gemm(up, Ws[l + 1], b_kmajor=False, grad_src=pres[l], grad_act=ACT_SILU, drop_p=seeds.p_hidden,
                              drop_seed=seeds.seed(1000 + ((b * nh + h) * 8 + l)))
                ops.gemm(dz, acts[l], a_kmajor=False, b_kmajor=False, out=gW[h][l], accumulate=True)
                ops.colsum(dz, out=gb[h][l], accumulate=True)
            ops.gemm(g if k == 1 else dz, Ws[0], b_kmajor=False, out=dx32, accumulate=True)
        ops.pair_x_bwd(ab[b], 0, N, ops.cast(dx32, dt) if dt != torch.float32 else dx32, d_ab[b])
    head_grads = []
    for h in range(nh):
        for l in range(k):
            head_grads += [gW[h][l], gb[h][l]]
    return d_ab, head_grads


class PEneoDecoder(nn.Module):
    """PEneo pair extraction downstream head (reference :201-443)."""

    def train(self, mode: bool = True):
        """Leaving training mode hands the step-sized buffers the saved-activation backward keeps between steps (engine.big_acquire:
        9.2 GB at 8 x 511 tokens) back to the allocator: inference needs none of them, the next training step takes them again."""
        if not mode:
            big_clear()
        return super().train(mode)

    def side_stream(self, device, which: int = 0) -> "torch.cuda.Stream":
        """Extra HIP streams of the chunked backward (created once per device)."""
        from .engine import side_stream
        return side_stream(device, "dec" if which == 0 else f"dec{which}")

    def __init__(self, config, input_size: int) -> None:
        super().__init__()
        self.decoder_shrink = config.peneo_decoder_shrink
        hidden = config.backbone_config["hidden_size"]
        self.dropout_p = config.backbone_config["hidden_dropout_prob"]
        self.num_cls_layers = int(config.peneo_classifier_num_layers)
        if self.num_cls_layers < 1:
            raise ValueError("peneo_classifier_num_layers must be >= 1")
        if self.decoder_shrink:
            D = hidden // 2
            self.shrink_projection = nn.Sequential(
                nn.Linear(input_size, hidden), nn.SiLU(), nn.Dropout(self.dropout_p),
                nn.Linear(hidden, D), nn.SiLU(), nn.Dropout(self.dropout_p))
        else:
            D = input_size
        if D % 32 != 0:
            raise ValueError(f"decoder hidden size {D} must be a multiple of 32 for the MFMA pair-heads kernel")
        self.decoder_hidden_size = D
        self.pair_heads_format = "bf16"   # set_pair_heads_format
        self.pair_heads_train_format = "bf16"   # set_pair_heads_train_format
        self.pair_act_format = "f16"            # set_pair_act_format
        # forwards without gradients that received an attention mask skip the pairs touching the padding (set_skip_padded_pairs)
        self.skip_padded_pairs = os.environ.get("PENEO_SKIP_PADDED_PAIRS", "0") == "1"
        self.handshaking_kernel = HandshakingKernel(D)
        self.inference_mode = config.inference_mode

        def build_classifier(out_size: int) -> nn.Module:
            """Reference :231-271: one Linear for a single layer, else (Linear, SiLU, Dropout) x (k - 1) + Linear; the shipped
            k = 2 runs in the fused pair kernels, every other depth in the materialising per-document path below."""
            if self.num_cls_layers == 1:
                return nn.Linear(D, out_size)
            mods = []
            for _ in range(self.num_cls_layers - 1):
                mods += [nn.Linear(D, D), nn.SiLU(), nn.Dropout(self.dropout_p)]
            mods.append(nn.Linear(D, out_size))
            return nn.Sequential(*mods)

        self.line_extraction_fc = build_classifier(2)
        self.ent_linking_h2h_fc = build_classifier(3)
        self.ent_linking_t2t_fc = build_classifier(3)
        self.line_grouping_h2h_fc = build_classifier(3)
        self.line_grouping_t2t_fc = build_classifier(3)

        self.loss_ratio = config.peneo_loss_ratio
        if self.loss_ratio is not None:
            assert len(self.loss_ratio) == 5, "loss_ratio must be a list of 5 elements"
        cw = config.peneo_category_weights
        assert cw is not None and len(cw) == 3, "category_weights must be a list of 3 elements"
        self.link_loss = _ClassWeightedCE(torch.tensor(cw).float(), config.peneo_ohem_num_positive,
                                          config.peneo_ohem_num_negative)
        self.le_loss = _ClassWeightedCE(torch.tensor(cw[:-1]).float(), config.peneo_ohem_num_positive,
                                        config.peneo_ohem_num_negative)
        self.weight_cache = WeightCache()
        self.train_logits = False    # True: PEneoOutput.*_shaking_outputs are also written in training steps
        # pairs per backward chunk: the z / dz buffer is chunk x 5D (a whole base document is 0.5 GB in bf16, small against
        # 288 GB of HBM), and long launches amortise tile tails and the split-k reduction of the weight-gradient GEMM
        self.bwd_chunk_pairs = int(os.environ.get("PENEO_BWD_CHUNK_PAIRS", 1 << 18))
        self.fused_dz = os.environ.get("PENEO_DZ_FUSED", "1") != "0"            # bf16: dz without x / z in memory
        self.fused_bwd = os.environ.get("PENEO_BWD_FUSED", "1") != "0"          # bf16: the whole pair-space backward in one kernel
        self.save_pair_act = os.environ.get("PENEO_PAIR_SAVE", "1") != "0"      # D = 384: the forward saves the classifiers' pre-activations
        self.pair_wide = os.environ.get("PENEO_PAIR_WIDE", "1") != "0"          # bf16, 512 < D <= 1024: the fused four-wave forward
        # bf16, 512 < D <= 1024: the chunked backward takes the fused_dz branch on the four-wave peneo_pair_dz_fused (needs fused_dz).
        # Off by default: DESIGN 28 has the measurement.  dz_wide_writes_x: that kernel also stores x / a_i + b_j (no peneo_pair_x_fwd launch)
        self.fused_dz_wide = os.environ.get("PENEO_DZ_FUSED_WIDE", "0") == "1"
        self.dz_wide_writes_x = os.environ.get("PENEO_DZ_WIDE_X", "0") == "1"
        self.dw1_on_side = os.environ.get("PENEO_DW1_SIDE", "1") != "0"          # its dW1 GEMM beside the following stages
        self.dw1_hold = os.environ.get("PENEO_DW1_HOLD", "1") != "0"             # ... joined at the end of the backward only
        self.dw1_side_split = int(os.environ.get("PENEO_DW1_SPLIT", "0"))   # fixed split-k of that GEMM; 0: from the targets below
        self.dw1_side_rows = 600_000     # ... none of them with more rows of K than this
        self.dw1_side_wgs = 144          # ... of about this many long workgroups (measured 18.10 ms per step against 18.56 at 495)
        self.dw1_side_big_wgs = 60       # ... of this many 8-wave workgroups where the GEMM runs on 384 x 192 tiles (10 tiles x split 6:
        #     15.19 ms per step against 15.67 / 15.51 / 15.46 at split 5 / 7 / 8 and 15.79 on the 128 x 128 kernel, profiles/r07_dw1_nn384.txt)
        self._ratio = {}

    def set_pair_heads_format(self, fmt: str, *, wide: bool = False) -> None:
        """"bf16" (default): the pair heads run in the compute dtype.  "mxfp8": eval forwards (no gradients) run the first
        layer of the five classifiers on block-scaled e4m3 (include/peneo_hip.h, peneo_pair_heads_fwd_mxfp8); a forward with
        gradients raises.  Needs the 2-layer classifiers and a decoder width the kernel holds: up to 512, and with ``wide=True``
        also 512 < D <= 1024 (the decoder shrink off: peneo_pair_heads_fwd_mxfp8_wide, same numeric contract).  ``wide`` changes
        nothing at D <= 512."""
        if fmt not in ("bf16", "mxfp8"):
            raise ValueError(f"unknown pair-heads format {fmt!r} (expected 'bf16' or 'mxfp8')")
        if fmt == "mxfp8":
            D, nh = self.decoder_hidden_size, len(HEAD_NAMES)
            if self.num_cls_layers != 2:
                raise ValueError(f"mxfp8 pair heads need peneo_classifier_num_layers == 2, not {self.num_cls_layers}")
            if not (ops.pair_mxfp8_supported(D, nh) or (wide and ops.pair_mxfp8_wide_supported(D, nh))):
                hint = "" if wide or not ops.pair_mxfp8_wide_supported(D, nh) else \
                    " (above 512 the kernel is opt-in: set_pair_heads_format('mxfp8', wide=True))"
                raise ValueError(f"mxfp8 pair heads do not support decoder width D = {D}{hint}")
            if self.skip_padded_pairs:
                raise ValueError("the mxfp8 pair heads have no length-aware form: switch set_skip_padded_pairs(False) first")
        self.pair_heads_format = fmt

    def set_skip_padded_pairs(self, on: bool) -> None:
        """False (default; PENEO_SKIP_PADDED_PAIRS=1 turns it on at construction): every forward scores all P = N (N + 1) / 2 pairs
        of the padded sequence.  True: a forward that needs no gradients and received an ``attention_mask`` takes each document's
        length from it (1 + the last non-zero position of the cropped mask) and runs the fused pair heads over the pairs of real
        tokens only (peneo_pair_heads_fwd_lens).  The maps keep their [B, P, C] layout; a pair that touches the padding holds
        (0, -1e30, ...), which decodes to nothing, and the returned losses are the LIVE-PAIR losses: class-weighted means over the
        pairs of real tokens, not the reference's means over all P pairs.  Forwards with gradients (the training objective includes
        the padded pairs), forwards without a mask, the materialising path (other classifier depths / widths) and OHEM losses are
        exactly what they are with the switch off.  Not together with set_pair_heads_format("mxfp8"): ValueError."""
        if on and self.pair_heads_format == "mxfp8":
            raise ValueError("skip_padded_pairs has no mxfp8 form: switch back with set_pair_heads_format('bf16') first")
        self.skip_padded_pairs = bool(on)

    def set_pair_heads_train_format(self, fmt: str, compute_dtype: torch.dtype = torch.bfloat16) -> None:
        """"bf16" (default): forwards with gradients run the pair heads in the compute dtype.  "mxfp8": a forward that needs
        gradients and would save its activations for the fused backward (pair_heads_fwd(save=True)) runs the first layer of the
        five classifiers on block-scaled e4m3 instead (peneo_pair_heads_fwd_mxfp8_save); the backward is unchanged, so the
        gradients are straight-through on the bf16 weights, taken at the forward's quantized z.  Independent of
        set_pair_heads_format (forwards without gradients).  Needs bf16 compute, the 2-layer classifiers, a width both the saved
        backward and the MXFP8 kernel hold, and the saved backward switched on (_check_saved_format)."""
        if fmt not in ("bf16", "mxfp8"):
            raise ValueError(f"unknown pair-heads train format {fmt!r} (expected 'bf16' or 'mxfp8')")
        if fmt == "mxfp8":
            self._check_saved_format("mxfp8", compute_dtype, "switch back with set_pair_act_format('f16') first", setter=True)
        self.pair_heads_train_format = fmt

    def set_pair_act_format(self, fmt: str, compute_dtype: torch.dtype = torch.bfloat16) -> None:
        """"f16" (default): a train step that saves the classifiers' pre-activations for the fused backward (save_pair_act) keeps them
        as f16, 2 bytes per pair and hidden unit.  "e4m3": as e4m3fn bytes (peneo_pair_heads_fwd_save_e4m3 / peneo_pair_bwd_saved_e4m3;
        include/peneo_hip.h): half the buffer and half the bytes streamed; the forward's losses are unchanged, the backward takes
        SiLU and SiLU' at z rounded to 3 mantissa bits (|z| above 448 saturates).  Needs bf16 compute, the 2-layer classifiers, a width
        the e4m3 form holds (384) and the saved backward switched on (_check_saved_format); not together with
        set_pair_heads_train_format("mxfp8"), whose kernel writes f16 records.
        Memory: the step-sized buffers are kept between steps and a kept buffer that is large enough is handed out again
        (engine.big_acquire), so a process that has already trained with "f16" keeps its full-sized buffer after the switch; the saving
        shows once the kept buffers are dropped (train(False) or engine.big_clear()) or in a process that starts with "e4m3"."""
        if fmt not in ops.PAIR_ACT_FORMATS:
            raise ValueError(f"unknown pair activation format {fmt!r} (expected 'f16' or 'e4m3')")
        if fmt == "e4m3":
            self._check_saved_format("e4m3", compute_dtype, "switch back with set_pair_heads_train_format('bf16') first", setter=True)
        self.pair_act_format = fmt

    def _check_saved_format(self, fmt: str, dt: torch.dtype, way_out: str, setter: bool = False) -> None:
        """What "mxfp8" (set_pair_heads_train_format) and "e4m3" (set_pair_act_format) need, both riding on the saved backward:
        bf16 compute, save_pair_act and fused_bwd on, and not each other (`way_out`: what the message advises).  Checked by the
        setters, which also check the classifier depth and the width, and again by every forward with gradients: what a setter
        checked may have been changed since."""
        mx = fmt == "mxfp8"
        it, s, does = ("the mxfp8 train format of the pair heads", "s", "does") if mx else ("the e4m3 pair activations", "", "do")
        D, nh = self.decoder_hidden_size, len(HEAD_NAMES)
        if dt != torch.bfloat16:
            raise ValueError(f"{it} need{s} compute dtype torch.bfloat16")
        if setter and self.num_cls_layers != 2:
            raise ValueError(f"{it} need{s} peneo_classifier_num_layers == 2, not {self.num_cls_layers}")
        if setter and not (ops.pair_mxfp8_save_supported(D, nh) if mx else ops.pair_save_e4m3_supported(torch.bfloat16, D, nh)):
            raise ValueError(f"{it} {does} not support decoder width D = {D}")
        if not (self.save_pair_act and self.fused_bwd):
            raise ValueError(f"{it} {'feeds' if mx else 'are those of'} the saved backward: save_pair_act and fused_bwd must be on")
        if (self.pair_act_format == "e4m3") if mx else (self.pair_heads_train_format == "mxfp8"):
            raise ValueError(f"the mxfp8 train forward writes f16 records: {way_out}")

    def fused_pair_heads(self, dt: torch.dtype, D: int) -> bool:
        """True where the forward runs the fused pair-heads kernel: the 2-layer classifiers at a (dtype, width) the library has one
        for.  Everything else takes the materialising per-document path, forward and backward.  Above 512 (bf16, the four-wave
        kernel of pair_heads_wide.hip) ``pair_wide`` / PENEO_PAIR_WIDE=0 switches the fused kernel off: the A/B arm."""
        if self.num_cls_layers != 2 or not ops.pair_heads_supported(dt, D, len(HEAD_NAMES)):
            return False
        return D <= 512 or self.pair_wide

    def stacked_combine_weight(self, wc_w: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
        """[Wc[:, :D]; Wc[:, D:]] as a [2D, D] working-precision matrix, so one GEMM yields [a | b]."""
        D = wc_w.shape[0]
        return self.weight_cache.get(("dec.ab", dt), [wc_w], lambda: ops.cast(
            torch.cat([wc_w.detach()[:, :D], wc_w.detach()[:, D:]], dim=0).contiguous(), dt))

    def loss_ratio_tensor(self, dev) -> torch.Tensor:
        key = str(dev)
        if key not in self._ratio:
            r = self.loss_ratio if self.loss_ratio is not None else [1.0] * 5
            self._ratio[key] = torch.tensor(r, dtype=torch.float32, device=dev)
        return self._ratio[key]

    def stage_params(self) -> List[torch.Tensor]:
        ps: List[torch.Tensor] = []
        if self.decoder_shrink:
            ps += [self.shrink_projection[0].weight, self.shrink_projection[0].bias,
                   self.shrink_projection[3].weight, self.shrink_projection[3].bias]
        ps += [self.handshaking_kernel.combine_fc.weight, self.handshaking_kernel.combine_fc.bias]
        for name in HEAD_NAMES:
            for lin in self.head_linears(name):
                ps += [lin.weight, lin.bias]
        return ps

    def head_linears(self, name: str) -> List[nn.Linear]:
        fc = getattr(self, name + "_fc")
        return [fc] if isinstance(fc, nn.Linear) else [m for m in fc if isinstance(m, nn.Linear)]

    def forward(self, sequence_output: torch.Tensor, orig_bbox: torch.Tensor = None, line_extraction_shaking_tag=None,
                ent_linking_head_rel_shaking_tag=None, ent_linking_tail_rel_shaking_tag=None,
                line_grouping_head_rel_shaking_tag=None, line_grouping_tail_rel_shaking_tag=None, **kwargs):
        """``sequence_output``: [B, N, Hin] in the working dtype, already cropped (CLS / visual tokens removed)."""
        B, N, Hin = sequence_output.shape
        tags = [line_extraction_shaking_tag, ent_linking_head_rel_shaking_tag, ent_linking_tail_rel_shaking_tag,
                line_grouping_head_rel_shaking_tag, line_grouping_tail_rel_shaking_tag]
        P = N * (N + 1) // 2
        if all(t is None for t in tags) and not self.inference_mode and "line_extraction_matrix_spots" in kwargs:
            # sparse labels of DataCollatorForPEneo(sparse_tags=True): (b, i, j, tag) rows, scattered on the device
            assert kwargs.get("shaking_seq_len", N) == N, "spots were collated for another padded length"
            tags = [ops.spots_to_tags(kwargs[f"{k}_matrix_spots"], N, sequence_output.device, B=B)
                    for k in ("line_extraction", "ent_linking_head_rel", "ent_linking_tail_rel", "line_grouping_head_rel",
                              "line_grouping_tail_rel")]
        if all(t is not None for t in tags):
            for t in tags:
                assert t.shape == (B, P), f"label map shape {tuple(t.shape)} != {(B, P)}"
            tags = [t.contiguous() for t in tags]
        elif self.inference_mode:
            tags = None
        else:
            # the reference asserts on `pred.shape[:-1] == target.shape` with target None -> AttributeError
            raise AssertionError("the five *_shaking_tag label maps are required unless config.inference_mode is set")
        if self.inference_mode:
            tags = None
        params = self.stage_params()
        # autograd is off inside Function.forward, so decide here whether the backward will need dlogits
        need_grad = torch.is_grad_enabled() and (sequence_output.requires_grad or any(p.requires_grad for p in params))
        # The logit maps of a TRAINING step (7.3 MB per document in fp32) are read by nobody: the reference's trainer takes
        # outputs["loss"] and decodes predictions under model.eval() only (pipeline/trainer.py:116-156).  They stay in the
        # kernel's registers unless `train_logits` asks for them; eval / inference always returns them.
        want_logits = bool(self.train_logits) or not (self.training and need_grad and tags is not None) \
            or (tags is not None and self.le_loss.ohem)
        if self.pair_heads_format == "mxfp8":
            if need_grad:
                raise ValueError("mxfp8 pair heads are inference-only: run the forward under torch.no_grad() or switch back "
                                 "with set_pair_heads_format('bf16')")
            if sequence_output.dtype != torch.bfloat16:
                raise ValueError("mxfp8 pair heads need compute dtype torch.bfloat16")
        if self.pair_heads_train_format == "mxfp8" and need_grad:
            self._check_saved_format("mxfp8", sequence_output.dtype, "it cannot run with the e4m3 pair activations")
        if self.pair_act_format == "e4m3" and need_grad:
            self._check_saved_format("e4m3", sequence_output.dtype, "it cannot run with the e4m3 pair activations")
        # (skip_padded_pairs: the cropped mask the model passes on; pair_route decides whether the step reads it)
        mask = kwargs.get("attention_mask") if self.skip_padded_pairs else None
        if mask is not None and tuple(mask.shape) != (B, N):
            raise ValueError(f"skip_padded_pairs: attention_mask {tuple(mask.shape)} does not match the cropped sequence {(B, N)}")
        res = _DecoderStage.apply(self, sequence_output.reshape(B * N, Hin), B, N, tags, want_logits, need_grad, mask, *params)
        loss, l_le, l_elh, l_elt, l_lgh, l_lgt, o_le, o_elh, o_elt, o_lgh, o_lgt = res
        if self.inference_mode:
            # NB the reference's tuple order differs from the dataclass field order (:365-373)
            return (o_le, o_elh, o_elt, o_lgh, o_lgt, orig_bbox)
        return PEneoOutput(
            loss=loss, line_extraction_loss=l_le, ent_linking_h2h_loss=l_elh, ent_linking_t2t_loss=l_elt,
            line_grouping_h2h_loss=l_lgh, line_grouping_t2t_loss=l_lgt, line_extraction_shaking_outputs=o_le,
            ent_linking_h2h_shaking_outputs=o_elh, ent_linking_t2t_shaking_outputs=o_elt,
            line_grouping_h2h_shaking_outputs=o_lgh, line_grouping_t2t_shaking_outputs=o_lgt, orig_bbox=orig_bbox)
