"""LiLT backbone (BASELINE config 5) on libpeneo_hip kernels.

Reference: model/backbone/lilt/modeling_lilt.py — text stream (hidden H) and layout stream (H / r) with
shared attention scores (BiACM, :398-404).  Parameter names reproduce the reference
(``embeddings.*``, ``layout_embeddings.*``, ``encoder.layer.{i}.attention.self.{query,key,value,layout_query,...}``,
``attention.output`` / ``attention.layout_output``, ``intermediate`` / ``layout_intermediate``,
``output`` / ``layout_output``).

Device mapping: per layer two fused QKV GEMMs (text, layout), the attention, then the same GEMM(+bias/GELU/residual/dropout) +
LayerNorm chain as LayoutLMv3 for the two streams in lock step.  ``lilt_route`` decides once per forward how a step runs
(``LiltRoute``); every layer's forward and backward follow it.  The attention is one of three arms.  "concat": q/k/v of both
streams are concatenated per head (``peneo_head_concat``, q pre-scaled by 1/sqrt(d) resp. 1/sqrt(d_l)) so ONE flash-attention
call over head dim d + d_l produces the summed scores, one softmax and both context streams.  "attn2_eval" (forwards without
autograd and attention dropout) and "attn2_train" (opt-in) run the two-stream kernels on the QKV buffers as they are, bit-identical
to it and without the packed copies.  On the grouped route every pair of same-role GEMMs of the two streams is one
``ops.gemm_group`` launch.  Deviation in *train* mode only: the reference draws two independent attention-dropout masks for the
two (identical) probability matrices; here both streams share one mask.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import List, NamedTuple

import torch
import torch.nn as nn

from .. import ops
from ..hip import ACT_GELU, PeneoHipError
from .configuration_peneo import LiltConfig
from .engine import DropoutSeeds, WeightCache, zeros_like_param, zeros_like_params
from .engine import can_defer, defer_join, join_pending
from .engine import side_stream as engine_side_stream


class _SelfParams(nn.Module):
    def __init__(self, H: int, Hl: int):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)
        self.layout_query, self.layout_key, self.layout_value = nn.Linear(Hl, Hl), nn.Linear(Hl, Hl), nn.Linear(Hl, Hl)


class _DenseLN(nn.Module):
    def __init__(self, fan_in: int, fan_out: int, eps: float):
        super().__init__()
        self.dense = nn.Linear(fan_in, fan_out)
        self.LayerNorm = nn.LayerNorm(fan_out, eps=eps)


class _Dense(nn.Module):
    def __init__(self, fan_in: int, fan_out: int):
        super().__init__()
        self.dense = nn.Linear(fan_in, fan_out)


class _AttentionParams(nn.Module):
    def __init__(self, cfg, H, Hl):
        super().__init__()
        self.self = _SelfParams(H, Hl)
        self.output = _DenseLN(H, H, cfg.layer_norm_eps)
        self.layout_output = _DenseLN(Hl, Hl, cfg.layer_norm_eps)


class LiltLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H, r = cfg.hidden_size, cfg.channel_shrink_ratio
        Hl, I, Il = H // r, cfg.intermediate_size, cfg.intermediate_size // r
        self.attention = _AttentionParams(cfg, H, Hl)
        self.intermediate = _Dense(H, I)
        self.output = _DenseLN(I, H, cfg.layer_norm_eps)
        self.layout_intermediate = _Dense(Hl, Il)
        self.layout_output = _DenseLN(Il, Hl, cfg.layer_norm_eps)


class LiltEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([LiltLayer(cfg) for _ in range(cfg.num_hidden_layers)])


class LiltTextEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H = cfg.hidden_size
        self.word_embeddings = nn.Embedding(cfg.vocab_size, H, padding_idx=cfg.pad_token_id)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, H, padding_idx=cfg.pad_token_id)
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab_size, H)
        self.LayerNorm = nn.LayerNorm(H, eps=cfg.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(cfg.max_position_embeddings).expand((1, -1)))


class LiltLayoutEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        H, Hl = cfg.hidden_size, cfg.hidden_size // cfg.channel_shrink_ratio
        for n in ("x", "y", "h", "w"):
            setattr(self, f"{n}_position_embeddings", nn.Embedding(cfg.max_2d_position_embeddings, H // 6))
        self.box_position_embeddings = nn.Embedding(cfg.max_position_embeddings, Hl, padding_idx=cfg.pad_token_id)
        self.box_linear_embeddings = nn.Linear(H, Hl)
        self.LayerNorm = nn.LayerNorm(Hl, eps=cfg.layer_norm_eps)


# ------------------------------------------------------------------------------------------------
# everything of a transformer layer after the attention context, the two streams in lock step: every pair of same-role Linear
# layers is ONE grouped launch on the grouped route (ops.gemm_group with per-problem epilogues).  The layout stream's GEMMs
# ([4096, 192] x [192, 576] ...) are all fixed cost on their own (11-18 us for 1-2 us of MFMA work), and a LiLT step issued launch
# by launch is host-bound (18.5 ms of host against 20 ms of device time).
# ------------------------------------------------------------------------------------------------
def _gemms(grouped: bool, problems, **layout) -> List[torch.Tensor]:
    """Same-role products of the two streams, [(A, B, epilogue options), ...]: one ops.gemm_group launch on the grouped route,
    else one ops.gemm each, in order."""
    if grouped:
        return ops.gemm_group([(a, b, None, ep) for a, b, ep in problems], **layout)
    return [ops.gemm(a, b, **layout, **ep) for a, b, ep in problems]


class _PostParams(NamedTuple):
    """one stream's parameters behind the attention, in parameter order (_post_params)"""
    wo: torch.Tensor
    bo: torch.Tensor
    g1: torch.Tensor
    b1: torch.Tensor
    wi: torch.Tensor
    bi: torch.Tensor
    wo2: torch.Tensor
    bo2: torch.Tensor
    g2: torch.Tensor
    b2: torch.Tensor

    def cast(self, wc: WeightCache, key: str, dt):
        return wc.cast(key + ".o", self.wo, dt), wc.cast(key + ".i", self.wi, dt), wc.cast(key + ".o2", self.wo2, dt)


def _post_attn_fwd(wc: WeightCache, idx: int, dt, eps, seeds: DropoutSeeds, grouped: bool, site_t, site_l, x, att, tp, l, latt, lp):
    """out-proj + residual -> LN -> FFN1 + GELU -> FFN2 + residual -> LN.  -> (out, lout, saved text, saved layout)"""
    Wo, Wi, Wo2 = tp.cast(wc, f"L{idx}.t", dt)
    lWo, lWi, lWo2 = lp.cast(wc, f"L{idx}.l", dt)
    p = seeds.p_hidden
    h1, lh1 = _gemms(grouped, [(att, Wo, dict(bias=tp.bo, residual=x, drop_p=p, drop_seed=seeds.seed(site_t))),
                               (latt, lWo, dict(bias=lp.bo, residual=l, drop_p=p, drop_seed=seeds.seed(site_l)))])
    a, m1, r1 = ops.layernorm_fwd(h1, tp.g1, tp.b1, eps)
    la, lm1, lr1 = ops.layernorm_fwd(lh1, lp.g1, lp.b1, eps)
    zi = torch.empty((x.shape[0], tp.wi.shape[0]), dtype=dt, device=x.device)
    lzi = torch.empty((l.shape[0], lp.wi.shape[0]), dtype=dt, device=x.device)
    inter, linter = _gemms(grouped, [(a, Wi, dict(bias=tp.bi, act=ACT_GELU, preact=zi)),
                                     (la, lWi, dict(bias=lp.bi, act=ACT_GELU, preact=lzi))])
    h2, lh2 = _gemms(grouped, [(inter, Wo2, dict(bias=tp.bo2, residual=a, drop_p=p, drop_seed=seeds.seed(site_t + 1))),
                               (linter, lWo2, dict(bias=lp.bo2, residual=la, drop_p=p, drop_seed=seeds.seed(site_l + 1)))])
    out, m2, r2 = ops.layernorm_fwd(h2, tp.g2, tp.b2, eps)
    lout, lm2, lr2 = ops.layernorm_fwd(lh2, lp.g2, lp.b2, eps)
    return out, lout, (att, h1, m1, r1, a, zi, inter, h2, m2, r2), (latt, lh1, lm1, lr1, la, lzi, linter, lh2, lm2, lr2)


def _post_attn_bwd(wc: WeightCache, idx: int, dt, seeds: DropoutSeeds, grouped: bool, site_t, site_l, d_out, d_lout, sv_t, sv_l,
                   tp, lp, on_side):
    """-> (d_att, d_x_residual, text grads, d_latt, d_l_residual, layout grads, wg_t, wg_l): the three dgrad GEMM pairs on the main
    stream; ``on_side(fn, operands)`` runs the bias column sums on the stage's second stream, off the activation-gradient critical
    path (``operands``: the tensors that work READS, kept alive until the join; its outputs are never kept: they are returned as
    gradients, and an extra reference would make AccumulateGrad clone them on the main stream instead of storing them).  The six
    weight gradients leave as operand pairs (wg_t -> dwi, dwo2, dwo; wg_l likewise; their slots in the grads are None): the caller
    runs them behind the attention backward, together with the two QKV weight gradients - on the grouped route as TWO grouped
    launches (four text, four layout; each tile with its full K = tokens) instead of split-k launches + reductions, the schedule
    that measured best for the LayoutLMv3 layer (csrc/stages.hip), and 7 launches per layer less for a step that is close to
    host-bound."""
    att, h1, m1, r1, a, zi, inter, h2, m2, r2 = sv_t
    latt, lh1, lm1, lr1, la, lzi, linter, lh2, lm2, lr2 = sv_l
    Wo, Wi, Wo2 = tp.cast(wc, f"L{idx}.t", dt)
    lWo, lWi, lWo2 = lp.cast(wc, f"L{idx}.l", dt)
    Hs, Is, Hl, Il = tp.wo.shape[0], tp.wi.shape[0], lp.wo.shape[0], lp.wi.shape[0]
    sizes = [Hs] * 5 + [Is, Hs] + [Hl] * 5 + [Il, Hl]
    pool = torch.zeros(sum(sizes), dtype=torch.float32, device=d_out.device)   # one fill for all small accumulators
    dg2, db2, dg1, db1, dbo2, dbi, dbo, ldg2, ldb2, ldg1, ldb1, ldbo2, ldbi, ldbo = pool.split(sizes)
    p = seeds.p_hidden

    def ln_bwd(site, dy, h, g, m, r, dg, db):
        """-> (d_h, the same behind the dropout of the Linear in front: LayerNorm's dx_dropped output, d_h itself without dropout)"""
        dd = torch.empty_like(h) if p > 0 else None
        d_h = ops.layernorm_bwd(dy, h, g, m, r, dg, db, dx_dropped=dd, drop2_p=p, drop2_seed=seeds.seed(site))
        return d_h, (dd if p > 0 else d_h)

    d_h2, d_dense2 = ln_bwd(site_t + 1, d_out.contiguous(), h2, tp.g2, m2, r2, dg2, db2)
    d_lh2, d_ldense2 = ln_bwd(site_l + 1, d_lout.contiguous(), lh2, lp.g2, lm2, lr2, ldg2, ldb2)
    d_zi, d_lzi = _gemms(grouped, [(d_dense2, Wo2, dict(grad_src=zi, grad_act=ACT_GELU)),
                                   (d_ldense2, lWo2, dict(grad_src=lzi, grad_act=ACT_GELU))], b_kmajor=False)
    d_a, d_la = _gemms(grouped, [(d_zi, Wi, dict(residual=d_h2)), (d_lzi, lWi, dict(residual=d_lh2))], b_kmajor=False)
    d_h1, d_dense1 = ln_bwd(site_t, d_a, h1, tp.g1, m1, r1, dg1, db1)
    d_lh1, d_ldense1 = ln_bwd(site_l, d_la, lh1, lp.g1, lm1, lr1, ldg1, ldb1)
    d_att, d_latt = _gemms(grouped, [(d_dense1, Wo, {}), (d_ldense1, lWo, {})], b_kmajor=False)

    def side_work():
        ops.colsum(d_dense2, out=dbo2, accumulate=True)
        ops.colsum(d_zi, out=dbi, accumulate=True)
        ops.colsum(d_dense1, out=dbo, accumulate=True)
        ops.colsum(d_ldense2, out=ldbo2, accumulate=True)
        ops.colsum(d_lzi, out=ldbi, accumulate=True)
        ops.colsum(d_ldense1, out=ldbo, accumulate=True)
    on_side(side_work, (d_dense2, d_zi, d_dense1, d_ldense2, d_lzi, d_ldense1))
    wg_t = [(d_zi, a), (d_dense2, inter), (d_dense1, att)]                 # -> dwi, dwo2, dwo
    wg_l = [(d_lzi, la), (d_ldense2, linter), (d_ldense1, latt)]          # -> ldwi, ldwo2, ldwo
    gt = (None, dbo, dg1, db1, None, dbi, None, dbo2, dg2, db2)
    gl = (None, ldbo, ldg1, ldb1, None, ldbi, None, ldbo2, ldg2, ldb2)
    return d_att, d_h1, gt, d_latt, d_lh1, gl, wg_t, wg_l


class _State:
    def __init__(self):
        self.key_bias = None
        self.seeds = None
        self.dtype = torch.float32
        self.dims = None
        self.route = None         # this forward's LiltRoute


@dataclass(frozen=True)
class LiltRoute:
    """Which launches one step of the layer stages runs.  ``lilt_route`` decides it once per forward (LiltModel.forward); every layer's
    forward and backward dispatch on the route the forward stored and read no switch again, so a switch changed between the forward
    and the backward of one step does not affect that step."""
    attention: str      # "attn2_eval": ops.attn2_fwd, nothing kept | "attn2_train": attn2_fwd with the keep words + attn2_bwd | "concat"
    grouped: bool       # the layers issue their same-role GEMM pairs as ops.gemm_group
    defer_join: bool    # the layers defer the side-stream join by one stage (where engine.can_defer allows it at backward time)


def lilt_route(cfg: LiltConfig, dt: torch.dtype, seeds: DropoutSeeds, grad_enabled: bool) -> LiltRoute:
    """The route of a forward at compute dtype `dt` from the widths, the switches and the library's host-side query (no GPU).
    grad_enabled: torch.is_grad_enabled() of the caller (it is always off inside an autograd.Function).  The two-stream attention is
    bit-identical to the concat path it replaces (tests/test_gpu_attn2.py, tests/test_gpu_attn2_bwd.py); forwards without autograd
    and without attention dropout take it unless PENEO_LILT_ATTN2=0, training forwards only with PENEO_LILT_ATTN2_TRAIN=1."""
    H, nh, r, I = cfg.hidden_size, cfg.num_attention_heads, cfg.channel_shrink_ratio, cfg.intermediate_size
    env, bf16 = os.environ.get, dt == torch.bfloat16
    train = grad_enabled or seeds.p_attn > 0.0
    switch = env("PENEO_LILT_ATTN2_TRAIN", "0") == "1" if train else env("PENEO_LILT_ATTN2", "1") != "0"
    attention = "concat"
    if bf16 and switch and ops.attn2_supported(dt, H // nh, H // r // nh):
        attention = "attn2_train" if train else "attn2_eval"
    grouped = bf16 and all(w % 8 == 0 for w in (H, H // r, I, I // r)) and env("PENEO_LILT_GROUPS", "1") != "0"
    return LiltRoute(attention, grouped, env("PENEO_DEFER_JOIN", "1") != "0")


class _LiltEmbedStage(torch.autograd.Function):
    """text: word + type + pos -> LN (+dropout); layout: cat(6 tables) -> Linear -> + box_pos[pid] -> LN (+dropout)."""

    @staticmethod
    def forward(ctx, model, st, input_ids, bbox, *params):
        (word, type_w, pos_w, ln_g, ln_b, xw, yw, hw, ww, boxpos, lin_w, lin_b, lln_g, lln_b) = params
        cfg, wc, dt = model.config, model.weight_cache, st.dtype
        B, S = input_ids.shape
        H, Hl = cfg.hidden_size, cfg.hidden_size // cfg.channel_shrink_ratio
        dev = input_ids.device
        seeds = st.seeds
        # the bbox range check of the reference is the layout embedding kernel's sticky device flag (see LayoutLMv3's _EmbedStage):
        # check_inputs = True reads it at once (one host sync), "deferred" leaves it to raise_on_bad_inputs(), False ignores it
        check = getattr(model, "check_inputs", True)
        seeds.prepare_attn_words(cfg.num_hidden_layers, B, cfg.num_attention_heads, S, dev)
        pid = ops.position_ids(input_ids, cfg.pad_token_id)
        x0 = torch.empty((B * S, H), dtype=dt, device=dev)
        ops.embed_fwd(dt, x0, B, S, H, input_ids=input_ids, pos_ids=pid, word=word, type0=type_w[0], pos=pos_w)
        x, m1, r1 = ops.layernorm_fwd(x0, ln_g, ln_b, cfg.layer_norm_eps, drop_p=seeds.p_hidden, drop_seed=seeds.seed(1))
        # layout stream
        status = model.input_status(dev) if check else None
        sp = torch.empty((B * S, H), dtype=dt, device=dev)
        ops.embed_fwd(dt, sp, B, S, H, bbox=bbox, x=xw, y=yw, h=hw, w=ww, clip_hw=False, status=status)
        bp = torch.empty((B * S, Hl), dtype=dt, device=dev)
        zero_type = model.zeros("type", Hl, dev)
        zero_pos = model.zeros("pos", (1, Hl), dev)
        zpid = model.zeros_i32("zpid", (B, S), dev)
        ops.embed_fwd(dt, bp, B, S, Hl, input_ids=pid.to(torch.int64), pos_ids=zpid, word=boxpos, type0=zero_type, pos=zero_pos)
        Wl = wc.cast("boxlin", lin_w, dt)
        l0 = ops.gemm(sp, Wl, bias=lin_b, residual=bp)
        l, m2, r2 = ops.layernorm_fwd(l0, lln_g, lln_b, cfg.layer_norm_eps, drop_p=seeds.p_hidden, drop_seed=seeds.seed(2))
        if check is True:
            model.raise_on_bad_inputs()
        ctx.model, ctx.st = model, st
        ctx.saved = (pid, x0, m1, r1, sp, l0, m2, r2)
        ctx.inputs = (input_ids, bbox)
        ctx.params = params
        return x, l

    @staticmethod
    def backward(ctx, d_x, d_l):
        model, st = ctx.model, ctx.st
        (word, type_w, pos_w, ln_g, ln_b, xw, yw, hw, ww, boxpos, lin_w, lin_b, lln_g, lln_b) = ctx.params
        pid, x0, m1, r1, sp, l0, m2, r2 = ctx.saved
        input_ids, bbox = ctx.inputs
        cfg, wc, dt = model.config, model.weight_cache, st.dtype
        B, S = input_ids.shape
        H, Hl = cfg.hidden_size, cfg.hidden_size // cfg.channel_shrink_ratio
        seeds = st.seeds
        g = zeros_like_params(ctx.params)
        d_x0 = ops.layernorm_bwd(d_x.contiguous(), x0, ln_g, m1, r1, g[id(ln_g)], g[id(ln_b)], drop_p=seeds.p_hidden,
                                 drop_seed=seeds.seed(1))
        ops.embed_bwd(d_x0, B, S, H, input_ids=input_ids, pos_ids=pid, g_word=g[id(word)], g_pos=g[id(pos_w)],
                      pad_id=cfg.pad_token_id)
        ops.colsum(d_x0, out=g[id(type_w)][0], accumulate=True)
        d_l0 = ops.layernorm_bwd(d_l.contiguous(), l0, lln_g, m2, r2, g[id(lln_g)], g[id(lln_b)], drop_p=seeds.p_hidden,
                                 drop_seed=seeds.seed(2))
        # box position table: rows = position ids (pad rows skipped, like padding_idx)
        scratch_pos = torch.zeros((1, Hl), dtype=torch.float32, device=d_l0.device)
        ops.embed_bwd(d_l0, B, S, Hl, input_ids=pid.to(torch.int64), pos_ids=model.zeros_i32("zpid", (B, S), d_l0.device),
                      g_word=g[id(boxpos)], g_pos=scratch_pos, pad_id=cfg.pad_token_id)
        ops.colsum(d_l0, out=g[id(lin_b)], accumulate=True)
        ops.gemm(d_l0, sp, a_kmajor=False, b_kmajor=False, out=g[id(lin_w)], accumulate=True)
        d_sp = ops.gemm(d_l0, wc.cast("boxlin", lin_w, dt), b_kmajor=False)
        ops.embed_bwd(d_sp, B, S, H, bbox=bbox, g_x=g[id(xw)], g_y=g[id(yw)], g_h=g[id(hw)], g_w=g[id(ww)], clip_hw=False,
                      pad_id=cfg.pad_token_id)
        join_pending()     # weight-gradient work the layer stages left on the side stream
        grads = tuple(g[id(p)] if p.requires_grad else None for p in ctx.params)
        return (None, None, None, None) + grads


# ------------------------------------------------------------------------------------------------
# the attention of a layer, one arm per LiltRoute.attention.  Forward: (cfg, st, idx, qkv, lqkv) -> (att, latt, kept); backward:
# (cfg, st, idx, kept, att, latt, d_att, d_latt, dqkv, dlqkv) fills dqkv / dlqkv.  `kept` is the arm's own: only its backward reads it.
# ------------------------------------------------------------------------------------------------
def _geometry(cfg, st):
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    Hl = H // cfg.channel_shrink_ratio
    return st.dims[0], st.dims[1], H, Hl, nh, H // nh, Hl // nh


def _thirds(t):
    w = t.shape[1] // 3
    return t[:, :w], t[:, w:2 * w], t[:, 2 * w:]


def _contexts(qkv, lqkv):
    return qkv.new_empty((qkv.shape[0], qkv.shape[1] // 3)), lqkv.new_empty((lqkv.shape[0], lqkv.shape[1] // 3))


def _attn2_eval_fwd(cfg, st, idx, qkv, lqkv):
    """no autograd, no attention dropout: the two-stream kernel reads q | k | v where the QKV GEMMs left them and writes both context
    streams - no packed copy `cat`, no `attc`, nothing kept for a backward"""
    B, S, _, _, nh, d, dl = _geometry(cfg, st)
    att, latt = _contexts(qkv, lqkv)
    ops.attn2_fwd(*_thirds(qkv), *_thirds(lqkv), B, nh, S, 1.0 / math.sqrt(d), 1.0 / math.sqrt(dl), st.key_bias, out_a=att, out_b=latt)
    return att, latt, ()


def _attn2_train_fwd(cfg, st, idx, qkv, lqkv):
    """the training form of the above: the same kernel with the layer's keep words; the backward reads qkv / lqkv in place"""
    B, S, _, _, nh, d, dl = _geometry(cfg, st)
    att, latt = _contexts(qkv, lqkv)
    _, _, lse = ops.attn2_fwd(*_thirds(qkv), *_thirds(lqkv), B, nh, S, 1.0 / math.sqrt(d), 1.0 / math.sqrt(dl), st.key_bias,
                              out_a=att, out_b=latt, drop_p=st.seeds.p_attn,
                              drop_words=st.seeds.attn_words(idx, cfg.num_hidden_layers, B, nh, S, qkv.device))
    return att, latt, (qkv, lqkv, lse)


def _attn2_train_bwd(cfg, st, idx, kept, att, latt, d_att, d_latt, dqkv, dlqkv):
    B, S, _, _, nh, d, dl = _geometry(cfg, st)
    qkv, lqkv, lse = kept
    ops.attn2_bwd(*_thirds(qkv), *_thirds(lqkv), att, d_att, latt, d_latt, lse, B, nh, S, 1.0 / math.sqrt(d), 1.0 / math.sqrt(dl),
                  st.key_bias, dqkv, dlqkv, drop_p=st.seeds.p_attn,
                  drop_words=st.seeds.attn_words(idx, cfg.num_hidden_layers, B, nh, S, dqkv.device))


def _concat_fwd(cfg, st, idx, qkv, lqkv):
    """q/k/v of both streams packed per head (q pre-scaled), ONE attention call at head dim d + d_l, the context unpacked"""
    B, S, H, Hl, nh, d, dl = _geometry(cfg, st)
    w = nh * (d + dl)
    cat = torch.empty((qkv.shape[0], 3 * w), dtype=qkv.dtype, device=qkv.device)
    ops.head_concat(qkv[:, :H], lqkv[:, :Hl], nh, cat[:, :w], 1.0 / math.sqrt(d), 1.0 / math.sqrt(dl))
    ops.head_concat(qkv[:, H:], lqkv[:, Hl:], 2 * nh, cat[:, w:])      # k and v in one launch: 2 nh "heads"
    attc, lse = ops.attn_fwd(*_thirds(cat), B, nh, S, d + dl, 1.0, None, st.key_bias, drop_p=st.seeds.p_attn,
                             drop_words=st.seeds.attn_words(idx, cfg.num_hidden_layers, B, nh, S, qkv.device))
    att, latt = _contexts(qkv, lqkv)
    ops.head_split(attc, nh, att, latt)
    return att, latt, (cat, attc, lse)


def _concat_bwd(cfg, st, idx, kept, att, latt, d_att, d_latt, dqkv, dlqkv):
    B, S, H, Hl, nh, d, dl = _geometry(cfg, st)
    w = nh * (d + dl)
    cat, attc, lse = kept
    d_attc = torch.empty((cat.shape[0], w), dtype=cat.dtype, device=cat.device)
    ops.head_concat(d_att, d_latt, nh, d_attc)
    dcat = torch.empty_like(cat)
    ops.attn_bwd(*_thirds(cat), attc, d_attc, lse, B, nh, S, d + dl, 1.0, None, st.key_bias, dcat, None, drop_p=st.seeds.p_attn,
                 drop_words=st.seeds.attn_words(idx, cfg.num_hidden_layers, B, nh, S, dcat.device))
    ops.head_split(dcat[:, :w], nh, dqkv[:, :H], dlqkv[:, :Hl], 1.0 / math.sqrt(d), 1.0 / math.sqrt(dl))
    ops.head_split(dcat[:, w:], 2 * nh, dqkv[:, H:], dlqkv[:, Hl:])


_ATTN_FWD = {"attn2_eval": _attn2_eval_fwd, "attn2_train": _attn2_train_fwd, "concat": _concat_fwd}
_ATTN_BWD = {"attn2_train": _attn2_train_bwd, "concat": _concat_bwd}


class _LayerSaved(NamedTuple):
    """what a layer's forward leaves for its backward"""
    x: torch.Tensor
    l: torch.Tensor
    attn: tuple       # the attention arm's kept tensors; ctx.route.attention says whose (_ATTN_BWD reads them)
    post_t: tuple     # _post_attn_fwd's saved activations, text stream (att first)
    post_l: tuple     # ... layout stream (latt first)


class _LiltLayerStage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, st, idx, x, l, *params):
        (wq, bq, wk, bk, wv, bv, lwq, lbq, lwk, lbk, lwv, lbv, *rest) = params
        tp, lp = _PostParams(*rest[:10]), _PostParams(*rest[10:])
        cfg, wc, dt, route = model.config, model.weight_cache, st.dtype, st.route
        site = 32 * (idx + 1)
        Wqkv = wc.cat_rows(f"L{idx}.qkv", [wq, wk, wv], dt)
        bqkv = wc.cat_vec(f"L{idx}.bqkv", [bq, bk, bv], [bq.numel(), bk.numel(), bv.numel()])
        Wlqkv = wc.cat_rows(f"L{idx}.lqkv", [lwq, lwk, lwv], dt)
        blqkv = wc.cat_vec(f"L{idx}.blqkv", [lbq, lbk, lbv], [lbq.numel(), lbk.numel(), lbv.numel()])
        qkv, lqkv = _gemms(route.grouped, [(x, Wqkv, dict(bias=bqkv)), (l, Wlqkv, dict(bias=blqkv))])    # [R, 3H], [R, 3Hl]
        att, latt, kept = _ATTN_FWD[route.attention](cfg, st, idx, qkv, lqkv)
        xo, lo, sv_t, sv_l = _post_attn_fwd(wc, idx, dt, cfg.layer_norm_eps, st.seeds, route.grouped, site + 2, site + 6,
                                            x, att, tp, l, latt, lp)
        ctx.model, ctx.st, ctx.idx, ctx.route = model, st, idx, route
        ctx.saved = _LayerSaved(x, l, kept, sv_t, sv_l)
        ctx.params = params
        return xo, lo

    @staticmethod
    def backward(ctx, d_xo, d_lo):
        model, st, idx, route = ctx.model, ctx.st, ctx.idx, ctx.route
        (wq, bq, wk, bk, wv, bv, lwq, lbq, lwk, lbk, lwv, lbv, *rest) = ctx.params
        tp, lp = _PostParams(*rest[:10]), _PostParams(*rest[10:])
        x, l, attn_kept, sv_t, sv_l = ctx.saved
        cfg, wc, dt = model.config, model.weight_cache, st.dtype
        H, Hl = cfg.hidden_size, cfg.hidden_size // cfg.channel_shrink_ratio
        site = 32 * (idx + 1)
        main = torch.cuda.current_stream()
        side = model.side_stream(x.device)

        # operand tensors of the side-stream work, referenced until the (deferred) join.  Only what the side stream READS:
        # a reference to one of its OUTPUTS (the bias-gradient slices are returned as gradients) would push that tensor's
        # use count to 2, AccumulateGrad would clone it on the main stream instead of storing it, and the clone would race
        # the side stream's column sums
        kept = []

        def on_side(fn, operands=()):
            kept.extend(operands)
            ev = torch.cuda.Event()
            ev.record(main)
            with torch.cuda.stream(side):
                side.wait_event(ev)
                return fn()

        d_att, d_x_res, gt, d_latt, d_l_res, gl, wg_t, wg_l = _post_attn_bwd(wc, idx, dt, st.seeds, route.grouped, site + 2, site + 6,
                                                                             d_xo, d_lo, sv_t, sv_l, tp, lp, on_side)
        dqkv = torch.empty((x.shape[0], 3 * H), dtype=dt, device=x.device)
        dlqkv = torch.empty((x.shape[0], 3 * Hl), dtype=dt, device=x.device)
        _ATTN_BWD[route.attention](cfg, st, idx, attn_kept, sv_t[0], sv_l[0], d_att, d_latt, dqkv, dlqkv)
        Wqkv = wc.cat_rows(f"L{idx}.qkv", [wq, wk, wv], dt)
        Wlqkv = wc.cat_rows(f"L{idx}.lqkv", [lwq, lwk, lwv], dt)

        # the QKV weight gradient and _post_attn_bwd's three, per stream: one grouped launch, else one split-k GEMM each
        wgrads = lambda pairs: _gemms(route.grouped, [(dy, xin, {}) for dy, xin in pairs], a_kmajor=False, b_kmajor=False,
                                      out_dtype=torch.float32)

        def all_wgrads():
            gt_ = wgrads([(dqkv, x)] + wg_t)
            gl_ = wgrads([(dlqkv, l)] + wg_l)
            return ops.colsum(dqkv), ops.colsum(dlqkv), gt_, gl_
        dbqkv, dblqkv, gt_, gl_ = on_side(all_wgrads, (dqkv, dlqkv, x, l) + tuple(t for pr in wg_t + wg_l for t in pr))
        dwqkv, dwi_, dwo2_, dwo_ = gt_
        dwlqkv, ldwi_, ldwo2_, ldwo_ = gl_
        gt = (dwo_,) + gt[1:4] + (dwi_,) + gt[5:6] + (dwo2_,) + gt[7:]
        gl = (ldwo_,) + gl[1:4] + (ldwi_,) + gl[5:6] + (ldwo2_,) + gl[7:]
        d_x, d_l = _gemms(route.grouped, [(dqkv, Wqkv, dict(residual=d_x_res)), (dlqkv, Wlqkv, dict(residual=d_l_res))], b_kmajor=False)
        if route.defer_join and can_defer(ctx.params):
            defer_join(side, keep=kept)   # joined one stage later: the critical path does not wait for the QKV wgrads (engine.py)
        else:
            main.wait_stream(side)
        grads = (dwqkv[:H], dbqkv[:H], dwqkv[H:2 * H], dbqkv[H:2 * H], dwqkv[2 * H:], dbqkv[2 * H:],
                 dwlqkv[:Hl], dblqkv[:Hl], dwlqkv[Hl:2 * Hl], dblqkv[Hl:2 * Hl], dwlqkv[2 * Hl:], dblqkv[2 * Hl:]) + gt + gl
        grads = tuple(gr if p.requires_grad else None for gr, p in zip(grads, ctx.params))
        return (None, None, None, d_x, d_l) + grads


class _CatStage(torch.autograd.Function):
    """last_hidden_state = cat(text, layout) along the feature dim (:987)."""

    @staticmethod
    def forward(ctx, x, l):
        out = torch.empty((x.shape[0], x.shape[1] + l.shape[1]), dtype=x.dtype, device=x.device)
        ops.copy2d(x, out[:, :x.shape[1]])
        ops.copy2d(l, out[:, x.shape[1]:])
        ctx.hx = x.shape[1]
        return out

    @staticmethod
    def backward(ctx, d):
        return ops.copy2d(d[:, :ctx.hx]), ops.copy2d(d[:, ctx.hx:])


def _post_params(dln: _DenseLN, inter: _Dense, out: _DenseLN) -> List[torch.Tensor]:
    return [dln.dense.weight, dln.dense.bias, dln.LayerNorm.weight, dln.LayerNorm.bias, inter.dense.weight, inter.dense.bias,
            out.dense.weight, out.dense.bias, out.LayerNorm.weight, out.LayerNorm.bias]


class LiltModel(nn.Module):
    """Counterpart of the reference ``LiltModel`` for the PEneo call pattern:
    ``forward(input_ids, bbox, attention_mask)`` -> ``(cat(text, layout) [B, S, H + H/r],)``."""

    config_class = LiltConfig

    def __init__(self, config: LiltConfig):
        super().__init__()
        self.config = config
        H, nh, r = config.hidden_size, config.num_attention_heads, config.channel_shrink_ratio
        if H % 6 or H % nh or (H // r) % nh:
            raise ValueError("LiLT needs hidden_size divisible by 6, by num_attention_heads and (H / r) by the heads")
        self.embeddings = LiltTextEmbeddings(config)
        self.layout_embeddings = LiltLayoutEmbeddings(config)
        self.encoder = LiltEncoder(config)
        self.weight_cache = WeightCache()
        self.compute_dtype = torch.float32
        self._consts = {}

    def side_stream(self, device) -> "torch.cuda.Stream":
        return engine_side_stream(device, "wgrad")

    def input_status(self, dev) -> torch.Tensor:
        """int32 [1] on `dev`, sticky: set to 1 by the layout embedding kernel when a box coordinate is out of range."""
        return self.zeros_i32("input_status", 1, dev)

    def raise_on_bad_inputs(self) -> None:
        """Read (one host sync per flag) and clear the input flags; raises the reference's IndexError if any forward since the last
        call saw a bbox coordinate outside its table (reference modeling_lilt.py)."""
        for key, st in self._consts.items():
            if key[0] == "input_status" and int(st) != 0:
                st.zero_()
                raise IndexError("The :obj:`bbox`coordinate values should be within 0-1000 range.")

    def zeros(self, key, shape, dev):
        k = (key, str(shape), str(dev))
        if k not in self._consts:
            self._consts[k] = torch.zeros(shape, dtype=torch.float32, device=dev)
        return self._consts[k]

    def zeros_i32(self, key, shape, dev):
        k = (key, str(shape), str(dev))
        if k not in self._consts:
            self._consts[k] = torch.zeros(shape, dtype=torch.int32, device=dev)
        return self._consts[k]

    def _init_weights(self, module) -> None:
        std = self.config.initializer_range
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def forward(self, input_ids=None, bbox=None, attention_mask=None, **unused):
        if input_ids is None:
            raise ValueError("You have to specify either input_ids or inputs_embeds")
        if not input_ids.is_cuda:
            raise PeneoHipError("peneo_amd runs on the GPU only: move the model and the batch to 'cuda' "
                                "(there is no CPU fallback; the CPU oracle lives in oracle/ for tests)")
        cfg = self.config
        B, S = input_ids.shape
        dev = input_ids.device
        if bbox is None:
            bbox = torch.zeros((B, S, 4), dtype=torch.long, device=dev)
        if attention_mask is None:
            attention_mask = torch.ones((B, S), dtype=torch.long, device=dev)
        st = _State()
        st.dtype = self.compute_dtype
        st.dims = (B, S)
        st.seeds = DropoutSeeds(self.training, cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob)
        kb = torch.zeros((B, ops.attn_padded_len(S)), dtype=torch.float32, device=dev)
        kb[:, :S].masked_fill_(attention_mask == 0, -1.0e30)
        st.key_bias = kb
        st.route = lilt_route(cfg, st.dtype, st.seeds, torch.is_grad_enabled())   # once per forward; the layers follow
        e, le = self.embeddings, self.layout_embeddings
        eparams = [e.word_embeddings.weight, e.token_type_embeddings.weight, e.position_embeddings.weight,
                   e.LayerNorm.weight, e.LayerNorm.bias, le.x_position_embeddings.weight, le.y_position_embeddings.weight,
                   le.h_position_embeddings.weight, le.w_position_embeddings.weight, le.box_position_embeddings.weight,
                   le.box_linear_embeddings.weight, le.box_linear_embeddings.bias, le.LayerNorm.weight, le.LayerNorm.bias]
        x, l = _LiltEmbedStage.apply(self, st, input_ids.contiguous(), bbox.contiguous(), *eparams)
        for i, layer in enumerate(self.encoder.layer):
            s = layer.attention.self
            params = [s.query.weight, s.query.bias, s.key.weight, s.key.bias, s.value.weight, s.value.bias,
                      s.layout_query.weight, s.layout_query.bias, s.layout_key.weight, s.layout_key.bias,
                      s.layout_value.weight, s.layout_value.bias]
            params += _post_params(layer.attention.output, layer.intermediate, layer.output)
            params += _post_params(layer.attention.layout_output, layer.layout_intermediate, layer.layout_output)
            x, l = _LiltLayerStage.apply(self, st, i, x, l, *params)
        out = _CatStage.apply(x, l)
        return (out.view(B, S, out.shape[1]),)
