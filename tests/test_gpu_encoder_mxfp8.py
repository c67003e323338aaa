"""MXFP8 inference path of the encoder layers: peneo_encoder_layer_fwd_mxfp8 against the step-by-step composition of the public entry
points, its refusals, the model switch set_encoder_format, accuracy at random init and the decision-level agreement on a trained batch."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_KEYS = ["line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t"]
TRAIN_STEPS, TRAIN_LR = 400, 1e-4   # as test_gpu_pair_mxfp8.py: backbone lr (decoder x 30), warm-up + linear decay
COSINE_FLOOR = 0.989                # 1 - 0.15^2 / 2: twice the relative error (0.076) of a CPU fake-quant emulation of the same stack


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


# ---- 8. the composite is the composition ----------------------------------------------------------------------------------------
class LayerCase:
    def __init__(self, ops, B, T, H, nh, I, key_bias, seed=3):
        from peneo_amd import hip
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s, std=1.0: torch.randn(s, device=DEV, generator=g) * std
        R = B * T
        self.dims = (B, T, H, nh, I, R)
        self.x = rn(R, H).to(torch.bfloat16)
        self.w = [ops.mxfp8_quantize_rows(rn(n, k, std=0.03)) for n, k in ((3 * H, H), (H, H), (I, H), (H, I))]
        self.b = [rn(n, std=0.1) for n in (3 * H, H, I, H)]
        self.ln = [1.0 + rn(H, std=0.1), rn(H, std=0.1), 1.0 + rn(H, std=0.1), rn(H, std=0.1)]
        self.kb = None
        if key_bias:
            self.kb = torch.zeros((B, (T + 127) // 128 * 128), device=DEV)
            self.kb[-1, T - T // 3:T] = -1.0e30
        self.eps, self.scale = 1e-5, 1.0 / math.sqrt(H // nh)
        self.hip = hip

    def describe(self, p_hidden=0.0, p_attn=0.0, zi=False):
        """(layer struct, MX struct, the buffers they point to) for one call of the composite"""
        hip = self.hip
        B, T, H, nh, I, R = self.dims
        bf = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=DEV)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=DEV)
        keep = dict(qkv=bf(R, 3 * H), att=bf(R, H), h1=bf(R, H), a=bf(R, H), h2=bf(R, H), lse=f32(B, nh, T), m1=f32(R), r1=f32(R),
                    m2=f32(R), r2=f32(R), out=torch.zeros((R, H), dtype=torch.bfloat16, device=DEV), zi=bf(R, I) if zi else None,
                    x_q=u8(R, H), x_s=u8(R, H // 32), att_q=u8(R, H), att_s=u8(R, H // 32), a_q=u8(R, H), a_s=u8(R, H // 32),
                    inter_q=u8(R, I), inter_s=u8(R, I // 32))
        L, X = hip.EncoderLayer(), hip.EncoderLayerMxfp8()
        for name, (q, s) in zip(("Wqkv", "Wo", "Wi", "Wo2"), self.w):
            setattr(X, name + "_q", q.data_ptr())
            setattr(X, name + "_s", s.data_ptr())
        for name in ("x_q", "x_s", "att_q", "att_s", "a_q", "a_s", "inter_q", "inter_s"):
            setattr(X, name, keep[name].data_ptr())
        L.bqkv, L.bo, L.bi, L.bo2 = (t.data_ptr() for t in self.b)
        L.g1, L.b1, L.g2, L.b2 = (t.data_ptr() for t in self.ln)
        if self.kb is not None:
            L.key_bias = self.kb.data_ptr()
        L.x = self.x.data_ptr()
        for name in ("qkv", "att", "h1", "a", "h2", "lse", "m1", "r1", "m2", "r2"):
            setattr(L, name, keep[name].data_ptr())
        if zi:
            L.zi = keep["zi"].data_ptr()
        L.B, L.T, L.H, L.nh, L.I = B, T, H, nh, I
        L.eps, L.attn_scale, L.p_hidden, L.p_attn = self.eps, self.scale, p_hidden, p_attn
        return L, X, keep

    def composite(self, ops, p_hidden=0.0, p_attn=0.0, zi=False, raw=False):
        hip = self.hip
        L, X, keep = self.describe(p_hidden, p_attn, zi)
        if raw:
            rc = hip.lib().peneo_encoder_layer_fwd_mxfp8(C.byref(L), C.byref(X), keep["out"].data_ptr(), hip.stream())
            torch.cuda.synchronize()
            return rc, keep
        ops.encoder_layer_fwd_mxfp8(L, X, keep["out"])
        torch.cuda.synchronize()
        return keep

    def stepwise(self, ops):
        from peneo_amd.hip import ACT_GELU
        B, T, H, nh, I, R = self.dims
        (wqkv, wo, wi, wo2), (bqkv, bo, bi, bo2), (g1, b1, g2, b2) = self.w, self.b, self.ln
        xq, xs = ops.mxfp8_quantize_rows_bf16(self.x)
        qkv = ops.gemm_mxfp8(xq, xs, *wqkv, bias=bqkv)
        att, _ = ops.attn_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, nh, T, H // nh, self.scale, None, self.kb)
        h1 = ops.gemm_mxfp8(*ops.mxfp8_quantize_rows_bf16(att), *wo, bias=bo, residual=self.x)
        a, _, _ = ops.layernorm_fwd(h1, g1, b1, self.eps)
        none, iq, isc = ops.gemm_mxfp8(*ops.mxfp8_quantize_rows_bf16(a), *wi, bias=bi, act=ACT_GELU, mx_out=True, store_c=False)
        h2 = ops.gemm_mxfp8(iq, isc, *wo2, bias=bo2, residual=a)
        out, _, _ = ops.layernorm_fwd(h2, g2, b2, self.eps)
        return dict(qkv=qkv, att=att, h1=h1, a=a, inter_q=iq, inter_s=isc, h2=h2, out=out)


@pytest.mark.parametrize("key_bias", [False, True])
@pytest.mark.parametrize("B,T,H,nh,I", [(2, 709, 768, 12, 3072), (2, 333, 1024, 16, 4096)])
def test_composite_equals_the_step_by_step_composition(ops, B, T, H, nh, I, key_bias):
    case = LayerCase(ops, B, T, H, nh, I, key_bias)
    got, want = case.composite(ops), case.stepwise(ops)
    for name in ("qkv", "att", "h1", "a", "inter_q", "inter_s", "h2", "out"):
        assert torch.equal(got[name], want[name]), name
    assert bool(torch.isfinite(got["out"].float()).all()) and float(got["out"].float().abs().max()) > 0.1


@pytest.mark.parametrize("rows,H", [(1418, 768), (333, 1024), (9, 256)])
def test_fused_layernorm_equals_layernorm_then_quantizer(ops, rows, H):
    assert ops.layernorm_mxfp8_supported(H)
    g = torch.Generator(device=DEV).manual_seed(rows)
    x = (torch.randn((rows, H), device=DEV, generator=g) * 3.0 + 0.5).to(torch.bfloat16)
    x[1] = 0.25                                                            # a constant row: y == beta
    gamma, beta = 1.0 + 0.1 * torch.randn(H, device=DEV, generator=g), 0.1 * torch.randn(H, device=DEV, generator=g)
    beta[32:64] = 0.0
    y, m, r, q, s = ops.layernorm_fwd_mxfp8(x, gamma, beta, 1e-5)
    y0, m0, r0 = ops.layernorm_fwd(x, gamma, beta, 1e-5)
    assert torch.equal(y, y0) and torch.equal(m, m0) and torch.equal(r, r0)
    q0, s0 = ops.mxfp8_quantize_rows_bf16(y0)
    assert torch.equal(q, q0) and torch.equal(s, s0)


def test_chained_layers_equal_unchained_ones(ops):
    """out_q / out_s of a layer are the quantization of its out, and a layer told that x_q / x_s are valid gives the same result"""
    case = LayerCase(ops, 2, 333, 768, 12, 3072, True)
    plain = case.composite(ops)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    R, H = case.dims[5], case.dims[2]
    L, X, keep = case.describe()
    oq, os_ = u8(R, H), u8(R, H // 32)
    X.out_q, X.out_s = oq.data_ptr(), os_.data_ptr()
    xq, xs = ops.mxfp8_quantize_rows_bf16(case.x)
    X.x_q, X.x_s, X.x_prequantized = xq.data_ptr(), xs.data_ptr(), 1
    ops.encoder_layer_fwd_mxfp8(L, X, keep["out"])
    torch.cuda.synchronize()
    assert torch.equal(keep["out"], plain["out"])
    q, s = ops.mxfp8_quantize_rows_bf16(plain["out"])
    assert torch.equal(oq, q) and torch.equal(os_, s)


def test_composite_refuses_dropout_and_zi(ops):
    case = LayerCase(ops, 1, 64, 768, 12, 3072, False)
    for kw in (dict(p_hidden=0.1), dict(p_attn=0.1), dict(zi=True)):
        rc, keep = case.composite(ops, raw=True, **kw)
        assert rc == -1, kw
        assert int(keep["out"].float().abs().sum()) == 0        # nothing ran
    rc, keep = case.composite(ops, raw=True)
    assert rc == 0 and float(keep["out"].float().abs().sum()) > 0


# ---- 9. model wiring ----------------------------------------------------------------------------------------------------------
def _model(layers, seeded=True, seed=17):
    from seeded import layoutlmv3_config, peneo_config, seeded_fill_
    from peneo_amd.model import PEneoConfig, PEneoModel
    bc = dict(layoutlmv3_config("base"), num_hidden_layers=layers)
    pcfg = peneo_config("layoutlmv3-base", bc)
    torch.manual_seed(seed)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))     # the model's own init (initializer_range)
    if seeded:
        seeded_fill_(m.state_dict(), seed)
    return m.cuda().set_compute_dtype(torch.bfloat16).eval(), pcfg


def _batch(pcfg, seed=4):
    from peneo_amd.data import synthetic_rfund_batch
    b = synthetic_rfund_batch(2, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=seed, ragged=True)
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def _spy_layers(ops, monkeypatch):
    from peneo_amd.model import modeling_layoutlmv3 as ml
    calls = {"mxfp8": 0, "bf16": 0}
    real_mx, real_stage = ops.encoder_layer_fwd_mxfp8, ml._LayerStage.forward
    monkeypatch.setattr(ops, "encoder_layer_fwd_mxfp8", lambda *a, **k: (calls.__setitem__("mxfp8", calls["mxfp8"] + 1), real_mx(*a, **k))[1])
    monkeypatch.setattr(ml._LayerStage, "forward",
                        staticmethod(lambda *a, **k: (calls.__setitem__("bf16", calls["bf16"] + 1), real_stage(*a, **k))[1]))
    return calls


@pytest.mark.parametrize("layers", [2, 12])
def test_model_runs_every_layer_through_the_mxfp8_composite_and_switches_back_bit_identically(ops, monkeypatch, layers):
    m, pcfg = _model(layers)
    never, _ = _model(layers)
    batch = _batch(pcfg)
    calls = _spy_layers(ops, monkeypatch)
    with torch.no_grad():
        ref = m(**batch)
    assert calls == {"mxfp8": 0, "bf16": layers}                 # the default is untouched
    m.set_encoder_format("mxfp8")
    with torch.no_grad():
        out = m(**batch)
    assert calls == {"mxfp8": layers, "bf16": layers}
    assert any(k[-1] == "mxfp8" for k in m.backbone.weight_cache._store)      # quantized weights cached beside the bf16 copies
    n_keys = len(m.backbone.weight_cache._store)
    with torch.no_grad():
        again = m(**batch)
    assert len(m.backbone.weight_cache._store) == n_keys
    for k in OUT_KEYS:
        assert torch.isfinite(out[k + "_shaking_outputs"]).all()
        assert torch.equal(out[k + "_shaking_outputs"], again[k + "_shaking_outputs"])
        assert not torch.equal(out[k + "_shaking_outputs"], ref[k + "_shaking_outputs"])
    m.set_encoder_format("bf16")
    with torch.no_grad():
        back, other = m(**batch), never(**batch)
    assert calls["mxfp8"] == 2 * layers
    for k in OUT_KEYS:
        assert torch.equal(back[k + "_shaking_outputs"], other[k + "_shaking_outputs"])
        assert torch.equal(back[k + "_shaking_outputs"], ref[k + "_shaking_outputs"])
    assert torch.equal(back["loss"], other["loss"])


def test_quantized_weights_follow_the_masters(ops):
    m, pcfg = _model(2)
    batch = _batch(pcfg)
    m.set_encoder_format("mxfp8")
    with torch.no_grad():
        a = m(**batch)
        w = m.backbone.encoder.layer[0].intermediate.dense.weight
        w.mul_(2.0)                                               # bumps the parameter's version: the cache entry is rebuilt
        b = m(**batch)
        w.div_(2.0)
        c = m(**batch)
    k = "line_extraction_shaking_outputs"
    assert not torch.equal(a[k], b[k])
    assert torch.equal(a[k], c[k])


def test_model_refusals(ops, monkeypatch):
    from seeded import lilt_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    m, pcfg = _model(2)
    batch = _batch(pcfg)
    calls = _spy_layers(ops, monkeypatch)
    import functools
    real_embed = m.backbone.embed_params
    monkeypatch.setattr(m.backbone, "embed_params", functools.wraps(real_embed)(lambda: (calls.__setitem__("embed", 1), real_embed())[1]))
    with pytest.raises(ValueError):
        m.set_encoder_format("fp8")
    m.set_encoder_format("mxfp8")
    with pytest.raises(ValueError):                               # gradients enabled
        m(**batch)
    m.set_compute_dtype(torch.float32)
    with torch.no_grad(), pytest.raises(ValueError):              # fp32 compute chosen after the format
        m(**batch)
    assert calls == {"mxfp8": 0, "bf16": 0}                       # refused before any kernel ran (not even the embedding stage)
    f32, _ = _model(2)
    f32.set_compute_dtype(torch.float32)
    with pytest.raises(ValueError):
        f32.set_encoder_format("mxfp8")
    lc = peneo_config("lilt-roberta-en-base", dict(lilt_config("base"), num_hidden_layers=2))
    lilt = PEneoModel(PEneoConfig(**{k: v for k, v in lc.items() if k != "model_type"})).cuda().set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError, match="LiLT"):
        lilt.set_encoder_format("mxfp8")


def test_both_switches_are_independent(ops, monkeypatch):
    m, pcfg = _model(2)
    batch = _batch(pcfg)
    calls = _spy_layers(ops, monkeypatch)
    m.set_encoder_format("mxfp8").set_pair_heads_format("mxfp8")
    assert m.peneo_decoder.pair_heads_format == "mxfp8" and m.backbone.encoder_format == "mxfp8"
    with torch.no_grad():
        both = m(**batch)
    m.set_pair_heads_format("bf16")
    assert m.backbone.encoder_format == "mxfp8"
    with torch.no_grad():
        enc_only = m(**batch)
    assert calls == {"mxfp8": 4, "bf16": 0}
    k = "line_extraction_shaking_outputs"
    assert torch.isfinite(both[k]).all() and not torch.equal(both[k], enc_only[k])


# ---- 10. accuracy at random init ----------------------------------------------------------------------------------------------
def random_init_accuracy(layers=12):
    """cosine of last_hidden_state (asserted) and of the five logit maps (reported), "mxfp8" against "bf16", at the model's own init"""
    m, pcfg = _model(layers, seeded=False, seed=23)
    batch = _batch(pcfg)
    hidden = {}
    real = m.backbone.forward
    import functools

    def grab(*a, **k):
        r = real(*a, **k)
        hidden["h"] = r[0].detach().clone()
        return r
    m.backbone.forward = functools.wraps(real)(grab)
    with torch.no_grad():
        ref = m(**batch)
        h16 = hidden["h"]
        m.set_encoder_format("mxfp8")
        out = m(**batch)
        hmx = hidden["h"]
    cos_h = float(F.cosine_similarity(hmx.flatten().double(), h16.flatten().double(), dim=0))
    rel = float((hmx.double() - h16.double()).norm() / h16.double().norm())
    maps = {k: float(F.cosine_similarity(out[k + "_shaking_outputs"].flatten().double(), ref[k + "_shaking_outputs"].flatten().double(), dim=0))
            for k in OUT_KEYS}
    return {"cosine_last_hidden_state": cos_h, "relative_error_last_hidden_state": rel, "cosine_logit_maps": maps}


def test_random_init_accuracy_of_the_12_layer_base_model():
    """Floor 0.989: a CPU fake-quant emulation of the same stack (post-LN layers, H = 768, I = 3072, 12 heads, 12 layers, N(0, 0.02^2)
    weights, both operands of the four linears through the MX emulation, fp32 elsewhere) gave cosine 0.9971 / relative error 0.076; the
    kernel path adds bf16 stores and the bias tensor, so twice that relative error is allowed: 1 - 0.15^2 / 2."""
    res = random_init_accuracy()
    print("random init, encoder mxfp8 against bf16:", res)
    assert res["cosine_last_hidden_state"] >= COSINE_FLOOR, res


# ---- 11. decision level -------------------------------------------------------------------------------------------------------
def trained_spot_agreement(steps=TRAIN_STEPS, lr=TRAIN_LR):
    """bench.py's indices_agree_trained over both switches: train a 2-layer base-width LayoutLMv3 model on ONE synthetic batch in bf16
    (the procedure of test_gpu_pair_mxfp8.py), then decode the batch with get_spots_from_shaking_tag under encoder x heads in
    {bf16, mxfp8}^2.  Per setting and map: spots in one list only against bf16 + bf16, argmax flips and the largest bf16 top-2 margin
    of a flipped pair."""
    from peneo_amd.model import HandshakingTaggingScheme
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    m, pcfg = _model(2)
    batch = _batch(pcfg, seed=6)
    opt = FusedAdamW(peneo_param_groups(m, lr, 0.01, 30.0), max_grad_norm=1.0)
    base = [g_["lr"] for g_ in opt.param_groups]
    for it in range(steps):
        f_ = min(1.0, (it + 1) / max(1, steps // 20)) * max(0.0, 1.0 - it / steps)
        for g_, lr0 in zip(opt.param_groups, base):
            g_["lr"] = lr0 * f_
        for p_ in m.parameters():
            p_.grad = None
        out = m(**batch)
        out["loss"].backward()
        opt.step()
    res = {"loss_after": float(out["loss"].detach())}
    nn_ = batch["input_ids"].shape[1] - 1
    outs = {}
    with torch.no_grad():
        for enc in ("bf16", "mxfp8"):
            for heads in ("bf16", "mxfp8"):
                m.set_encoder_format(enc).set_pair_heads_format(heads)
                outs[(enc, heads)] = m(**batch)
        m.set_encoder_format("bf16").set_pair_heads_format("bf16")
    o16 = outs[("bf16", "bf16")]
    spots = lambda t: [set(tuple(x[:3]) for x in HandshakingTaggingScheme.get_spots_from_shaking_tag(t[b_], seq_len=nn_))
                       for b_ in range(t.shape[0])]
    for k in OUT_KEYS:
        a16 = o16[k + "_shaking_outputs"]
        s16 = spots(a16)
        top2 = a16.float().topk(2, dim=-1).values
        margin = top2[..., 0] - top2[..., 1]
        res[k] = {"spots_bf16": sum(len(s) for s in s16)}
        for key, o in outs.items():
            if key == ("bf16", "bf16"):
                continue
            amx = o[k + "_shaking_outputs"]
            diff = a16.argmax(-1) != amx.argmax(-1)
            res[k]["enc_%s+heads_%s" % key] = {
                "spots_differing": sum(len(x ^ y) for x, y in zip(s16, spots(amx))), "argmax_flips": int(diff.sum()),
                "largest_bf16_margin_of_a_flip": float(margin[diff].max()) if bool(diff.any()) else 0.0}
    return res


def test_trained_batch_decodes_the_same_spots_in_all_four_settings():
    res = trained_spot_agreement()
    print("trained batch, encoder x heads against bf16 + bf16:", res)
    assert sum(res[k]["spots_bf16"] for k in OUT_KEYS) > 0, res          # the comparison decodes something
    for k in OUT_KEYS:
        for setting, r in res[k].items():
            if setting != "spots_bf16":
                assert r["spots_differing"] == 0, (k, setting, res[k])
