"""MXFP8 inference path of the pair-classifier heads (pair_heads_mx.hip): the quantizer bit for bit, the fused kernel against a
torch emulation of its numeric contract (include/peneo_hip.h), the loss rows, repeatability, and the model-level switch."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CLASSES = [2, 3, 3, 3, 3]
TRAIN_STEPS, TRAIN_LR = 400, 1e-4   # trained-batch agreement: backbone lr (decoder x 30), warm-up + linear decay


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


# ---- torch emulation of the contract -------------------------------------------------------------------------------------
def mx_emulate(v: torch.Tensor):
    """[..., K] fp32 -> (e4m3 bytes, E8M0 bytes, dequantized fp64 values) per OCP MX block of 32 along the last dim."""
    vb = v.float().reshape(*v.shape[:-1], v.shape[-1] // 32, 32)
    amax = vb.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(amax)                                  # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex - 9, torch.full_like(ex, -127)).clamp(-127, 127)
    scaled = (vb.double() * torch.pow(2.0, -e.double())).float()   # exact power-of-two division
    q = scaled.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    deq = q.double() * torch.pow(2.0, e.double())
    return (q.view(torch.uint8).reshape(v.shape), (e + 127).to(torch.uint8).squeeze(-1), deq.reshape(v.shape))


def emulate_logits(ab, w1, b1, w2, b2, classes=CLASSES):
    B, N, D2 = ab.shape
    D = D2 // 2
    ii, jj = torch.triu_indices(N, N, device=ab.device)
    x = F.silu(ab.float()[:, ii, :D] + ab.float()[:, jj, D:])
    xq = mx_emulate(x)[2]
    out, off = [], 0
    for h, c in enumerate(classes):
        wq = mx_emulate(w1[h].float())[2]
        z = (xq @ wq.t()).float() + b1[h * D:(h + 1) * D].float()
        y = F.silu(z).to(torch.bfloat16).float()
        out.append(F.linear(y, w2[h].to(torch.bfloat16).float(), b2[off:off + c].float()))
        off += c
    return out


def make_case(N, D, seed, wide=False):
    g = torch.Generator().manual_seed(seed)
    ab = torch.randn(2, N, 2 * D, generator=g)
    if wide:   # channels spanning 1e-3 .. 1e2 in magnitude
        ab = ab * torch.logspace(-3, 2, 2 * D)[torch.randperm(2 * D, generator=g)]
    ab = ab.to(DEV).to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).to(DEV) for c in CLASSES]
    b1 = (0.1 * torch.randn(len(CLASSES) * D, generator=g)).to(DEV)
    b2 = torch.randn(sum(CLASSES), generator=g).to(DEV)
    return ab, w1, w2, b1, b2


def check_close(got, want, rel_to_max=False):
    for g_, w_ in zip(got, want):
        scale = float(w_.abs().max()) if rel_to_max else 1.0
        d = (g_ - w_).abs() / scale
        assert float(d.max()) < 3e-2 and float(d.mean()) < 1e-3, (float(d.max()), float(d.mean()))


# ---- 1. quantizer ------------------------------------------------------------------------------------------------------------
def test_quantize_rows_matches_the_emulation_bit_for_bit(ops):
    g = torch.Generator().manual_seed(3)
    rows, cols = 64, 256
    mag = torch.pow(10.0, torch.empty(rows, cols).uniform_(-6, 4, generator=g))       # 1e-6 .. 1e4
    v = mag * torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    v[0, :32] = 0.0                                                                     # an all-zero block
    v[1, :32] = 1.0
    v[1, 0] = 255.5                                  # amax 255.5: scale 2^-1, the top element scales to 511 -> saturates to 448
    v[2, 32:64] = torch.linspace(-470, 470, 32)      # scale 2^0: +-464 .. +-470 saturate
    v[3, :32] = torch.linspace(-1, 1, 32) * 2 ** -8  # next to amax 2^8 below: e4m3 subnormals
    v[3, 0] = 256.0
    q, sc = ops.mxfp8_quantize_rows(v.to(DEV))
    wq, ws, _ = mx_emulate(v)
    assert torch.equal(sc.cpu(), ws)
    assert torch.equal(q.cpu(), wq)
    # the cases above were present
    assert bool((wq.view(torch.float8_e4m3fn).float().abs() == 448).any())
    sub = wq.view(torch.float8_e4m3fn).float().abs()
    assert bool(((sub > 0) & (sub < 2 ** -6)).any())
    assert not torch.isnan(q.cpu().view(torch.float8_e4m3fn).float()).any()


# ---- 2. fused kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", [(33, 384), (130, 384), (511, 384), (70, 512), (301, 512),
                                 (70, 64), (70, 128), (70, 192), (70, 256), (70, 320), (70, 448)])   # every width the query accepts
def test_fused_kernel_matches_the_emulation(ops, N, D):
    ab, w1, w2, b1, b2 = make_case(N, D, N * 7 + D)
    wp = ops.pair_heads_pack_mxfp8(w1, w2)
    logits, _, _ = ops.pair_heads_fwd_mxfp8(ab, wp, b1, b2, CLASSES)
    check_close(logits, emulate_logits(ab, w1, b1, w2, b2))


def test_fused_kernel_with_wide_channel_range(ops):
    ab, w1, w2, b1, b2 = make_case(130, 384, 11, wide=True)
    wp = ops.pair_heads_pack_mxfp8(w1, w2)
    logits, _, _ = ops.pair_heads_fwd_mxfp8(ab, wp, b1, b2, CLASSES)
    check_close(logits, emulate_logits(ab, w1, b1, w2, b2), rel_to_max=True)


# ---- 3. loss / 4. repeatability ----------------------------------------------------------------------------------------------
def test_loss_partials_match_cross_entropy_on_the_kernels_logits(ops):
    N, D = 130, 384
    ab, w1, w2, b1, b2 = make_case(N, D, 5)
    P = N * (N + 1) // 2
    g = torch.Generator().manual_seed(9)
    tags = [torch.randint(0, c, (2, P), generator=g).to(DEV) for c in CLASSES]
    tags[1][0, :5] = -100                                                   # ignored labels carry no weight
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device=DEV) for c in CLASSES]
    wp = ops.pair_heads_pack_mxfp8(w1, w2)
    logits, partials, _ = ops.pair_heads_fwd_mxfp8(ab, wp, b1, b2, CLASSES, tags=tags, class_weights=cw)
    tot = partials.double().sum(0)
    for h in range(len(CLASSES)):
        want = F.cross_entropy(logits[h].reshape(-1, CLASSES[h]).double(), tags[h].reshape(-1), weight=cw[h].double(),
                               reduction="sum", ignore_index=-100)
        den = cw[h].double()[tags[h][tags[h] >= 0]].sum()
        assert abs(float(tot[h]) - float(want)) <= 1e-4 * abs(float(want))
        assert abs(float(tot[8 + h]) - float(den)) <= 1e-4 * float(den)
    none, partials2, _ = ops.pair_heads_fwd_mxfp8(ab, wp, b1, b2, CLASSES, want_logits=False, tags=tags, class_weights=cw)
    assert none is None and torch.equal(partials, partials2)


def test_three_launches_are_bit_identical(ops):
    ab, w1, w2, b1, b2 = make_case(301, 512, 21)
    P = 301 * 302 // 2
    g = torch.Generator().manual_seed(1)
    tags = [torch.randint(0, c, (2, P), generator=g).to(DEV) for c in CLASSES]
    wp = ops.pair_heads_pack_mxfp8(w1, w2)
    ref = None
    for _ in range(3):
        logits, partials, _ = ops.pair_heads_fwd_mxfp8(ab, wp, b1, b2, CLASSES, tags=tags)
        cur = [partials.clone()] + [l.clone() for l in logits]
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(cur, ref))


def test_unsupported_arguments_are_refused(ops):
    from peneo_amd.hip import PeneoHipError
    ab, w1, w2, b1, b2 = make_case(33, 384, 2)
    with pytest.raises(ValueError):
        ops.pair_heads_pack_mxfp8([w[:, :96].contiguous() for w in w1], [w[:, :96].contiguous() for w in w2])
    wp = ops.pair_heads_pack_mxfp8(w1, w2)
    bad = ab[:, :, :2 * 96].contiguous()
    with pytest.raises(PeneoHipError):
        ops.pair_heads_fwd_mxfp8(bad, wp, b1, b2, CLASSES)
    # the eval-only refusals of the C entry point: dropout, and dlogits in the loss block
    N = ab.shape[1]
    P = N * (N + 1) // 2
    tags = [torch.zeros((2, P), dtype=torch.int64, device=DEV) for _ in CLASSES]
    dlog = [torch.empty((2, P, c), dtype=torch.float32, device=DEV) for c in CLASSES]
    partials = torch.empty((ops.lib().peneo_pair_loss_partials(2, N), 32), dtype=torch.float32, device=DEV)
    rc, msg = _raw_fwd(ab, wp, b1, b2, drop_p=0.1)
    assert rc == -1 and "drop_p" in msg, (rc, msg)                      # PENEO_ERR_INVALID
    rc, msg = _raw_fwd(ab, wp, b1, b2, loss=(tags, dlog, partials))
    assert rc == -1 and "dlogits" in msg, (rc, msg)
    rc, msg = _raw_fwd(ab, wp, b1, b2, loss=(tags, None, partials))       # the same call without them is accepted
    torch.cuda.synchronize()
    assert rc == 0, msg


def _raw_fwd(ab, wp, b1, b2, drop_p=0.0, loss=None):
    """peneo_pair_heads_fwd_mxfp8 through the C ABI directly: (return code, peneo_last_error)"""
    import ctypes
    from peneo_amd import hip
    B, N, D2 = ab.shape
    desc = hip.PairHeadsDesc()
    desc.num_heads, desc.D = len(CLASSES), D2 // 2
    for h, c in enumerate(CLASSES):
        desc.classes[h] = c
    desc.w_packed, desc.b1, desc.b2 = hip.ptr(wp), hip.ptr(b1), hip.ptr(b2)
    desc.drop_p, desc.drop_seed = drop_p, 1
    pl = None
    if loss is not None:
        tags, dlog, partials = loss
        pl = hip.PairLoss()
        for h in range(len(CLASSES)):
            pl.tags[h] = hip.ptr(tags[h])
            pl.dlogits[h] = hip.ptr(dlog[h]) if dlog is not None else None
        pl.partials = hip.ptr(partials)
    rc = hip.lib().peneo_pair_heads_fwd_mxfp8(hip.ptr(ab), B, N, ctypes.byref(desc), None,
                                              ctypes.byref(pl) if pl is not None else None, hip.stream())
    return rc, (hip.lib().peneo_last_error() or b"").decode()


# ---- 5. / 6. model wiring and accuracy ---------------------------------------------------------------------------------------
def _model(backbone):
    from seeded import layoutlmv3_config, lilt_config, peneo_config, seeded_fill_
    from peneo_amd.model import PEneoConfig, PEneoModel
    if backbone == "lmv3":
        bc = dict(layoutlmv3_config("base"), num_hidden_layers=2)
        pcfg = peneo_config("layoutlmv3-base", bc)
    else:
        bc = dict(lilt_config("base"), num_hidden_layers=2)
        pcfg = peneo_config("lilt-roberta-en-base", bc)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 17)
    return m.cuda().set_compute_dtype(torch.bfloat16).eval(), pcfg


def _batch(pcfg, backbone, seed=4):
    from peneo_amd.data import synthetic_rfund_batch
    b = synthetic_rfund_batch(2, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=seed, ragged=True)
    if backbone == "lilt":
        b.pop("image", None)
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


OUT_KEYS = ["line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t"]


@pytest.mark.parametrize("backbone", ["lmv3", "lilt"])
def test_model_mxfp8_logits_match_the_emulation_on_the_models_weights(ops, monkeypatch, backbone):
    m, pcfg = _model(backbone)
    batch = _batch(pcfg, backbone)
    with torch.no_grad():
        ref = m(**batch)
    m.set_pair_heads_format("mxfp8")
    seen = {}
    real = ops.pair_heads_fwd_mxfp8

    def spy(ab, *a, **k):
        seen["ab"] = ab.clone()
        return real(ab, *a, **k)
    monkeypatch.setattr(ops, "pair_heads_fwd_mxfp8", spy)
    with torch.no_grad():
        out = m(**batch)
    assert "ab" in seen
    dec = m.peneo_decoder
    lins = [dec.head_linears(n) for n in ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h",
                                          "line_grouping_t2t")]
    w1 = [l[0].weight.detach() for l in lins]
    b1 = torch.cat([l[0].bias.detach() for l in lins])
    w2 = [l[1].weight.detach() for l in lins]
    b2 = torch.cat([l[1].bias.detach() for l in lins])
    want = emulate_logits(seen["ab"], w1, b1, w2, b2)
    got = [out[k + "_shaking_outputs"] for k in OUT_KEYS]
    for g_ in got:
        assert g_.dtype == torch.float32
    check_close([g_.reshape(w_.shape) for g_, w_ in zip(got, want)], want)
    assert torch.isfinite(out["loss"])
    # against the bf16 format of the same model at random init: e4m3 carries 3 mantissa bits, so z = W1 x has a relative
    # error near 5 % in both operands' quantization and the logit maps a cosine near 0.9988 (measured; DESIGN.md, MXFP8 section)
    cos = map_cosines(out, ref)
    print("cosine mxfp8 / bf16:", cos)
    assert min(cos.values()) >= 0.995, cos


def map_cosines(out, ref):
    return {k: float(F.cosine_similarity(out[k + "_shaking_outputs"].flatten().double(),
                                         ref[k + "_shaking_outputs"].flatten().double(), dim=0)) for k in OUT_KEYS}


def random_init_cosines(backbone):
    """cosine of every mxfp8 logit map against the bf16 one, 2-layer base-width model at random init (tools/run_pair_mxfp8.py)"""
    m, pcfg = _model(backbone)
    batch = _batch(pcfg, backbone)
    with torch.no_grad():
        ref = m(**batch)
        m.set_pair_heads_format("mxfp8")
        out = m(**batch)
    return map_cosines(out, ref)


def trained_spot_agreement(steps=TRAIN_STEPS, lr=TRAIN_LR):
    """bench.py's indices_agree_trained, bf16 against mxfp8: train a 2-layer base-width LayoutLMv3 model on ONE synthetic batch
    (B = 2, S = 512) with FusedAdamW, the reference's parameter groups (decoder lr x 30), warm-up then linear decay, in eval mode
    (no dropout) and the bf16 format; then decode the batch in both formats with get_spots_from_shaking_tag.  Per map: decoded
    bf16 spots, spots in one list only, argmax flips and the largest bf16 top-2 margin of a flipped pair, cosine."""
    from peneo_amd.model import HandshakingTaggingScheme
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    m, pcfg = _model("lmv3")
    batch = _batch(pcfg, "lmv3", seed=6)
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
    with torch.no_grad():
        o16 = m(**batch)
        m.set_pair_heads_format("mxfp8")
        omx = m(**batch)
        m.set_pair_heads_format("bf16")
    cos = map_cosines(omx, o16)
    for k in OUT_KEYS:
        a16, amx = o16[k + "_shaking_outputs"], omx[k + "_shaking_outputs"]
        diff = a16.argmax(-1) != amx.argmax(-1)
        top2 = a16.float().topk(2, dim=-1).values
        margin = top2[..., 0] - top2[..., 1]
        n_spots = n_differ = 0
        for b_ in range(a16.shape[0]):
            s16 = HandshakingTaggingScheme.get_spots_from_shaking_tag(a16[b_], seq_len=nn_)
            smx = HandshakingTaggingScheme.get_spots_from_shaking_tag(amx[b_], seq_len=nn_)
            n_spots += len(s16)
            n_differ += len(set(tuple(x[:3]) for x in s16) ^ set(tuple(x[:3]) for x in smx))
        res[k] = {"spots_bf16": n_spots, "spots_differing": n_differ, "argmax_flips": int(diff.sum()),
                  "largest_bf16_margin_of_a_flip": float(margin[diff].max()) if bool(diff.any()) else 0.0, "cosine": cos[k]}
    return res


def test_trained_batch_decodes_the_same_spots_in_both_formats():
    res = trained_spot_agreement()
    print("trained batch, mxfp8 against bf16:", res)
    assert sum(res[k]["spots_bf16"] for k in OUT_KEYS) > 0, res          # the comparison decodes something
    for k in OUT_KEYS:
        assert res[k]["spots_differing"] == 0, (k, res[k])


# ---- 7. refusals / 8. default untouched --------------------------------------------------------------------------------------
def test_refusals(ops, monkeypatch):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("tiny"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})).cuda()
    with pytest.raises(ValueError):
        m.set_pair_heads_format("mxfp8")                    # fp32 compute
    m.set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError):
        m.set_pair_heads_format("fp8")
    cfg3 = dict(pcfg, peneo_classifier_num_layers=3)
    m3 = PEneoModel(PEneoConfig(**{k: v for k, v in cfg3.items() if k != "model_type"})).cuda().set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError):
        m3.set_pair_heads_format("mxfp8")
    # a base-width model in training with gradients: refused before anything runs (no backbone forward, no pair-heads entry point)
    import functools
    mb, pb = _model("lmv3")
    mb.set_pair_heads_format("mxfp8")
    mb.train()
    calls = []
    for name in ("pair_heads_fwd", "pair_heads_fwd_mxfp8", "pair_heads_pack", "pair_heads_pack_mxfp8"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    real_bb = mb.backbone.forward
    monkeypatch.setattr(mb.backbone, "forward",
                        functools.wraps(real_bb)(lambda *a, **k: (calls.append("backbone"), real_bb(*a, **k))[1]))
    batch = _batch(pb, "lmv3")
    with pytest.raises(ValueError):
        mb(**batch)
    # ... and an fp32 compute dtype chosen after the format, without gradients
    mb.eval().set_compute_dtype(torch.float32)
    with torch.no_grad(), pytest.raises(ValueError):
        mb(**batch)
    assert calls == []


def test_switching_back_to_bf16_is_bit_identical(ops):
    m1, pcfg = _model("lmv3")
    m2, _ = _model("lmv3")
    batch = _batch(pcfg, "lmv3", seed=8)
    m1.set_pair_heads_format("mxfp8")
    with torch.no_grad():
        m1(**batch)
    m1.set_pair_heads_format("bf16")
    with torch.no_grad():
        a, b = m1(**batch), m2(**batch)
    for k in OUT_KEYS:
        assert torch.equal(a[k + "_shaking_outputs"], b[k + "_shaking_outputs"]), k
    assert torch.equal(a["loss"], b["loss"])
