"""PEneoModel.set_pair_heads_train_format("mxfp8"): which kernels a train step runs, its gradients against the bf16 step with the
same seeds, the refusals, the untouched default, and a trained batch against a bf16-trained control."""
import pytest
import torch

from test_gpu_pair_mxfp8 import OUT_KEYS, TRAIN_LR, TRAIN_STEPS, _batch, _model

pytestmark = pytest.mark.gpu

COUNTED = ("pair_heads_fwd_mxfp8_save", "pair_bwd_saved", "pair_heads_fwd", "pair_heads_fwd_mxfp8", "pair_bwd_fused")


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the pair-space ops"""
    from peneo_amd import ops
    seen = {n: 0 for n in COUNTED}

    def wrap(name):
        real = getattr(ops, name)

        def counting(*a, **kw):
            seen[name] += 1
            return real(*a, **kw)
        monkeypatch.setattr(ops, name, counting)
    for n in COUNTED:
        wrap(n)
    return seen


def _train_step(m, batch, step=40):
    """one seeded train step (dropout active): loss and every gradient"""
    from peneo_amd.model.engine import DropoutSeeds
    DropoutSeeds._step, m._step = step, step
    m.train()
    try:
        m.zero_grad(set_to_none=True)
        out = m(**batch)
        out["loss"].backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and p.grad is not None}
        return out["loss"].detach().clone(), grads
    finally:
        m.eval()
        m.zero_grad(set_to_none=True)


# ---- 1. call counts / 2. gradient cosine -------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["lmv3", "lilt"])
def test_train_step_runs_the_mxfp8_forward_and_the_saved_backward(calls, backbone):
    m, pcfg = _model(backbone)
    batch = _batch(pcfg, backbone)
    loss0, g0 = _train_step(m, batch)                                     # the bf16 step, same seeds
    assert calls["pair_heads_fwd"] == 1 and calls["pair_bwd_saved"] == 1 and calls["pair_heads_fwd_mxfp8_save"] == 0
    for k in calls:
        calls[k] = 0
    assert m.set_pair_heads_train_format("mxfp8") is m
    loss1, g1 = _train_step(m, batch)
    assert calls["pair_heads_fwd_mxfp8_save"] == 1 and calls["pair_bwd_saved"] == 1
    assert calls["pair_heads_fwd"] == 0 and calls["pair_heads_fwd_mxfp8"] == 0 and calls["pair_bwd_fused"] == 0
    assert torch.isfinite(loss1) and g1.keys() == g0.keys() and len(g1) > 50
    for n in g1:
        assert torch.isfinite(g1[n]).all(), n
    # e4m3 leaves about 5 % rms error on z, hence at most about 7 % on the terms that depend on it: a cosine near
    # 0.9975; the floor leaves four times that distance.  The gradient of an attention KEY bias is analytically zero (a key bias
    # shifts every score of a query by the same amount, and softmax ignores that): what the step leaves there is rounding noise in
    # both formats and its direction means nothing (tests/test_oracle_golden.py gives it an absolute floor for the same reason).
    # Measured cosines of those: LayoutLMv3 0.62 .. 0.74; LiLT 0.77 .. 0.83 (key) and 0.80 .. 0.88 (layout_key), at 0.0006 .. 0.0023 of
    # the query-bias gradient's norm.  They are held to the
    # noise level instead: at most 2^-4 of the same layer's query-bias gradient (bf16 rounds at 2^-8; 16 times that), both formats.
    cos, noise = {}, {}
    for n in g0:
        a, b = g1[n].double().flatten(), g0[n].double().flatten()
        if n.endswith("key.bias"):
            qn = g0[n.replace("key.bias", "query.bias")].double().norm()
            noise[n] = (float(b.norm() / qn), float(a.norm() / qn), float(torch.dot(a, b) / (a.norm() * b.norm())))
            continue
        if float(b.norm()) == 0.0:
            assert float(a.norm()) == 0.0, n
            continue
        cos[n] = float(torch.dot(a, b) / (a.norm() * b.norm()))
    low = sorted(cos.items(), key=lambda kv: kv[1])[:8]
    print(f"{backbone}: loss bf16 {float(loss0):.6f} mxfp8 {float(loss1):.6f}; lowest gradient cosines: {low}")
    print(f"{backbone}: key-bias gradients (|g| / |g query bias| in bf16, in mxfp8, cosine): {noise}")
    assert len(noise) == (2 if backbone == "lmv3" else 4) and len(cos) > 50
    assert min(cos.values()) >= 0.99, low
    assert max(max(v[0], v[1]) for v in noise.values()) <= 2.0 ** -4, noise
    # a forward without gradients is untouched by the train format: the bf16 kernel
    for k in calls:
        calls[k] = 0
    with torch.no_grad():
        m(**batch)
    assert calls["pair_heads_fwd"] == 1 and calls["pair_heads_fwd_mxfp8_save"] == 0


# ---- 3. refusals and the default ---------------------------------------------------------------------------------------------
def test_refusals():
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig, PEneoModel
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("tiny"))
    mk = lambda cfg: PEneoModel(PEneoConfig(**{k: v for k, v in cfg.items() if k != "model_type"})).cuda()
    mb, pb = _model("lmv3")                                               # base width, bf16
    batch = _batch(pb, "lmv3")
    with pytest.raises(ValueError):
        mb.set_pair_heads_train_format("fp8")
    mb.set_compute_dtype(torch.float32)
    with pytest.raises(ValueError):
        mb.set_pair_heads_train_format("mxfp8")                           # fp32 compute
    mb.set_compute_dtype(torch.bfloat16)
    bc3 = dict(pcfg, peneo_classifier_num_layers=3)
    with pytest.raises(ValueError):
        mk(bc3).set_compute_dtype(torch.bfloat16).set_pair_heads_train_format("mxfp8")      # 3-layer classifiers
    with pytest.raises(ValueError):
        mk(pcfg).set_compute_dtype(torch.bfloat16).set_pair_heads_train_format("mxfp8")     # a width without the saved backward
    for attr in ("save_pair_act", "fused_bwd"):                           # the saved backward switched off
        setattr(mb.peneo_decoder, attr, False)
        with pytest.raises(ValueError):
            mb.set_pair_heads_train_format("mxfp8")
        setattr(mb.peneo_decoder, attr, True)
    assert mb.peneo_decoder.pair_heads_train_format == "bf16"             # none of the refused calls changed it
    mb.set_pair_heads_train_format("mxfp8")
    # ... switched off after the setter: refused at the forward
    mb.peneo_decoder.save_pair_act = False
    with pytest.raises(ValueError):
        mb(**batch)
    mb.peneo_decoder.save_pair_act = True
    # the eval format stays inference-only, whatever the train format says
    mb.set_pair_heads_format("mxfp8")
    mb.train()
    with pytest.raises(ValueError):
        mb(**batch)
    mb.eval()
    with torch.no_grad():
        assert torch.isfinite(mb(**batch)["loss"])


def test_switching_back_to_bf16_is_the_untouched_step(calls):
    m1, pcfg = _model("lmv3")
    m2, _ = _model("lmv3")
    batch = _batch(pcfg, "lmv3", seed=8)
    m1.set_pair_heads_train_format("mxfp8")
    _train_step(m1, batch)
    assert calls["pair_heads_fwd_mxfp8_save"] == 1
    m1.set_pair_heads_train_format("bf16")
    la, ga = _train_step(m1, batch)
    lb, gb = _train_step(m2, batch)
    lc, gc = _train_step(m2, batch)
    assert calls["pair_heads_fwd_mxfp8_save"] == 1 and calls["pair_heads_fwd"] == 3
    assert torch.equal(la, lb) and ga.keys() == gb.keys()
    # Two steps of the UNTOUCHED model with the same seeds do not repeat bit for bit in every gradient: the final sums of about half
    # of them end in fp32 atomics (34 and 39 of 78 gradients repeated in two runs of this test, and not the same ones: a sum that
    # repeats once may not repeat the next time).  So "the same step" is: the loss bit for bit (the forward has no atomics), the
    # first-layer weight gradients of the pair heads bit for bit (dW1: one GEMM on the saved backward's dz and the forward's x rows,
    # the tensors the MXFP8 format would change), and every other gradient up to summation order (key biases: rounding noise around
    # an analytic zero, see above).
    same = [n for n in gb if torch.equal(ga[n], gb[n])]
    print(f"{len(same)} of {len(gb)} gradients are the untouched model's bits; the untouched model repeats "
          f"{sum(torch.equal(gb[n], gc[n]) for n in gb)} of them itself")
    for name in ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t"):
        n = f"peneo_decoder.{name}_fc.0.weight"
        assert torch.equal(gb[n], gc[n]) and torch.equal(ga[n], gb[n]), n
    for n in gb:
        if not n.endswith("key.bias"):
            assert float((ga[n] - gb[n]).abs().max()) <= 1e-4 * float(gb[n].abs().max()), n


# ---- 4. trained batch --------------------------------------------------------------------------------------------------------
def _train_and_decode(train_fmt, steps=TRAIN_STEPS, lr=TRAIN_LR):
    """the procedure of test_gpu_pair_mxfp8.trained_spot_agreement with the given train format; decoded in the bf16 eval format"""
    from peneo_amd.model import HandshakingTaggingScheme
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    m, pcfg = _model("lmv3")
    m.set_pair_heads_train_format(train_fmt)
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
    loss = float(out["loss"].detach())
    nn_ = batch["input_ids"].shape[1] - 1
    m.set_pair_heads_train_format("bf16")
    with torch.no_grad():
        o = m(**batch)
    spots = {}
    for k in OUT_KEYS:
        a = o[k + "_shaking_outputs"]
        spots[k] = [sorted(tuple(x[:3]) for x in HandshakingTaggingScheme.get_spots_from_shaking_tag(a[b_], seq_len=nn_))
                    for b_ in range(a.shape[0])]
    return loss, spots


def test_trained_batch_decodes_the_same_spots_as_a_bf16_trained_control(calls):
    loss_mx, spots_mx = _train_and_decode("mxfp8")
    assert calls["pair_heads_fwd_mxfp8_save"] == TRAIN_STEPS and calls["pair_bwd_saved"] == TRAIN_STEPS
    loss_16, spots_16 = _train_and_decode("bf16")
    assert calls["pair_heads_fwd_mxfp8_save"] == TRAIN_STEPS
    n = {k: sum(len(s) for s in spots_16[k]) for k in OUT_KEYS}
    print(f"final loss: mxfp8-trained {loss_mx:.3e}, bf16-trained {loss_16:.3e}; bf16 spots per map: {n}")
    assert sum(n.values()) > 0, n                                        # the comparison decodes something
    for k in OUT_KEYS:
        assert spots_mx[k] == spots_16[k], k
