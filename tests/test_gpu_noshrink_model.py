"""peneo_decoder_shrink = False, model level: the decoder runs at the backbone's output width (768 / 960 / 1024).
fp32 takes the materialising per-document path and is held to the fixture the real reference wrote and to the oracle; bf16 takes
the fused four-wave pair-heads forward (pair_heads_wide.hip) and the chunked backward and is held to the fp32 path, at the bar the
materialising bf16 path (PEneoDecoder.pair_wide = False, i.e. PENEO_PAIR_WIDE=0) sets on the same inputs.
Every model has one encoder layer, a 1000-word vocabulary, B = 2, S = 48 (N = 47, P = 1128), ragged documents."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
TAGS = ("line_extraction_shaking_tag", "ent_linking_head_rel_shaking_tag", "ent_linking_tail_rel_shaking_tag",
        "line_grouping_head_rel_shaking_tag", "line_grouping_tail_rel_shaking_tag")
WIDTHS = {"lmv3_base": 768, "lilt_base": 960, "lmv3_large": 1024}


def build_model(pcfg, dtype=torch.float32):
    from peneo_amd.model import PEneoConfig, PEneoModel
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    return m.cuda().set_compute_dtype(dtype)


def to_cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def maxdiff(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max())


def _config(which, **over):
    from seeded import layoutlmv3_config, lilt_config, peneo_config
    if which == "lilt_base":
        bcfg, name = lilt_config("base"), "lilt-roberta-en-base"
    else:
        bcfg, name = layoutlmv3_config("large" if which == "lmv3_large" else "base"), "layoutlmv3-base"
    bcfg = dict(bcfg, num_hidden_layers=1, vocab_size=1000)
    bcfg.update(over)
    return dict(peneo_config(name, bcfg), peneo_decoder_shrink=False)


@functools.lru_cache(maxsize=None)
def _case(which):
    """(pcfg, model with seeded weights in eval mode, host batch, device batch); tests restore what they switch on the model"""
    from seeded import seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    pcfg = _config(which)
    lilt = which == "lilt_base"
    m = build_model(pcfg)
    seeded_fill_(m.state_dict(), 21)
    assert m.peneo_decoder.decoder_hidden_size == WIDTHS[which]
    batch = synthetic_rfund_batch(2, 48, 12, 1000, seed=13, ragged=True, with_image=not lilt, add_sep=not lilt)
    if lilt:
        batch.pop("image", None)
    return pcfg, m.eval(), batch, to_cuda(batch)


@functools.lru_cache(maxsize=None)
def _oracle(which):
    from oracle import peneo_oracle as O
    pcfg, m, batch, _ = _case(which)
    with torch.no_grad():
        return O.peneo_forward({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, pcfg, batch, training=False,
                               as_executed=False)


def _fwd_bwd(m, batch, dt, seed_step=None):
    """(loss, {name: gradient}, outputs) of one forward + backward in compute dtype `dt`; `seed_step` resets the dropout seed
    counters first, so that two train-mode calls see the same masks (tests/test_gpu_model.py::_fwd_bwd)"""
    from peneo_amd.model.engine import DropoutSeeds
    m.set_compute_dtype(dt)
    if seed_step is not None:
        DropoutSeeds._step, m._step = seed_step, seed_step
    for p in m.parameters():
        p.grad = None
    out = m(**batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    return float(out["loss"]), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}, out


def _grad_stats(got, ref):
    """{name: (cosine, norm ratio, reference norm)}"""
    stats = {}
    for n, g in ref.items():
        a, r = got[n].double().flatten(), g.double().flatten()
        stats[n] = (float(torch.dot(a, r) / (a.norm() * r.norm() + 1e-300)), float(a.norm() / (r.norm() + 1e-300)), float(r.norm()))
    return stats


def _worst(stats):
    """(worst cosine, worst |norm ratio - 1|) over the gradients above 1e-6 of the largest norm"""
    gmax = max(v[2] for v in stats.values())
    big = [v for v in stats.values() if v[2] > 1e-6 * gmax]
    return min(v[0] for v in big), max(abs(v[1] - 1) for v in big)


@pytest.fixture
def fused_calls(monkeypatch):
    """the calls of ops.pair_heads_fwd (the fused kernel) as a list of their keyword arguments"""
    from peneo_amd import ops
    calls, orig = [], ops.pair_heads_fwd

    def spy(*a, **k):
        calls.append(dict(k, dtype=a[0].dtype, D=a[0].shape[-1] // 2))
        return orig(*a, **k)
    monkeypatch.setattr(ops, "pair_heads_fwd", spy)
    return calls


# ---------------------------------------------------------------------------------------------- the reference's fixture
def test_fp32_matches_the_reference_fixture(fused_calls):
    """tests/golden/lmv3_h768_noshrink.pt (the real reference, shrink off, D = 768): the bounds of
    test_fp32_forward_matches_reference / test_fp32_gradients_match_reference / test_base_s512_matches_reference_golden."""
    from seeded import seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    fx = load_golden("lmv3_h768_noshrink")
    m = build_model(fx["config"])
    seeded_fill_(m.state_dict(), fx["seed"])
    m = m.eval()
    out = m(**to_cuda(synthetic_rfund_batch(**fx["batch_args"])))
    assert not fused_calls                                   # fp32 at D = 768: the materialising path
    for h in HEADS:
        got, ref = out[h + "_shaking_outputs"], fx["logits"][h]
        assert got.dtype == torch.float32 and got.shape == ref.shape
        print(f"{h}: logits max diff {maxdiff(got, ref):.3e}")
        assert maxdiff(got, ref) < 5e-5, (h, maxdiff(got, ref))
        assert torch.equal(got.argmax(-1).cpu(), ref.argmax(-1)), h
        assert abs(float(out[h + "_loss"]) - float(fx["losses"][h + "_loss"])) < 1e-4
    assert abs(float(out["loss"]) - float(fx["losses"]["loss"])) < 1e-4
    out["loss"].backward()
    named = dict(m.named_parameters())
    for n, g in fx["grads_full"].items():
        err = maxdiff(named[n].grad, g)
        assert err <= 2e-3 * float(g.abs().max()) + 1e-6, (n, err, float(g.abs().max()))
    worst = 0.0
    for n, ref in fx["grad_norms"].items():
        if ref < 1e-7:
            continue
        worst = max(worst, abs(float(named[n].grad.norm()) - ref) / ref)
    print(f"worst relative gradient-norm error {worst:.3e}")
    assert worst < 5e-3, worst


# ---------------------------------------------------------------------------------------------- the oracle, three widths
@pytest.mark.parametrize("which", list(WIDTHS))
def test_fp32_matches_the_oracle(which, fused_calls):
    pcfg, m, _, batch = _case(which)
    ref = _oracle(which)
    m.set_compute_dtype(torch.float32)
    with torch.no_grad():
        out = m(**batch)
    assert not fused_calls
    for h in HEADS:
        k = h + "_shaking_outputs"
        assert maxdiff(out[k], ref[k]) < 1e-3, (k, maxdiff(out[k], ref[k]))
        lg, rg = out[k].cpu(), ref[k]
        top2 = rg.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 2e-3
        close = int((~clear).sum())
        print(f"{which} {h}: logits max diff {maxdiff(out[k], ref[k]):.3e}, {close} of {clear.numel()} pairs under the margin")
        assert close <= 0.01 * clear.numel(), (k, close)
        assert torch.equal(lg.argmax(-1)[clear], rg.argmax(-1)[clear]), k
    assert abs(float(out["loss"]) - float(ref["loss"])) < 1e-4


# ---------------------------------------------------------------------------------------------- bf16 against fp32
@pytest.mark.parametrize("which", list(WIDTHS))
def test_bf16_fused_path_against_fp32_at_the_bar_of_the_materialising_path(which, fused_calls):
    """Eval mode.  The fused forward + chunked backward may be no worse against fp32 than the materialising bf16 path by more than
    0.002 in the worst cosine and 0.005 in the worst norm ratio, and never below cosine 0.98."""
    pcfg, m, _, batch = _case(which)
    dec = m.peneo_decoder
    assert dec.pair_wide
    try:
        l32, g32, o32 = _fwd_bwd(m, batch, torch.float32)
        assert not fused_calls
        l16, g16, o16 = _fwd_bwd(m, batch, torch.bfloat16)
        assert len(fused_calls) == 1 and fused_calls[0]["D"] == WIDTHS[which] and fused_calls[0]["dtype"] == torch.bfloat16
        dec.pair_wide = False
        l16m, g16m, o16m = _fwd_bwd(m, batch, torch.bfloat16)
        assert len(fused_calls) == 1                         # the A/B arm really is the other path
    finally:
        dec.pair_wide = True
        m.set_compute_dtype(torch.float32)
    assert abs(l16 - l32) < 3e-2 * abs(l32), (l16, l32)
    assert abs(l16m - l32) < 3e-2 * abs(l32), (l16m, l32)
    for n, g in g16.items():
        assert torch.isfinite(g).all(), n
    assert g16.keys() == g32.keys() == g16m.keys()
    for h in HEADS:
        k = h + "_shaking_outputs"
        scale = float(o32[k].abs().max())
        assert maxdiff(o16[k], o32[k]) < 4e-2 * scale and maxdiff(o16m[k], o32[k]) < 4e-2 * scale and \
            maxdiff(o16[k], o16m[k]) < 4e-2 * scale, (k, maxdiff(o16[k], o32[k]), maxdiff(o16m[k], o32[k]), scale)
    cos_f, nr_f = _worst(_grad_stats(g16, g32))
    cos_m, nr_m = _worst(_grad_stats(g16m, g32))
    print(f"{which} D={WIDTHS[which]}: loss fp32 {l32:.6f} fused {l16:.6f} materialising {l16m:.6f}; worst cosine fused {cos_f:.6f} "
          f"materialising {cos_m:.6f}; worst |norm ratio - 1| fused {nr_f:.6f} materialising {nr_m:.6f}")
    assert cos_f >= cos_m - 0.002 and nr_f <= nr_m + 0.005, (cos_f, cos_m, nr_f, nr_m)
    assert cos_f >= 0.98, cos_f


# ---------------------------------------------------------------------------------------------- train mode, bf16, D = 768
def test_bf16_train_steps_repeat_and_differ_from_eval(fused_calls):
    """Two train-mode steps from the same seed counters: the same loss (1e-6 relative) and gradients equal up to the order of the
    fp32 atomics (the criterion of tests/test_gpu_model.py::_grad_agreement(repeat=True)); dropout really on."""
    pcfg, m, _, batch = _case("lmv3_base")
    torch.manual_seed(20251003)
    try:
        l_eval, _, _ = _fwd_bwd(m, batch, torch.bfloat16)
        m.train()
        la, ga, _ = _fwd_bwd(m, batch, torch.bfloat16, seed_step=4000)
        lb, gb, _ = _fwd_bwd(m, batch, torch.bfloat16, seed_step=4000)
    finally:
        m.eval()
        m.set_compute_dtype(torch.float32)
    assert len(fused_calls) == 3 and fused_calls[1]["drop_p"] > 0 and fused_calls[1]["drop_seed"] == fused_calls[2]["drop_seed"]
    assert abs(lb - la) < 1e-6 * abs(la), (la, lb)
    rep = _grad_stats(gb, ga)
    gmax = max(v[2] for v in rep.values())
    moved = {n: v[:2] for n, v in rep.items() if v[2] > 1e-6 * gmax and (v[0] < 1 - 1e-5 or abs(v[1] - 1) > 1e-3)}
    assert not moved, sorted(moved.items(), key=lambda kv: kv[1][0])[:12]
    assert abs(la - l_eval) > 1e-3 * abs(l_eval), (la, l_eval)


def test_bf16_train_decoder_gradients_match_autograd_with_the_host_mask(fused_calls):
    """The decoder stage alone at D = 768, N = 47, train mode: fused forward with the K12 mask, chunked backward regenerating it.
    Gradients of combine_fc and the five heads against torch autograd of the explicit computation with the mask of
    tests/dropout_ref.py: cosine >= 0.99, norm ratio within 3 %."""
    from dropout_ref import k12_keep, k12_scale
    pcfg, m, _, batch = _case("lmv3_base")
    dec = m.peneo_decoder
    D, B = 768, 2
    tags = [batch[k] for k in TAGS]
    P = tags[0].shape[1]
    N = int(((8 * P + 1) ** 0.5 - 1) // 2)
    assert N == 47
    g = torch.Generator().manual_seed(5)
    seq = torch.randn(B, N, D, generator=g).cuda().to(torch.bfloat16)
    for p in m.parameters():
        p.grad = None
    try:
        dec.train()
        out = dec(seq, **dict(zip(TAGS, tags)))
        out["loss"].backward()
        torch.cuda.synchronize()
    finally:
        dec.eval()
    assert len(fused_calls) == 1 and fused_calls[0]["drop_p"] > 0
    p_drop, seed = fused_calls[0]["drop_p"], int(fused_calls[0]["drop_seed"]) & 0xFFFFFFFF
    # the explicit computation: fp32 autograd on bf16-rounded operands (straight-through), the mask from the host restatement
    q = lambda t: t + (t.to(torch.bfloat16).float() - t).detach()
    named = dict(dec.named_parameters())
    leaf = {n: p.detach().clone().requires_grad_(True) for n, p in named.items()}
    wc, bc = leaf["handshaking_kernel.combine_fc.weight"], leaf["handshaking_kernel.combine_fc.bias"]
    h = seq.float()
    a = q(F.linear(h, q(wc[:, :D])))
    b_ = q(F.linear(h, q(wc[:, D:]), bc))
    ii, jj = torch.triu_indices(N, N, device="cuda")
    x = q(F.silu(a[:, ii] + b_[:, jj]))
    keep = torch.stack([k12_keep(seed, b, 0, P, len(HEADS) * D, p_drop) for b in range(B)]).cuda()
    cw = torch.tensor(pcfg["peneo_category_weights"], device="cuda")
    loss = 0.0
    for hd, name in enumerate(HEADS):
        w1, b1 = leaf[f"{name}_fc.0.weight"], leaf[f"{name}_fc.0.bias"]
        w2, b2 = leaf[f"{name}_fc.3.weight"], leaf[f"{name}_fc.3.bias"]
        y = F.silu(F.linear(x, q(w1), b1)) * keep[:, :, hd * D:(hd + 1) * D] * k12_scale(p_drop)
        lg = F.linear(q(y), q(w2), b2)
        C = lg.shape[-1]
        loss = loss + F.cross_entropy(lg.view(-1, C), tags[hd].view(-1), weight=cw[:C])
    assert abs(float(out["loss"]) - float(loss)) < 3e-2 * abs(float(loss)), (float(out["loss"]), float(loss))
    loss.backward()
    stats = _grad_stats({n: named[n].grad for n in leaf}, {n: leaf[n].grad for n in leaf})
    assert len(stats) == 2 + 4 * len(HEADS)
    for n, (cos, ratio, norm) in sorted(stats.items()):
        print(f"{n}: cosine {cos:.5f} norm ratio {ratio:.4f}")
    bad = {n: v[:2] for n, v in stats.items() if v[0] < 0.99 or abs(v[1] - 1) > 0.03}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- other behaviour
def test_mxfp8_setters_refuse_the_width():
    _, m, _, _ = _case("lmv3_base")
    try:
        m.set_compute_dtype(torch.bfloat16)
        with pytest.raises(ValueError, match="D = 768"):
            m.set_pair_heads_format("mxfp8")
        with pytest.raises(ValueError, match="D = 768"):
            m.set_pair_heads_train_format("mxfp8")
        assert m.peneo_decoder.pair_heads_format == "bf16" and m.peneo_decoder.pair_heads_train_format == "bf16"
    finally:
        m.set_compute_dtype(torch.float32)


def test_deterministic_mode_2_refuses_the_wide_backward_and_mode_1_runs_it():
    import peneo_amd
    from peneo_amd import hip
    _, m, _, batch = _case("lmv3_base")
    try:
        m.set_compute_dtype(torch.bfloat16)
        with peneo_amd.deterministic(2):
            with pytest.raises(ValueError, match="the decoder backward at D = 768 without peneo_pair_bwd_fused and peneo_pair_dz_fused"):
                m(**batch)["loss"].backward()
        m.zero_grad(set_to_none=True)
        with peneo_amd.deterministic(1):
            c0 = hip.order_dependent_launches()
            out = m(**batch)
            out["loss"].backward()
            torch.cuda.synchronize()
            assert hip.order_dependent_launches() > c0
        assert torch.isfinite(out["loss"])
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    finally:
        m.zero_grad(set_to_none=True)
        m.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_width_without_a_fused_kernel_runs_on_the_materialising_path(dtype, fused_calls):
    """hidden 320, shrink off: D = 320 (D / 16 = 20 is in no kernel's list), one layer; forward and backward in both dtypes, fp32
    against the oracle."""
    from oracle import peneo_oracle as O
    from seeded import seeded_fill_
    from peneo_amd import ops
    from peneo_amd.data import synthetic_rfund_batch
    assert not ops.pair_heads_supported(dtype, 320, 5)
    pcfg = _config("lmv3_base", hidden_size=320, num_attention_heads=5, intermediate_size=640, max_position_embeddings=66,
                   coordinate_size=54, shape_size=52)
    m = build_model(pcfg, dtype)
    sd = seeded_fill_(m.state_dict(), 23)
    assert m.peneo_decoder.decoder_hidden_size == 320
    batch = synthetic_rfund_batch(2, 48, 12, 1000, seed=14, ragged=True, with_image=True, add_sep=True)
    m = m.eval()
    out = m(**to_cuda(batch))
    out["loss"].backward()
    torch.cuda.synchronize()
    assert not fused_calls
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(torch.isfinite(g_).all() for g_ in grads)
    with torch.no_grad():
        ref = O.peneo_forward({k: v.detach().cpu().clone() for k, v in sd.items()}, pcfg, batch, training=False, as_executed=False)
    tol = 1e-4 if dtype == torch.float32 else 3e-2 * abs(float(ref["loss"]))
    assert abs(float(out["loss"]) - float(ref["loss"])) < tol, (float(out["loss"]), float(ref["loss"]))
    for h in HEADS:
        k = h + "_shaking_outputs"
        bound = 1e-3 if dtype == torch.float32 else 4e-2 * float(ref[k].abs().max())
        assert maxdiff(out[k], ref[k]) < bound, (k, maxdiff(out[k], ref[k]))
