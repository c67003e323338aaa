"""PEneoDecoder.fused_dz_wide (PENEO_DZ_FUSED_WIDE), model level: with the switch on, the chunked decoder backward at 512 < D <= 1024
takes the fused_dz branch on the four-wave peneo_pair_dz_fused (pair_dz_wide.hip); with it off nothing changes.
One-layer models with seeded weights, a 1000-word vocabulary, B = 2, S = 48 (N = 47, P = 1128), ragged documents, shrink off: the
models of tests/test_gpu_noshrink_model.py, whose helpers are restated here."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
TAGS = ("line_extraction_shaking_tag", "ent_linking_head_rel_shaking_tag", "ent_linking_tail_rel_shaking_tag",
        "line_grouping_head_rel_shaking_tag", "line_grouping_tail_rel_shaking_tag")
WIDTHS = {"lmv3_base": 768, "lilt_base": 960, "lmv3_large": 1024}
B, N = 2, 47


def _to_cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


@functools.lru_cache(maxsize=None)
def _case(which):
    """(pcfg, model with seeded weights in eval mode, device batch); tests restore what they switch on the model"""
    from seeded import layoutlmv3_config, lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    from peneo_amd.model import PEneoConfig, PEneoModel
    lilt = which == "lilt_base"
    if lilt:
        bcfg, name = lilt_config("base"), "lilt-roberta-en-base"
    else:
        bcfg, name = layoutlmv3_config("large" if which == "lmv3_large" else "base"), "layoutlmv3-base"
    pcfg = dict(peneo_config(name, dict(bcfg, num_hidden_layers=1, vocab_size=1000)), peneo_decoder_shrink=False)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})).cuda().set_compute_dtype(torch.float32)
    seeded_fill_(m.state_dict(), 21)
    assert m.peneo_decoder.decoder_hidden_size == WIDTHS[which]
    assert m.peneo_decoder.fused_dz_wide is False and m.peneo_decoder.fused_dz is True       # the defaults
    batch = synthetic_rfund_batch(2, 48, 12, 1000, seed=13, ragged=True, with_image=not lilt, add_sep=not lilt)
    if lilt:
        batch.pop("image", None)
    return pcfg, m.eval(), _to_cuda(batch)


def _fwd_bwd(m, batch, dt):
    m.set_compute_dtype(dt)
    for p in m.parameters():
        p.grad = None
    out = m(**batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out["loss"].detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


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
def spies(monkeypatch):
    """calls of ops.pair_dz_fused (their D and whether x / pre were asked for), of ops.pair_dz, and of ops.gemm with pair_dz="""
    from peneo_amd import ops
    seen = dict(fused=[], dz=0, gemm_dz=0)
    o_fused, o_dz, o_gemm = ops.pair_dz_fused, ops.pair_dz, ops.gemm

    def fused(ab_doc, *a, **k):
        seen["fused"].append(ab_doc.shape[-1] // 2)
        return o_fused(ab_doc, *a, **k)

    def dz(*a, **k):
        seen["dz"] += 1
        return o_dz(*a, **k)

    def gemm(*a, **k):
        seen["gemm_dz"] += k.get("pair_dz") is not None
        return o_gemm(*a, **k)
    monkeypatch.setattr(ops, "pair_dz_fused", fused)
    monkeypatch.setattr(ops, "pair_dz", dz)
    monkeypatch.setattr(ops, "gemm", gemm)
    return seen


@pytest.mark.parametrize("which", list(WIDTHS))
def test_eval_gradients_against_fp32_at_the_bar_of_the_parent_arm(which, spies):
    """Eval mode, bf16 with the switch on and off, both against the fp32 path: the new arm may be no worse than the parent arm by more
    than 0.002 in the worst cosine and 0.005 in the worst |norm ratio - 1|, and never below cosine 0.98 (the bar of
    test_bf16_fused_path_against_fp32_at_the_bar_of_the_materialising_path)."""
    _, m, batch = _case(which)
    dec = m.peneo_decoder
    try:
        _, g32 = _fwd_bwd(m, batch, torch.float32)
        spies["dz"] = spies["gemm_dz"] = 0                     # (the materialising fp32 path is not what is counted)
        _, g_off = _fwd_bwd(m, batch, torch.bfloat16)
        assert not spies["fused"] and spies["gemm_dz"] == B
        dec.fused_dz_wide = True
        _, g_on = _fwd_bwd(m, batch, torch.bfloat16)
        assert spies["fused"] == [WIDTHS[which]] * B and spies["gemm_dz"] == B
    finally:
        dec.fused_dz_wide = False
        m.set_compute_dtype(torch.float32)
    assert g_on.keys() == g_off.keys() == g32.keys()
    assert all(torch.isfinite(g).all() for g in g_on.values())
    cos_on, nr_on = _worst(_grad_stats(g_on, g32))
    cos_off, nr_off = _worst(_grad_stats(g_off, g32))
    print(f"{which} D={WIDTHS[which]}: worst cosine wide dz {cos_on:.6f} parent {cos_off:.6f}; worst |norm ratio - 1| wide dz {nr_on:.6f} "
          f"parent {nr_off:.6f}")
    assert cos_on >= cos_off - 0.002 and nr_on <= nr_off + 0.005, (cos_on, cos_off, nr_on, nr_off)
    assert cos_on >= 0.98, cos_on


@pytest.mark.parametrize("writes_x", [False, True])
def test_train_decoder_gradients_match_autograd_with_the_host_mask(writes_x, spies, monkeypatch):
    """The decoder stage alone at D = 768, N = 47, train mode, the switch on (the kernel regenerates the K12 mask), in both arrangements
    of x / pre: the construction and the bounds of test_bf16_train_decoder_gradients_match_autograd_with_the_host_mask
    (cosine >= 0.99, norm ratio within 3 %)."""
    from dropout_ref import k12_keep, k12_scale
    from peneo_amd import ops
    pcfg, m, batch = _case("lmv3_base")
    dec = m.peneo_decoder
    D = 768
    tags = [batch[k] for k in TAGS]
    P = tags[0].shape[1]
    assert P == N * (N + 1) // 2
    fwd, o_fwd = [], ops.pair_heads_fwd

    def fwd_spy(*a, **k):
        fwd.append(k)
        return o_fwd(*a, **k)
    monkeypatch.setattr(ops, "pair_heads_fwd", fwd_spy)
    g = torch.Generator().manual_seed(5)
    seq = torch.randn(B, N, D, generator=g).cuda().to(torch.bfloat16)
    for p in m.parameters():
        p.grad = None
    try:
        dec.fused_dz_wide, dec.dz_wide_writes_x = True, writes_x
        dec.train()
        out = dec(seq, **dict(zip(TAGS, tags)))
        out["loss"].backward()
        torch.cuda.synchronize()
    finally:
        dec.eval()
        dec.fused_dz_wide, dec.dz_wide_writes_x = False, False
    assert spies["fused"] == [D] * B and spies["dz"] == 0 and spies["gemm_dz"] == 0
    assert len(fwd) == 1 and fwd[0]["drop_p"] > 0
    p_drop, seed = fwd[0]["drop_p"], int(fwd[0]["drop_seed"]) & 0xFFFFFFFF
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
    assert abs(float(out["loss"].detach()) - float(loss.detach())) < 3e-2 * abs(float(loss.detach())), (float(out["loss"].detach()), float(loss.detach()))
    loss.backward()
    stats = _grad_stats({n: named[n].grad for n in leaf}, {n: leaf[n].grad for n in leaf})
    assert len(stats) == 2 + 4 * len(HEADS)
    for n, (cos, ratio, norm) in sorted(stats.items()):
        print(f"writes_x={writes_x} {n}: cosine {cos:.5f} norm ratio {ratio:.4f}")
    bad = {n: v[:2] for n, v in stats.items() if v[0] < 0.99 or abs(v[1] - 1) > 0.03}
    assert not bad, bad


@pytest.mark.parametrize("train", [False, True])
def test_routing_and_the_untouched_forward(train, spies):
    """B x chunks calls of ops.pair_dz_fused at the model's D with the switch on and none with it off; no ops.pair_dz and no pair_dz=
    GEMM with it on; the two arms' losses are the same bits (the forward is untouched)."""
    from peneo_amd.model.engine import DropoutSeeds
    from peneo_amd.model.peneo_decoder import _row_chunks
    _, m, batch = _case("lmv3_base")
    dec = m.peneo_decoder
    chunk_pairs = dec.bwd_chunk_pairs
    try:
        dec.bwd_chunk_pairs = 400                              # three chunks a document instead of one
        nchunks = len(_row_chunks(N, 400))
        assert nchunks == 3
        m.train(train)
        DropoutSeeds._step, m._step = 4100, 4100
        l_off, _ = _fwd_bwd(m, batch, torch.bfloat16)
        assert not spies["fused"]
        assert (spies["dz"], spies["gemm_dz"]) == ((B * nchunks, 0) if train else (0, B * nchunks))
        spies["dz"] = spies["gemm_dz"] = 0
        dec.fused_dz_wide = True
        DropoutSeeds._step, m._step = 4100, 4100
        l_on, g_on = _fwd_bwd(m, batch, torch.bfloat16)
        assert spies["fused"] == [768] * (B * nchunks)
        assert spies["dz"] == 0 and spies["gemm_dz"] == 0
    finally:
        dec.fused_dz_wide = False
        dec.bwd_chunk_pairs = chunk_pairs
        m.eval()
        m.set_compute_dtype(torch.float32)
    assert torch.equal(l_on, l_off), (float(l_on), float(l_off))
    assert all(torch.isfinite(g).all() for g in g_on.values())


def test_deterministic_mode_2_still_refuses_and_mode_1_runs(spies):
    import peneo_amd
    _, m, batch = _case("lmv3_base")
    dec = m.peneo_decoder
    try:
        m.set_compute_dtype(torch.bfloat16)
        dec.fused_dz_wide = True
        with peneo_amd.deterministic(2):
            with pytest.raises(ValueError, match="the decoder backward at D = 768 without peneo_pair_bwd_fused and peneo_pair_dz_fused"):
                m(**batch)["loss"].backward()
        assert not spies["fused"]
        m.zero_grad(set_to_none=True)
        with peneo_amd.deterministic(1):
            out = m(**batch)
            out["loss"].backward()
            torch.cuda.synchronize()
        assert spies["fused"] == [768] * B
        assert torch.isfinite(out["loss"])
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    finally:
        dec.fused_dz_wide = False
        m.zero_grad(set_to_none=True)
        m.set_compute_dtype(torch.float32)
