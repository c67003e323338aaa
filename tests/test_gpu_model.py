"""End-to-end parity of the HIP PEneoModel against the reference-generated golden fixtures
(logits / losses / gradients) and the CPU oracle."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")


def build_model(pcfg, state_dict=None, dtype=torch.float32):
    from peneo_amd.model import PEneoConfig, PEneoModel
    cfg = PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"})
    m = PEneoModel(cfg)
    if state_dict is not None:
        m.load_state_dict(state_dict, strict=True)
    return m.cuda().set_compute_dtype(dtype)


def to_cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def maxdiff(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max())


@pytest.mark.parametrize("name", ["lmv3_tiny", "lmv3_tiny_s24", "lilt_tiny", "lmv3_tiny_cls1", "lmv3_tiny_cls3"])
def test_fp32_forward_matches_reference(name):
    fx = load_golden(name)
    m = build_model(fx["config"], fx["state_dict"]).eval()
    with torch.no_grad():
        out = m(**to_cuda(fx["batch"]))
    ref = fx["outputs"]
    for h in HEADS:
        k = h + "_shaking_outputs"
        assert out[k].dtype == torch.float32 and out[k].shape == ref[k].shape
        assert maxdiff(out[k], ref[k]) < 1e-3, (k, maxdiff(out[k], ref[k]))       # north_star tolerance
        assert maxdiff(out[k], ref[k]) < 5e-5, (k, maxdiff(out[k], ref[k]))       # what fp32 MFMA actually achieves
        assert torch.equal(out[k].argmax(-1).cpu(), ref[k].argmax(-1)), k            # pair-tag indices bit-exact
        assert abs(float(out[h + "_loss"]) - float(ref[h + "_loss"])) < 1e-4
    assert abs(float(out["loss"]) - float(ref["loss"])) < 1e-4
    assert torch.equal(out["orig_bbox"].cpu(), ref["orig_bbox"])


@pytest.mark.parametrize("name", ["lmv3_tiny", "lmv3_tiny_s24", "lilt_tiny", "lmv3_tiny_cls1", "lmv3_tiny_cls3"])
def test_fp32_gradients_match_reference(name):
    fx = load_golden(name)
    m = build_model(fx["config"], fx["state_dict"]).eval()   # eval: dropout off, like the fixture
    out = m(**to_cuda(fx["batch"]))
    out["loss"].backward()
    checked = 0
    for n, p in m.named_parameters():
        g = fx["grads"].get(n)
        if g is None:
            continue
        assert p.grad is not None, n
        err = maxdiff(p.grad, g)
        assert err <= 2e-3 * float(g.abs().max()) + 1e-6, (n, err, float(g.abs().max()))
        checked += 1
    assert checked == len(fx["grads"])


@pytest.mark.parametrize("name", ["lmv3_tiny", "lilt_tiny", "lmv3_tiny_cls1", "lmv3_tiny_cls3"])
def test_bf16_forward_close_to_reference(name):
    fx = load_golden(name)
    m = build_model(fx["config"], fx["state_dict"], torch.bfloat16).eval()
    with torch.no_grad():
        out = m(**to_cuda(fx["batch"]))
    ref = fx["outputs"]
    for h in HEADS:
        k = h + "_shaking_outputs"
        scale = float(ref[k].abs().max())
        assert maxdiff(out[k], ref[k]) < 4e-2 * scale, (k, maxdiff(out[k], ref[k]), scale)
    assert abs(float(out["loss"]) - float(ref["loss"])) < 2e-2 * float(ref["loss"])


@pytest.mark.parametrize("name", ["lmv3_tiny", "lilt_tiny", "lmv3_tiny_cls1", "lmv3_tiny_cls3"])
def test_bf16_gradients_close_to_reference(name):
    fx = load_golden(name)
    m = build_model(fx["config"], fx["state_dict"], torch.bfloat16).eval()
    out = m(**to_cuda(fx["batch"]))
    out["loss"].backward()
    bad = []
    for n, p in m.named_parameters():
        g = fx["grads"].get(n)
        if g is None:
            continue
        # cosine similarity is the robust statement for bf16 gradients
        a, b = p.grad.float().cpu().flatten(), g.flatten()
        if float(b.norm()) < 1e-6:
            continue
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-12))
        if cos < 0.98:
            bad.append((n, cos))
    assert not bad, bad


def test_inference_mode_tuple_and_decode():
    from peneo_amd.model import HandshakingTaggingScheme
    from oracle import peneo_oracle as O
    fx = load_golden("lmv3_tiny")
    pcfg = dict(fx["config"], inference_mode=True)
    m = build_model(pcfg, fx["state_dict"]).eval()
    b = to_cuda(fx["batch"])
    with torch.no_grad():
        res = m(input_ids=b["input_ids"], bbox=b["bbox"], orig_bbox=b["orig_bbox"], attention_mask=b["attention_mask"],
                image=b["image"], fname=["a", "b"], text=[["x"], ["y"]])   # extra non-tensor keys are tolerated
    assert isinstance(res, tuple) and len(res) == 6
    ref = fx["outputs"]
    order = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")
    for t, h in zip(res[:5], order):
        assert maxdiff(t, ref[h + "_shaking_outputs"]) < 5e-5
    assert torch.equal(res[5].cpu(), ref["orig_bbox"])
    # K14: device decode of one map == the oracle's Python loop on the reference logits
    spots = HandshakingTaggingScheme.get_spots_from_shaking_tag(res[1][0], seq_len=39)
    want = O.spots_from_logits(ref["ent_linking_h2h_shaking_outputs"][0])
    assert [(i, j, t) for i, j, t, _ in spots] == [(i, j, t) for i, j, t, _ in want]
    assert max(abs(a[3] - b_[3]) for a, b_ in zip(spots, want)) < 1e-5 if want else True


def test_missing_labels_raise():
    fx = load_golden("lmv3_tiny")
    m = build_model(fx["config"], fx["state_dict"]).eval()
    b = to_cuda(fx["batch"])
    with pytest.raises(AssertionError):
        m(input_ids=b["input_ids"], bbox=b["bbox"], orig_bbox=b["orig_bbox"], attention_mask=b["attention_mask"],
          image=b["image"])
    bad = dict(b)
    bad["bbox"] = b["bbox"].clone()
    bad["bbox"][0, 2, 0] = 1200
    with pytest.raises(IndexError):
        m(**bad)


@pytest.mark.parametrize("name", ["lmv3_tiny", "lilt_tiny"])
def test_bbox_out_of_range_raises_like_the_reference(name):
    """Reference modeling_layoutlmv3.py:133 / modeling_lilt.py raise IndexError on a bbox coordinate outside 0..1000-ish tables.  Here
    the embedding kernel sets a sticky device flag: read at once by default (the reference's behaviour), left on the device with
    check_inputs = "deferred" until raise_on_bad_inputs() (what bench.py runs with), ignored with check_inputs = False."""
    fx = load_golden(name)
    m = build_model(fx["config"], fx["state_dict"]).eval()
    good = to_cuda(fx["batch"])
    bad = dict(good)
    bad["bbox"] = good["bbox"].clone()
    bad["bbox"][0, 3, 2] = 5000
    with torch.no_grad():
        m(**good)                                             # clean inputs: no flag
        m.backbone.raise_on_bad_inputs()
        with pytest.raises(IndexError):
            m(**bad)
        m.backbone.check_inputs = "deferred"
        m(**bad)                                              # no host sync, no exception here ...
        m(**good)                                             # ... the flag is sticky across forwards ...
        with pytest.raises(IndexError):
            m.backbone.raise_on_bad_inputs()                  # ... until it is read
        m.backbone.raise_on_bad_inputs()                      # and cleared by the read
        m.backbone.check_inputs = False
        m(**bad)
        m.backbone.check_inputs = "deferred"
        m.backbone.raise_on_bad_inputs()                      # (nothing was recorded with the check off)


def test_cpu_tensors_are_rejected_loudly():
    from peneo_amd.hip import PeneoHipError
    fx = load_golden("lmv3_tiny")
    m = build_model(fx["config"], fx["state_dict"]).eval()
    with pytest.raises(PeneoHipError):
        m(**fx["batch"])


def test_train_mode_dropout_runs_and_is_seeded():
    fx = load_golden("lmv3_tiny")
    m = build_model(fx["config"], fx["state_dict"], torch.bfloat16).train()
    b = to_cuda(fx["batch"])
    out = m(**b)
    out["loss"].backward()
    assert torch.isfinite(out["loss"])
    gn = sum(float(p.grad.float().norm()) for p in m.parameters() if p.grad is not None)
    assert gn > 0 and gn == gn
    eval_loss = float(fx["outputs"]["loss"])
    assert abs(float(out["loss"]) - eval_loss) < 0.5 * eval_loss   # perturbed by dropout, not garbage


def test_base_s512_matches_reference_golden():
    """LayoutLMv3-base, seq 512, 128 lines, B=2 (BASELINE config 2 shape): weights regenerated from the seed."""
    from seeded import seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    fx = load_golden("lmv3_base_s512")
    m = build_model(fx["config"])
    seeded_fill_(m.state_dict(), fx["seed"])
    m = m.eval()
    batch = to_cuda(synthetic_rfund_batch(**fx["batch_args"]))
    out = m(**batch)
    for h in HEADS:
        lg = out[h + "_shaking_outputs"]
        s = fx["samples"][h]
        got = lg[:, s["idx"].cuda()].cpu()
        assert (got - s["logits"]).abs().max() < 1e-3, (h, float((got - s["logits"]).abs().max()))
        pred = lg.argmax(-1).cpu()
        ref_nz = fx["argmax"][h]
        # exact away from near-ties (margin < 2e-3 in the reference); count mismatches
        P = lg.shape[1]
        cs = int((pred * (torch.arange(P) % 65521 + 1)).sum())
        nz = int((pred != 0).sum())
        assert abs(nz - ref_nz["count_nonzero"]) <= ref_nz["near_ties"], (h, nz, ref_nz["count_nonzero"])
        if ref_nz["near_ties"] == 0:
            assert cs == ref_nz["checksum"]
        assert abs(float(out[h + "_loss"]) - float(fx["losses"][h + "_loss"])) < 1e-4
    assert abs(float(out["loss"]) - float(fx["losses"]["loss"])) < 1e-4
    out["loss"].backward()
    worst = 0.0
    for n, p in m.named_parameters():
        ref = fx["grad_norms"].get(n)
        if ref is None or ref < 1e-7:
            continue
        worst = max(worst, abs(float(p.grad.norm()) - ref) / ref)
    assert worst < 5e-3, worst
    for n, g in fx["grads_full"].items():
        p = dict(m.named_parameters())[n]
        assert maxdiff(p.grad, g) <= 2e-3 * float(g.abs().max()) + 1e-7, n


@pytest.mark.parametrize("which", ["lmv3_large_s1024", "lilt_base_s512", "lmv3_chinese_s512", "lilt_infoxlm_s512"])
def test_full_width_shapes_match_the_oracle(which):
    """BASELINE config 4 / 5 widths (H = 1024, 16 heads, S = 1024, N = 1023, D = 512; LiLT H = 768 + 192, head dim 64 + 16)
    with ONE encoder layer so that the CPU oracle finishes in seconds: fp32 logits / loss parity on seeded weights,
    ragged attention masks, then a bf16 forward + backward through the same shapes."""
    from oracle import peneo_oracle as O
    from seeded import layoutlmv3_config, lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    if which == "lmv3_large_s1024":
        bcfg = dict(layoutlmv3_config("large"), num_hidden_layers=1)
        pcfg = peneo_config("layoutlmv3-base", bcfg)
        batch = synthetic_rfund_batch(1, 1024, 256, bcfg["vocab_size"], seed=3)
    elif which == "lmv3_chinese_s512":
        # the XLM-R-vocabulary registry entry (model/backbone_mapping.py:325-336): vocab 250 002 = a 768 MB fp32 word table,
        # token ids drawn from the whole vocabulary, S = 512, one encoder layer
        bcfg = dict(layoutlmv3_config("base"), num_hidden_layers=1, vocab_size=250002)
        pcfg = peneo_config("layoutlmv3-base-chinese", bcfg)
        batch = synthetic_rfund_batch(2, 512, 128, bcfg["vocab_size"], seed=5, ragged=True)
    elif which == "lilt_infoxlm_s512":
        bcfg = dict(lilt_config("base"), num_hidden_layers=1, vocab_size=250002)    # model/backbone_mapping.py:277-288
        pcfg = peneo_config("lilt-infoxlm-base", bcfg)
        batch = synthetic_rfund_batch(2, 512, 128, bcfg["vocab_size"], seed=6, ragged=True, add_sep=False)
        batch.pop("image", None)
    else:
        bcfg = dict(lilt_config("base"), num_hidden_layers=1)
        pcfg = peneo_config("lilt-roberta-en-base", bcfg)
        batch = synthetic_rfund_batch(2, 512, 128, bcfg["vocab_size"], seed=4)
        batch.pop("image", None)
        # ragged: the second document ends early (pad id 1, mask 0, zero boxes)
        batch["input_ids"][1, 400:] = bcfg["pad_token_id"]
        batch["attention_mask"][1, 400:] = 0
        batch["bbox"][1, 400:] = 0
    m = build_model(pcfg)
    sd = m.state_dict()
    seeded_fill_(sd, 21)
    m = m.eval()
    with torch.no_grad():
        out = m(**to_cuda(batch))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        ref = O.peneo_forward({k: v.cpu() for k, v in sd.items()}, pcfg, batch, training=False, as_executed=False)
    for h in HEADS:
        k = h + "_shaking_outputs"
        assert maxdiff(out[k], ref[k]) < 1e-3, (k, maxdiff(out[k], ref[k]))
        lg, rg = out[k].cpu(), ref[k]
        top2 = rg.topk(2, dim=-1).values
        clear = (top2[..., 0] - top2[..., 1]) > 2e-3
        assert torch.equal(lg.argmax(-1)[clear], rg.argmax(-1)[clear]), k
    assert abs(float(out["loss"]) - float(ref["loss"])) < 1e-4
    # bf16 throughput mode through the same shapes: finite loss close to fp32, finite gradients everywhere
    m.set_compute_dtype(torch.bfloat16)
    o2 = m(**to_cuda(batch))
    o2["loss"].backward()
    assert abs(float(o2["loss"]) - float(ref["loss"])) < 3e-2 * abs(float(ref["loss"]))
    for n, p in m.named_parameters():
        if p.requires_grad and p.grad is not None:
            assert torch.isfinite(p.grad).all(), n
    if "250002" in str(bcfg["vocab_size"]):
        # the word-table gradient (scatter of 1024 token rows into 250 002): rows of tokens that occur, and only those, are hit
        g = m.backbone.embeddings.word_embeddings.weight.grad
        used = torch.zeros(bcfg["vocab_size"], dtype=torch.bool)
        ids = batch["input_ids"][batch["attention_mask"].bool()]
        used[ids] = True
        used[bcfg["pad_token_id"]] = False
        hit = (g.abs().sum(1) > 0).cpu()
        assert int(ids.max()) > 200000 and torch.equal(hit, used)


def _fwd_bwd(m, batch, dt, seed_step=None):
    """(loss, {name: gradient}) of one forward + backward of `m` in compute dtype `dt`; `seed_step` resets the dropout seed
    counters first, so that two calls in train mode see the same masks (every mask is a pure function of (seed, element))."""
    from peneo_amd.model.engine import DropoutSeeds
    m.set_compute_dtype(dt)
    if seed_step is not None:
        DropoutSeeds._step, m._step = seed_step, seed_step
    for p in m.parameters():
        p.grad = None
    out = m(**batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    return float(out["loss"]), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _grad_stats(got, ref):
    """{name: (cosine, norm ratio, reference norm)}"""
    stats = {}
    for n, g in ref.items():
        a, r = got[n].double().flatten(), g.double().flatten()
        stats[n] = (float(torch.dot(a, r) / (a.norm() * r.norm() + 1e-300)), float(a.norm() / (r.norm() + 1e-300)), float(r.norm()))
    return stats


def _grad_agreement(m, batch, seed_step=None, repeat=True):
    """(loss_fp32, loss_bf16, {name: (cosine, norm ratio, norm)}) of the default bf16 path against the fp32 path of the same
    model, and -- `repeat` -- a second bf16 step whose GRADIENTS (not only the loss) must reproduce the first up to the order
    of the fp32 atomics."""
    l32, g32 = _fwd_bwd(m, batch, torch.float32, seed_step)
    l16, g16 = _fwd_bwd(m, batch, torch.bfloat16, seed_step)
    if repeat:
        l16b, g16b = _fwd_bwd(m, batch, torch.bfloat16, seed_step)
        assert abs(l16b - l16) < 1e-6 * abs(l16), (l16b, l16)
        rep = _grad_stats(g16b, g16)
        gmax = max(v[2] for v in rep.values())
        moved = {n: v[:2] for n, v in rep.items() if v[2] > 1e-6 * gmax and (v[0] < 1 - 1e-5 or abs(v[1] - 1) > 1e-3)}
        assert not moved, sorted(moved.items(), key=lambda kv: kv[1][0])[:12]
    return l32, l16, _grad_stats(g16, g32)


def _assert_agreement(l32, l16, stats, cos_min, norm_tol, loss_tol=2e-2):
    assert abs(l16 - l32) < loss_tol * abs(l32), (l16, l32)
    gmax = max(v[2] for v in stats.values())
    bad = {n: v[:2] for n, v in stats.items() if v[2] > 1e-6 * gmax and (v[0] < cos_min or abs(v[1] - 1) > norm_tol)}
    assert not bad, sorted(bad.items(), key=lambda kv: kv[1][0])[:12]


def test_bf16_path_matches_fp32_path_at_the_benchmark_size():
    """BASELINE config 2 exactly as bench.py runs it (LayoutLMv3-base, B = 8 documents, S = 512, N = 511, bf16; dropout off):
    every parameter gradient of the default bf16 path -- fused pair backward (8 448 blocks, the 256-slot workspace wrapped
    33x) with the held side-stream dW1 GEMM, single-pass attention backward at T = 709 / 576 workgroups, the bf16 dS^T-slab
    rel-pos reduction over 12 layers, LDS-DMA GEMMs -- against the fp32 path of the same model, which
    test_base_s512_matches_reference_golden pins to the reference.  (reference: model/peneo_decoder.py:349-428,
    modeling_layoutlmv3.py:365-404)"""
    from seeded import layoutlmv3_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = build_model(pcfg)
    seeded_fill_(m.state_dict(), 11)
    m = m.eval()
    batch = to_cuda(synthetic_rfund_batch(8, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=1008))
    l32, l16, stats = _grad_agreement(m, batch)     # incl. a repeated bf16 step: same gradients up to atomic ordering
    _assert_agreement(l32, l16, stats, 0.995, 0.02)


def test_bf16_path_matches_fp32_path_at_the_benchmark_size_with_dropout_on():
    """The step bench.py TIMES: LayoutLMv3-base, B = 8, S = 512, train mode -- every dropout site on (embedding / hidden /
    attention-probability dropout of the encoder, modeling_layoutlmv3.py:227,396-399,429,497, and the Dropout inside the five
    pair classifiers, peneo_decoder.py:253-271, which runs in pair_heads_fwd_kernel<..., DROP> and on the consumer waves of the
    fused pair backward).  Every mask is a pure function of (seed, element index), so the fp32 path (chunked decoder backward,
    two-kernel attention backward) and the default bf16 path see the same masks under the same seed counters: losses and every
    parameter gradient must agree to bf16 accuracy, and the loss must differ from the eval-mode one (dropout really on)."""
    from seeded import layoutlmv3_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    torch.manual_seed(20251003)      # (the dropout seed base is torch.initial_seed(): fixed, so that the run is the same every time)
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = build_model(pcfg)
    seeded_fill_(m.state_dict(), 11)
    batch = to_cuda(synthetic_rfund_batch(8, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=1008))
    m = m.eval()
    l_eval, _ = _fwd_bwd(m, batch, torch.bfloat16)
    m = m.train()
    l32, l16, stats = _grad_agreement(m, batch, seed_step=4000)
    assert abs(l32 - l_eval) > 1e-3 * abs(l_eval), (l32, l_eval)
    _assert_agreement(l32, l16, stats, 0.99, 0.03, loss_tol=3e-2)


def test_saved_pair_activations_keep_the_gradients():
    """Round 5: in a bf16 train step at D = 384 the decoder forward saves the classifiers' pre-activations (f16, dropout applied) for
    its backward (peneo_pair_heads_fwd_save / peneo_pair_bwd_saved) in buffers the decoder keeps between steps.  Every parameter
    gradient of a train-mode step agrees with the step whose backward rebuilds them (PENEO_PAIR_SAVE=0's data flow; same masks: the
    dropout is a function of (seed, element)), and a second step reuses the kept buffers with the same result.
    (reference: model/peneo_decoder.py:231-292 and its autograd graph)"""
    from seeded import layoutlmv3_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    from peneo_amd.model import engine
    torch.manual_seed(20251003)
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("base"))
    m = build_model(pcfg)
    seeded_fill_(m.state_dict(), 11)
    batch = to_cuda(synthetic_rfund_batch(2, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=1008))
    m = m.train()
    dec = m.peneo_decoder
    assert dec.save_pair_act
    l_on, g_on = _fwd_bwd(m, batch, torch.bfloat16, seed_step=4000)
    kept = {k: [b.data_ptr() for b in v] for k, v in engine._BIG_FREE.items() if k[0].startswith("pair_")}
    assert sorted(k[0] for k in kept) == ["pair_act", "pair_dz", "pair_x"] and all(len(v) == 1 for v in kept.values()), kept
    l_again, g_again = _fwd_bwd(m, batch, torch.bfloat16, seed_step=4000)
    assert {k: [b.data_ptr() for b in v] for k, v in engine._BIG_FREE.items() if k[0].startswith("pair_")} == kept      # the same three buffers
    m.eval()                                                   # leaving training mode hands them back (PEneoDecoder.train -> engine.big_clear)
    assert not any(k[0].startswith("pair_") for k in engine._BIG_FREE)
    m.train()
    dec.save_pair_act = False
    try:
        l_off, g_off = _fwd_bwd(m, batch, torch.bfloat16, seed_step=4000)
    finally:
        dec.save_pair_act = True
    assert abs(l_on - l_off) <= 1e-6 * abs(l_off) and l_again == l_on, (l_on, l_again, l_off)      # the forward is the same arithmetic per pair

    def close(stats, cos_min, tol):      # (gradients that are zero in exact arithmetic - the key biases - are rounding noise: skipped by norm)
        gmax = max(v[2] for v in stats.values())
        bad = {n: v for n, v in stats.items() if v[2] > 1e-4 * gmax and (v[0] < cos_min or abs(v[1] - 1) > tol)}
        assert not bad, sorted(bad.items(), key=lambda kv: kv[1][0])[:8]
    close(_grad_stats(g_on, g_off), 0.999, 1e-2)
    close(_grad_stats(g_again, g_on), 0.9999, 2e-3)       # (the same step again: equal up to the order of the fp32 atomics)


def test_lilt_base_bf16_path_matches_fp32_path():
    """BASELINE config 5 at full size: LiLT-base (12 layers, text H = 768 + layout H = 192, head dim 64 + 16 = 80 in ONE attention
    call, modeling_lilt.py:269-429), B = 8, S = 512, ragged masks: every parameter gradient of the bf16 path (head-dim-80
    single-pass attention backward, 16-byte head concat / split kernels, half-wave LayerNorms at H = 192, fused pair backward)
    against the fp32 path of the same model (which lilt_tiny.pt and the one-layer oracle test pin to the reference)."""
    from seeded import lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    pcfg = peneo_config("lilt-roberta-en-base", lilt_config("base"))
    m = build_model(pcfg)
    seeded_fill_(m.state_dict(), 13)
    m = m.eval()
    b = synthetic_rfund_batch(8, 512, 128, pcfg["backbone_config"]["vocab_size"], seed=1010, ragged=True)
    b.pop("image", None)
    l32, l16, stats = _grad_agreement(m, to_cuda(b))
    _assert_agreement(l32, l16, stats, 0.99, 0.03)


def test_large_full_depth_bf16_path_matches_fp32_path():
    """BASELINE config 4 at full depth: LayoutLMv3-large (24 layers, H = 1024, 16 heads), S = 1024, N = 1023, D = 512, B = 2.
    The CPU oracle is too slow at this depth (its one-layer slice is test_full_width_shapes_match_the_oracle); here the bf16
    path is held to the fp32 path of the same model."""
    from seeded import layoutlmv3_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    pcfg = peneo_config("layoutlmv3-base", layoutlmv3_config("large"))
    m = build_model(pcfg)
    seeded_fill_(m.state_dict(), 12)
    m = m.eval()
    batch = to_cuda(synthetic_rfund_batch(2, 1024, 256, pcfg["backbone_config"]["vocab_size"], seed=2004))
    l32, l16, stats = _grad_agreement(m, batch, repeat=False)
    _assert_agreement(l32, l16, stats, 0.99, 0.03)


@pytest.mark.parametrize("name", ["lmv3_tiny", "lilt_tiny"])
def test_train_mode_masks_are_the_same_function_in_both_precisions(name):
    """Train mode (every dropout site active, incl. the classifier dropout inside the pair kernels): all masks are pure
    functions of (seed, element index), so the fp32 path (chunked decoder backward, stand-alone dz kernel, two-kernel
    attention backward) and the bf16 path (fused kernels) of ONE model see the same masks when the seed counters are
    reset -- losses and gradients must then agree to bf16 accuracy, and differ clearly from the eval-mode ones."""
    from peneo_amd.model.engine import DropoutSeeds
    # (the seed base is torch.initial_seed(), random per process: with an unlucky one the train-mode loss of these tiny fixtures
    # lands within 1e-3 of the eval loss and the "dropout really was on" check below fails - about one run in twelve before this line)
    torch.manual_seed(20251003)
    fx = load_golden(name)
    b = to_cuda(fx["batch"])
    m = build_model(fx["config"], fx["state_dict"]).train()
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        m.set_compute_dtype(dt)
        DropoutSeeds._step, m._step = 1000, 1000
        for p in m.parameters():
            p.grad = None
        out = m(**b)
        out["loss"].backward()
        torch.cuda.synchronize()
        res[dt] = (float(out["loss"]), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    l32, l16 = res[torch.float32][0], res[torch.bfloat16][0]
    assert abs(l16 - l32) < 3e-2 * abs(l32), (l16, l32)
    assert abs(l32 - float(fx["outputs"]["loss"])) > 1e-3 * abs(l32)          # dropout really was on
    bad = []
    for n, g in res[torch.float32][1].items():
        a, r = res[torch.bfloat16][1][n].double().flatten(), g.double().flatten()
        if float(r.norm()) < 1e-7:
            continue
        cos = float(torch.dot(a, r) / (a.norm() * r.norm() + 1e-300))
        if cos < 0.97:
            bad.append((n, cos))
    assert not bad, bad


@pytest.mark.parametrize("name", ["lmv3_tiny", "lilt_tiny"])
def test_deferred_joins_do_not_change_the_gradients(name):
    """The side-stream joins deferred by one stage (engine.defer_join) against immediate joins: only the PLACE of a stream
    wait differs, so all gradients must agree to fp32 summation-order noise and most of them bit for bit (a clone of a bias
    gradient racing the side stream's column sums would show here)."""
    import peneo_amd.model.engine as E
    fx = load_golden(name)
    b = to_cuda(fx["batch"])
    m = build_model(fx["config"], fx["state_dict"], torch.bfloat16).eval()

    def run():
        for p in m.parameters():
            p.grad = None
        m(**b)["loss"].backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    a1 = run()
    E.DEFER_ALLOWED[0] = False
    try:
        c = run()
    finally:
        E.DEFER_ALLOWED[0] = True
    exact = 0
    for n in a1:
        # fp32 atomics (LayerNorm / embedding / column-sum reductions) reorder sums from launch to launch: last-bit noise.
        # A gradient cloned while the side stream is still adding to it would miss whole contributions (errors >> 1e-3)
        assert maxdiff(c[n], a1[n]) <= 2e-5 * float(a1[n].abs().max()) + 1e-9, n
        exact += int(torch.equal(c[n], a1[n]))
    assert exact > len(a1) // 2


def test_working_weights_follow_the_parameters():
    """The bf16 working copies (one multi-tensor cast for the encoder layers, lazy casts / packs elsewhere) are rebuilt when a
    parameter changes, through `.data` writes + epoch bump (FusedAdamW) as well as through versioned in-place ops (torch
    optimizers), and reused otherwise: outputs must equal those of a freshly built model with the same weights."""
    from peneo_amd.model.engine import bump_param_epoch
    fx = load_golden("lmv3_tiny")
    b = to_cuda(fx["batch"])
    m = build_model(fx["config"], fx["state_dict"], torch.bfloat16).eval()
    with torch.no_grad():
        l0 = float(m(**b)["loss"])
        assert float(m(**b)["loss"]) == l0                              # cached copies
        w = m.backbone.encoder.layer[1].intermediate.dense.weight
        w.mul_(1.5)                                                    # versioned in-place update
        l1 = float(m(**b)["loss"])
        w.data.mul_(1.0 / 1.5); w.data.mul_(1.25)                      # unversioned writes + the optimizer's epoch bump
        m.peneo_decoder.ent_linking_h2h_fc[0].weight.data.mul_(0.5)
        bump_param_epoch()
        l2 = float(m(**b)["loss"])
    ref = build_model(fx["config"], {k: v.clone() for k, v in m.state_dict().items()}, torch.bfloat16).eval()
    with torch.no_grad():
        l2_ref = float(ref(**b)["loss"])
    assert l1 != l0 and l2 != l1 and l2 == l2_ref, (l0, l1, l2, l2_ref)


def test_fused_adamw_training_steps_reduce_the_loss():
    """Three optimizer steps on one batch with the reference's parameter groups: the C-ABI update must invalidate the
    working-precision weight copies (loss changes and goes down)."""
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    fx = load_golden("lmv3_tiny")
    m = build_model(fx["config"], fx["state_dict"], torch.bfloat16).eval()   # eval: dropout off, deterministic
    b = to_cuda(fx["batch"])
    opt = FusedAdamW(peneo_param_groups(m, 2e-4, 0.01, fx["config"]["peneo_downstream_speedup_ratio"]))
    losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        out = m(**b)
        out["loss"].backward()
        losses.append(float(out["loss"].detach()))
        opt.step()
    assert losses[1] < losses[0] and losses[3] < losses[1], losses


@pytest.mark.parametrize("env", [{"PENEO_STAGE_CALLS": "0"}, {"PENEO_WGRAD_STREAM": "0"}, {"PENEO_STAGE_CALLS": "0", "PENEO_WGRAD_STREAM": "0"},
                                 {"PENEO_BWD_FUSED": "0", "PENEO_BWD_CHUNK_PAIRS": "300"},
                                 {"PENEO_BWD_FUSED": "0", "PENEO_DZ_FUSED": "0"}, {"PENEO_DEFER_JOIN": "0", "PENEO_DW1_HOLD": "0"},
                                 {"PENEO_DW1_SIDE": "0"}])
def test_optional_execution_modes_keep_the_gradients(env):
    """The remaining stream / chunking options (weight gradients on the main stream, the chunked decoder backward with and
    without the fused dz kernel, immediate joins, dW1 on the main stream) are read at construction time: run the bf16
    gradient check of the tiny golden in a subprocess per setting."""
    import os, subprocess, sys
    code = """
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from conftest import load_golden
from peneo_amd.model import PEneoConfig, PEneoModel
fx = load_golden("lmv3_tiny")
m = PEneoModel(PEneoConfig(**{k: v for k, v in fx["config"].items() if k != "model_type"}))
m.load_state_dict(fx["state_dict"], strict=True)
m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in fx["batch"].items()}
out = m(**b); out["loss"].backward()
assert abs(float(out["loss"]) - float(fx["outputs"]["loss"])) < 2e-2 * float(fx["outputs"]["loss"])
bad = []
for n, p in m.named_parameters():
    g = fx["grads"].get(n)
    if g is None or float(g.norm()) < 1e-6: continue
    a, r = p.grad.float().cpu().flatten(), g.flatten()
    cos = float(torch.dot(a, r) / (a.norm() * r.norm() + 1e-12))
    if cos < 0.98: bad.append((n, cos))
assert not bad, bad
print("ok")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("chunks", ["1", "many"])
def test_flat_grad_data_parallel_over_rccl_world_of_one(chunks):
    """The data-parallel wrapper on the real backend (RCCL) with a single rank: gradients pass through the bf16 wire buffer
    and the all-reduce unchanged up to bf16 rounding, on three consecutive steps.  chunks = many (the default mode, with
    a chunk size that cuts the tiny model into several): step 1 learns the arrival order, steps 2 and 3 put chunks on the
    wire DURING the backward; the layout must end with the embedding stage and the held dW1 weights, and no gradient that
    arrives late (rel-pos tables, patch embedding, embedding LayerNorms; dW1 completes at the end of the backward) may be lost."""
    import os, subprocess, sys
    code = """
import os, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29571")
import torch.distributed as dist
from conftest import load_golden
from peneo_amd.model import PEneoConfig, PEneoModel
from peneo_amd.parallel import wrap_data_parallel, FlatGradDataParallel
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
fx = load_golden("lmv3_tiny")
m = PEneoModel(PEneoConfig(**{k: v for k, v in fx["config"].items() if k != "model_type"}))
m.load_state_dict(fx["state_dict"], strict=True)
m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in fx["batch"].items()}
def grads(net):
    for p in m.parameters(): p.grad = None
    out = net(**b); out["loss"].backward()
    torch.cuda.synchronize()
    return {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}
ref = grads(m)
net = wrap_data_parallel(m, device_ids=[0])
assert isinstance(net, FlatGradDataParallel) and net.flat.dtype == torch.bfloat16
for step in range(3):
    got = grads(net)
    assert set(got) == set(ref)
    for n in ref:
        err = float((got[n] - ref[n]).abs().max() / ref[n].abs().max().clamp_min(1e-12))
        assert err < 1e-2, (step, n, err)
        assert float(ref[n].abs().max()) == 0 or float(got[n].abs().max()) > 0, n
assert net.sync_calls == 3, net.sync_calls        # armed from the PEneoOutput fields, once per backward
if os.environ.get("PENEO_DP_CHUNKS") != "1":
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    order = [names[i] for i in net.order]
    assert len(net.chunks) >= 3, [len(c[0]) for c in net.chunks]
    assert net.early_calls == 2 * (len(net.chunks) - 1), (net.early_calls, len(net.chunks))
    first_layer = min(i for i, n in enumerate(order) if ".encoder.layer." in n)
    last_layer = max(i for i, n in enumerate(order) if ".encoder.layer." in n)
    dec_early = [i for i, n in enumerate(order) if "peneo_decoder" in n and not n.endswith("_fc.0.weight")]
    late = [i for i, n in enumerate(order) if n.endswith("_fc.0.weight")]
    emb = [i for i, n in enumerate(order) if "embeddings" in n or "rel_pos" in n or "patch_embed" in n]
    assert max(dec_early) < first_layer and min(emb) > last_layer and min(late) > max(emb), order
    lay = [int(n.split(".encoder.layer.")[1].split(".")[0]) for n in order if ".encoder.layer." in n]
    assert lay == sorted(lay, reverse=True), lay            # layers in the order the backward visits them
with net.no_sync():
    got = grads(net)
assert net.sync_calls == 3
assert all(float((got[n] - ref[n]).abs().max() / ref[n].abs().max().clamp_min(1e-12)) < 5e-4 for n in ref)   # no wire round trip (fp32 atomics reorder sums)
dist.destroy_process_group()
print("ok")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PENEO_DP_CHUNKS="1") if chunks == "1" else dict(os.environ, PENEO_DP_CHUNK_MB="0.03")
    env.pop("PENEO_DP_CHUNKS", None) if chunks != "1" else None
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_flat_grad_data_parallel_layout_learned_while_the_dw1_gemm_could_not_be_held():
    """The layout-learning step runs with PRE-EXISTING .grad tensors (zero_grad(set_to_none=False)): the decoder cannot hold
    its dW1 GEMM then, so the five *_fc.0.weight gradients arrive early and the learned layout puts them in an EARLY chunk.
    Later steps start from .grad = None, the GEMM is held on the side stream until the end of the backward -- the early pack
    of that chunk must join the held work before it reads the gradients (decided per launch, parallel.py:_pack), and the
    gradients on the wire must equal the un-wrapped ones on every step."""
    import os, subprocess, sys
    code = """
import os, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29573")
import torch.distributed as dist
from conftest import load_golden
from peneo_amd import parallel
from peneo_amd.model import PEneoConfig, PEneoModel, engine
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
fx = load_golden("lmv3_tiny")
m = PEneoModel(PEneoConfig(**{k: v for k, v in fx["config"].items() if k != "model_type"}))
m.load_state_dict(fx["state_dict"], strict=True)
m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
b = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in fx["batch"].items()}
def grads(net, keep_grads=False):
    for p in m.parameters():
        if keep_grads and p.grad is not None: p.grad.zero_()
        else: p.grad = None
    out = net(**b); out["loss"].backward()
    torch.cuda.synchronize()
    return {n: p.grad.float().clone() for n, p in m.named_parameters() if p.grad is not None}
ref = grads(m)
assert not any(engine.is_late(p) for p in m.parameters()) or True
engine._LATE.clear()                                  # as in a process whose first backward is the wrapped one
net = parallel.wrap_data_parallel(m, device_ids=[0])
calls = []
orig = parallel._join_side_streams
def spy(held=True):
    calls.append(held); orig(held=held)
parallel._join_side_streams = spy
got = grads(net, keep_grads=True)                     # learning step: every .grad exists -> nothing deferred, nothing late
names = [n for n, p in m.named_parameters() if p.requires_grad]
w1 = [i for i, n in enumerate(names) if n.endswith("_fc.0.weight")]
assert len(w1) == 5 and len(net.chunks) >= 3
assert not any(engine.is_late(net.params[i]) for i in w1)
early_w1 = [i for i in w1 if net._chunk_of[i] < len(net.chunks) - 1]
assert early_w1, "the layout learned without a held GEMM should carry dW1 in an early chunk"
for step in range(2):
    calls.clear()
    got = grads(net)                                  # .grad is None: the dW1 GEMM is held now
    assert all(engine.is_late(net.params[i]) for i in w1)
    c_w1 = sorted({net._chunk_of[i] for i in early_w1})
    assert all(calls[c] for c in c_w1), (calls, c_w1)  # the chunk with the late gradients joined the held work
    for n in ref:
        err = float((got[n] - ref[n]).abs().max() / ref[n].abs().max().clamp_min(1e-12))
        assert err < 1e-2, (step, n, err)
dist.destroy_process_group()
print("ok")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PENEO_DP_CHUNK_MB="0.03"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_data_parallel_two_processes_on_one_gpu_match_a_single_process(tmp_path):
    """Two FRESH child processes (gloo, both on GPU 0) run the real tiny PEneoModel (bf16 HIP path) behind the flat
    data-parallel wrapper on their shards of a 4-document batch for three steps; the averaged gradients every rank ends up
    with must equal the mean of the two shards' gradients computed by ONE process without any wrapper
    (reference: torchrun + DDP, README.md:206-218)."""
    import os, subprocess, sys
    root, here = os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))
    child = """
import os, sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from conftest import load_golden
from peneo_amd.model import PEneoConfig, PEneoModel
from peneo_amd.parallel import init_distributed, shard_documents, wrap_data_parallel
from peneo_amd.data import synthetic_rfund_batch
rank, local, world = init_distributed()
torch.cuda.set_device(local)
fx = load_golden("lmv3_tiny")
m = PEneoModel(PEneoConfig(**{k: v for k, v in fx["config"].items() if k != "model_type"}))
m.load_state_dict(fx["state_dict"], strict=True)
m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
full = synthetic_rfund_batch(4, 40, 8, fx["config"]["backbone_config"]["vocab_size"], seed=11, ragged=True)
def shard(r, w):
    idx = list(shard_documents(4, r, w))
    return {k: v[idx].cuda() for k, v in full.items()}
if world == 1:                                   # the single-process reference: mean of the shards' gradients
    acc = {}
    for r in range(2):
        for p in m.parameters(): p.grad = None
        m(**shard(r, 2))["loss"].backward()
        for n, p in m.named_parameters():
            acc[n] = acc.get(n, 0) + p.grad.float() / 2
    torch.save({n: g.cpu() for n, g in acc.items()}, sys.argv[1])
else:
    net = wrap_data_parallel(m, device_ids=[local])
    for step in range(3):
        for p in m.parameters(): p.grad = None
        net(**shard(rank, world))["loss"].backward()
    torch.cuda.synchronize()
    torch.save({"grads": {n: p.grad.float().cpu() for n, p in m.named_parameters()}, "chunks": len(net.chunks),
                "early": net.early_calls}, sys.argv[1] + str(rank))
    torch.distributed.destroy_process_group()
print("ok")
""" % (root, here)
    script = tmp_path / "child.py"
    script.write_text(child)
    base = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29583", PENEO_DIST_BACKEND="gloo", PENEO_DEVICE="0",
                GPU_MAX_HW_QUEUES="8", PENEO_DP_CHUNK_MB="0.05")
    ref_file, out = str(tmp_path / "ref.pt"), str(tmp_path / "rank")
    r = subprocess.run([sys.executable, str(script), ref_file], env=dict(base, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    procs = [subprocess.Popen([sys.executable, str(script), out], env=dict(base, WORLD_SIZE="2", RANK=str(k), LOCAL_RANK=str(k)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k in range(2)]
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    ref = torch.load(ref_file)
    for k in range(2):
        got = torch.load(out + str(k))
        assert got["chunks"] >= 2 and got["early"] >= 2, (got["chunks"], got["early"])
        for n, g in ref.items():
            err = float((got["grads"][n] - g).abs().max() / g.abs().max().clamp_min(1e-12))
            assert err < 5e-3, (k, n, err)      # fp32 wire on gloo: only the side-stream / atomic summation order differs


def test_bench_starts_its_own_ranks(tmp_path):
    """BASELINE config 3's launch path on ONE GPU: `python bench.py --gpus 2` with no launcher in the environment must start
    two fresh rank processes itself (torch.distributed.run children; here both on GPU 0 over gloo), reduce the gradients over
    a process group of two ranks and say so in its line (reference: torchrun --nproc_per_node N, README.md:206-218)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PENEO_DIST_BACKEND="gloo", PENEO_DEVICE="0", GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2",
                        "--docs-per-gpu", "2", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                    # rank 0 prints ONE line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["dist_backend"] == "gloo", rec
    assert rec["config"]["parallelism"] == "dp2" and rec["value"] > 0
    # and a world that is not what --gpus says is an error, not a relabelled single-GPU run
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1"],
                        env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert r2.returncode != 0 and not [l for l in r2.stdout.splitlines() if l.startswith("{")]


def test_bench_plain_run_is_lean_dumps_its_outputs_and_full_adds_the_side_measurements(tmp_path):
    """`bench.py` without --full times exactly --steps steps and prints the headline line only; --dump-outputs writes the last
    timed step's losses and sampled gradients (same inputs on every run: two runs agree up to summation order); --full brings
    back every side measurement."""
    import json, os, subprocess, sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--docs-per-gpu", "2", *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])

    side = ("roofline", "roofline_pair_heads_fwd", "forward_only", "indices_agree", "indices_agree_trained", "ragged",
            "embed_bwd", "with_weight_recast", "optimizer_step_ms", "cpu_baseline")
    dumps = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        rec = run("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "docs/s", rec
        assert rec["higher_is_better"] is True and rec["dtype"] == "bf16" and not any(s in rec for s in side), rec
        files = sorted(os.listdir(d))
        assert "loss.npy" in files and sum(f.startswith("grad.") for f in files) > 100, files
        arrs = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert abs(float(arrs["loss.npy"]) - rec["config"]["final_loss"]) < 1e-4
        dumps.append(arrs)
    a, b = dumps
    assert sorted(a) == sorted(b) and all(a[f].shape == b[f].shape for f in a)
    assert abs(float(a["loss.npy"]) - float(b["loss.npy"])) < 1e-3 * max(1.0, abs(float(b["loss.npy"])))
    ga = np.concatenate([a[f].ravel() for f in sorted(a) if f.startswith("grad.")]).astype(np.float64)
    gb = np.concatenate([b[f].ravel() for f in sorted(b) if f.startswith("grad.")]).astype(np.float64)
    assert np.linalg.norm(ga - gb) <= 2e-2 * np.linalg.norm(gb)

    rec = run("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert all(s in rec for s in side), sorted(rec)
    assert rec["forward_only"]["ms_per_batch"] > 0 and rec["ragged"]["ms_per_step"] > 0 and rec["roofline"]["launches"] >= 2


def test_fused_adamw_resumes_from_state_dict_and_from_torch_adamw():
    """state_dict() carries torch.optim.AdamW's layout (per-parameter `step`, exp_avg, exp_avg_sq): 3 steps + save + load
    into a fresh optimizer + 3 steps == 6 uninterrupted steps of torch.optim.AdamW; a torch AdamW checkpoint (the
    reference's optimizer.pt) resumes too; load_state_dict() after a step() re-points the device table at the loaded moments."""
    from peneo_amd.optim import FusedAdamW

    def make():
        torch.manual_seed(3)
        return [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in [(70, 33), (70,), (5001, 70), (3,)]]

    gen = torch.Generator().manual_seed(4)
    grads = [[torch.randn(s, generator=gen).cuda() for s in [(70, 33), (70,), (5001, 70), (3,)]] for _ in range(6)]

    def run(opt, ps, steps):
        for k in steps:
            for p, g in zip(ps, grads[k]):
                p.grad = g.clone()
            opt.step()

    kw = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
    pr = make(); ref = torch.optim.AdamW(pr, **kw); run(ref, pr, range(6))
    # (a) fused -> state_dict -> fresh fused
    pa = make(); oa = FusedAdamW(pa, **kw); run(oa, pa, range(3))
    sd = oa.state_dict()
    assert all(float(st["step"]) == 3.0 for st in sd["state"].values()) and len(sd["state"]) == 4
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = FusedAdamW(pb, **kw); ob.load_state_dict(sd); run(ob, pb, range(3, 6))
    for a, r in zip(pb, pr):
        assert maxdiff(a, r) <= 2e-6 * float(r.abs().max()) + 1e-7
    assert all(float(st["step"]) == 6.0 for st in ob.state_dict()["state"].values())
    # (b) torch AdamW checkpoint -> fused
    import copy
    pt = make(); ot = torch.optim.AdamW(pt, **kw); run(ot, pt, range(3))
    ckpt = copy.deepcopy(ot.state_dict())            # load_state_dict() aliases same-dtype tensors: keep a pristine copy
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    oc = FusedAdamW(pc, **kw); oc.load_state_dict(copy.deepcopy(ckpt)); run(oc, pc, range(3, 6))
    for a, r in zip(pc, pr):
        assert maxdiff(a, r) <= 2e-6 * float(r.abs().max()) + 1e-7
    # (c) load_state_dict AFTER the first step of the same object: the loaded moments are the ones that get updated
    pd = make(); od = FusedAdamW(pd, **kw); run(od, pd, [5])           # some unrelated step first
    with torch.no_grad():
        for p, src in zip(pd, pt):
            p.copy_(src)
    od.load_state_dict(copy.deepcopy(ckpt)); run(od, pd, range(3, 6))
    for a, r in zip(pd, pr):
        assert maxdiff(a, r) <= 2e-6 * float(r.abs().max()) + 1e-7
    assert maxdiff(od.state_dict()["state"][0]["exp_avg"], ref.state_dict()["state"][0]["exp_avg"]) < 1e-6
    # (d) a parameter that gets its first gradient later starts its own bias correction at step 1
    pe = make(); oe = FusedAdamW(pe, **kw)
    pf = make(); of = torch.optim.AdamW(pf, **kw)
    for k in range(4):
        for j, (p, q, g) in enumerate(zip(pe, pf, grads[k])):
            if j == 3 and k < 2:
                p.grad = q.grad = None
            else:
                p.grad, q.grad = g.clone(), g.clone()
        oe.step(); of.step()
    for a, r in zip(pe, pf):
        assert maxdiff(a, r) <= 2e-6 * float(r.abs().max()) + 1e-7


def test_per_head_losses_are_differentiable_and_logits_are_not():
    """The five *_loss fields are ordinary differentiable outputs in the reference (peneo_decoder.py:375-428): backward from
    one of them, or from a re-weighted sum, must give the matching gradients; the logit maps carry no grad_fn."""
    fx = load_golden("lmv3_tiny")
    m = build_model(fx["config"], fx["state_dict"]).eval()
    b = to_cuda(fx["batch"])
    out = m(**b)
    for h in HEADS:
        assert not out[h + "_shaking_outputs"].requires_grad, h
    names = [n for n, p in m.named_parameters() if p.requires_grad]

    def grads_of(loss):
        for p in m.parameters():
            p.grad = None
        loss.backward()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    g_total = grads_of(out["loss"])                                   # ratios are all 1 in the fixture
    out = m(**b)
    g_sum = grads_of(sum(out[h + "_loss"] for h in HEADS))
    for n in g_total:
        assert maxdiff(g_sum[n], g_total[n]) <= 2e-4 * float(g_total[n].abs().max()) + 1e-7, n
    out = m(**b)
    g_le = grads_of(out["line_extraction_loss"])
    out = m(**b)
    g_rest = grads_of(sum(out[h + "_loss"] for h in HEADS[1:]))
    w = "peneo_decoder.line_extraction_fc.0.weight"
    assert float(g_le[w].abs().max()) > 0 and float(g_rest[w].abs().max()) == 0
    for n in g_total:
        tot = g_le[n] + g_rest[n]
        assert maxdiff(tot, g_total[n]) <= 2e-4 * float(g_total[n].abs().max()) + 1e-7, n
    out = m(**b)
    g_mix = grads_of(0.5 * out["loss"] + 2.0 * out["ent_linking_t2t_loss"])
    out = m(**b)
    g_elt = grads_of(out["ent_linking_t2t_loss"])
    for n in g_total:
        want = 0.5 * g_total[n] + 2.0 * g_elt[n]
        assert maxdiff(g_mix[n], want) <= 2e-4 * float(want.abs().max()) + 1e-7, n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ohem_model_matches_reference(dtype):
    """peneo_ohem_num_positive / _negative != -1: the five losses and every parameter gradient of the
    tiny LayoutLMv3 model against the real reference run with the same setting (tests/golden/ohem.pt)."""
    fx = load_golden("ohem")["model"]
    base = load_golden(fx["base_fixture"])
    m = build_model(fx["config"], base["state_dict"], dtype).eval()
    out = m(**to_cuda(base["batch"]))
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    for k, v in fx["losses"].items():
        assert abs(float(out[k]) - float(v)) <= tol * max(1.0, abs(float(v))), (k, float(out[k]), float(v))
    out["loss"].backward()
    bad = []
    for n, p in m.named_parameters():
        g = fx["grads"].get(n)
        if g is None or float(g.abs().max()) < 1e-7:
            continue
        assert p.grad is not None, n
        if dtype == torch.float32:
            assert maxdiff(p.grad, g) <= 2e-3 * float(g.abs().max()) + 1e-6, n
        else:
            # bf16 logits reorder near-equal losses, and the kept set (3 + 60 of 1560 pairs here) is a discrete function of
            # that order: the gradient is that of a slightly different subset, so only direction and finiteness are checked
            assert torch.isfinite(p.grad).all(), n
            a, r = p.grad.float().cpu().flatten(), g.flatten()
            cos = float(torch.dot(a, r) / (a.norm() * r.norm() + 1e-12))
            if cos < 0.6:
                bad.append((n, cos))
    assert not bad, bad


def test_decode_from_device_logits_matches_reference():
    """SURVEY §8f rank 1 end to end: device logits -> peneo_spots_compact (one launch + one copy per score map) -> host graph
    walk -> the reference's kv pairs, lines and link dictionaries (tests/golden/decode.pt, produced by pipeline/decode.py)."""
    from peneo_amd.model import HandshakingTaggingScheme
    from peneo_amd.pipeline import sample_decode_peneo
    fx = load_golden("decode")
    T = HandshakingTaggingScheme()
    for d in fx["docs"]:
        for kw, key in ((dict(bbox=d["bbox"]), "pred"), (dict(score_thresh=0.6), "pred_thr")):
            got = sample_decode_peneo(T, d["text"], *[l.cuda() for l in d["logits"]], seq_len=d["n"], **kw)
            want = d[key]
            assert [kv[:2] for kv in got[0]] == [kv[:2] for kv in want[0]]
            if "bbox" in kw:
                assert [list(kv[2]) + list(kv[3]) for kv in got[0]] == [list(kv[2]) + list(kv[3]) for kv in want[0]]
            assert [l[0] if isinstance(l, tuple) else l for l in got[1]] == [l[0] if isinstance(l, tuple) else l for l in want[1]]
            for a, b in zip(got[2:], want[2:]):
                assert dict(a) == dict(b)
        got = sample_decode_peneo(T, d["text"], *[t.cuda() for t in d["tags"]], bbox=d["bbox"], seq_len=d["n"], decode_gt=True)
        assert [kv[:2] for kv in got[0]] == [kv[:2] for kv in d["gt"][0]] and dict(got[2]) == dict(d["gt"][2])
