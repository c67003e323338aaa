"""Deterministic mode, whole training iterations: under peneo_amd.deterministic(2) forward + backward + FusedAdamW.step()
with clip, run twice from identical state, give the same bits (losses, every gradient, every parameter, both moments) and take no
order-dependent accumulation path; the gradients agree with the default path's at the bar tests/test_gpu_model.py::_grad_agreement
sets for "the same step up to summation order"; what the mode does not cover raises ValueError under mode 2 and runs under mode 1;
leaving the context restores the default path."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _build(pcfg, state_dict=None, dtype=torch.bfloat16):
    from peneo_amd.model import PEneoConfig, PEneoModel
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    if state_dict is not None:
        m.load_state_dict(state_dict, strict=True)
    return m.cuda().set_compute_dtype(dtype)


def _case(name):
    """(model, batch): the two tiny fixtures (weights and batch from tests/golden), and base-width cases - H = 768, D = 384, two
    layers, B = 2, S = 128, a synthetic batch with the second document's tail masked."""
    from seeded import layoutlmv3_config, lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    if name in ("lmv3_tiny", "lilt_tiny"):
        fx = load_golden(name)
        return _build(fx["config"], fx["state_dict"]), _cuda(fx["batch"])
    lilt = name == "lilt_base2"
    bcfg = dict((lilt_config if lilt else layoutlmv3_config)("base"), num_hidden_layers=2, vocab_size=1000)
    m = _build(peneo_config("lilt-roberta-en-base" if lilt else "layoutlmv3-base", bcfg))
    seeded_fill_(m.state_dict(), 17)
    batch = synthetic_rfund_batch(2, 128, 32, bcfg["vocab_size"], seed=9, with_image=not lilt)
    batch["input_ids"][1, 100:] = bcfg["pad_token_id"]
    batch["attention_mask"][1, 100:] = 0
    batch["bbox"][1, 100:] = 0
    return m, _cuda(batch)


def _iteration(m, batch, state0, emit=False):
    """One training iteration from identical state: parameters from `state0`, a fresh FusedAdamW (zero moments, step 1) with clip,
    the dropout seed counters reset (every mask is a function of (seed, element)), train mode with every dropout site on.
    -> (loss, {gradients}, {parameters after the step}, {exp_avg}, {exp_avg_sq}, order-dependent launches it made)"""
    from peneo_amd import hip
    from peneo_amd.model.engine import DropoutSeeds
    from peneo_amd.optim import FusedAdamW, peneo_param_groups
    m.load_state_dict(state0, strict=True)
    opt = FusedAdamW(peneo_param_groups(m, 2e-3, 0.01, 30.0), max_grad_norm=1.0, emit_into=m if emit else None)
    DropoutSeeds._step, m._step = 40, 40
    m.train()
    try:
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        c0 = hip.order_dependent_launches()
        out = m(**batch)
        out["loss"].backward()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
        moved = hip.order_dependent_launches() - c0
        named = dict(m.named_parameters())
        params = {n: p.detach().clone() for n, p in named.items()}
        m1 = {n: opt.state[p]["exp_avg"].clone() for n, p in named.items() if p in opt.state and "exp_avg" in opt.state[p]}
        m2 = {n: opt.state[p]["exp_avg_sq"].clone() for n, p in named.items() if p in opt.state and "exp_avg_sq" in opt.state[p]}
        assert len(grads) > 20 and m1.keys() == grads.keys() == m2.keys()
        return out["loss"].detach().clone(), grads, params, m1, m2, moved
    finally:
        m.eval()
        m.zero_grad(set_to_none=True)


def _unequal(a, b):
    return sorted(n for n in a if not torch.equal(a[n], b[n]))


def _moved(got, ref):
    """tests/test_gpu_model.py::_grad_agreement's repeat leg: gradients above 1e-6 of the largest norm whose cosine is below
    1 - 1e-5 or whose norm is off by more than 1e-3"""
    stats = {}
    for n, g in ref.items():
        a, r = got[n].double().flatten(), g.double().flatten()
        stats[n] = (float(torch.dot(a, r) / (a.norm() * r.norm() + 1e-300)), float(a.norm() / (r.norm() + 1e-300)), float(r.norm()))
    gmax = max(v[2] for v in stats.values())
    worst = min((v[0], n) for n, v in stats.items() if v[2] > 1e-6 * gmax)
    print(f"worst cosine {worst[0]:.9f} ({worst[1]}), largest norm deviation "
          f"{max(abs(v[1] - 1) for v in stats.values() if v[2] > 1e-6 * gmax):.3e}")
    return {n: v[:2] for n, v in stats.items() if v[2] > 1e-6 * gmax and (v[0] < 1 - 1e-5 or abs(v[1] - 1) > 1e-3)}


CASES = [("lmv3_tiny", {}), ("lilt_tiny", {}), ("lilt_tiny", {"attn2": True}), ("lmv3_base2", {}), ("lmv3_base2", {"mxfp8": True}),
         ("lilt_base2", {"attn2": True}), ("lmv3_tiny", {"emit": True})]


@pytest.mark.parametrize("name,opts", CASES, ids=[n + "".join("-" + k for k in o) for n, o in CASES])
def test_training_iteration_is_bit_reproducible_and_takes_no_order_dependent_path(name, opts, monkeypatch):
    import peneo_amd
    from peneo_amd import hip
    if opts.get("attn2"):
        monkeypatch.setenv("PENEO_LILT_ATTN2_TRAIN", "1")        # the two-stream LiLT attention (taken at the widths it holds)
    else:
        monkeypatch.delenv("PENEO_LILT_ATTN2_TRAIN", raising=False)
    m, batch = _case(name)
    if opts.get("mxfp8"):
        m.set_pair_heads_train_format("mxfp8")
    emit = bool(opts.get("emit"))
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    before = hip.deterministic_mode()
    loss0, g0, p0, _, _, moved0 = _iteration(m, batch, state0, emit)                  # the default path
    assert moved0 > 0, "the default step took no order-dependent path: the counter proves nothing"
    with peneo_amd.deterministic(2):
        la, ga, pa, m1a, m2a, moved_a = _iteration(m, batch, state0, emit)
        lb, gb, pb, m1b, m2b, moved_b = _iteration(m, batch, state0, emit)
    assert moved_a == 0 and moved_b == 0, (moved_a, moved_b)
    assert torch.equal(la, lb), (float(la), float(lb))
    assert not _unequal(ga, gb), _unequal(ga, gb)[:8]
    assert not _unequal(pa, pb), _unequal(pa, pb)[:8]
    assert not _unequal(m1a, m1b) and not _unequal(m2a, m2b)
    assert torch.isfinite(la) and abs(float(la) - float(loss0)) <= 1e-6 * abs(float(loss0)) + 1e-7, (float(la), float(loss0))
    moved = _moved(ga, g0)                                                            # against the default path's gradients
    assert not moved, sorted(moved.items(), key=lambda kv: kv[1][0])[:12]
    # leaving the context: the default path again, the same gradients as before entering
    assert hip.deterministic_mode() == before
    loss1, g1, _, _, _, moved1 = _iteration(m, batch, state0, emit)
    assert moved1 > 0
    back = _moved(g1, g0)
    assert not back, sorted(back.items(), key=lambda kv: kv[1][0])[:12]


@pytest.mark.parametrize("what,match", [("fp32", "fp32 compute"), ("cls3", "3-layer classifier"), ("ohem", "OHEM")])
def test_strict_mode_names_what_it_does_not_cover_and_mode_1_runs_it(what, match):
    import peneo_amd
    from peneo_amd import hip
    if what == "ohem":
        fx = load_golden("ohem")["model"]
        base = load_golden(fx["base_fixture"])
        m, batch = _build(fx["config"], base["state_dict"]), _cuda(base["batch"])
    else:
        fx = load_golden("lmv3_tiny_cls3" if what == "cls3" else "lmv3_tiny")
        m, batch = _build(fx["config"], fx["state_dict"], torch.float32 if what == "fp32" else torch.bfloat16), _cuda(fx["batch"])
    m.eval()
    with peneo_amd.deterministic(2):
        with pytest.raises(ValueError, match=match):
            m(**batch)["loss"].backward()
    m.zero_grad(set_to_none=True)
    with peneo_amd.deterministic(1):
        c0 = hip.order_dependent_launches()
        out = m(**batch)
        out["loss"].backward()
        torch.cuda.synchronize()
        assert hip.order_dependent_launches() > c0                 # it ran, and was counted
    assert torch.isfinite(out["loss"])
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
