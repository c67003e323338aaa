"""LiLT training on the two-stream attention (ops.attn2_fwd with dropout + ops.attn2_bwd, PENEO_LILT_ATTN2_TRAIN=1): the train step
gives what the concat path gives, the copies are gone, and without the switch - or at widths the kernels do not hold - nothing changes."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
COUNTED = ("attn2_fwd", "attn2_bwd", "head_concat", "head_split", "attn_fwd", "attn_bwd")


def _cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _model(pcfg, state_dict=None, dtype=torch.bfloat16):
    from peneo_amd.model import PEneoConfig, PEneoModel
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    if state_dict is not None:
        m.load_state_dict(state_dict, strict=True)
    return m.cuda().set_compute_dtype(dtype)


@pytest.fixture(scope="module")
def base():
    """LiLT-base widths (head dims 64 + 16), two layers, B = 2, S = 96, the second document's last 30 tokens masked
    (tests/test_gpu_attn2_model.py's fixture)."""
    from seeded import lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    bcfg = dict(lilt_config("base"), num_hidden_layers=2, vocab_size=1000)
    m = _model(peneo_config("lilt-roberta-en-base", bcfg))
    seeded_fill_(m.state_dict(), 17)
    batch = synthetic_rfund_batch(2, 96, 24, bcfg["vocab_size"], seed=9, with_image=False)
    batch["input_ids"][1, 66:] = bcfg["pad_token_id"]
    batch["attention_mask"][1, 66:] = 0
    batch["bbox"][1, 66:] = 0
    return m, _cuda(batch)


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the attention ops"""
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


def test_train_step_with_the_switch_equals_the_concat_path(base, calls, monkeypatch):
    m, batch = base
    layers = 2
    monkeypatch.delenv("PENEO_LILT_ATTN2_TRAIN", raising=False)
    loss0, g0 = _train_step(m, batch)
    assert calls["attn2_bwd"] == 0 and calls["attn2_fwd"] == 0            # switch unset: the concat path
    assert calls["attn_bwd"] == layers and calls["head_concat"] == 3 * layers and calls["head_split"] == 3 * layers
    loss1, g1 = _train_step(m, batch)
    for k in calls:
        calls[k] = 0
    monkeypatch.setenv("PENEO_LILT_ATTN2_TRAIN", "1")
    loss2, g2 = _train_step(m, batch)
    assert calls["attn2_fwd"] == layers and calls["attn2_bwd"] == layers   # once per layer
    assert calls["head_concat"] == 0 and calls["head_split"] == 0 and calls["attn_bwd"] == 0 and calls["attn_fwd"] == 0
    assert torch.isfinite(loss2) and len(g2) > 50 and g2.keys() == g0.keys()
    repeatable = torch.equal(loss0, loss1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    print(f"off-runs repeat bit for bit: {repeatable}; loss off {float(loss0):.6f} on {float(loss2):.6f}")
    if repeatable:
        # the kernels are bit-identical to the concat path (tests/test_gpu_attn2_bwd.py), so is the step
        assert torch.equal(loss2, loss0)
        for n in g0:
            assert torch.equal(g2[n], g0[n]), n
    else:
        # (the step has fp32 atomics elsewhere) README's bf16 bar
        assert abs(float(loss2) - float(loss0)) <= 1e-3 * abs(float(loss0))
        for n in g0:
            assert torch.isfinite(g2[n]).all(), n
            a, b = g2[n].double().flatten(), g0[n].double().flatten()
            if float(b.norm()) == 0.0:
                assert float(a.norm()) == 0.0, n
                continue
            cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
            assert cos >= 0.995, (n, cos)


def test_tiny_widths_keep_the_concat_path_with_the_switch_on(calls, monkeypatch):
    monkeypatch.setenv("PENEO_LILT_ATTN2_TRAIN", "1")
    fx = load_golden("lilt_tiny")                    # head dims 48 + 12: not a pair peneo_attn2_supported takes
    m = _model(fx["config"], fx["state_dict"])
    _, grads = _train_step(m, _cuda(fx["batch"]))
    assert calls["attn2_fwd"] == 0 and calls["attn2_bwd"] == 0 and calls["attn_bwd"] > 0
    assert len(grads) > 20 and all(torch.isfinite(g).all() for g in grads.values())


def test_fp32_keeps_the_concat_path_with_the_switch_on(base, calls, monkeypatch):
    monkeypatch.setenv("PENEO_LILT_ATTN2_TRAIN", "1")
    m, batch = base
    m.set_compute_dtype(torch.float32)
    try:
        _, grads = _train_step(m, batch)
    finally:
        m.set_compute_dtype(torch.bfloat16)
    assert calls["attn2_fwd"] == 0 and calls["attn2_bwd"] == 0 and calls["attn_bwd"] > 0
    assert len(grads) > 50 and all(torch.isfinite(g).all() for g in grads.values())
