"""LiLT on the two-stream attention forward (ops.attn2_fwd): forwards without autograd take it by default and give exactly what the
concat path gives (PENEO_LILT_ATTN2=0); every other forward - with autograd, at widths the kernel does not hold - is untouched."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
HEADS = ("line_extraction", "ent_linking_h2h", "ent_linking_t2t", "line_grouping_h2h", "line_grouping_t2t")


def _cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _model(pcfg, state_dict=None):
    from peneo_amd.model import PEneoConfig, PEneoModel
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    if state_dict is not None:
        m.load_state_dict(state_dict, strict=True)
    return m.cuda().set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module")
def base():
    """LiLT-base widths (head dims 64 + 16), two layers, B = 2, S = 96, the second document's last 30 tokens masked."""
    from seeded import lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    bcfg = dict(lilt_config("base"), num_hidden_layers=2, vocab_size=1000)
    m = _model(peneo_config("lilt-roberta-en-base", bcfg))
    seeded_fill_(m.state_dict(), 17)
    batch = synthetic_rfund_batch(2, 96, 24, bcfg["vocab_size"], seed=9, with_image=False)
    batch["input_ids"][1, 66:] = bcfg["pad_token_id"]
    batch["attention_mask"][1, 66:] = 0
    batch["bbox"][1, 66:] = 0
    return m.eval(), _cuda(batch)


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of ops.attn2_fwd"""
    from peneo_amd import ops
    seen = []
    real = ops.attn2_fwd

    def counting(*a, **kw):
        seen.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "attn2_fwd", counting)
    return seen


def test_switch_on_equals_switch_off(base, calls, monkeypatch):
    m, batch = base
    monkeypatch.delenv("PENEO_LILT_ATTN2", raising=False)
    with torch.no_grad():
        on = m(**batch)
    assert len(calls) == 2                           # one call per layer
    monkeypatch.setenv("PENEO_LILT_ATTN2", "0")
    with torch.no_grad():
        off = m(**batch)
    assert len(calls) == 2                           # none with the switch off
    for h in HEADS:
        k = h + "_shaking_outputs"
        assert torch.isfinite(on[k]).all(), k
        assert torch.equal(on[k], off[k]), k
    assert torch.equal(on["orig_bbox"], off["orig_bbox"])


def test_forward_with_autograd_keeps_the_concat_path(base, calls, monkeypatch):
    m, batch = base
    monkeypatch.delenv("PENEO_LILT_ATTN2", raising=False)
    m.train()
    try:
        m.zero_grad(set_to_none=True)
        out = m(**batch)
        out["loss"].backward()
    finally:
        m.eval()
    assert len(calls) == 0
    assert torch.isfinite(out["loss"])
    grads = [(n, p.grad) for n, p in m.named_parameters() if p.requires_grad and p.grad is not None]
    assert len(grads) > 50
    for n, g in grads:
        assert torch.isfinite(g).all(), n
    m.zero_grad(set_to_none=True)


def test_tiny_widths_keep_the_concat_path(calls, monkeypatch):
    monkeypatch.delenv("PENEO_LILT_ATTN2", raising=False)
    fx = load_golden("lilt_tiny")                    # head dims 48 + 12: not a pair peneo_attn2_supported takes
    m = _model(fx["config"], fx["state_dict"]).eval()
    with torch.no_grad():
        out = m(**_cuda(fx["batch"]))
    assert len(calls) == 0
    assert all(torch.isfinite(out[h + "_shaking_outputs"]).all() for h in HEADS)
