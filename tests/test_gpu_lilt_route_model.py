"""The LiLT layer stages follow one LiltRoute per forward: the launches of a step, counted per route (the literals below are the
counts of the commit before LiltRoute, taken with this recorder), and a step whose switches change between its forward and its
backward finishes on the forward's route."""
import pytest
import torch

pytestmark = pytest.mark.gpu
COUNTED = ("gemm_group", "gemm", "layernorm_fwd", "layernorm_bwd", "colsum", "head_concat", "head_split", "attn_fwd", "attn_bwd",
           "attn2_fwd", "attn2_bwd", "copy2d")
SWITCHES = ("PENEO_LILT_ATTN2", "PENEO_LILT_ATTN2_TRAIN", "PENEO_LILT_GROUPS", "PENEO_DEFER_JOIN")
LAYERS = 2

# Two layers, the backbone alone.  Outside the layers: the embedding stage (forward 1 gemm + 2 layernorm_fwd; backward 2 gemm + 2
# layernorm_bwd + 2 colsum) and the final cat (2 copy2d each way).  Per layer, grouped: 4 + 6 gemm_group; ungrouped: 8 + 16 gemm.
_NONE = dict.fromkeys(COUNTED, 0)
_STEP = dict(_NONE, layernorm_fwd=10, layernorm_bwd=10, colsum=18, copy2d=4)
_CONCAT = dict(head_concat=6, head_split=6, attn_fwd=2, attn_bwd=2)
_ATTN2 = dict(attn2_fwd=2, attn2_bwd=2)
_EVAL = dict(_NONE, layernorm_fwd=10, copy2d=2)
TRAIN_STEPS = {
    "concat_grouped": ({}, dict(_STEP, gemm_group=20, gemm=3, **_CONCAT)),
    "concat_ungrouped": ({"PENEO_LILT_GROUPS": "0"}, dict(_STEP, gemm_group=0, gemm=51, **_CONCAT)),
    "attn2_train_grouped": ({"PENEO_LILT_ATTN2_TRAIN": "1"}, dict(_STEP, gemm_group=20, gemm=3, **_ATTN2)),
    "attn2_train_ungrouped": ({"PENEO_LILT_ATTN2_TRAIN": "1", "PENEO_LILT_GROUPS": "0"}, dict(_STEP, gemm_group=0, gemm=51, **_ATTN2)),
}
EVAL_FORWARDS = {
    "attn2_eval": ({}, dict(_EVAL, gemm_group=8, gemm=1, attn2_fwd=2)),
    "concat": ({"PENEO_LILT_ATTN2": "0"}, dict(_EVAL, gemm_group=8, gemm=1, head_concat=4, head_split=2, attn_fwd=2)),
}
# what of a grouped concat training step belongs to its backward
CONCAT_GROUPED_BACKWARD = dict(_NONE, gemm_group=12, gemm=2, layernorm_bwd=10, colsum=18, head_concat=2, head_split=4, attn_bwd=2,
                               copy2d=2)


def _set(monkeypatch, env):
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)


def _forward(m, batch, train):
    """the backbone alone (the decoder's launches stay out of the counts) -> the sum of its output"""
    from peneo_amd.model.engine import DropoutSeeds
    DropoutSeeds._step, m._step = 40, 40
    m.train(train)
    m.zero_grad(set_to_none=True)
    out = m.backbone(input_ids=batch["input_ids"], bbox=batch["bbox"], attention_mask=batch["attention_mask"])[0]
    return out.float().sum()


@pytest.fixture(scope="module")
def base():
    """LiLT-base widths (head dims 64 + 16), two layers, B = 2, S = 96, the second document's last 30 tokens masked
    (tests/test_gpu_attn2_train_model.py's fixture); one step run, so that the weight cache's copies are made."""
    from seeded import lilt_config, peneo_config, seeded_fill_
    from peneo_amd.data import synthetic_rfund_batch
    from peneo_amd.model import PEneoConfig, PEneoModel
    bcfg = dict(lilt_config("base"), num_hidden_layers=LAYERS, vocab_size=1000)
    pcfg = peneo_config("lilt-roberta-en-base", bcfg)
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    m = m.cuda().set_compute_dtype(torch.bfloat16)
    seeded_fill_(m.state_dict(), 17)
    batch = synthetic_rfund_batch(2, 96, 24, bcfg["vocab_size"], seed=9, with_image=False)
    batch["input_ids"][1, 66:] = bcfg["pad_token_id"]
    batch["attention_mask"][1, 66:] = 0
    batch["bbox"][1, 66:] = 0
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    _forward(m, batch, True).backward()
    torch.cuda.synchronize()
    yield m, batch
    m.eval()
    m.zero_grad(set_to_none=True)


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the ops the layer stages launch, and of modeling_lilt.defer_join"""
    from peneo_amd import ops
    from peneo_amd.model import modeling_lilt
    seen = dict.fromkeys(COUNTED + ("defer_join",), 0)

    def wrap(owner, name):
        real = getattr(owner, name)

        def counting(*a, **kw):
            seen[name] += 1
            return real(*a, **kw)
        monkeypatch.setattr(owner, name, counting)
    for n in COUNTED:
        wrap(ops, n)
    wrap(modeling_lilt, "defer_join")
    return seen


def _ops_counts(seen):
    return {n: seen[n] for n in COUNTED}


@pytest.mark.parametrize("name", sorted(TRAIN_STEPS))
def test_launches_of_a_training_step(base, calls, monkeypatch, name):
    m, batch = base
    env, expected = TRAIN_STEPS[name]
    _set(monkeypatch, env)
    _forward(m, batch, True).backward()
    torch.cuda.synchronize()
    print(name, _ops_counts(calls), "defer_join", calls["defer_join"])
    assert _ops_counts(calls) == expected
    assert calls["defer_join"] == LAYERS
    grads = [p.grad for p in m.backbone.parameters() if p.grad is not None]
    assert len(grads) > 50 and all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("name", sorted(EVAL_FORWARDS))
def test_launches_of_an_eval_forward(base, calls, monkeypatch, name):
    m, batch = base
    env, expected = EVAL_FORWARDS[name]
    _set(monkeypatch, env)
    with torch.no_grad():
        out = _forward(m, batch, False)
    torch.cuda.synchronize()
    print(name, _ops_counts(calls))
    assert _ops_counts(calls) == expected
    assert torch.isfinite(out)


def test_the_route_of_a_step_is_the_forwards_route(base, calls, monkeypatch):
    m, batch = base
    _set(monkeypatch, {})
    loss = _forward(m, batch, True)
    forward = _ops_counts(calls)
    _set(monkeypatch, {"PENEO_LILT_GROUPS": "0", "PENEO_LILT_ATTN2_TRAIN": "1", "PENEO_DEFER_JOIN": "0"})
    loss.backward()
    torch.cuda.synchronize()
    backward = {n: calls[n] - forward[n] for n in COUNTED}
    print("backward", backward, "defer_join", calls["defer_join"])
    assert backward == CONCAT_GROUPED_BACKWARD
    assert {n: forward[n] + backward[n] for n in COUNTED} == TRAIN_STEPS["concat_grouped"][1]
    assert calls["defer_join"] == LAYERS
