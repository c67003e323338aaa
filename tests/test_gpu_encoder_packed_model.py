"""PEneoModel.set_skip_padded_tokens: the packed encoder forward against the default path on the 2-layer base-width
LayoutLMv3 model and the ragged batch of test_gpu_pair_lens_model.py (B = 4 at 48 tokens with an image, decoder lengths N, N - 1, 28, 1).

Measured on an MI355X (e_def = max |bf16 default - fp32|, e_pack = max |bf16 packed - fp32| over the live pairs, per map; the bound is
e_pack <= 1.5 e_def): see profiles/encoder_packed.txt."""
import pytest
import torch

from test_gpu_pair_lens_model import CLASSES, LENS, N, P, PAD, SEQ, _batch, _live, _maps
from test_gpu_pair_mxfp8 import _model

pytestmark = pytest.mark.gpu

PACKED_OPS = ("pack_plan", "rows_pack", "rows_unpack", "encoder_layer_fwd_packed")
LAYERS = 2
MARGIN = 0.05           # decisions are compared where the fp32 top-1 / top-2 margin exceeds this
BOUND = 1.5             # e_pack <= BOUND * e_def


@pytest.fixture
def calls(monkeypatch):
    from peneo_amd import ops
    seen = {name: 0 for name in PACKED_OPS}
    for name in seen:
        real = getattr(ops, name)

        def counting(*a, _real=real, _name=name, **kw):
            seen[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counting)
    return seen


NONE = {name: 0 for name in PACKED_OPS}
ONE_FORWARD = {"pack_plan": 1, "rows_pack": 4, "rows_unpack": 1, "encoder_layer_fwd_packed": LAYERS}    # rows_pack: pos, xs, ys, x


def _same(a, b):
    for x, y in zip(_maps(a), _maps(b)):
        assert torch.equal(x, y)
    assert torch.equal(a["loss"], b["loss"])


def _hidden_of(m, batch):
    """(model output, the backbone's hidden state [B, T, H]) of one eval forward without gradients"""
    got = {}
    hook = m.backbone.register_forward_hook(lambda mod, args, out: got.__setitem__("h", out[0].detach().clone()))
    try:
        with torch.no_grad():
            out = m(**batch)
    finally:
        hook.remove()
    return out, got["h"]


@pytest.fixture(scope="module")
def ragged():
    """The three forwards every ragged-mask test reads, computed once: fp32 default (the reference), bf16 default, bf16 packed."""
    m, pcfg = _model("lmv3")
    batch = _batch(pcfg, "lmv3")
    with torch.no_grad():
        ref32 = m.set_compute_dtype(torch.float32)(**batch)
    m.set_compute_dtype(torch.bfloat16)
    off, h_off = _hidden_of(m, batch)
    assert m.set_skip_padded_tokens(True) is m
    on, h_on = _hidden_of(m, batch)
    m.set_skip_padded_tokens(False)
    return dict(m=m, batch=batch, ref32=ref32, off=off, on=on, h_off=h_off, h_on=h_on, live=_live())


def _errors(tag, got, off, ref32, live):
    """prints and checks e_pack <= BOUND * e_def per map over the live pairs"""
    for k, a, d, r in zip(CLASSES, _maps(got), _maps(off), _maps(ref32)):
        assert a.shape == d.shape == r.shape == (len(LENS), P, k)
        e_def = float((d[live] - r[live]).abs().max())
        e_pack = float((a[live] - r[live]).abs().max())
        print(f"{tag} map C={k}: e_def {e_def:.4e}  e_pack {e_pack:.4e}  ratio {e_pack / e_def:.3f}")
        assert e_def > 0.0 and e_pack <= BOUND * e_def, (tag, k, e_pack, e_def)


def test_all_ones_mask_is_the_default_path_bit_for_bit(calls):
    from peneo_amd.data import synthetic_rfund_batch
    m, pcfg = _model("lmv3")
    b = synthetic_rfund_batch(len(LENS), SEQ, 10, pcfg["backbone_config"]["vocab_size"], seed=6)
    assert bool(b["attention_mask"].all())
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    off, h_off = _hidden_of(m, batch)
    assert calls == NONE
    m.set_skip_padded_tokens(True)
    on, h_on = _hidden_of(m, batch)
    assert calls == ONE_FORWARD                                            # the packed forward was taken
    _same(on, off)
    assert torch.equal(h_on, h_off)


def test_ragged_mask_live_pairs_against_fp32(ragged):
    r = ragged
    _errors("packed", r["on"], r["off"], r["ref32"], r["live"])


def test_ragged_mask_decisions_on_live_pairs(ragged):
    r = ragged
    live = r["live"]
    decoded = 0
    for k, a, d, f in zip(CLASSES, _maps(r["on"]), _maps(r["off"]), _maps(r["ref32"])):
        top2 = f.topk(2, dim=-1).values
        clear = ((top2[..., 0] - top2[..., 1]) > MARGIN) & live
        decoded += int((d.argmax(-1)[live] != 0).sum())
        assert int(clear.sum()) > 0
        assert torch.equal(a.argmax(-1)[clear], d.argmax(-1)[clear]), k
    assert decoded > 0                                                     # guard: the default path decodes a live spot


def test_ragged_mask_hidden_rows_of_masked_tokens_are_zero(ragged):
    r = ragged
    h_on, h_off, mask = r["h_on"], r["h_off"], r["batch"]["attention_mask"]
    S = mask.shape[1]
    assert h_on.shape == h_off.shape and h_on.shape[1] > S                # text + visual tokens
    dead = torch.zeros(h_on.shape[:2], dtype=torch.bool, device=h_on.device)
    dead[:, :S] = mask == 0
    assert int(dead.sum()) == sum(SEQ - 1 - n for n in LENS)
    assert bool((h_on[dead] == 0).all())
    assert bool((h_off[dead] != 0).any())                                  # (the default path leaves something there)
    assert bool((h_on[~dead] != 0).any(dim=-1).all())                      # every live row, the visual ones among them, is written


def test_other_forwards_are_untouched_and_not_packed(calls):
    from peneo_amd.model.engine import DropoutSeeds
    m, pcfg = _model("lmv3")
    batch = _batch(pcfg, "lmv3")

    def both(run):
        """the same forward with the switch off and on, from the same dropout-seed state"""
        s0, p0 = DropoutSeeds._step, m._step
        m.set_skip_padded_tokens(False)
        off = run()
        DropoutSeeds._step, m._step = s0, p0
        m.set_skip_padded_tokens(True)
        on = run()
        m.set_skip_padded_tokens(False)
        return off, on

    off, on = both(lambda: m(**batch))                                     # with gradients (eval mode)
    assert off["loss"].requires_grad
    _same(on, off)

    def nomask():
        with torch.no_grad():
            return m(**dict(batch, attention_mask=None))
    _same(*both(nomask))

    def train_mode():
        m.train()
        try:
            with torch.no_grad():
                return m(**batch)
        finally:
            m.eval()
    off, on = both(train_mode)
    _same(on, off)
    assert calls == NONE
    # ... and the switch does take the eval forward without gradients of this very model
    m.set_skip_padded_tokens(True)
    with torch.no_grad():
        m(**batch)
    assert calls == ONE_FORWARD


def test_with_skip_padded_pairs_also_on(ragged):
    r = ragged
    m, live = r["m"], r["live"]
    m.set_skip_padded_tokens(True).set_skip_padded_pairs(True)
    try:
        with torch.no_grad():
            both = m(**r["batch"])
    finally:
        m.set_skip_padded_tokens(False).set_skip_padded_pairs(False)
    for k, a in zip(CLASSES, _maps(both)):
        bg = torch.tensor([0.0] + [PAD] * (k - 1), dtype=torch.float32, device=a.device)
        assert torch.equal(a[~live], bg.expand(int((~live).sum()), k))    # padding pairs hold the background row exactly
    _errors("packed + pair lens", both, r["off"], r["ref32"], live)
    assert bool(torch.isfinite(both["loss"]))


def test_mxfp8_pair_heads_combine_with_the_switch(ragged, calls):
    r = ragged
    m = r["m"]
    m.set_pair_heads_format("mxfp8")
    try:
        with torch.no_grad():
            off = m(**r["batch"])
            assert calls == NONE
            on = m.set_skip_padded_tokens(True)(**r["batch"])
    finally:
        m.set_skip_padded_tokens(False).set_pair_heads_format("bf16")
    assert calls == ONE_FORWARD
    live = r["live"]
    for a, d in zip(_maps(on), _maps(off)):
        assert bool(torch.isfinite(a[live]).all())
        assert float((a[live] - d[live]).abs().max()) < 0.5               # (same heads on hidden states that agree to bf16 noise)
