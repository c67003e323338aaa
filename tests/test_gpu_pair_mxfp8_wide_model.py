"""PEneoModel.set_pair_heads_format("mxfp8", wide=True): the MXFP8 pair heads of models with the decoder shrink off, decoder widths
768 (LayoutLMv3-base), 960 (LiLT-base) and 1024 (LayoutLMv3-large).  The one-layer models, seeded weights and the ragged 2 x 48
token batch of tests/test_gpu_noshrink_model.py, in bf16; the emulation, its bounds and the cosine bar (0.995, set from the 0.9988
measured on the narrow path) are those of tests/test_gpu_pair_mxfp8.py."""
import functools

import pytest
import torch

from test_gpu_noshrink_model import WIDTHS, _config, build_model, to_cuda
from test_gpu_pair_mxfp8 import OUT_KEYS, check_close, emulate_logits, map_cosines

pytestmark = pytest.mark.gpu
MODELS = ("lmv3_base", "lilt_base", "lmv3_large")
PAIR_OPS = ("pair_heads_fwd", "pair_heads_fwd_lens", "pair_heads_fwd_mxfp8", "pair_heads_fwd_mxfp8_wide", "pair_heads_pack",
            "pair_heads_pack_mxfp8", "pair_heads_pack_mxfp8_wide")


def _batch(which):
    from peneo_amd.data import synthetic_rfund_batch
    lilt = which == "lilt_base"
    batch = synthetic_rfund_batch(2, 48, 12, 1000, seed=13, ragged=True, with_image=not lilt, add_sep=not lilt)
    if lilt:
        batch.pop("image", None)
    return to_cuda(batch)


def _model(which):
    from seeded import seeded_fill_
    m = build_model(_config(which), torch.bfloat16)
    seeded_fill_(m.state_dict(), 21)
    assert m.peneo_decoder.decoder_hidden_size == WIDTHS[which]
    return m.eval()


@functools.lru_cache(maxsize=None)
def _default(which):
    """(device batch, outputs of the default bf16 eval forward of a model that never switched)"""
    batch = _batch(which)
    with torch.no_grad():
        return batch, _model(which)(**batch)


@pytest.fixture
def calls(monkeypatch):
    """the pair-heads ops as they are called, by name"""
    from peneo_amd import ops
    seen = []
    for name in PAIR_OPS:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (seen.append(_n), _r(*a, **k))[1])
    return seen


@pytest.mark.parametrize("which", MODELS)
def test_model_logits_match_the_emulation_on_the_models_weights(monkeypatch, calls, which):
    from peneo_amd import ops
    batch, ref = _default(which)
    m = _model(which)
    del calls[:]                                                 # (the default forward, where this test is the first to need it)
    with pytest.raises(ValueError, match=f"D = {WIDTHS[which]}"):
        m.set_pair_heads_format("mxfp8")
    m.set_pair_heads_format("mxfp8", wide=True)
    seen = {}
    real = ops.pair_heads_fwd_mxfp8_wide

    def spy(ab, *a, **k):
        seen["ab"] = ab.clone()
        return real(ab, *a, **k)
    monkeypatch.setattr(ops, "pair_heads_fwd_mxfp8_wide", spy)
    with torch.no_grad():
        out = m(**batch)
        out2 = m(**batch)                                        # the cached pack
    assert "ab" in seen and seen["ab"].shape[-1] == 2 * WIDTHS[which]
    assert calls == ["pair_heads_pack_mxfp8_wide", "pair_heads_fwd_mxfp8_wide", "pair_heads_fwd_mxfp8_wide"], calls
    dec = m.peneo_decoder
    lins = [dec.head_linears(n) for n in OUT_KEYS]
    w1 = [l[0].weight.detach() for l in lins]
    b1 = torch.cat([l[0].bias.detach() for l in lins])
    w2 = [l[1].weight.detach() for l in lins]
    b2 = torch.cat([l[1].bias.detach() for l in lins])
    want = emulate_logits(seen["ab"], w1, b1, w2, b2)
    got = [out[k + "_shaking_outputs"] for k in OUT_KEYS]
    for g_, g2 in zip(got, [out2[k + "_shaking_outputs"] for k in OUT_KEYS]):
        assert g_.dtype == torch.float32 and torch.equal(g_, g2)
    check_close([g_.reshape(w_.shape) for g_, w_ in zip(got, want)], want)
    assert torch.isfinite(out["loss"])
    cos = map_cosines(out, ref)
    print(f"cosine mxfp8 wide / bf16, {which} (D = {WIDTHS[which]}):", cos)
    assert min(cos.values()) >= 0.995, cos


def test_refused_before_anything_runs(monkeypatch, calls):
    """a forward with gradients, and an fp32 compute dtype chosen afterwards: no backbone forward, no pair-heads op"""
    batch, _ = _default("lmv3_base")
    m = _model("lmv3_base")
    del calls[:]
    m.set_pair_heads_format("mxfp8", wide=True)
    with pytest.raises(ValueError):
        m.set_pair_heads_train_format("mxfp8")
    with pytest.raises(ValueError, match="mxfp8"):
        m.set_skip_padded_pairs(True)
    real_bb = m.backbone.forward
    monkeypatch.setattr(m.backbone, "forward", functools.wraps(real_bb)(lambda *a, **k: (calls.append("backbone"), real_bb(*a, **k))[1]))
    m.train()
    with pytest.raises(ValueError, match="inference-only"):
        m(**batch)
    m.eval().set_compute_dtype(torch.float32)
    with torch.no_grad(), pytest.raises(ValueError, match="bfloat16"):
        m(**batch)
    assert calls == []


def test_switching_back_to_bf16_is_bit_identical(calls):
    batch, ref = _default("lmv3_base")
    m = _model("lmv3_base")
    m.set_pair_heads_format("mxfp8", wide=True)
    with torch.no_grad():
        m(**batch)
    m.set_pair_heads_format("bf16")
    del calls[:]
    with torch.no_grad():
        a = m(**batch)
    assert calls == ["pair_heads_pack", "pair_heads_fwd"], calls
    for k in OUT_KEYS:
        assert torch.equal(a[k + "_shaking_outputs"], ref[k + "_shaking_outputs"]), k
    assert torch.equal(a["loss"], ref["loss"])
