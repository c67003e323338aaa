"""The pair-head route of the decoder stage, host side (no GPU): peneo_decoder.pair_route for a table of cases written out here, the
strict-mode verdict of every row, and the width list the route function no longer spells out."""
import pytest
import torch

from peneo_amd.model.peneo_decoder import PairRoute

BF16, F32 = torch.bfloat16, torch.float32
WIDTH = "the decoder backward at D = {} without peneo_pair_bwd_fused and peneo_pair_dz_fused"
FP32 = "fp32 compute"

# what a row may change: attrs (set on the decoder), setters (called on it, in order), kcls, need_grad, tags, p (classifier dropout)
# -> the expected route, and what deterministic mode 2 says to a training step on it (None: accepted; rows without a backward: None)
CASES = {
    "bf16_384_train": (BF16, 384, {}, PairRoute("bf16", save=True, save_format="f16", backward="saved"), None),
    "bf16_384_e4m3": (BF16, 384, dict(setters=[("set_pair_act_format", "e4m3")]),
                      PairRoute("bf16", save=True, save_format="e4m3", backward="saved"), None),
    "bf16_384_mxfp8_train": (BF16, 384, dict(setters=[("set_pair_heads_train_format", "mxfp8")]),
                             PairRoute("mxfp8_save", save=True, save_format="f16", backward="saved"), None),
    "bf16_384_mxfp8_train_no_save": (BF16, 384, dict(setters=[("set_pair_heads_train_format", "mxfp8")], attrs=dict(save_pair_act=False)),
                                     PairRoute("bf16", backward="fused"), None),   # (falls through to the bf16 forward)
    "bf16_384_no_save": (BF16, 384, dict(attrs=dict(save_pair_act=False)), PairRoute("bf16", backward="fused"), None),
    "bf16_384_no_fused_bwd": (BF16, 384, dict(attrs=dict(fused_bwd=False)), PairRoute("bf16", backward="chunked", dz="fused"), None),
    "bf16_512": (BF16, 512, {}, PairRoute("bf16", backward="fused"), None),
    "bf16_256": (BF16, 256, {}, PairRoute("bf16", backward="chunked", dz="fused"), None),
    "bf16_192": (BF16, 192, dict(p=0.1), PairRoute("bf16", backward="chunked", dz="fused"), None),
    "bf16_256_no_fused_dz_p0": (BF16, 256, dict(attrs=dict(fused_dz=False)),
                                PairRoute("bf16", backward="chunked", dz="epilogue"), WIDTH.format(256)),
    "bf16_192_no_fused_dz_p": (BF16, 192, dict(attrs=dict(fused_dz=False), p=0.1),
                               PairRoute("bf16", backward="chunked", dz="standalone"), WIDTH.format(192)),
    "bf16_768_p0": (BF16, 768, {}, PairRoute("bf16", backward="chunked", dz="epilogue"), WIDTH.format(768)),
    "bf16_768_p": (BF16, 768, dict(p=0.1), PairRoute("bf16", backward="chunked", dz="standalone"), WIDTH.format(768)),
    "bf16_768_wide": (BF16, 768, dict(attrs=dict(fused_dz_wide=True), p=0.1),
                      PairRoute("bf16", backward="chunked", dz="wide", writes_x=False), WIDTH.format(768)),
    "bf16_768_wide_x": (BF16, 768, dict(attrs=dict(fused_dz_wide=True, dz_wide_writes_x=True)),
                        PairRoute("bf16", backward="chunked", dz="wide", writes_x=True), WIDTH.format(768)),
    "bf16_768_wide_without_fused_dz": (BF16, 768, dict(attrs=dict(fused_dz_wide=True, fused_dz=False)),
                                       PairRoute("bf16", backward="chunked", dz="epilogue"), WIDTH.format(768)),
    "bf16_384_wide_switch_is_not_asked": (BF16, 384, dict(attrs=dict(fused_bwd=False, fused_dz_wide=True, dz_wide_writes_x=True)),
                                          PairRoute("bf16", backward="chunked", dz="fused"), None),
    "bf16_768_no_pair_wide": (BF16, 768, dict(attrs=dict(pair_wide=False)), PairRoute("generic", backward="generic"), WIDTH.format(768)),
    "fp32_384_p0": (F32, 384, {}, PairRoute("bf16", backward="chunked", dz="epilogue"), FP32),
    "fp32_384_p": (F32, 384, dict(p=0.1), PairRoute("bf16", backward="chunked", dz="standalone"), FP32),
    "fp32_768": (F32, 768, {}, PairRoute("generic", backward="generic"), FP32),
    "three_layers": (BF16, 384, dict(kcls=3), PairRoute("generic", backward="generic"), "a 3-layer classifier"),
    "one_layer_fp32": (F32, 384, dict(kcls=1), PairRoute("generic", backward="generic"), FP32),
    "mxfp8_eval": (BF16, 384, dict(setters=[("set_pair_heads_format", "mxfp8")], need_grad=False), PairRoute("mxfp8_eval"), None),
    "mxfp8_eval_no_tags": (BF16, 384, dict(setters=[("set_pair_heads_format", "mxfp8")], need_grad=False, tags=False),
                           PairRoute("mxfp8_eval"), None),
    "no_tags": (BF16, 384, dict(tags=False), PairRoute("bf16"), None),
    "no_grad": (BF16, 384, dict(need_grad=False), PairRoute("bf16"), None),
    "no_grad_e4m3": (BF16, 384, dict(setters=[("set_pair_act_format", "e4m3")], need_grad=False), PairRoute("bf16"), None),
    "generic_no_grad": (BF16, 384, dict(kcls=3, need_grad=False), PairRoute("generic"), None),
}


def _decoder(D, kcls=2, ohem=False):
    from seeded import layoutlmv3_config, peneo_config
    from peneo_amd.model import PEneoConfig
    from peneo_amd.model.peneo_decoder import PEneoDecoder
    bcfg = layoutlmv3_config("tiny")
    over = dict(peneo_decoder_shrink=False, peneo_classifier_num_layers=kcls)
    if ohem:
        over.update(peneo_ohem_num_positive=8, peneo_ohem_num_negative=8)
    return PEneoDecoder(config=PEneoConfig(**dict(peneo_config("layoutlmv3-base", bcfg), **over)), input_size=D)


def _case(name, monkeypatch):
    dt, D, how, route, verdict = CASES[name]
    for var in ("PENEO_DZ_FUSED", "PENEO_BWD_FUSED", "PENEO_PAIR_SAVE", "PENEO_PAIR_WIDE", "PENEO_DZ_FUSED_WIDE", "PENEO_DZ_WIDE_X"):
        monkeypatch.delenv(var, raising=False)
    dec = _decoder(D, how.get("kcls", 2))
    for setter, fmt in how.get("setters", ()):
        getattr(dec, setter)(fmt)
    for k, v in how.get("attrs", {}).items():
        assert hasattr(dec, k), k
        setattr(dec, k, v)
    return dec, dt, D, how.get("need_grad", True), how.get("tags", True), how.get("p", 0.0), route, verdict


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_of_the_table(name, monkeypatch):
    from peneo_amd.model.peneo_decoder import pair_route
    dec, dt, D, need_grad, tags, p, route, _ = _case(name, monkeypatch)
    got = pair_route(dec, dt, D, need_grad, tags, p)
    assert got == route, (name, got)
    # the fields hang together: a saved backward is the one with a saving forward, dz belongs to the chunked backward
    assert (got.backward == "saved") == got.save and (got.dz is not None) == (got.backward == "chunked")
    assert (got.backward is None) == (not (need_grad and tags))
    assert got.backward is None or (got.forward == "generic") == (got.backward == "generic")
    with pytest.raises(Exception):                                        # immutable
        got.save = not got.save


@pytest.mark.parametrize("name", sorted(CASES))
def test_strict_mode_verdict_of_the_table(name, monkeypatch):
    """Deterministic mode 2 on every row: which message refuses it, or that it is accepted - and, for a refused row, that the stage's
    forward raises exactly that before it has run a kernel (it is given host tensors here)."""
    import peneo_amd
    from peneo_amd.model.peneo_decoder import pair_route, strict_refusal
    dec, dt, D, need_grad, tags, p, _, verdict = _case(name, monkeypatch)
    if not (need_grad and tags):
        assert verdict is None                                            # (nothing to refuse: no backward)
        return
    what = strict_refusal(dec, pair_route(dec, dt, D, need_grad, tags, p), dt, D)
    if verdict is None:
        assert what is None, what
        return
    assert what is not None and what.startswith(verdict), what
    B, N = 1, 4
    seq = torch.zeros(B, N, D, dtype=dt, requires_grad=True)
    labels = [torch.zeros(B, N * (N + 1) // 2, dtype=torch.int64) for _ in range(5)]
    dec.train(p > 0.0)
    with peneo_amd.deterministic(2):
        with pytest.raises(ValueError) as err:
            dec(seq, None, *labels)
    assert str(err.value) == f"deterministic mode 2 does not cover {what}; use mode 1 to run it and count it"


def test_strict_mode_messages_keep_their_order(monkeypatch):
    """fp32 before the classifier depth before OHEM before the width"""
    from peneo_amd.model.peneo_decoder import pair_route, strict_refusal
    for var in ("PENEO_DZ_FUSED", "PENEO_BWD_FUSED", "PENEO_PAIR_WIDE"):
        monkeypatch.delenv(var, raising=False)
    dec = _decoder(768, kcls=3, ohem=True)
    say = lambda d, dt, D: strict_refusal(d, pair_route(d, dt, D, True, True, 0.0), dt, D)
    assert say(dec, F32, 768).startswith("fp32 compute (the chunked decoder backward adds into d_ab")
    assert say(dec, BF16, 768).startswith("a 3-layer classifier (only the 2-layer heads have the fused backward")
    dec = _decoder(768, ohem=True)
    assert say(dec, BF16, 768) == "OHEM (peneo_ohem_ce sums the kept pairs with float atomics)"
    dec = _decoder(768)
    assert say(dec, BF16, 768) == ("the decoder backward at D = 768 without peneo_pair_bwd_fused and peneo_pair_dz_fused (the pair_dz GEMM "
                                   "epilogue adds with float atomics)")
    assert say(_decoder(384, ohem=True), BF16, 384).startswith("OHEM")
    assert say(_decoder(384), BF16, 384) is None


def test_narrow_dz_widths_are_the_list_the_decoder_used_to_spell_out():
    from peneo_amd import ops
    for D in range(16, 1088 + 1, 16):
        listed = D % 32 == 0 and D // 16 in (2, 4, 6, 8, 12, 16, 24, 32)
        assert (ops.pair_dz_fused_supported(BF16, D, 5) and D <= 512) == listed, D
        assert not ops.pair_dz_fused_supported(F32, D, 5), D
