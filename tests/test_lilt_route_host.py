"""The route of a LiLT forward, host side (no GPU): modeling_lilt.lilt_route for a table of cases written out here."""
from types import SimpleNamespace

import pytest
import torch

from peneo_amd.model.modeling_lilt import LiltRoute

BF16, F32 = torch.bfloat16, torch.float32
SWITCHES = ("PENEO_LILT_ATTN2", "PENEO_LILT_ATTN2_TRAIN", "PENEO_LILT_GROUPS", "PENEO_DEFER_JOIN")
TRAIN_ON = {"PENEO_LILT_ATTN2_TRAIN": "1"}
ALL_ON = {"PENEO_LILT_ATTN2": "1", "PENEO_LILT_ATTN2_TRAIN": "1", "PENEO_LILT_GROUPS": "1", "PENEO_DEFER_JOIN": "1"}

# name -> (widths, dtype, autograd on, attention dropout in force, environment (every switch not named is unset), expected route)
# widths: "base" = LiLT-base (head dims 64 + 16), "tiny" = the lilt_tiny golden's (48 + 12), "odd_ffn" = base with an intermediate
# size that is no multiple of 8
CASES = {
    "eval_no_grad": ("base", BF16, False, 0.0, {}, LiltRoute("attn2_eval", True, True)),
    "eval_no_grad_attn2_off": ("base", BF16, False, 0.0, {"PENEO_LILT_ATTN2": "0"}, LiltRoute("concat", True, True)),
    "eval_no_grad_train_switch_is_not_asked": ("base", BF16, False, 0.0, TRAIN_ON, LiltRoute("attn2_eval", True, True)),
    "train_default": ("base", BF16, True, 0.1, {}, LiltRoute("concat", True, True)),
    "train_switch_1": ("base", BF16, True, 0.1, TRAIN_ON, LiltRoute("attn2_train", True, True)),
    "train_switch_empty": ("base", BF16, True, 0.1, {"PENEO_LILT_ATTN2_TRAIN": ""}, LiltRoute("concat", True, True)),
    "train_switch_0": ("base", BF16, True, 0.1, {"PENEO_LILT_ATTN2_TRAIN": "0"}, LiltRoute("concat", True, True)),
    "train_eval_switch_is_not_asked": ("base", BF16, True, 0.1, {"PENEO_LILT_ATTN2": "0", **TRAIN_ON}, LiltRoute("attn2_train", True, True)),
    "eval_mode_with_autograd": ("base", BF16, True, 0.0, {}, LiltRoute("concat", True, True)),
    "eval_mode_with_autograd_switch": ("base", BF16, True, 0.0, TRAIN_ON, LiltRoute("attn2_train", True, True)),
    "no_grad_with_dropout": ("base", BF16, False, 0.1, {}, LiltRoute("concat", True, True)),
    "no_grad_with_dropout_switch": ("base", BF16, False, 0.1, TRAIN_ON, LiltRoute("attn2_train", True, True)),
    "fp32_train": ("base", F32, True, 0.1, {}, LiltRoute("concat", False, True)),
    "fp32_train_switches_on": ("base", F32, True, 0.1, ALL_ON, LiltRoute("concat", False, True)),
    "fp32_eval": ("base", F32, False, 0.0, {}, LiltRoute("concat", False, True)),
    "fp32_eval_switches_on": ("base", F32, False, 0.0, ALL_ON, LiltRoute("concat", False, True)),
    "tiny_train_switches_on": ("tiny", BF16, True, 0.1, ALL_ON, LiltRoute("concat", True, True)),
    "tiny_eval_switches_on": ("tiny", BF16, False, 0.0, ALL_ON, LiltRoute("concat", True, True)),
    "odd_ffn": ("odd_ffn", BF16, True, 0.1, {}, LiltRoute("concat", False, True)),
    "odd_ffn_eval": ("odd_ffn", BF16, False, 0.0, {}, LiltRoute("attn2_eval", False, True)),
    "groups_off": ("base", BF16, True, 0.1, {"PENEO_LILT_GROUPS": "0"}, LiltRoute("concat", False, True)),
    "groups_off_eval": ("base", BF16, False, 0.0, {"PENEO_LILT_GROUPS": "0"}, LiltRoute("attn2_eval", False, True)),
    "defer_join_off": ("base", BF16, True, 0.1, {"PENEO_DEFER_JOIN": "0"}, LiltRoute("concat", True, False)),
    "everything_off": ("base", BF16, False, 0.0, {"PENEO_LILT_ATTN2": "0", "PENEO_LILT_GROUPS": "0", "PENEO_DEFER_JOIN": "0"},
                       LiltRoute("concat", False, False)),
}


def _config(widths):
    from seeded import lilt_config
    from peneo_amd.model.configuration_peneo import LiltConfig
    over = dict(intermediate_size=3076) if widths == "odd_ffn" else {}      # 3076 / 4 = 769
    cfg = dict(lilt_config("tiny" if widths == "tiny" else "base"), **over)
    return LiltConfig(**{k: v for k, v in cfg.items() if k != "model_type"})


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_of_the_table(name, monkeypatch):
    from peneo_amd.model.modeling_lilt import lilt_route
    widths, dt, grad, p_attn, env, route = CASES[name]
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    cfg = _config(widths)
    nh, r = cfg.num_attention_heads, cfg.channel_shrink_ratio
    assert (cfg.hidden_size // nh, cfg.hidden_size // r // nh) == ((48, 12) if widths == "tiny" else (64, 16))
    with torch.enable_grad():                                 # the function is told; it does not ask torch
        got = lilt_route(cfg, dt, SimpleNamespace(p_attn=p_attn), grad)
    assert got == route, (name, got)
    assert got.attention in ("attn2_eval", "attn2_train", "concat")
    assert (got.attention == "attn2_eval") <= (not grad and p_attn <= 0.0)
    assert (got.attention == "attn2_train") <= (grad or p_attn > 0.0)


def test_route_is_immutable():
    route = LiltRoute("concat", True, True)
    for field, value in (("attention", "attn2_train"), ("grouped", False), ("defer_join", False)):
        with pytest.raises(Exception):
            setattr(route, field, value)
    assert route == LiltRoute("concat", True, True)
