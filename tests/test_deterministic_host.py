"""Deterministic mode, host side (no GPU): the new entry points in header, exports and ctypes table; the switch and its context
manager; the counter; the size queries under each mode; PENEO_DETERMINISTIC in a fresh process; the strict refusal of a call that
returns before it touches a device."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ["peneo_set_deterministic", "peneo_deterministic", "peneo_order_dependent_launches",
                    "peneo_pair_bwd_workspace_rows", "peneo_pair_dz_fused_workspace_rows", "peneo_relpos_bwd_workspace_bytes",
                    "peneo_relpos_bias_bwd_layers_ws", "peneo_relpos_bias_bwd_ws", "peneo_grad_sqnorm_workspace_bytes",
                    "peneo_grad_sqnorm_ws"]


@pytest.fixture
def hip():
    """the binding module, with the mode it found restored afterwards"""
    from peneo_amd import hip as h
    h.load_library()
    before = h.deterministic_mode()
    yield h
    h.set_deterministic(before)


def test_header_exports_and_ctypes_table_agree_on_the_new_entry_points(hip):
    src = open(os.path.join(ROOT, "include", "peneo_hip.h")).read()
    declared = set(re.findall(r"\b(peneo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    lib = hip.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in include/peneo_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in hip.SIGNATURES, f"{name} is missing from the ctypes table"
    assert sorted(hip.SIGNATURES) == sorted(declared)
    assert lib.peneo_version() >= 107


def test_mode_round_trips_and_the_context_manager_restores_it(hip):
    import peneo_amd
    for mode in (0, 1, 2, 0):
        peneo_amd.set_deterministic(mode)
        assert hip.deterministic_mode() == mode and hip.lib().peneo_deterministic() == mode
        assert peneo_amd.is_deterministic() == (mode != 0)
    peneo_amd.set_deterministic(True)
    assert hip.deterministic_mode() == 1
    peneo_amd.set_deterministic(False)
    assert hip.deterministic_mode() == 0
    with pytest.raises(ValueError):
        peneo_amd.set_deterministic(3)
    assert hip.deterministic_mode() == 0
    for outer in (0, 1, 2):
        peneo_amd.set_deterministic(outer)
        with peneo_amd.deterministic():                       # default: strict
            assert hip.deterministic_mode() == 2
            with peneo_amd.deterministic(1):
                assert hip.deterministic_mode() == 1
            assert hip.deterministic_mode() == 2
        assert hip.deterministic_mode() == outer
        with pytest.raises(RuntimeError, match="boom"):       # restored when the body raises, too
            with peneo_amd.deterministic(2 - outer):
                raise RuntimeError("boom")
        assert hip.deterministic_mode() == outer


def test_size_queries_follow_the_mode(hip):
    """Mode 0 answers today's sizes (256 workspace rows, no extra workspace); modes 1 and 2 the deterministic forms': one pair
    workspace row per workgroup (B x blocks of the triangle: 8 x 1056 = 8 448 rows = 260 MB at 8 x 511 tokens, as documented), 8
    bytes per (head, bin) for the relative-position fold, 8 bytes per chunk for the gradient norm."""
    lib = hip.lib()
    blocks_511 = lib.peneo_pair_bwd_rows(511) // 128
    assert blocks_511 == 1056
    hip.set_deterministic(0)
    assert lib.peneo_pair_bwd_workspace_rows(8, 511) == 256 and lib.peneo_pair_bwd_workspace_rows(1, 9) == 256
    assert lib.peneo_relpos_bwd_workspace_bytes(12, 32, 64) == 0
    assert lib.peneo_grad_sqnorm_workspace_bytes(70) == 0
    assert lib.peneo_pair_dz_fused_workspace_rows(1) == 256 and lib.peneo_pair_dz_fused_workspace_rows(1 << 18) == 256
    for mode in (1, 2):
        hip.set_deterministic(mode)
        assert lib.peneo_pair_bwd_workspace_rows(8, 511) == 8 * blocks_511 == 8448
        assert 8448 * 4 * 5 * 384 * 4 == 259_522_560                              # the documented 260 MB
        assert lib.peneo_pair_bwd_workspace_rows(2, 40) == 2 * (lib.peneo_pair_bwd_rows(40) // 128)
        assert lib.peneo_pair_bwd_workspace_rows(0, 40) == 0
        assert lib.peneo_relpos_bwd_workspace_bytes(12, 32, 64) == 8 * 12 * (32 + 2 * 64)
        assert lib.peneo_relpos_bwd_workspace_bytes(4, 32, 0) == 8 * 4 * 32
        assert lib.peneo_grad_sqnorm_workspace_bytes(70) == 8 * 70
        # the chunked decoder backward (peneo_pair_dz_fused): a row per workgroup of 256 pairs, never fewer than the default's 256
        assert lib.peneo_pair_dz_fused_workspace_rows(1) == 256 and lib.peneo_pair_dz_fused_workspace_rows(256 * 256) == 256
        assert lib.peneo_pair_dz_fused_workspace_rows(256 * 256 + 1) == 257 and lib.peneo_pair_dz_fused_workspace_rows(1 << 18) == 1024
        assert lib.peneo_pair_bwd_supported(hip.BF16, 96, 5) == 0               # (which widths take which backward does not change)
    hip.set_deterministic(0)
    assert lib.peneo_pair_bwd_workspace_rows(8, 511) == 256


def test_strict_mode_refuses_and_every_mode_counts_a_call_that_has_no_deterministic_form(hip):
    """peneo_grad_sqnorm (no workspace) decides before it touches the device: under mode 2 it returns PENEO_ERR_INVALID with a message
    that names it; the counter moves either way.  (The pointers are never dereferenced on that path.)"""
    lib = hip.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    hip.set_deterministic(2)
    before = hip.order_dependent_launches()
    rc = lib.peneo_grad_sqnorm(p, p, p, 1, p, None)
    assert rc != 0 and hip.order_dependent_launches() == before + 1
    msg = lib.peneo_last_error().decode()
    assert "peneo_grad_sqnorm" in msg and "deterministic" in msg
    with pytest.raises(hip.PeneoHipError, match="peneo_grad_sqnorm"):
        hip.check(rc, "peneo_grad_sqnorm")
    # the _ws form under the mode wants its workspace, and says how much
    rc = lib.peneo_grad_sqnorm_ws(p, p, p, 70, p, None, 0, None)
    assert rc != 0 and "560" in lib.peneo_last_error().decode() and hip.order_dependent_launches() == before + 1


_CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.peneo_order_dependent_launches.restype = ctypes.c_uint64
print(lib.peneo_deterministic(), lib.peneo_order_dependent_launches())
"""


@pytest.mark.parametrize("env,want", [(None, 0), ("0", 0), ("1", 1), ("2", 2), ("7", 2)])
def test_environment_variable_sets_the_initial_mode_and_the_counter_starts_at_zero(env, want):
    from peneo_amd import hip as h
    e = {k: v for k, v in os.environ.items() if k != "PENEO_DETERMINISTIC"}
    if env is not None:
        e["PENEO_DETERMINISTIC"] = env
    r = subprocess.run([sys.executable, "-c", _CHILD, h.LIB_PATH], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-400:]
    assert r.stdout.split() == [str(want), "0"], r.stdout
