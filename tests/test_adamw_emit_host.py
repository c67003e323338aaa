"""Host-side checks of the AdamW step that also writes the weights' working copies (no GPU needed): export, binding,
version, struct size, and the argument checks of the Python layers above the C ABI."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from peneo_amd import hip
    return ctypes.CDLL(hip.LIB_PATH)


def test_symbol_is_exported_and_bound(lib):
    from peneo_amd import hip
    assert hasattr(lib, "peneo_adamw_step_emit")
    assert "peneo_adamw_step_emit" in hip.SIGNATURES
    # the arguments of peneo_adamw_step_clip plus the two arrays of the emission table (the stream stays last)
    assert len(hip.SIGNATURES["peneo_adamw_step_emit"][1]) == len(hip.SIGNATURES["peneo_adamw_step_clip"][1]) + 2
    fn = hip.lib().peneo_adamw_step_emit
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert lib.peneo_version() >= 106


def test_struct_size_matches_the_c_side(lib):
    from peneo_amd import hip
    lib.peneo_struct_bytes.restype = ctypes.c_size_t
    assert lib.peneo_struct_bytes(4) == ctypes.sizeof(hip.AdamwEmit) == 16
    assert hip.AdamwEmit.dst.offset == 0 and hip.AdamwEmit.tensor.offset == 8 and hip.AdamwEmit.dtype.offset == 12


def _table():
    from peneo_amd import ops
    p = torch.zeros(6, 4)
    return ops, p, ops.AdamwEmitTable([p, torch.zeros(3)])


def test_wrapper_accepts_a_good_pair():
    ops, p, tab = _table()
    big = torch.zeros(40, dtype=torch.bfloat16)
    recs = tab.records([(p, big[1:25]), (tab.params[1], torch.zeros(3)), (p, torch.zeros(24))])
    assert [r[0] for r in recs] == [0, 0, 1] and recs[0][1] == big.data_ptr() + 2
    assert [r[2] for r in recs] == [1, 0, 0]                       # PENEO_BF16, PENEO_F32, PENEO_F32
    assert tab.records([(p.view(-1), big[:24])])[0][0] == 0          # a full view of a parameter is that parameter


def test_wrapper_rejects_a_strided_destination():
    ops, p, tab = _table()
    with pytest.raises(ValueError, match="contiguous"):
        tab.records([(p, torch.zeros(48)[::2])])


def test_wrapper_rejects_a_destination_on_another_device():
    ops, p, tab = _table()
    with pytest.raises(ValueError, match="destination on"):
        tab.records([(p, torch.zeros(24, device="meta"))])


def test_wrapper_rejects_other_dtypes():
    ops, p, tab = _table()
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="neither bf16 nor fp32"):
            tab.records([(p, torch.zeros(24, dtype=dt))])


def test_wrapper_rejects_a_wrong_size():
    ops, p, tab = _table()
    with pytest.raises(ValueError, match="elements"):
        tab.records([(p, torch.zeros(23))])
    with pytest.raises(ValueError, match="not one of the step's tensors"):
        tab.records([(torch.zeros(24), torch.zeros(24))])


def test_optimizer_rejects_an_emit_target_that_is_no_module():
    from peneo_amd.model.engine import WeightCache
    from peneo_amd.optim import FusedAdamW
    w = torch.nn.Parameter(torch.zeros(4))
    for bad in (WeightCache(), [torch.nn.Linear(2, 2)], "model", 1):
        with pytest.raises(TypeError, match="emit_into"):
            FusedAdamW([w], emit_into=bad)
    assert FusedAdamW([w])._emit_into is None                       # off by default
    lin = torch.nn.Linear(2, 2)
    assert FusedAdamW(lin.parameters(), emit_into=lin)._emit_into is lin


def test_weight_cache_knows_its_declarative_entries():
    """What the optimizer asks of a cache, on the host-only parts: keys that were never built are not offered."""
    from peneo_amd.model.engine import WeightCache
    wc = WeightCache()
    assert wc.declarative() == [] and wc.builds == {}
    p = torch.zeros(3, 2)
    assert wc.cast("w", p, torch.float32).data_ptr() == p.data_ptr()     # fp32: the parameter itself, no entry
    assert wc.declarative() == [] and wc.builds == {}
    n = []
    assert wc.get(("opaque",), [p], lambda: n.append(1) or 7) == 7 and wc.get(("opaque",), [p], lambda: n.append(1) or 8) == 7
    assert wc.builds == {("opaque",): 1} and wc.declarative() == []       # entries made through get() stay lazy
