"""The e4m3 form of the saved pair activations at kernel level (include/peneo_hip.h, version 109): peneo_pair_heads_fwd_save_e4m3
against peneo_pair_heads_fwd_save, and peneo_pair_bwd_saved_e4m3 on its records against peneo_pair_bwd_saved on the f16 records
requantised on the host by the documented rule e4m3fn(RNE(clamp(v, -448, 448))).  The comparison never looks inside a record, so it
holds for any layout: it pins the forward's rounding and clamp, the record addressing and the backward's decode at once."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D, CLASSES, NH = 384, [2, 3, 3, 3, 3], 5
DT, DEV = torch.bfloat16, "cuda"
# small triangles: partial blocks on the diagonal and in the last block row, one and several documents, an odd and an even
# number of blocks (the saving forward walks two blocks per workgroup)
SHAPES = [(1, 9, 0.0), (2, 40, 0.1), (3, 97, 0.2)]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


def requantise(act_f16_bytes: torch.Tensor) -> torch.Tensor:
    """the f16 records with every value replaced by the f16 value of its e4m3 byte (torch's cast alone gives NaN beyond +-448)"""
    v = act_f16_bytes.cpu().view(torch.float16).float()
    q = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float16)
    return q.view(torch.uint8).to(act_f16_bytes.device)


_CASES = {}


def case(ops, B, N, drop, w1_scale=1.0):
    """inputs as in test_gpu_kernels.py::test_pair_saved_activations_path_is_the_recomputing_path, both forwards, and the three
    backwards (f16 records, requantised f16 records, e4m3 records) on ONE set of dlogits; computed once per shape"""
    key = (B, N, drop, w1_scale)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(N + int(100 * drop))
    P = N * (N + 1) // 2
    ab = torch.randn(B, N, 2 * D, generator=g).to(DEV).to(DT)
    w1 = [(w1_scale * torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).to(DEV) for c in CLASSES]
    b1, b2 = (0.1 * torch.randn(NH * D, generator=g)).to(DEV), (0.1 * torch.randn(14, generator=g)).to(DEV)
    wp = ops.pair_heads_pack(DT, w1, w2)
    tags = [torch.randint(0, c, (B, P), generator=g).to(DEV) for c in CLASSES]
    cw = [(torch.rand(c, generator=g) + 0.5).to(DEV) for c in CLASSES]
    kw = dict(tags=tags, class_weights=cw, want_dlogits=True, want_logits=True, drop_p=drop, drop_seed=77, save=True)
    f16 = ops.pair_heads_fwd(ab, wp, b1, b2, CLASSES, save_format="f16", **kw)
    e4 = ops.pair_heads_fwd(ab, wp, b1, b2, CLASSES, save_format="e4m3", **kw)
    torch.cuda.synchronize()
    scale = (torch.rand(NH, generator=g) + 0.5).to(DEV)
    c = dict(B=B, N=N, drop=drop, ab=ab, w1=w1, w2=w2, wp2=ops.pair_bwd_pack(w1), f16=f16, e4=e4, scale=scale,
             act_q=requantise(f16[3][0]))
    c["bwd_f16"] = backward(ops, c, f16[3][0], "f16")
    c["bwd_q"] = backward(ops, c, c["act_q"], "f16")
    from peneo_amd import hip
    n0 = hip.order_dependent_launches()
    c["bwd_e4"] = backward(ops, c, e4[3][0], "e4m3")
    c["counted"] = hip.order_dependent_launches() - n0
    _CASES[key] = c
    return c


def backward(ops, c, act, fmt):
    """-> (dz, d_ab, workspace) of one saved backward under the mode in force; dz pre-filled with 3.0 so unwritten rows show"""
    B, N = c["B"], c["N"]
    dz = torch.full((B * ops.pair_bwd_rows(N), NH * D), 3.0, device=DEV, dtype=DT)
    d_ab = torch.zeros(B, N, 2 * D, device=DEV)
    ws = ops.pair_bwd_workspace(B, N, NH, D, DEV)
    args = ops.pair_dz_args(D, CLASSES, c["f16"][2], c["w2"], c["scale"], drop_p=c["drop"], drop_seed=77)
    ops.pair_bwd_saved(c["ab"], c["wp2"], args, act, dz, d_ab, ws, act_format=fmt)
    torch.cuda.synchronize()
    return dz, d_ab, ws


def assert_same_backward(ops, c):
    from peneo_amd import hip
    (dz_q, dab_q, ws_q), (dz_e, dab_e, ws_e) = c["bwd_q"], c["bwd_e4"]
    assert torch.isfinite(dz_e.float()).all() and torch.isfinite(dab_e).all() and torch.isfinite(ws_e).all()
    assert torch.equal(dz_q, dz_e)                                        # no atomics in either
    assert torch.equal(dab_q, dab_e)
    assert not (dz_e == 3.0).all(dim=1).any()                             # every row of the block walk was written
    # default mode: the same terms met in another order (the bound the f16 saved-path test uses for its partial rows)
    s_q, s_e = ws_q.sum(0), ws_e.sum(0)
    print(f"B={c['B']} N={c['N']} drop={c['drop']}: workspace sums differ by {float((s_q - s_e).abs().max() / s_q.abs().max()):.3e} relative")
    assert float((s_q - s_e).abs().max() / s_q.abs().max()) < 1e-5
    # deterministic mode: a workspace row per workgroup, one add per address - the rows themselves are the same bits
    prev = hip.deterministic_mode()
    hip.set_deterministic(1)
    try:
        n0 = hip.order_dependent_launches()
        det_q = backward(ops, c, c["act_q"], "f16")
        det_e = backward(ops, c, c["e4"][3][0], "e4m3")
        assert hip.order_dependent_launches() == n0                       # routed to the row-per-workgroup form
    finally:
        hip.set_deterministic(prev)
    assert det_e[2].shape[0] == ops.pair_bwd_rows(c["N"]) // 128 * c["B"]
    for a, b in zip(det_q, det_e):
        assert torch.equal(a, b)
    assert torch.equal(det_e[0], dz_e) and torch.equal(det_e[1], dab_e)


@pytest.mark.parametrize("B,N,drop", SHAPES)
def test_forward_is_the_f16_saving_forward_but_for_the_records(ops, B, N, drop):
    c = case(ops, B, N, drop)
    (lg0, pt0, dl0, (act0, x0)), (lg1, pt1, dl1, (act1, x1)) = c["f16"], c["e4"]
    assert act1.numel() == ops.pair_save_e4m3_bytes(B, N, NH, D) == act0.numel() // 2
    for h in range(NH):
        assert torch.equal(lg0[h], lg1[h]) and torch.equal(dl0[h], dl1[h]), h
    assert torch.equal(pt0, pt1)                                          # same walk, same rows
    assert torch.equal(x0, x1)


@pytest.mark.parametrize("B,N,drop", SHAPES)
def test_records_and_backward_are_the_requantised_f16_path(ops, B, N, drop):
    c = case(ops, B, N, drop)
    assert_same_backward(ops, c)
    assert c["counted"] == 1                                              # in the default mode the launch is listed as order-dependent
    # the requantisation changed something (else this test would compare the f16 path with itself) and stayed close
    dz_f, dz_q = c["bwd_f16"][0].float(), c["bwd_q"][0].float()
    rel = float((dz_f - dz_q).norm() / dz_f.norm())
    print(f"B={B} N={N} drop={drop}: dz from e4m3 records against dz from f16 records: {rel:.3e} relative")
    assert 0.0 < rel < 0.1


@pytest.mark.parametrize("w1_scale", [300.0, 0.01])
def test_saturation_and_subnormals_follow_the_host_rule(ops, w1_scale):
    """w1 x 300 pushes many kept |z| beyond 448 (finite, equal to the host clamp); w1 x 0.01 pushes values into e4m3 subnormals, -0"""
    c = case(ops, 2, 40, 0.1, w1_scale)
    z = c["f16"][3][0].cpu().view(torch.float16).float()
    kept = z > -20000.0
    if w1_scale > 1:
        assert int((z[kept].abs() > 448).sum()) > 1000                    # the case does saturate kept units
    else:
        assert int((z.abs() < 2.0 ** -6).sum()) > 1000                    # below the smallest e4m3 normal
        q = c["act_q"].cpu().view(torch.float16)
        assert int(((q == 0) & torch.signbit(q)).sum()) > 0               # -0 occurs
    for h in range(NH):
        assert torch.isfinite(c["e4"][0][h]).all()
    assert_same_backward(ops, c)


@pytest.mark.parametrize("B,N,drop", [s for s in SHAPES if s[2] > 0])
def test_dropout_zeros_are_those_of_the_f16_saved_backward(ops, B, N, drop):
    c = case(ops, B, N, drop)
    zero_f, zero_e = c["bwd_f16"][0] == 0, c["bwd_e4"][0] == 0
    assert torch.equal(zero_f, zero_e)
    frac = float(zero_e.float().mean())
    assert drop * 0.5 < frac < 1.0                                        # (rows outside the triangle are zero as well)


def test_three_launches_give_the_same_bits(ops):
    c = case(ops, 3, 97, 0.2)
    for _ in range(3):
        dz, d_ab, _ws = backward(ops, c, c["e4"][3][0], "e4m3")
        assert torch.equal(dz, c["bwd_e4"][0]) and torch.equal(d_ab, c["bwd_e4"][1])


def test_argument_errors(ops, monkeypatch):
    from peneo_amd.hip import PeneoHipError
    c = case(ops, 1, 9, 0.0)
    B, N = 1, 9
    g = torch.Generator().manual_seed(3)
    b1, b2 = torch.zeros(NH * D, device=DEV), torch.zeros(14, device=DEV)
    wp = ops.pair_heads_pack(DT, c["w1"], c["w2"])
    nbytes = ops.pair_save_e4m3_bytes(B, N, NH, D)
    store = torch.zeros(nbytes + 16, dtype=torch.uint8, device=DEV)
    xr = torch.empty(B * ops.pair_bwd_rows(N), D, dtype=DT, device=DEV)
    real = ops.ptr

    def run_both(act, act_ptr):
        monkeypatch.setattr(ops, "ptr", lambda t: act_ptr if t is act else real(t))
        try:
            with pytest.raises(PeneoHipError, match="peneo_pair_heads_fwd_save_e4m3"):
                ops.pair_heads_fwd(c["ab"], wp, b1, b2, CLASSES, save=True, save_buffers=(act, xr), save_format="e4m3")
            with pytest.raises(PeneoHipError, match="peneo_pair_bwd_saved_e4m3"):
                backward(ops, c, act, "e4m3")
        finally:
            monkeypatch.setattr(ops, "ptr", real)

    act = store[:nbytes]
    run_both(act, None)                                                   # NULL act
    run_both(act, act.data_ptr() + 8)                                     # misaligned act (never dereferenced: refused first)
    # D = 512: no e4m3 form (nor an f16 one)
    D5 = 512
    ab5 = torch.randn(1, 9, 2 * D5, generator=g).to(DEV).to(DT)
    w15 = [(torch.randn(D5, D5, generator=g) / math.sqrt(D5)).to(DEV) for _ in CLASSES]
    w25 = [(torch.randn(k, D5, generator=g) / math.sqrt(D5)).to(DEV) for k in CLASSES]
    with pytest.raises(PeneoHipError, match="peneo_pair_heads_fwd_save_e4m3"):
        ops.pair_heads_fwd(ab5, ops.pair_heads_pack(DT, w15, w25), torch.zeros(NH * D5, device=DEV), b2, CLASSES, save=True,
                           save_format="e4m3")
    dl5 = [torch.zeros(1, 45, k, device=DEV) for k in CLASSES]
    args5 = ops.pair_dz_args(D5, CLASSES, dl5, w25, c["scale"])
    with pytest.raises(PeneoHipError, match="peneo_pair_bwd_saved_e4m3"):
        ops.pair_bwd_saved(ab5, ops.pair_bwd_pack(w15), args5, torch.zeros(1 << 20, dtype=torch.uint8, device=DEV),
                           torch.zeros(ops.pair_bwd_rows(9), NH * D5, device=DEV, dtype=DT), torch.zeros(1, 9, 2 * D5, device=DEV),
                           ops.pair_bwd_workspace(1, 9, NH, D5, DEV), act_format="e4m3")
