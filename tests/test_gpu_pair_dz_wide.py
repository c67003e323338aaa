"""peneo_pair_dz_fused at decoder widths 512 < D <= 1024 (pair_dz_wide.hip; bf16, four waves, 256 pairs a workgroup in two rounds of
128), op level: what test_pair_dz_fused_matches_the_gemm_epilogue (test_gpu_kernels.py) asks of the narrower kernel, at (N, D, rows)
    (33, 768, (0, 33))     561 pairs: two full workgroups + one with a full wave, a 17-pair wave, two empty waves, no second round
    (40, 768, (5, 17))     354 pairs: a chunk that starts mid-triangle, a partial second workgroup, a non-zero first pair for the mask
    (47, 768, (46, 47))    a single pair
    (71, 960, (0, 71))     2556 pairs: KS = 60, a ragged second round
    (70, 1024, (0, 70))    2485 pairs: the register and LDS ceiling
    (362, 768, (0, 362))   65 703 pairs: 257 workgroups, so workspace rows are shared modulo 256 (against the GEMM chain only)
References are computed once per case and never modified.  2e-2 is tol(bf16) of test_gpu_kernels.py."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = torch.bfloat16
CLASSES = [2, 3, 3, 3, 3]
NH = len(CLASSES)
SMALL = [(33, 768, (0, 33)), (40, 768, (5, 17)), (47, 768, (46, 47)), (71, 960, (0, 71)), (70, 1024, (0, 70))]
BIG = (362, 768, (0, 362))
CASES = SMALL + [BIG]
TOL = 2e-2
P_DROP, DROP_DOC, DROP_SEED = 0.1, 3, 77


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _autograd(xq, w1cat, b1cat, w2, dl, scale, D, keep=None):
    """fp32 autograd of the block on bf16-rounded operands: (dz, db1, [dW2_h])"""
    zr = (xq @ w1cat.float().t() + b1cat).requires_grad_(True)
    w2r = [w.clone().requires_grad_(True) for w in w2]
    tot = 0
    for h in range(NH):
        y = F.silu(zr[:, h * D:(h + 1) * D])
        if keep is not None:
            y = y * keep[:, h * D:(h + 1) * D]
        tot = tot + ((y @ w2r[h].t()) * dl[h] * scale[h]).sum()
    tot.backward()
    return zr.grad, zr.grad.sum(0), [w.grad for w in w2r]


@functools.lru_cache(maxsize=None)
def _case(N, D, rows):
    from peneo_amd import ops
    from dropout_ref import k12_keep, k12_scale
    g = torch.Generator().manual_seed(N * 1000 + D)
    ab = torch.randn(N, 2 * D, generator=g).to(DEV).to(DT)
    i0, i1 = rows
    p0, p1 = i0 * N - i0 * (i0 - 1) // 2, i1 * N - i1 * (i1 - 1) // 2
    npairs = p1 - p0
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [torch.randn(c, D, generator=g).to(DEV) for c in CLASSES]
    b1cat = (0.1 * torch.randn(NH * D, generator=g)).to(DEV)
    dl = [torch.randn(npairs, c, generator=g).to(DEV) for c in CLASSES]
    scale = torch.rand(NH, generator=g).to(DEV) + 0.5
    w1cat = torch.cat(w1).to(DT)
    wp = ops.pair_heads_pack(DT, w1, w2)
    c = dict(N=N, D=D, i0=i0, i1=i1, p0=p0, npairs=npairs, ab=ab, w2=w2, b1cat=b1cat, dl=dl, scale=scale, wp=wp)
    # the chain the kernel replaces: pair_x_fwd + the z GEMM with the pair_dz epilogue
    args = ops.pair_dz_args(D, CLASSES, dl, w2, scale)
    x = torch.empty(npairs, D, device=DEV, dtype=DT)
    pre = torch.empty_like(x)
    ops.pair_x_fwd(ab, i0, i1, x, pre)
    ws_a = ops.pair_dz_workspace(NH, D, DEV)
    za = torch.empty(npairs, NH * D, device=DEV, dtype=DT)
    ops.gemm(x, w1cat, bias=b1cat, out=za, pair_dz=args, pair_dz_ws=ws_a)
    dw2a, db1a = ops.pair_dz_finish(ws_a, NH, D, CLASSES)
    c.update(x=x, pre=pre, za=za, dw2a=dw2a, db1a=db1a)
    if (N, D, rows) != BIG:
        abf = ab.float()
        ii, jj = torch.triu_indices(N, N, device=DEV)
        xq = F.silu(abf[ii, :D] + abf[jj, D:])[p0:p1].to(DT).float()          # the kernel keeps x as bf16 fragments
        c["ref"] = _autograd(xq, w1cat, b1cat, w2, dl, scale, D)
        keep = k12_keep(DROP_SEED, DROP_DOC, p0, p1, NH * D, P_DROP).to(DEV)
        c["keep"] = keep
        c["ref_drop"] = _autograd(xq, w1cat, b1cat, w2, dl, scale, D, keep.float() * k12_scale(P_DROP))
    torch.cuda.synchronize()
    return c


def _launch(ops, c, x_out=False, rows=None, **drop):
    """one launch into guarded buffers: (dz with 3 guard rows, workspace, x, pre with 2 guard rows each or None)"""
    npairs, D = c["npairs"], c["D"]
    args = ops.pair_dz_args(D, CLASSES, c["dl"], c["w2"], c["scale"], **drop)
    ws = torch.zeros((rows, 4 * NH * D), dtype=torch.float32, device=DEV) if rows else ops.pair_dz_workspace(NH, D, DEV, slots=256)
    dz = torch.full((npairs + 3, NH * D), 7.0, device=DEV, dtype=DT)
    xo = torch.full((npairs + 2, D), 3.0, device=DEV, dtype=DT) if x_out else None
    po = torch.full((npairs + 2, D), 3.0, device=DEV, dtype=DT) if x_out else None
    ops.pair_dz_fused(c["ab"], c["i0"], c["i1"], c["wp"], c["b1cat"], args, dz, ws, xo, po)
    torch.cuda.synchronize()
    return dz, ws, xo, po


@pytest.mark.parametrize("N,D,rows", CASES)
def test_wide_dz_matches_the_gemm_chain_and_autograd(ops, N, D, rows):
    c = _case(N, D, rows)
    npairs = c["npairs"]
    assert ops.pair_dz_fused_supported(DT, D, NH)
    dz, ws, _, _ = _launch(ops, c)
    assert bool((dz[npairs:] == 7.0).all()), "guard rows behind dz were written"
    dw2, db1 = ops.pair_dz_finish(ws, NH, D, CLASSES)
    e_dz, e_db1 = rel_err(dz[:npairs], c["za"]), rel_err(db1, c["db1a"])
    e_dw2 = max(rel_err(dw2[h], c["dw2a"][h]) for h in range(NH))
    print(f"({N}, {D}, {rows}) {npairs} pairs, against the GEMM chain: dz {e_dz:.3e} db1 {e_db1:.3e} dW2 {e_dw2:.3e}")
    assert e_dz < TOL and e_db1 < TOL and e_dw2 < TOL, (e_dz, e_db1, e_dw2)
    if "ref" in c:
        rdz, rdb1, rdw2 = c["ref"]
        f_dz, f_db1 = rel_err(dz[:npairs], rdz), rel_err(db1, rdb1)
        f_dw2 = max(rel_err(dw2[h], rdw2[h]) for h in range(NH))
        print(f"({N}, {D}, {rows}) against fp32 autograd: dz {f_dz:.3e} db1 {f_db1:.3e} dW2 {f_dw2:.3e}")
        assert f_dz < TOL and f_db1 < TOL and f_dw2 < TOL, (f_dz, f_db1, f_dw2)
    # the same call can leave x and a_i + b_j, bit for bit what pair_x_fwd writes; dz does not change
    dz2, ws2, xo, po = _launch(ops, c, x_out=True)
    assert torch.equal(dz2, dz)
    assert torch.equal(xo[:npairs], c["x"]) and torch.equal(po[:npairs], c["pre"])
    assert bool((xo[npairs:] == 3.0).all()) and bool((po[npairs:] == 3.0).all()), "guard rows behind x / pre were written"
    dw2x, db1x = ops.pair_dz_finish(ws2, NH, D, CLASSES)
    assert rel_err(db1x, c["db1a"]) < TOL


@pytest.mark.parametrize("N,D,rows", SMALL)
def test_wide_dz_regenerates_the_k12_mask(ops, N, D, rows):
    """drop_p = 0.1, document 3, the chunk's first pair: the elements the host mask drops are exactly 0, dz and the sums match
    autograd with the host mask and scale, another seed gives another mask."""
    c = _case(N, D, rows)
    npairs, keep = c["npairs"], c["keep"]
    dz, ws, _, _ = _launch(ops, c, drop_p=P_DROP, drop_seed=DROP_SEED, drop_doc=DROP_DOC, drop_pair0=c["p0"])
    assert bool((dz[npairs:] == 7.0).all())
    dz = dz[:npairs]
    assert bool((dz[~keep] == 0).all()), "a dropped element is not zero"
    dw2, db1 = ops.pair_dz_finish(ws, NH, D, CLASSES)
    rdz, rdb1, rdw2 = c["ref_drop"]
    e_dz, e_db1 = rel_err(dz, rdz), rel_err(db1, rdb1)
    e_dw2 = max(rel_err(dw2[h], rdw2[h]) for h in range(NH))
    print(f"({N}, {D}, {rows}) with the K12 mask, against fp32 autograd: dz {e_dz:.3e} db1 {e_db1:.3e} dW2 {e_dw2:.3e}")
    assert e_dz < TOL and e_db1 < TOL and e_dw2 < TOL, (e_dz, e_db1, e_dw2)
    other, _, _, _ = _launch(ops, c, drop_p=P_DROP, drop_seed=DROP_SEED + 1, drop_doc=DROP_DOC, drop_pair0=c["p0"])
    assert not torch.equal(other[:npairs] == 0, dz == 0)
    # the mask is a function of the pair's place in the document: another first pair moves it
    if npairs > 1:
        moved, _, _, _ = _launch(ops, c, drop_p=P_DROP, drop_seed=DROP_SEED, drop_doc=DROP_DOC, drop_pair0=c["p0"] + 1)
        assert bool((moved[:npairs - 1][~keep[1:]] == 0).all())


@pytest.mark.parametrize("N,D,rows", [SMALL[0], SMALL[3], BIG])
def test_three_identical_launches(ops, N, D, rows):
    """Mode 0: dz is bit-identical, the sums agree up to the order of the fp32 atomics (rows shared modulo 256 in the large case).
    peneo_set_deterministic(1): every workgroup has its own workspace row and adds to each address of it twice, from one lane in
    program order - a single writer in a fixed order: the workspace bits repeat too, and the call is not counted as order-dependent."""
    from peneo_amd import hip
    c = _case(N, D, rows)
    npairs = c["npairs"]
    before = hip.deterministic_mode()
    try:
        hip.set_deterministic(0)
        dz0, ws0, _, _ = _launch(ops, c)
        s0 = ws0.sum(0)
        for _ in range(2):
            dz, ws, _, _ = _launch(ops, c)
            assert torch.equal(dz, dz0)
            # at most 4 + 256 fp32 adds per column in another order: 260 x 2^-24 = 1.6e-5 of the largest partial sum at the very worst
            assert rel_err(ws.sum(0), s0) < 1e-4
        hip.set_deterministic(1)
        nrows = ops.pair_dz_fused_workspace_rows(npairs)
        assert nrows == max(256, -(-npairs // 256))
        counted = hip.order_dependent_launches()
        dz1, ws1, _, _ = _launch(ops, c, rows=nrows)
        for _ in range(2):
            dz, ws, _, _ = _launch(ops, c, rows=nrows)
            assert torch.equal(dz, dz1) and torch.equal(ws, ws1)
        assert hip.order_dependent_launches() == counted
        assert torch.equal(dz1, dz0)
        used = -(-npairs // 256)
        assert bool((ws1[used:] == 0).all()) and bool((ws1[:used] != 0).any(dim=1).all())   # a row per workgroup, no other
        assert rel_err(ws1.sum(0), s0) < 1e-4
    finally:
        hip.set_deterministic(before)


def test_refusals_name_the_entry_point(ops):
    from peneo_amd import hip
    c = _case(*SMALL[0])
    N, D, npairs = c["N"], c["D"], c["npairs"]
    args = ops.pair_dz_args(D, CLASSES, c["dl"], c["w2"], c["scale"])
    dz = torch.empty(npairs, NH * D, device=DEV, dtype=DT)
    ws = ops.pair_dz_workspace(NH, D, DEV, slots=256)
    xo = torch.empty(npairs, D, device=DEV, dtype=DT)
    with pytest.raises(hip.PeneoHipError, match="peneo_pair_dz_fused.*bf16 only"):
        ops.pair_dz_fused(c["ab"].float(), 0, N, c["wp"], c["b1cat"], args, dz, ws)
    with pytest.raises(hip.PeneoHipError, match="peneo_pair_dz_fused.*come together"):
        ops.pair_dz_fused(c["ab"], 0, N, c["wp"], c["b1cat"], args, dz, ws, xo, None)
    flat = torch.zeros(N * 2 * D + 8, device=DEV, dtype=DT)
    skew = flat[1:1 + N * 2 * D].view(N, 2 * D)                 # 2 bytes off a 16-byte boundary
    with pytest.raises(hip.PeneoHipError, match="peneo_pair_dz_fused.*16-byte aligned"):
        ops.pair_dz_fused(skew, 0, N, c["wp"], c["b1cat"], args, dz, ws)
    # D = 800: a multiple of 32 but in neither family of widths (nothing is launched: the buffers are never read)
    D8 = 800
    assert not ops.pair_dz_fused_supported(DT, D8, NH)
    ab8 = torch.zeros(N, 2 * D8, device=DEV, dtype=DT)
    w28 = [torch.zeros(k, D8, device=DEV) for k in CLASSES]
    args8 = ops.pair_dz_args(D8, CLASSES, c["dl"], w28, c["scale"])
    with pytest.raises(hip.PeneoHipError, match="peneo_pair_dz_fused: D=800 not supported.*512 < D <= 1024"):
        ops.pair_dz_fused(ab8, 0, N, c["wp"], torch.zeros(NH * D8, device=DEV), args8,
                          torch.empty(npairs, NH * D8, device=DEV, dtype=DT), torch.zeros(256, 4 * NH * D8, device=DEV))
    torch.cuda.synchronize()
