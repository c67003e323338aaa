"""MXFP8 train forward of the pair heads (peneo_pair_heads_fwd_mxfp8_save): x rows, dropout mask, f16 records, logits, loss rows and
dlogits against the bf16 saving forward, the eval MXFP8 kernel, the torch emulation of the MXFP8 contract and float64 formulas; the
straight-through gradients through the unchanged saved backward against fp32 autograd; canaries, repeatability, refusals."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 384
CLASSES = [2, 3, 3, 3, 3]
NH = len(CLASSES)
SEED = 77
# (B, N, p): 33 and 97 have an odd block count (the last workgroup's second block is absent), 48 and 16 an even one
# (test_pair_mxfp8_train_host.py checks the parities); every shape has diagonal and ragged blocks
SHAPES = [(2, 33, 0.1), (3, 97, 0.2), (1, 48, 0.0), (1, 16, 0.1)]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


def _inputs(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    ab = torch.randn(B, N, 2 * D, generator=g).to(DEV).to(torch.bfloat16)
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [(torch.randn(c, D, generator=g) / math.sqrt(D)).to(DEV) for c in CLASSES]
    b1 = (0.1 * torch.randn(NH * D, generator=g)).to(DEV)
    b2 = torch.randn(sum(CLASSES), generator=g).to(DEV)
    P = N * (N + 1) // 2
    tags = [torch.randint(0, c, (B, P), generator=g).to(DEV) for c in CLASSES]
    tags[1][0, :5] = -100                                    # ignored labels carry no weight
    cw = [torch.tensor([1.0, 10.0, 10.0][:c], device=DEV) for c in CLASSES]
    return ab, w1, w2, b1, b2, tags, cw


def block_rows(N):
    """block-row order of the saved buffers (common.h): per block of 8 x 16 pairs four groups of 32 rows, row r of group g =
    pair (8 ti + 2 g + (r >> 4), 16 tj + (r & 15)).  Returns (valid [rows] bool, packed pair index [rows])."""
    valid, pidx = [], []
    for ti in range((N + 7) // 8):
        for tj in range(ti >> 1, (N + 15) // 16):
            for g in range(4):
                for r in range(32):
                    i, j = 8 * ti + 2 * g + (r >> 4), 16 * tj + (r & 15)
                    ok = i < N and j < N and i <= j
                    valid.append(ok)
                    pidx.append(i * N - i * (i - 1) // 2 + (j - i) if ok else 0)
    return torch.tensor(valid, device=DEV), torch.tensor(pidx, device=DEV)


def decode_records(act, B, N):
    """act bytes -> z [B, P, NH * D] f16 by packed pair index, from the documented layout: per (document, block, 32-unit slab, group) a
    2 KiB record = [2 halves of 16 units][32 rows of 32 bytes][16 units], rows in the group's pair order, the second half's at pair ^ 4."""
    nslab = NH * D // 32
    valid, pidx = block_rows(N)
    nt = valid.numel() // 128
    rec = act[:B * nt * nslab * 4 * 2048].view(torch.float16).view(B, nt, nslab, 4, 2, 32, 16)
    swz = torch.arange(32, device=DEV) ^ 4
    z = torch.cat([rec[..., 0, :, :], rec[..., 1, :, :][..., swz, :]], dim=-1)        # [B, nt, nslab, 4, 32 pairs, 32 units]
    z = z.permute(0, 1, 3, 4, 2, 5).reshape(B, nt * 128, nslab * 32)                  # block-row order x hidden column
    P = N * (N + 1) // 2
    out = torch.empty(B, P, nslab * 32, dtype=torch.float16, device=DEV)
    out[:, pidx[valid]] = z[:, valid]
    assert int(valid.sum()) == P and pidx[valid].unique().numel() == P                # every pair exactly once
    return out


@functools.lru_cache(maxsize=None)
def case(B, N, p):
    """one shape: inputs, the kernel's outputs, the bf16 saving forward's and the float64 emulation of z - computed once, shared, never
    modified by the tests"""
    from peneo_amd import ops
    from dropout_ref import k12_keep
    from test_gpu_pair_mxfp8 import mx_emulate
    ab, w1, w2, b1, b2, tags, cw = _inputs(B, N, 1000 * N + B)
    wpm = ops.pair_heads_pack_mxfp8(w1, w2)
    kw = dict(tags=tags, class_weights=cw, want_dlogits=True, want_logits=True, drop_p=p, drop_seed=SEED)
    lg, pt, dl, (act, xr) = ops.pair_heads_fwd_mxfp8_save(ab, wpm, b1, b2, CLASSES, **kw)
    wp = ops.pair_heads_pack(torch.bfloat16, w1, w2)
    _, _, _, (act16, xr16) = ops.pair_heads_fwd(ab, wp, b1, b2, CLASSES, save=True, **kw)
    torch.cuda.synchronize()
    P = N * (N + 1) // 2
    keep = torch.stack([k12_keep(SEED, b, 0, P, NH * D, p) for b in range(B)]).to(DEV)
    ii, jj = torch.triu_indices(N, N, device=DEV)
    x = F.silu(ab.float()[:, ii, :D] + ab.float()[:, jj, D:])
    xq = mx_emulate(x)[2]
    wq = torch.cat([mx_emulate(w.float())[2] for w in w1])                             # [NH * D, D] float64
    z64 = xq @ wq.t() + b1.double()
    return dict(ab=ab, w1=w1, w2=w2, b1=b1, b2=b2, tags=tags, cw=cw, wpm=wpm, kw=kw, lg=lg, pt=pt, dl=dl, act=act, xr=xr,
                act16=act16, xr16=xr16, keep=keep, z64=z64, z=decode_records(act, B, N), z16=decode_records(act16, B, N), P=P)


# ---- 1. x rows and mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,p", SHAPES)
def test_x_rows_and_mask_are_those_of_the_bf16_saving_forward(B, N, p):
    c = case(B, N, p)
    assert torch.equal(c["xr"], c["xr16"])
    dropped = c["z"].float() <= -20000
    assert torch.equal(dropped, ~c["keep"])
    assert torch.equal(dropped, c["z16"].float() <= -20000)
    if p > 0:
        frac = float(dropped.float().mean())
        assert abs(frac - p) < 0.01, frac
    else:
        assert not bool(dropped.any())


# ---- 2. records --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,p", SHAPES)
def test_records_hold_the_emulated_preactivation(B, N, p):
    """f16 keeps 11 significant bits (2^-11 |z| rounding); one more bit covers the fp32 accumulation order: 2^-10 |z| + 2^-10"""
    c = case(B, N, p)
    z, want, keep = c["z"].double(), c["z64"], c["keep"]
    assert bool(torch.isfinite(z).all())
    err = (z - want).abs()[keep]
    bound = (2.0 ** -10 * want.abs() + 2.0 ** -10)[keep]
    worst = float((err / bound).max())
    print(f"records B={B} N={N} p={p}: max |err| / bound = {worst:.3f}, max |z| = {float(want.abs().max()):.2f}")
    assert worst <= 1.0, worst


# ---- 3. bit-identity with the eval kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 48), (2, 33)])
def test_without_dropout_the_logits_are_the_eval_kernels(ops, B, N):
    """the same arithmetic per pair on another walk of the triangle (even and odd block counts)"""
    ab, w1, w2, b1, b2, tags, cw = _inputs(B, N, 1000 * N + B)
    wpm = ops.pair_heads_pack_mxfp8(w1, w2)
    lg = ops.pair_heads_fwd_mxfp8_save(ab, wpm, b1, b2, CLASSES, drop_p=0.0)[0]
    ev, _, _ = ops.pair_heads_fwd_mxfp8(ab, wpm, b1, b2, CLASSES)
    for h in range(NH):
        assert torch.equal(lg[h], ev[h]), h


# ---- 4. logits with dropout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,p", SHAPES)
def test_logits_match_the_emulation_with_mask_and_scale(B, N, p):
    from dropout_ref import k12_scale
    from test_gpu_pair_mxfp8 import check_close
    c = case(B, N, p)
    s = k12_scale(p)
    want, off = [], 0
    for h, cl in enumerate(CLASSES):
        y = F.silu(c["z64"][..., h * D:(h + 1) * D].float()).to(torch.bfloat16).float() * c["keep"][..., h * D:(h + 1) * D]
        want.append((y @ c["w2"][h].to(torch.bfloat16).float().t()) * s + c["b2"][off:off + cl])
        off += cl
    # the bounds of check_close times the dropout scale (errors of the second layer's sums scale with it)
    check_close([g_ / s for g_ in c["lg"]], [w_ / s for w_ in want])


# ---- 5. loss rows and dlogits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,p", SHAPES)
def test_loss_rows_and_dlogits_follow_the_kernels_logits(ops, B, N, p):
    c = case(B, N, p)
    assert c["pt"].shape == (ops.lib().peneo_pair_loss_partials_save(B, N), 32)
    tot = c["pt"].double().sum(0)
    for h, cl in enumerate(CLASSES):
        lg, tg, cw = c["lg"][h].double(), c["tags"][h], c["cw"][h].double()
        want = F.cross_entropy(lg.reshape(-1, cl), tg.reshape(-1), weight=cw, reduction="sum", ignore_index=-100)
        den = cw[tg[tg >= 0]].sum()
        assert abs(float(tot[h]) - float(want)) <= 1e-4 * abs(float(want))
        assert abs(float(tot[8 + h]) - float(den)) <= 1e-4 * float(den)
        ok = tg >= 0
        w = torch.where(ok, cw[tg.clamp_min(0)], torch.zeros((), dtype=torch.float64, device=DEV))
        onehot = F.one_hot(tg.clamp_min(0), cl).double() * ok[..., None]
        dl = w[..., None] * (torch.softmax(lg, -1) - onehot)
        assert float((c["dl"][h].double() - dl).abs().max()) <= 2e-5 * float(cw.max())
        assert float(c["dl"][h][~ok].abs().max() if bool((~ok).any()) else 0.0) == 0.0


# ---- 6. gradients through the unchanged saved backward -----------------------------------------------------------------------
def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


@pytest.mark.parametrize("B,N,p", [(2, 33, 0.1), (1, 70, 0.0)])
def test_saved_backward_gives_straight_through_gradients(ops, B, N, p):
    """peneo_pair_bwd_saved on the MXFP8 forward's buffers, the dW1 GEMM and pair_dz_finish against fp32 autograd of
    z = W1 x + b1 + (z_emulated - (W1 x + b1)).detach(): the oracle of test_pair_bwd_fused_matches_autograd with that z."""
    from dropout_ref import k12_keep, k12_scale
    from test_gpu_pair_mxfp8 import mx_emulate
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(B * 100000 + N * 1000 + D)
    ab = torch.randn(B, N, 2 * D, generator=g).to(DEV).to(dtype)
    P = N * (N + 1) // 2
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [torch.randn(c, D, generator=g).to(DEV) for c in CLASSES]
    b1cat = (0.1 * torch.randn(NH * D, generator=g)).to(DEV)
    b2 = torch.zeros(sum(CLASSES), device=DEV)
    dl = [torch.randn(B, P, c, generator=g).to(DEV) for c in CLASSES]
    scale = torch.rand(NH, generator=g).to(DEV) + 0.5
    seed = 4242 + N
    rows = ops.pair_bwd_rows(N)
    wpm = ops.pair_heads_pack_mxfp8(w1, w2)
    _, _, _, (act, xrows) = ops.pair_heads_fwd_mxfp8_save(ab, wpm, b1cat, b2, CLASSES, want_logits=False, drop_p=p, drop_seed=seed)
    wp2 = ops.pair_bwd_pack(w1)
    args = ops.pair_dz_args(D, CLASSES, dl, w2, scale, drop_p=p, drop_seed=seed)
    dz = torch.full((B * rows, NH * D), 7.0, device=DEV, dtype=dtype)
    d_ab = torch.full((B, N, 2 * D), 5.0, device=DEV)
    ws = ops.pair_dz_workspace(NH, D, DEV, slots=256)
    ops.pair_bwd_saved(ab, wp2, args, act, dz, d_ab, ws)
    dW1 = ops.gemm(dz, xrows, a_kmajor=False, b_kmajor=False, out_dtype=torch.float32)
    dw2, db1 = ops.pair_dz_finish(ws, NH, D, CLASSES)
    torch.cuda.synchronize()
    # fp32 autograd (bf16-rounded operands where the backward rounds: ab, x, W1), the forward value of z replaced by the emulation
    abr = ab.float().clone().requires_grad_(True)
    ii, jj = torch.triu_indices(N, N, device=DEV)
    xr = F.silu(abr[:, ii, :D] + abr[:, jj, D:])
    xq = xr + (xr.detach().to(dtype).float() - xr.detach())
    xmx = mx_emulate(xr.detach())[2]
    w1r = [w.to(dtype).float().clone().requires_grad_(True) for w in w1]
    w2r = [w.clone().requires_grad_(True) for w in w2]
    b1r = b1cat.clone().requires_grad_(True)
    keep_all = torch.stack([k12_keep(seed, b, 0, P, NH * D, p) for b in range(B)]).to(DEV) if p > 0 else None
    for h in range(NH):
        zlin = xq @ w1r[h].t() + b1r[h * D:(h + 1) * D]
        zemu = ((xmx @ mx_emulate(w1[h])[2].t()) + b1cat[h * D:(h + 1) * D].double()).float()
        z = zlin + (zemu - zlin.detach())
        y = F.silu(z)
        if p > 0:
            y = y * keep_all[:, :, h * D:(h + 1) * D] * k12_scale(p)
        (((y @ w2r[h].t()) * dl[h] * scale[h]).sum()).backward(retain_graph=h + 1 < NH)
        del z, y, zlin, zemu
    t = 3e-2
    errs = dict(d_ab=rel_err(d_ab, abr.grad), db1=rel_err(db1, b1r.grad),
                dw2=max(rel_err(dw2[h], w2r[h].grad) for h in range(NH)),
                dW1=max(rel_err(dW1[h * D:(h + 1) * D], w1r[h].grad) for h in range(NH)))
    print(f"gradients B={B} N={N} p={p}:", errs)
    assert all(v < t for v in errs.values()), errs


# ---- the C entry point directly ----------------------------------------------------------------------------------------------
def _raw_save(ab, wp, b1, b2, *, D_=D, drop_p=0.0, loss=None, act=None, x_rows=None, logits=None):
    """peneo_pair_heads_fwd_mxfp8_save through the C ABI: (return code, peneo_last_error)"""
    from peneo_amd import hip
    B, N, _ = ab.shape
    desc = hip.PairHeadsDesc()
    desc.num_heads, desc.D = NH, D_
    for h, c in enumerate(CLASSES):
        desc.classes[h] = c
    desc.w_packed, desc.b1, desc.b2 = hip.ptr(wp), hip.ptr(b1), hip.ptr(b2)
    desc.drop_p, desc.drop_seed = drop_p, SEED
    pl = None
    if loss is not None:
        tags, cw, dlog, partials = loss
        pl = hip.PairLoss()
        for h in range(NH):
            pl.tags[h] = hip.ptr(tags[h])
            pl.class_weight[h] = hip.ptr(cw[h])
            pl.dlogits[h] = hip.ptr(dlog[h])
        pl.partials = hip.ptr(partials)
    lp = None
    if logits is not None:
        lp = (ctypes.c_void_p * NH)(*[hip.ptr(t) for t in logits])
    rc = hip.lib().peneo_pair_heads_fwd_mxfp8_save(hip.ptr(ab), B, N, ctypes.byref(desc), lp,
                                                   ctypes.byref(pl) if pl is not None else None,
                                                   hip.ptr(act) if act is not None else None,
                                                   hip.ptr(x_rows) if x_rows is not None else None, hip.stream())
    return rc, (hip.lib().peneo_last_error() or b"").decode()


# ---- 7. canaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,p", [(2, 33, 0.1), (1, 48, 0.0)])
def test_nothing_is_written_behind_the_buffers(ops, B, N, p):
    c = case(B, N, p)
    P, rows, PAD = c["P"], ops.pair_bwd_rows(N), 4096
    nact = ops.pair_save_bytes(B, N, NH, D)
    act = torch.full((nact + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    xr = torch.full((B * rows * D + PAD,), 7.0, dtype=torch.bfloat16, device=DEV)
    npart = ops.lib().peneo_pair_loss_partials_save(B, N)
    part = torch.full((npart * 32 + PAD,), 7.0, device=DEV)
    dlog = [torch.full((B * P * cl + PAD,), 7.0, device=DEV) for cl in CLASSES]
    lgt = [torch.full((B * P * cl + PAD,), 7.0, device=DEV) for cl in CLASSES]
    rc, msg = _raw_save(c["ab"], c["wpm"], c["b1"], c["b2"], drop_p=p, loss=(c["tags"], c["cw"], dlog, part), act=act, x_rows=xr,
                        logits=lgt)
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool((act[nact:] == 0xA5).all()) and bool((xr[B * rows * D:] == 7.0).all()) and bool((part[npart * 32:] == 7.0).all())
    for h, cl in enumerate(CLASSES):
        assert bool((dlog[h][B * P * cl:] == 7.0).all()) and bool((lgt[h][B * P * cl:] == 7.0).all())
        # ... and what lies in front of the canaries is the op's result
        assert torch.equal(dlog[h][:B * P * cl].view(B, P, cl), c["dl"][h]) and torch.equal(lgt[h][:B * P * cl].view(B, P, cl), c["lg"][h])
    assert torch.equal(act[:nact], c["act"][:nact]) and torch.equal(xr[:B * rows * D].view(B * rows, D), c["xr"])
    assert torch.equal(part[:npart * 32].view(npart, 32), c["pt"])


# ---- 8. repeatability --------------------------------------------------------------------------------------------------------
def test_three_launches_are_bit_identical(ops):
    B, N, p = 3, 97, 0.2
    c = case(B, N, p)
    for _ in range(2):                                       # the shared case was the first launch
        lg, pt, dl, (act, xr) = ops.pair_heads_fwd_mxfp8_save(c["ab"], c["wpm"], c["b1"], c["b2"], CLASSES, **c["kw"])
        assert torch.equal(pt, c["pt"]) and torch.equal(act, c["act"]) and torch.equal(xr, c["xr"])
        assert all(torch.equal(a, b_) for a, b_ in zip(lg + dl, c["lg"] + c["dl"]))


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_unsupported_arguments_are_refused(ops):
    c = case(1, 16, 0.1)
    ab, wpm, b1, b2 = c["ab"], c["wpm"], c["b1"], c["b2"]
    act, xr = torch.empty_like(c["act"]), torch.empty_like(c["xr"])
    rc, msg = _raw_save(ab, wpm, b1, b2, act=None, x_rows=xr)
    assert rc == -1 and "act" in msg, (rc, msg)                              # PENEO_ERR_INVALID
    rc, msg = _raw_save(ab, wpm, b1, b2, act=act, x_rows=None)
    assert rc == -1 and "x_rows" in msg, (rc, msg)
    rc, msg = _raw_save(ab, wpm, b1, b2, drop_p=1.0, act=act, x_rows=xr)
    assert rc == -1 and "drop_p" in msg, (rc, msg)
    # D = 512: the MXFP8 kernel holds it, the saved backward does not
    g = torch.Generator().manual_seed(1)
    ab512 = torch.randn(1, 16, 1024, generator=g).to(DEV).to(torch.bfloat16)
    w1 = [torch.randn(512, 512, generator=g).to(DEV) for _ in CLASSES]
    w2 = [torch.randn(cl, 512, generator=g).to(DEV) for cl in CLASSES]
    wp512 = ops.pair_heads_pack_mxfp8(w1, w2)
    b1_512 = torch.zeros(NH * 512, device=DEV)
    big = torch.empty(ops.pair_save_bytes(1, 16, NH, 512), dtype=torch.uint8, device=DEV)
    xr512 = torch.empty(ops.pair_bwd_rows(16), 512, dtype=torch.bfloat16, device=DEV)
    rc, msg = _raw_save(ab512, wp512, b1_512, b2, D_=512, act=big, x_rows=xr512)
    assert rc == -1 and "not supported" in msg, (rc, msg)
    with pytest.raises(ValueError):
        ops.pair_heads_fwd_mxfp8_save(ab512, wp512, b1_512, b2, CLASSES)
    # a bf16 pack: the C entry point takes a pointer without a size and cannot tell (include/peneo_hip.h says so); the Python op
    # knows the buffer's size and refuses
    wp16 = ops.pair_heads_pack(torch.bfloat16, c["w1"], c["w2"])
    assert wp16.numel() != wpm.numel()
    with pytest.raises(ValueError):
        ops.pair_heads_fwd_mxfp8_save(ab, wp16, b1, b2, CLASSES)
    # the same call with everything in place is accepted
    rc, msg = _raw_save(ab, wpm, b1, b2, drop_p=0.1, act=act, x_rows=xr)
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert torch.equal(act, c["act"]) and torch.equal(xr, c["xr"])
