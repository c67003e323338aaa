"""Deterministic mode, kernel by kernel.  For every order-dependent site of the covered path, under mode 2: three
launches on the same inputs are torch.equal, the counter of order-dependent launches does not move (and moves for the same call under
mode 0: a result cannot tell which kernel ran), and the result meets the reference and the tolerance that the test of the default
form in tests/test_gpu_kernels.py uses (named in each docstring) or, where no such test exists, a float64 sum with the derivable
bound n 2^-23 sum|x| per output (+ n 2^-32 for the fixed-point form).  The three strict refusals get one call each."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


@pytest.fixture(autouse=True)
def _restore_mode():
    from peneo_amd import hip
    before = hip.deterministic_mode()
    yield
    hip.set_deterministic(before)


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def both_modes(fn):
    """fn() -> tensors.  Runs it three times under mode 2 (equal bits, counter still) and once under mode 0 (counter moves);
    -> (mode-2 result, mode-0 result)."""
    import peneo_amd
    from peneo_amd import hip
    with peneo_amd.deterministic(2):
        c0 = hip.order_dependent_launches()
        runs = [fn() for _ in range(3)]
        torch.cuda.synchronize()
        assert hip.order_dependent_launches() == c0, "an order-dependent path ran under mode 2"
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2]), "not bit-reproducible under mode 2"
    with peneo_amd.deterministic(0):
        c0 = hip.order_dependent_launches()
        default = fn()
        torch.cuda.synchronize()
        assert hip.order_dependent_launches() > c0, "the default form did not count itself as order-dependent"
    return runs[0], default


def sum_bound(terms, n, fixed_point=False):
    """n 2^-23 sum|x| per output (float32 sums of n terms in any order), + n 2^-32 for the 2^-32 fixed-point grid"""
    b = n * 2.0 ** -23 * terms.double().abs().sum(0)
    return b + n * 2.0 ** -32 if fixed_point else b


# ---------------------------------------------------------------------------------------------- column sum
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [8, 100, 776])
@pytest.mark.parametrize("M", [1, 129, 1030])
def test_colsum(ops, dtype, M, N):
    """Reference and tolerance of test_cast_copy_colsum (rel_err against the fp32 torch sum < 1e-4), and the float64 bound.  One row,
    just past one 128-row block, ragged past two 512-row blocks; one vector, the scalar kernel (N % 8 != 0), just past a 256-column
    block; a row stride larger than N; accumulate onto a non-zero out."""
    g = torch.Generator().manual_seed(1000 * M + N)
    big = torch.randn(M, N + 24, generator=g).to(DEV).to(dtype)
    x = big[:, 8:8 + N]                                      # row stride N + 24
    assert x.stride(0) > N
    base = torch.randn(N, generator=g).to(DEV)

    def run():
        plain = ops.colsum(x)
        acc = base.clone()
        ops.colsum(x, out=acc, accumulate=True)
        return plain, acc
    (plain, acc), (plain0, acc0) = both_modes(run)
    ref64 = x.double().sum(0)
    assert rel_err(plain, x.float().sum(0)) < 1e-4 and rel_err(acc, base + x.float().sum(0)) < 1e-4
    bound = sum_bound(x, M) + 1e-30
    assert bool(((plain.double() - ref64).abs() <= bound).all()), float(((plain.double() - ref64).abs() / bound).max())
    assert bool(((acc.double() - (base.double() + ref64)).abs() <= bound + 2.0 ** -23 * (base.double() + ref64).abs()).all())
    assert rel_err(plain0, x.float().sum(0)) < 1e-4          # (the default form, same call)


# ---------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [64, 192, 768, 1024])
@pytest.mark.parametrize("rows", [1, 33, 700])
def test_layernorm_bwd(ops, dtype, rows, H):
    """dgamma / dbeta against fp32 autograd of F.layer_norm at rel_err < 5e-4 (test_layernorm_fwd_bwd), accumulated onto non-zero
    buffers; with the options the model passes (dx_dropped + drop2, dx_colsum) the column sums against the sums of the stored tensor
    at test_layernorm_bwd_column_sums_of_the_dropped_output's tolerance; dx and dx_dropped are the default form's bits."""
    g = torch.Generator().manual_seed(rows * 10000 + H)
    x = (torch.randn(rows, H, generator=g) * 2 + 0.3).to(DEV).to(dtype)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(H, generator=g)).to(DEV)
    dy = torch.randn(rows, H, generator=g).to(DEV).to(dtype)
    g0, b0 = torch.randn(H, generator=g).to(DEV), torch.randn(H, generator=g).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-5)
    xr = x.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    F.layer_norm(xr, (H,), gr, br, 1e-5).backward(dy.float())

    def run():
        dg, db = g0.clone(), b0.clone()
        dx = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db)
        dg2, db2, col = g0.clone(), b0.clone(), torch.full((H,), 0.5, device=DEV)
        dxd = torch.empty_like(x)
        dx2 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg2, db2, dx_dropped=dxd, drop2_p=0.2, drop2_seed=9, dx_colsum=col)
        col1 = torch.full((H,), 0.5, device=DEV)
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, g0.clone(), b0.clone(), dx_colsum=col1)
        return dg, db, dx, dg2, db2, dx2, dxd, col, col1
    det, default = both_modes(run)
    dg, db, dx, dg2, db2, dx2, dxd, col, col1 = det
    # (the norm of rel_err is the reference's largest entry: one row has no sum to speak of, so hold it to the same figure)
    assert rel_err(dg - g0, gr.grad) < 5e-4 and rel_err(db - b0, br.grad) < 5e-4
    assert torch.equal(dg, dg2) and torch.equal(db, db2)
    assert torch.equal(dx, default[2]) and torch.equal(dx2, default[5]) and torch.equal(dxd, default[6]) and torch.equal(dx, dx2)
    for c, src in ((col, dxd), (col1, dx)):
        ref = src.float().sum(0) + 0.5
        scale = float(src.float().abs().sum(0).max())
        assert float((c - ref).abs().max()) < (2e-5 if dtype == torch.float32 else 6e-3) * scale + 1e-6, (rows, H)
    assert rel_err(default[0] - g0, gr.grad) < 5e-4


def test_layernorm_bwd_in_place_and_with_the_input_dropout(ops):
    """dx may alias dy (include/peneo_hip.h): the deterministic form reads dy for dgamma / dbeta before the row kernel overwrites
    it.  With drop_p (the embedding LayerNorms) the column kernel regenerates the row kernel's mask: the same sums as the default
    form up to summation order (test_layernorm_dropout_fwd_bwd_share_the_mask compares at tol(dtype) = 2e-2 for bf16)."""
    rows, H = 300, 768
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, H, generator=g).to(DEV).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    dy = torch.randn(rows, H, generator=g).to(DEV).to(torch.bfloat16)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, torch.zeros(H, device=DEV), 1e-5)

    def run():
        dg, db = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        buf = dy.clone()
        dx = ops.layernorm_bwd(buf, x, gamma, mean, rstd, dg, db, dx=buf, drop_p=0.3, drop_seed=11)
        return dg, db, dx
    (dg, db, dx), (dg0, db0, dx0) = both_modes(run)
    assert torch.equal(dx, dx0)
    assert rel_err(dg, dg0) < 1e-4 and rel_err(db, db0) < 1e-4


# ---------------------------------------------------------------------------------------------- embedding tables
def _embed_inputs(H):
    B, S, V = 2, 40, 50
    g = torch.Generator().manual_seed(H)
    vals = torch.tensor([1, 7, 8, 9, 23, 41])                               # the pad id and five others: every table row collides
    ids = vals[torch.randint(0, 6, (B, S), generator=g)]
    ids[1, 30:] = 1
    boxes = torch.tensor([[10, 20, 110, 40], [10, 60, 300, 75], [110, 20, 300, 40]])   # three boxes; 110 / 300 are left of one, right of another
    bbox = boxes[torch.randint(0, 3, (B, S), generator=g)]
    return B, S, V, ids.to(DEV), bbox.to(DEV), g


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_bwd_in_lilts_three_call_forms(ops, dtype):
    """torch.index_add_ as in test_embed_bwd_with_the_collisions_of_real_batches, rel_err < 2e-5, tables accumulated into.  The three
    calls of modeling_lilt.py:213-225: word + position tables (H = 64), the box-position table through the word slot with zero
    position ids (H = 16), the four box tables with clip_hw off (H = 64); then LayoutLMv3's single call with all six tables."""
    H, Hl, cs, ss = 64, 16, 11, 10
    B, S, V, ids, bbox, g = _embed_inputs(H)
    pid = ops.position_ids(ids, 1)
    zpid = torch.zeros((B, S), dtype=torch.int32, device=DEV)
    d_x = torch.randn(B, S, H, generator=g).to(DEV).to(dtype)
    d_l = torch.randn(B, S, Hl, generator=g).to(DEV).to(dtype)
    d_sp = torch.randn(B, S, H, generator=g).to(DEV).to(dtype)
    shapes = dict(word=(V, H), pos=(S + 2, H), boxpos=(S + 2, Hl), x=(1024, cs), y=(1024, cs), h=(1024, ss), w=(1024, ss),
                  word2=(V, H), pos2=(S + 2, H), x2=(1024, cs), y2=(1024, cs), h2=(1024, ss), w2=(1024, ss))

    def run():
        t = {n: torch.full(sh, 0.25, device=DEV) for n, sh in shapes.items()}
        ops.embed_bwd(d_x, B, S, H, input_ids=ids, pos_ids=pid, g_word=t["word"], g_pos=t["pos"], pad_id=1)
        ops.embed_bwd(d_l, B, S, Hl, input_ids=pid.to(torch.int64), pos_ids=zpid, g_word=t["boxpos"],
                      g_pos=torch.zeros((1, Hl), device=DEV), pad_id=1)
        ops.embed_bwd(d_sp, B, S, H, bbox=bbox, g_x=t["x"], g_y=t["y"], g_h=t["h"], g_w=t["w"], clip_hw=False, pad_id=1)
        ops.embed_bwd(d_sp, B, S, H, input_ids=ids, pos_ids=pid, bbox=bbox, g_word=t["word2"], g_pos=t["pos2"], g_x=t["x2"],
                      g_y=t["y2"], g_h=t["h2"], g_w=t["w2"], pad_id=1)
        return tuple(t[n] for n in shapes)
    det, default = both_modes(run)
    ref = {n: torch.full(sh, 0.25, device=DEV) for n, sh in shapes.items()}
    keep, keep_p = ids.view(-1) != 1, pid.view(-1) != 1
    bb = bbox.view(-1, 4)
    for sfx, d in (("", d_x.float().view(B * S, H)), ("2", d_sp.float().view(B * S, H))):
        ref["word" + sfx].index_add_(0, ids.view(-1)[keep], d[keep])
        ref["pos" + sfx].index_add_(0, pid.view(-1).long()[keep_p], d[keep_p])
    ref["boxpos"].index_add_(0, pid.view(-1).long()[keep_p], d_l.float().view(B * S, Hl)[keep_p])
    d = d_sp.float().view(B * S, H)
    for sfx in ("", "2"):
        ref["x" + sfx].index_add_(0, bb[:, 0], d[:, 0:cs]); ref["x" + sfx].index_add_(0, bb[:, 2], d[:, 2 * cs:3 * cs])
        ref["y" + sfx].index_add_(0, bb[:, 1], d[:, cs:2 * cs]); ref["y" + sfx].index_add_(0, bb[:, 3], d[:, 3 * cs:4 * cs])
        ref["h" + sfx].index_add_(0, bb[:, 3] - bb[:, 1], d[:, 4 * cs:4 * cs + ss])
        ref["w" + sfx].index_add_(0, bb[:, 2] - bb[:, 0], d[:, 4 * cs + ss:4 * cs + 2 * ss])
    for n, got, got0 in zip(shapes, det, default):
        assert rel_err(got, ref[n]) < 2e-5, n
        assert rel_err(got0, ref[n]) < 2e-5, n
        assert torch.equal(got == 0.25, ref[n] == 0.25), n                      # rows nobody feeds keep what they held


# ---------------------------------------------------------------------------------------------- relative-position tables
def test_relpos_tables(ops):
    """The fp32-accumulator form against autograd at rel_err < 1e-4 (test_relpos_buckets_and_bias); the layered form (two layers of
    bf16 dS^T slabs; no test of the default form holds it to a sum, test_attention_bf16_single_pass_... compares it with the fp32
    form at 1e-2) against the float64 sum per bin with n 2^-23 sum|x| + n 2^-32.  B = 2, four heads, T = 70."""
    B, nh, T, b1n, b2n, scale = 2, 4, 70, 32, 64, 0.25
    Tp = ops.attn_padded_len(T)
    g = torch.Generator().manual_seed(70)
    bk = [torch.randint(0, n, (B, T, T), generator=g, dtype=torch.uint8).to(DEV) for n in (b1n, b2n, b2n)]
    gg = torch.zeros(B, nh, T, Tp, device=DEV)
    gg[..., :T] = torch.randn(B, nh, T, T, generator=g).to(DEV)
    ds = torch.zeros(2, B, nh, T, Tp, device=DEV, dtype=torch.bfloat16)            # [layer, b, h, key j, query i]
    ds[..., :T] = torch.randn(2, B, nh, T, T, generator=g).to(DEV).to(torch.bfloat16)
    bkt = [t.transpose(1, 2).contiguous() for t in bk]
    init = [torch.randn(nh, n, generator=g).to(DEV) for n in (b1n, b2n, b2n)]

    def run():
        a = [t.clone() for t in init]
        ops.relpos_bias_bwd(gg, bk[0], bk[1], bk[2], a[0], a[1], a[2], scale)
        l = [t.clone() for t in init]
        ops.relpos_bias_bwd_layers(ds, bkt[0], bkt[1], bkt[2], l[0], l[1], l[2], scale)
        only1 = init[0].clone()
        ops.relpos_bias_bwd(gg, bk[0], None, None, only1, None, None, scale)           # the 1-D table alone
        return tuple(a) + tuple(l) + (only1,)
    det, default = both_modes(run)
    ws = [torch.zeros(nh, n, device=DEV, requires_grad=True) for n in (b1n, b2n, b2n)]
    idx = [t.long() for t in bk]
    bias = scale * (ws[0].t()[idx[0]] + ws[1].t()[idx[1]] + ws[2].t()[idx[2]]).permute(0, 3, 1, 2)     # [B, nh, T(i), T(j)]
    (bias * gg[..., :T]).sum().backward()
    for k in range(3):
        assert rel_err(det[k] - init[k], ws[k].grad) < 1e-4 and rel_err(default[k] - init[k], ws[k].grad) < 1e-4
    assert torch.equal(det[6], det[0])
    # layered form: per (head, bin) the float64 sum of the two layers' entries (the kernel adds the layers in fp32 first: <= 1 ulp
    # of the pair, inside the bound's n = 2 x entries)
    v = ds[..., :T].double().sum(0)                                                  # [B, nh, j, i]
    for k, nb in enumerate((b1n, b2n, b2n)):
        onehot = F.one_hot(bkt[k].long(), nb).double()                               # [B, j, i, bin]
        ref = torch.einsum("bhji,bjic->hc", v, onehot) * scale
        mag = torch.einsum("bhji,bjic->hc", ds[..., :T].double().abs().sum(0), onehot) * scale
        n = 2 * B * T * T
        bound = n * 2.0 ** -23 * mag + n * 2.0 ** -32 + 2.0 ** -22 * init[k].double().abs()
        err = (det[3 + k].double() - init[k].double() - ref).abs()
        assert bool((err <= bound).all()), (k, float((err / bound).max()))


# ---------------------------------------------------------------------------------------------- pair backward
CLASSES = [2, 3, 3, 3, 3]


@functools.lru_cache(maxsize=None)
def _pair_case(D):
    """Inputs and the explicit-mask fp32 autograd reference of test_pair_bwd_fused_matches_autograd at B = 2, N = 40, dropout 0.1
    (computed once per width, shared by the recomputing and the saved form)."""
    from dropout_ref import k12_keep, k12_scale
    B, N, p_drop, nh = 2, 40, 0.1, len(CLASSES)
    g = torch.Generator().manual_seed(B * 100000 + N * 1000 + D)
    ab = torch.randn(B, N, 2 * D, generator=g).to(DEV).to(torch.bfloat16)
    P = N * (N + 1) // 2
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [torch.randn(c, D, generator=g).to(DEV) for c in CLASSES]
    b1cat = (0.1 * torch.randn(nh * D, generator=g)).to(DEV)
    dl = [torch.randn(B, P, c, generator=g).to(DEV) for c in CLASSES]
    scale = torch.rand(nh, generator=g).to(DEV) + 0.5
    seed = 4242 + N
    abr = ab.float().clone().requires_grad_(True)
    ii, jj = torch.triu_indices(N, N, device=DEV)
    xr = F.silu(abr[:, ii, :D] + abr[:, jj, D:])
    xq = xr + (xr.detach().to(torch.bfloat16).float() - xr.detach())
    w1r = [w.to(torch.bfloat16).float().clone().requires_grad_(True) for w in w1]
    w2r = [w.clone().requires_grad_(True) for w in w2]
    b1r = b1cat.clone().requires_grad_(True)
    keep_all = torch.stack([k12_keep(seed, b, 0, P, nh * D, p_drop) for b in range(B)]).to(DEV)
    for h in range(nh):
        y = F.silu(xq @ w1r[h].t() + b1r[h * D:(h + 1) * D]) * keep_all[:, :, h * D:(h + 1) * D] * k12_scale(p_drop)
        (((y @ w2r[h].t()) * dl[h] * scale[h]).sum()).backward(retain_graph=h + 1 < nh)
    ref = dict(d_ab=abr.grad.detach(), db1=b1r.grad.detach(), dw2=[w.grad.detach() for w in w2r])
    return dict(B=B, N=N, D=D, nh=nh, P=P, p_drop=p_drop, seed=seed, ab=ab, w1=w1, w2=w2, b1cat=b1cat, dl=dl, scale=scale, ref=ref)


@pytest.mark.parametrize("D,saved", [(32, False), (384, False), (384, True), (512, False)])
def test_pair_bwd(ops, D, saved):
    """dW2 / db1 (and d_ab) against the explicit-mask autograd reference of test_pair_bwd_fused_matches_autograd at its rel_err < 3e-2
    (the saved form: the same reference; test_pair_saved_activations_path_is_the_recomputing_path holds it to the recomputing form
    at 1e-3).  B = 2, N = 40, five heads, dropout on: fewer than 256 workgroups per document, so both documents' workgroups share
    workspace rows under mode 0 and own one each under the mode.  dz, x and d_ab are the default form's bits."""
    import peneo_amd
    from peneo_amd import hip
    c = _pair_case(D)
    B, N, nh = c["B"], c["N"], c["nh"]
    dt = torch.bfloat16
    rows = ops.pair_bwd_rows(N)
    assert rows // 128 < 256 and B * (rows // 128) > rows // 128
    wp2 = ops.pair_bwd_pack(c["w1"])
    act = xsaved = dl = None
    if saved:
        b2 = torch.zeros(sum(CLASSES), device=DEV)
        P = c["P"]
        tags = [torch.zeros(B, P, dtype=torch.int64, device=DEV) for _ in CLASSES]
        cw = [torch.ones(k, device=DEV) for k in CLASSES]
        wp = ops.pair_heads_pack(dt, c["w1"], c["w2"])
        _, _, _, (act, xsaved) = ops.pair_heads_fwd(c["ab"], wp, c["b1cat"], b2, CLASSES, tags=tags, class_weights=cw, want_dlogits=True,
                                                    want_logits=True, drop_p=c["p_drop"], drop_seed=c["seed"], save=True)
    args = ops.pair_dz_args(D, CLASSES, c["dl"], c["w2"], c["scale"], drop_p=c["p_drop"], drop_seed=c["seed"])

    def run():
        dz = torch.full((B * rows, nh * D), 7.0, device=DEV, dtype=dt)
        d_ab = torch.full((B, N, 2 * D), 5.0, device=DEV)
        ws = ops.pair_bwd_workspace(B, N, nh, D, DEV)
        assert ws.shape[0] == (B * (rows // 128) if hip.deterministic_mode() else 256)
        if saved:
            ops.pair_bwd_saved(c["ab"], wp2, args, act, dz, d_ab, ws)
            x = xsaved
        else:
            x = torch.full((B * rows, D), 7.0, device=DEV, dtype=dt)
            ops.pair_bwd_fused(c["ab"], wp2, c["b1cat"], args, dz, x, d_ab, ws)
        dw2, db1 = ops.pair_dz_finish(ws, nh, D, CLASSES)
        return tuple(w.clone() for w in dw2) + (db1.clone(), dz, x, d_ab)
    det, default = both_modes(run)
    t = 3e-2
    for res in (det, default):
        assert rel_err(res[nh], c["ref"]["db1"]) < t
        for h in range(nh):
            assert rel_err(res[h], c["ref"]["dw2"][h]) < t, h
        assert rel_err(res[nh + 3], c["ref"]["d_ab"]) < t
    for k in (nh + 1, nh + 2, nh + 3):                                      # dz, x, d_ab: bit for bit the default form's
        assert torch.equal(det[k], default[k]), k
    # under the mode a workspace sized for the default is refused before the launch (it would be written out of bounds)
    with peneo_amd.deterministic(1):
        with pytest.raises(hip.PeneoHipError, match="workspace"):
            small = ops.pair_dz_workspace(nh, D, DEV, slots=16)
            dz = torch.empty((B * rows, nh * D), device=DEV, dtype=dt)
            ops.pair_bwd_fused(c["ab"], wp2, c["b1cat"], args, dz, torch.empty((B * rows, D), device=DEV, dtype=dt),
                               torch.empty((B, N, 2 * D), device=DEV), small)


# ---------------------------------------------------------------------------------------------- chunked decoder backward
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_x_bwd(ops, dtype):
    """The scatter of the chunked decoder backward (widths without the fused kernel, e.g. the tiny LiLT's D = 96): d_a / d_b sums against
    fp32 autograd through x = SiLU(a_i + b_j) at test_pair_backward_blocks' tolerances (1e-4 / 2e-2; premultiplied bf16: 3e-2), rows
    7 .. 30 of N = 45, accumulated onto what a first chunk left."""
    N, D = 45, 128
    g = torch.Generator().manual_seed(9)
    ab = torch.randn(N, 2 * D, generator=g).to(DEV).to(dtype)
    ii, jj = torch.triu_indices(N, N, device=DEV)
    i0, i1 = 7, 30
    p0, p1 = i0 * N - i0 * (i0 - 1) // 2, i1 * N - i1 * (i1 - 1) // 2
    abr = ab.float().clone().requires_grad_(True)
    xr = F.silu(abr[ii, :D] + abr[jj, D:])[p0:p1]
    dx = torch.randn(p1 - p0, D, generator=g).to(DEV).to(dtype)
    xr.backward(dx.float())
    pre = (ab.float()[ii, :D] + ab.float()[jj, D:])[p0:p1]
    sg = torch.sigmoid(pre)
    du = (dx.float() * (sg * (1 + pre * (1 - sg)))).to(dtype)
    first = torch.randn(N, 2 * D, generator=g).to(DEV)

    def run():
        dab, dab2 = first.clone(), first.clone()
        ops.pair_x_bwd(ab, i0, i1, dx, dab)
        ops.pair_x_bwd(ab, i0, i1, du, dab2, premultiplied=True)
        return dab, dab2
    (dab, dab2), (dab0, _) = both_modes(run)
    assert rel_err(dab - first, abr.grad) < (1e-4 if dtype == torch.float32 else 2e-2)
    assert rel_err(dab2 - first, abr.grad) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert rel_err(dab0 - first, abr.grad) < (1e-4 if dtype == torch.float32 else 2e-2)


def test_pair_dz_fused(ops):
    """peneo_pair_dz_fused at D = 96, N = 370: 269 workgroups per launch, so rows are shared under mode 0 (256) and owned under the
    mode; two launches add into one workspace, as the chunks of a backward do.  dz, dW2 and db1 against fp32 autograd of the block at
    test_pair_dz_fused_matches_the_gemm_epilogue's rel_err < 2e-2; dz is the default form's bits."""
    N, D, dtype = 370, 96, torch.bfloat16
    nh = len(CLASSES)
    g = torch.Generator().manual_seed(N * 1000 + D)
    ab = torch.randn(N, 2 * D, generator=g).to(DEV).to(dtype)
    npairs = N * (N + 1) // 2
    assert (npairs + 255) // 256 > 256
    w1 = [(torch.randn(D, D, generator=g) / math.sqrt(D)).to(DEV) for _ in CLASSES]
    w2 = [torch.randn(c, D, generator=g).to(DEV) for c in CLASSES]
    b1cat = (0.1 * torch.randn(nh * D, generator=g)).to(DEV)
    dl = [torch.randn(npairs, c, generator=g).to(DEV) for c in CLASSES]
    scale = torch.rand(nh, generator=g).to(DEV) + 0.5
    wp = ops.pair_heads_pack(dtype, w1, w2)
    args = ops.pair_dz_args(D, CLASSES, dl, w2, scale)

    def run():
        rows = ops.pair_dz_fused_workspace_rows(npairs)
        ws = torch.zeros((rows, 4 * nh * D), device=DEV)
        z = torch.empty(npairs, nh * D, device=DEV, dtype=dtype)
        ops.pair_dz_fused(ab, 0, N, wp, b1cat, args, z, ws)
        ops.pair_dz_fused(ab, 0, N, wp, b1cat, args, z, ws)
        dw2, db1 = ops.pair_dz_finish(ws, nh, D, CLASSES)
        return tuple(w.clone() for w in dw2) + (db1.clone(), z, torch.tensor(rows))
    det, default = both_modes(run)
    assert int(det[nh + 2]) == (npairs + 255) // 256 == 269 and int(default[nh + 2]) == 256
    assert torch.equal(det[nh + 1], default[nh + 1])
    abf = ab.float()
    ii, jj = torch.triu_indices(N, N, device=DEV)
    xr = F.silu(abf[ii, :D] + abf[jj, D:]).to(dtype).float()
    zr = (xr @ torch.cat(w1).to(dtype).float().t() + b1cat).requires_grad_(True)
    w2r = [w.clone().requires_grad_(True) for w in w2]
    tot = 0
    for h in range(nh):
        tot = tot + ((F.silu(zr[:, h * D:(h + 1) * D]) @ w2r[h].t()) * dl[h] * scale[h]).sum()
    tot.backward()
    for res in (det, default):
        assert rel_err(res[nh + 1], zr.grad) < 2e-2
        assert rel_err(res[nh], 2 * zr.grad.sum(0)) < 2e-2
        for h in range(nh):
            assert rel_err(res[h], 2 * w2r[h].grad) < 2e-2
    import peneo_amd
    from peneo_amd import hip
    with peneo_amd.deterministic(1):                       # a workspace sized for the default is refused before the launch
        with pytest.raises(hip.PeneoHipError, match="workspace"):
            ops.pair_dz_fused(ab, 0, N, wp, b1cat, args, torch.empty(npairs, nh * D, device=DEV, dtype=dtype),
                              ops.pair_dz_workspace(nh, D, DEV, slots=256))


# ---------------------------------------------------------------------------------------------- gradient norm
def test_gradient_norm_and_the_clip_coefficient(ops):
    """A three-tensor table of 70 chunks (more than the 64 slots, so slots take two chunks by default): the norm against
    torch.nn.utils.clip_grad_norm_ at rel_err < 1e-5 (test_fused_adamw_clips_the_global_gradient_norm_like_clip_grad_norm) and against
    the float64 sum with n 2^-23 sum g^2; the slots the step reads, and with them the coefficient peneo_adamw_step_clip applies, and
    the parameters and both moments after the step are the same bits over three runs from the same state."""
    from peneo_amd.optim import FusedAdamW
    chunk = 4096
    sizes = [40 * chunk + 5, 26 * chunk - 100, 3 * chunk - 7]                # 41 + 26 + 3 chunks
    g = torch.Generator().manual_seed(70)
    p0 = [torch.randn(n, generator=g).to(DEV) for n in sizes]
    grads = [(torch.randn(n, generator=g) * 0.05).to(DEV) for n in sizes]

    def run():
        ps = [torch.nn.Parameter(p.clone()) for p in p0]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt = FusedAdamW([dict(params=ps, lr=1e-2, weight_decay=0.01)], betas=(0.9, 0.98), eps=1e-6, max_grad_norm=1.0)
        opt.step()
        assert opt._chunk_t.numel() == 70
        st = [opt.state[p] for p in ps]
        return (opt._sqnorm.clone(), opt.last_grad_norm().clone()) + tuple(p.detach().clone() for p in ps) + \
            tuple(s["exp_avg"].clone() for s in st) + tuple(s["exp_avg_sq"].clone() for s in st)
    det, default = both_modes(run)
    ref_params = [torch.nn.Parameter(p.clone()) for p in p0]
    for p, gr in zip(ref_params, grads):
        p.grad = gr.clone()
    want = torch.nn.utils.clip_grad_norm_(ref_params, 1.0)
    assert float(want) > 1.0                                               # the coefficient is not 1
    assert rel_err(det[1], want.reshape(1)) < 1e-5 and rel_err(default[1], want.reshape(1)) < 1e-5
    sq64 = sum(float((gr.double() ** 2).sum()) for gr in grads)
    n = sum(sizes)
    assert abs(float(det[0].sum()) - sq64) <= n * 2.0 ** -23 * sq64
    assert int((det[0] != 0).sum()) == 1 and float(det[0][0]) > 0          # the total in slot 0, the other slots cleared
    ob = torch.optim.AdamW([dict(params=ref_params, lr=1e-2, weight_decay=0.01)], betas=(0.9, 0.98), eps=1e-6)
    ob.step()                                                              # (on the clipped gradients)
    for k, p in enumerate(ref_params):
        assert rel_err(det[2 + k], p.detach()) < 3e-6


# ---------------------------------------------------------------------------------------------- strict refusals
def _refused_then_counted(call, name):
    """under mode 2 `call` raises and names its entry point; under mode 1 it runs and moves the counter"""
    import peneo_amd
    from peneo_amd import hip
    with peneo_amd.deterministic(2):
        with pytest.raises(hip.PeneoHipError, match=name):
            call()
    with peneo_amd.deterministic(1):
        c0 = hip.order_dependent_launches()
        out = call()
        torch.cuda.synchronize()
        assert hip.order_dependent_launches() > c0
    return out


def test_strict_mode_refuses_the_gemm_column_sum_epilogue(ops):
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(64, 40, generator=g).to(DEV).to(torch.bfloat16)
    x = torch.randn(64, 24, generator=g).to(DEV).to(torch.bfloat16)

    def call():
        db = torch.zeros(40, device=DEV)
        ops.gemm(dy, x, a_kmajor=False, b_kmajor=False, out_dtype=torch.float32, a_colsum=db)
        return db
    db = _refused_then_counted(call, "peneo_gemm")
    assert rel_err(db, dy.float().sum(0)) < 1e-4


def test_strict_mode_refuses_the_atomic_dq_of_the_attention_backward(ops):
    B, nh, T, d = 1, 2, 70, 64
    H = nh * d
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * T, 3 * H, generator=g).to(DEV).to(torch.bfloat16)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    Tp = ops.attn_padded_len(T)
    bias = torch.full((B, nh, T, Tp), -1.0e30, dtype=torch.bfloat16, device=DEV)      # the kernel's padded layout
    bias[..., :T] = (0.5 * torch.randn(B, nh, T, T, generator=g)).to(DEV).to(torch.bfloat16)
    out, lse = ops.attn_fwd(q, k, v, B, nh, T, d, 0.125, bias, None)
    d_out = torch.randn(B * T, H, generator=g).to(DEV).to(torch.bfloat16)

    def call(atomic=True):
        dqkv = torch.zeros_like(qkv)
        ops.attn_bwd(q, k, v, out, d_out, lse, B, nh, T, d, 0.125, bias, None, dqkv, None, dq_atomic=atomic)
        return dqkv
    got = _refused_then_counted(call, "peneo_attn_bwd")
    import peneo_amd
    from peneo_amd import hip
    with peneo_amd.deterministic(2):                                         # the default dQ (from the dS^T slab) is covered
        c0 = hip.order_dependent_launches()
        plain = call(atomic=False)
        assert hip.order_dependent_launches() == c0
    assert rel_err(got.float(), plain.float()) < 2e-2


def test_strict_mode_refuses_ohem(ops):
    g = torch.Generator().manual_seed(21)
    n = 5000
    lg = (torch.randn(n, 3, generator=g) * 1.5).to(DEV)
    tg = ((torch.rand(n, generator=g) < 0.05).long() * torch.randint(1, 3, (n,), generator=g)).to(DEV)
    w = torch.tensor([1.0, 10.0, 10.0], device=DEV)
    out8 = _refused_then_counted(lambda: ops.ohem_ce(lg, tg, w, 16, 200)[0], "peneo_ohem_ce")
    assert int(out8[5]) == 16 and int(out8[6]) == 200
