"""LayerNorm kernels (peneo_amd/csrc/layernorm.hip) against the float64 reference of tests/layernorm_ref.py, element by element, at
every edge of the dispatch: each half-wave fast instantiation and the generic kernels with 1 to 4 vector slots per lane, the
grid-stride second pass of the fast backward (atomic form from row 2048, partial form from row 8192) and of the generic backward
(from row 1024), the single-writer column kernel of the deterministic mode, the dropout masks against their host restatement, sliced
[B, R, H] row maps, in-place calls and the refusals.  Every comparison is (|got - ref| <= bound).all() with bound = u_out |ref| +
k 2^-23 A (layernorm_ref.bound); a failure names the worst ratio and its (row, col).

Not covered: views whose base or batch stride is not a multiple of 16 bytes, which push a fast H onto the generic kernels."""
import pytest
import torch

import layernorm_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


def on_dev(c):
    return tuple(t.to(DEV) for t in L.inputs(c.dtype, c.rows, c.H))


def within(what, c, got, ref, A, kind, out_dtype, base=None):
    """|got - ref| <= bound at every element.  base: the buffer the kernel accumulated onto, one more term of every element."""
    ref, A = ref.double(), A.double()
    if base is not None:
        ref, A = ref + base.double().cpu(), A + base.double().cpu().abs()
    bnd = L.bound(ref, A, L.k_for(kind, c.rows, c.H), out_dtype)
    ratio, at = L.worst(got.detach().cpu(), ref, bnd)
    assert ratio <= 1.0, f"{L.case_id(c)} {what}: worst |got - ref| / bound = {ratio:.4g} at {at}"


def is_fast(ops, c):
    from peneo_amd import hip
    return int(hip.lib().peneo_layernorm_bwd_partial_rows(hip.dtype_code(L.TORCH_DTYPE[c.dtype]), c.rows, c.H)) > 0


def bases(H, seed=3):
    g = torch.Generator().manual_seed(seed + H)
    return (0.5 * torch.randn(H, generator=g)).to(DEV), (0.5 * torch.randn(H, generator=g)).to(DEV)


def backward(ops, c, x, dy, gamma, mean, rstd, dgamma, dbeta, second=False, colsum=None, dx=None):
    """layernorm_bwd with the options of the input set -> (dx, dx_dropped)"""
    dxd = torch.empty(c.rows, c.H, dtype=x.dtype, device=DEV) if second else None
    dx = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dx=dx, drop_p=c.p_in, drop_seed=c.seed_in, dx_dropped=dxd,
                           drop2_p=c.p2 if second else 0.0, drop2_seed=c.seed2, dx_colsum=colsum)
    return dx, dxd


# ---------------------------------------------------------------------------------------------- every instantiation
@pytest.mark.parametrize("c", L.fwd_cases(), ids=L.case_id)
def test_forward_every_instantiation(ops, c):
    """y, mean and rstd of one row and of 13 (two workgroups of the fast kernel, four of the generic one) at every fast H and at
    generic H with 1, 2, 3 and 4 vector slots per lane, the last one ragged.  mean and rstd are the only place where one term
    dropped from a bf16 row sum shows."""
    x, _, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    assert is_fast(ops, c) == (c.H in L.FAST_H[c.dtype])
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS)
    within("y", c, y, ref.v["y"], ref.A["y"], "y", c.dtype)
    within("mean", c, mean, ref.v["mean"], ref.A["mean"], "mean", None)
    within("rstd", c, rstd, ref.v["rstd"], ref.A["rstd"], "rstd", None)


@pytest.mark.parametrize("c", L.bwd_cases(), ids=L.case_id)
def test_backward_every_instantiation(ops, c):
    """dx, and dgamma / dbeta accumulated onto non-zero buffers, of 13 rows at the same row lengths."""
    x, dy, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS)
    g0, b0 = bases(c.H)
    dg, db = g0.clone(), b0.clone()
    dx, _ = backward(ops, c, x, dy, gamma, mean, rstd, dg, db)
    within("dx", c, dx, ref.v["dx"], ref.A["dx"], "dx", c.dtype)
    within("dgamma", c, dg, ref.v["dgamma"], ref.A["dgamma"], "dgamma", None, base=g0)
    within("dbeta", c, db, ref.v["dbeta"], ref.A["dbeta"], "dbeta", None, base=b0)


# ---------------------------------------------------------------------------------------------- grid-stride loops
def _backward_with_every_sum(ops, c):
    x, dy, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS)
    g0, b0 = bases(c.H)
    dg, db, col = g0.clone(), b0.clone(), torch.full((c.H,), 0.5, device=DEV)
    dx, dxd = backward(ops, c, x, dy, gamma, mean, rstd, dg, db, second=True, colsum=col)
    within("dx", c, dx, ref.v["dx"], ref.A["dx"], "dx", c.dtype)
    within("dx_dropped", c, dxd, ref.v["dxd"], ref.A["dxd"], "dxd", c.dtype)
    within("dgamma", c, dg, ref.v["dgamma"], ref.A["dgamma"], "dgamma", None, base=g0)
    within("dbeta", c, db, ref.v["dbeta"], ref.A["dbeta"], "dbeta", None, base=b0)
    within("dx_colsum", c, col, ref.v["dcol"], ref.A["dcol"], "dcol", None, base=torch.full((c.H,), 0.5))


@pytest.mark.parametrize("c", L.grid_cases(), ids=L.case_id)
def test_fast_backward_second_and_third_pass(ops, c):
    """The atomic form of ln_bwd32_kernel runs 256 workgroups of 8 rows: at 2059 rows the half-waves of the first two workgroups
    take a second, prefetched row (2048..2058), at 4101 a third (4096..4100).  dx at every row, the dropped second output (its zeros
    are exactly keep_mask's), and the three column sums, which lose or double a row if the loop does."""
    assert is_fast(ops, c) and c.rows > 2048
    _backward_with_every_sum(ops, c)


@pytest.mark.parametrize("c", L.generic_cases(), ids=L.case_id)
def test_generic_backward_second_and_third_pass(ops, c):
    """ln_bwd_kernel runs 256 workgroups of 4 rows: a second pass from row 1024, a third from row 2048; H = 640 fills lane slots
    0 and 1 and, in fp32, a ragged slot 2."""
    assert not is_fast(ops, c) and c.rows > 1024
    _backward_with_every_sum(ops, c)


@pytest.mark.parametrize("c", L.partial_cases(), ids=L.case_id)
def test_partial_form_past_its_cap(ops, c):
    """peneo_layernorm_bwd_partial caps at 1024 workgroups, so 8205 rows give rows 8192..8204 to a second pass.  The column sums of
    the partials against the float64 dgamma | dbeta (not against the atomic form, which shares the kernel body), dx against the reference."""
    x, dy, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS)
    dx, part = ops.layernorm_bwd_partial(dy, x, gamma, mean, rstd)
    assert part.shape == (1024, 2 * c.H)
    sums = ops.colsum(part)
    within("dx", c, dx, ref.v["dx"], ref.A["dx"], "dx", c.dtype)
    within("dgamma", c, sums[:c.H], ref.v["dgamma"], ref.A["dgamma"], "dgamma", None)
    within("dbeta", c, sums[c.H:], ref.v["dbeta"], ref.A["dbeta"], "dbeta", None)


# ---------------------------------------------------------------------------------------------- deterministic mode
@pytest.mark.parametrize("c", L.det_cases(), ids=L.case_id)
def test_deterministic_column_kernel(ops, c):
    """ln_pgrad_det_kernel: 16 columns per workgroup (the last group only partly inside H = 24, 520, 20, 260), row lanes of 4 rows in
    flight (more than one unroll from 129 / 65 rows on), with the input dropout regenerated per element.  dgamma / dbeta against the
    float64 reference; dx_colsum against the float64 sum of the dx_dropped the kernel STORED, which is what the header promises; dx
    and dx_dropped are mode 0's bits."""
    import peneo_amd
    x, dy, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS)
    g0, b0 = bases(c.H)

    def run():
        dg, db, col = g0.clone(), b0.clone(), torch.full((c.H,), 0.5, device=DEV)
        dx, dxd = backward(ops, c, x, dy, gamma, mean, rstd, dg, db, second=True, colsum=col)
        return dg, db, col, dx, dxd
    with peneo_amd.deterministic(2):
        dg, db, col, dx, dxd = run()
        torch.cuda.synchronize()
    with peneo_amd.deterministic(0):
        _, _, _, dx0, dxd0 = run()
    assert torch.equal(dx, dx0) and torch.equal(dxd, dxd0)
    within("dx", c, dx, ref.v["dx"], ref.A["dx"], "dx", c.dtype)
    within("dx_dropped", c, dxd, ref.v["dxd"], ref.A["dxd"], "dxd", c.dtype)
    within("dgamma", c, dg, ref.v["dgamma"], ref.A["dgamma"], "dgamma", None, base=g0)
    within("dbeta", c, db, ref.v["dbeta"], ref.A["dbeta"], "dbeta", None, base=b0)
    stored = dxd.double().cpu()
    within("dx_colsum", c, col, stored.sum(0), stored.abs().sum(0), "dcol", None, base=torch.full((c.H,), 0.5))


# ---------------------------------------------------------------------------------------------- dropout masks
@pytest.mark.parametrize("c", L.mask_cases(), ids=L.case_id)
def test_dropout_masks_equal_the_host_restatement(ops, c):
    """The forward's y == 0 set, the backward's input mask (dbeta of a dy that is 1 on one row and 0 elsewhere) and the dx_dropped ==
    0 set are each keep_mask exactly, on a fast and on a generic row length; kept elements are within bound of ref / (1 - p).  The
    reference has no kept element that could round to zero (asserted on the reference)."""
    x, dy, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    keep_in, keep2 = L.case_masks(c)
    for kind, keep in (("y", keep_in), ("dxd", keep2)):
        bnd = L.bound(ref.v[kind], ref.A[kind], L.k_for(kind, c.rows, c.H), c.dtype)
        assert bool((ref.v[kind].abs()[keep] > 2 * bnd[keep]).all()), "choose inputs with no kept element this close to zero"
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS, drop_p=c.p_in, drop_seed=c.seed_in)
    assert torch.equal(y.cpu() == 0, ~keep_in)
    within("y", c, y, ref.v["y"], ref.A["y"], "y", c.dtype)
    dg, db = torch.zeros(c.H, device=DEV), torch.zeros(c.H, device=DEV)
    dx, dxd = backward(ops, c, x, dy, gamma, mean, rstd, dg, db, second=True)
    assert torch.equal(dxd.cpu() == 0, ~keep2)
    within("dx", c, dx, ref.v["dx"], ref.A["dx"], "dx", c.dtype)
    within("dx_dropped", c, dxd, ref.v["dxd"], ref.A["dxd"], "dxd", c.dtype)
    within("dbeta", c, db, ref.v["dbeta"], ref.A["dbeta"], "dbeta", None)
    scale = L.keep_scale(c.p_in)
    for r in range(c.rows):
        one = torch.zeros_like(dy)
        one[r] = 1
        db = torch.zeros(c.H, device=DEV)
        ops.layernorm_bwd(one, x, gamma, mean, rstd, dg, db, drop_p=c.p_in, drop_seed=c.seed_in)
        db = db.cpu()
        assert torch.equal(db != 0, keep_in[r]), r
        assert bool(((db[keep_in[r]].double() - scale).abs() <= 16 * L.UNIT * scale).all()), r


@pytest.mark.parametrize("dt", L.DTYPES)
@pytest.mark.parametrize("p", L.MASK_P)
def test_mask_is_one_function_of_seed_and_logical_index(ops, dt, p):
    """dropout_base + dropout_keep_b of the fast kernels and dropout_keep of the generic ones agree at the same r * H + c: a fast [15,
    H] and a generic [., 640] tensor cover the same flat indices.  Two seeds give different masks."""
    (rf, hf), (rg, hg) = L.MASK_FAST[dt], L.MASK_GENERIC[dt]
    assert rf * hf == rg * hg
    zeros = {}
    for rows, H in ((rf, hf), (rg, hg)):
        c = L.plain(dt, rows, H)
        x, _, gamma, beta = on_dev(c)
        assert is_fast(ops, c) == (H == hf)
        for seed in (L.SEED_IN, L.SEED_IN + 1):
            y, _, _ = ops.layernorm_fwd(x, gamma, beta, L.EPS, drop_p=p, drop_seed=seed)
            zeros[H, seed] = (y == 0).flatten().cpu()
            assert torch.equal(zeros[H, seed], ~L.keep_mask(seed, rows, H, p).flatten())
    for seed in (L.SEED_IN, L.SEED_IN + 1):
        assert torch.equal(zeros[hf, seed], zeros[hg, seed])
    assert not torch.equal(zeros[hf, L.SEED_IN], zeros[hf, L.SEED_IN + 1])


# ---------------------------------------------------------------------------------------------- row maps, aliasing
@pytest.mark.parametrize("c", L.sliced_cases(), ids=L.case_id)
def test_sliced_row_maps(ops, c):
    """x = buf[:, :20] and out = buf[:, 20:40] of a [3, 50, H] buffer (dy and dx likewise), with the input dropout: the contiguous
    call's bits, nothing written outside the slice, and a mask that follows the logical row b * 20 + j, not the memory offset."""
    B, R, S = L.SLICED
    x, dy, gamma, beta = on_dev(c)
    ref = L.case_reference(c)
    keep_in, _ = L.case_masks(c)
    y0, mean0, rstd0 = ops.layernorm_fwd(x, gamma, beta, L.EPS, drop_p=c.p_in, drop_seed=c.seed_in)
    buf = torch.full((B, R, c.H), 7.0, dtype=x.dtype, device=DEV)
    buf[:, :S] = x.view(B, S, c.H)
    y, mean, rstd = ops.layernorm_fwd(buf[:, :S], gamma, beta, L.EPS, out=buf[:, S:2 * S], drop_p=c.p_in, drop_seed=c.seed_in)
    assert y.data_ptr() == buf[:, S:2 * S].data_ptr()
    assert torch.equal(buf[:, S:2 * S].reshape(c.rows, c.H), y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    assert torch.equal(buf[:, :S].reshape(c.rows, c.H), x) and bool((buf[:, 2 * S:] == 7.0).all())
    assert torch.equal(y0.cpu() == 0, ~keep_in)
    within("y", c, y0, ref.v["y"], ref.A["y"], "y", c.dtype)

    dg0, db0 = torch.zeros(c.H, device=DEV), torch.zeros(c.H, device=DEV)
    dx0, _ = backward(ops, c, x, dy, gamma, mean0, rstd0, dg0, db0)
    dbuf = torch.full((B, R, c.H), 7.0, dtype=x.dtype, device=DEV)
    dbuf[:, :S] = dy.view(B, S, c.H)
    dg, db = torch.zeros(c.H, device=DEV), torch.zeros(c.H, device=DEV)
    backward(ops, c, buf[:, :S], dbuf[:, :S], gamma, mean0, rstd0, dg, db, dx=dbuf[:, S:2 * S])
    assert torch.equal(dbuf[:, S:2 * S].reshape(c.rows, c.H), dx0)
    assert torch.equal(dbuf[:, :S].reshape(c.rows, c.H), dy) and bool((dbuf[:, 2 * S:] == 7.0).all())
    within("dx", c, dx0, ref.v["dx"], ref.A["dx"], "dx", c.dtype)
    for what, got in (("contiguous", (dg0, db0)), ("sliced", (dg, db))):
        within(what + " dgamma", c, got[0], ref.v["dgamma"], ref.A["dgamma"], "dgamma", None)
        within(what + " dbeta", c, got[1], ref.v["dbeta"], ref.A["dbeta"], "dbeta", None)


@pytest.mark.parametrize("dt", L.DTYPES)
def test_in_place_on_the_fast_path(ops, dt):
    """out aliasing x in the forward and dx aliasing dy in the backward at 2059 rows of H = 768: the backward has fetched the next
    row of its half-wave before it stores this one.  Bit-equal to the out-of-place call, with and without the input dropout."""
    c = L.plain(dt, 2059, 768)
    x, dy, gamma, beta = on_dev(c)
    assert is_fast(ops, c)
    for p in (0.0, 0.1):
        y0, mean, rstd = ops.layernorm_fwd(x, gamma, beta, L.EPS, drop_p=p, drop_seed=L.SEED_IN)
        xb = x.clone()
        y1, mean1, rstd1 = ops.layernorm_fwd(xb, gamma, beta, L.EPS, out=xb, drop_p=p, drop_seed=L.SEED_IN)
        assert y1.data_ptr() == xb.data_ptr() and torch.equal(xb, y0) and torch.equal(mean, mean1) and torch.equal(rstd, rstd1)
        dg, db = torch.zeros(c.H, device=DEV), torch.zeros(c.H, device=DEV)
        dx0 = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, drop_p=p, drop_seed=L.SEED_IN)
        dyb = dy.clone()
        ops.layernorm_bwd(dyb, x, gamma, mean, rstd, dg, db, dx=dyb, drop_p=p, drop_seed=L.SEED_IN)
        assert torch.equal(dyb, dx0)


# ---------------------------------------------------------------------------------------------- refusals
def _refused(fn, *untouched):
    from peneo_amd import hip
    with pytest.raises(hip.PeneoHipError):
        fn()
    torch.cuda.synchronize()
    for t in untouched:
        assert bool((t == 7.0).all()), "a refused call wrote to its output"


@pytest.mark.parametrize("dt,H", [("bf16", 2056), ("f32", 1028), ("bf16", 12)])
def test_refused_row_lengths(ops, dt, H):
    """Past 64 lanes x 4 slots of 16 bytes, or not a whole number of 16-byte vectors: the library's error and no launch."""
    td = L.TORCH_DTYPE[dt]
    x = torch.ones(3, H, dtype=td, device=DEV)
    gamma, beta = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    stat = torch.ones(3, device=DEV)
    out = torch.full((3, H), 7.0, dtype=td, device=DEV)
    acc = torch.full((H,), 7.0, device=DEV)
    _refused(lambda: ops.layernorm_fwd(x, gamma, beta, L.EPS, out=out), out)
    _refused(lambda: ops.layernorm_bwd(x, x, gamma, stat, stat, acc, acc, dx=out), out, acc)
    from peneo_amd import hip
    assert int(hip.lib().peneo_layernorm_bwd_partial_rows(hip.dtype_code(td), 3, H)) == 0


def test_refused_drop_p_and_partial_rows(ops):
    from peneo_amd import hip
    H, rows = 256, 40
    x = torch.ones(rows, H, dtype=torch.bfloat16, device=DEV)
    gamma, beta = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    stat = torch.ones(rows, device=DEV)
    out = torch.full((rows, H), 7.0, dtype=torch.bfloat16, device=DEV)
    acc = torch.full((H,), 7.0, device=DEV)
    _refused(lambda: ops.layernorm_fwd(x, gamma, beta, L.EPS, out=out, drop_p=1.0, drop_seed=1), out)
    _refused(lambda: ops.layernorm_bwd(x, x, gamma, stat, stat, acc, acc, dx=out, drop_p=1.0, drop_seed=1), out, acc)
    _refused(lambda: ops.layernorm_bwd(x, x, gamma, stat, stat, acc, acc, dx=out, dx_dropped=out, drop2_p=1.0), out, acc)
    P = int(hip.lib().peneo_layernorm_bwd_partial_rows(hip.BF16, rows, H))
    assert P == 5
    part = torch.full((P + 1, 2 * H), 7.0, device=DEV)
    for wrong in (P + 1, P - 1, 0):
        def call():
            hip.check(hip.lib().peneo_layernorm_bwd_partial(hip.BF16, hip.ptr(x), 0, 0, hip.ptr(x), 0, 0, hip.ptr(out), 0, 0,
                                                            hip.ptr(gamma), hip.ptr(stat), hip.ptr(stat), hip.ptr(part), wrong, rows, H,
                                                            0.0, 0, None, 0.0, 0, hip.stream()), "peneo_layernorm_bwd_partial")
        _refused(call, out, part)
