"""tests/layernorm_ref.py checked on the CPU, over the input sets of tests/test_gpu_layernorm_edges.py: the plain fp32 torch
statement of LayerNorm lies inside the bounds at k / 8 (the constants are honest and the bounds reachable), a float64 result perturbed
the way a wrong kernel would be lies outside them (the bounds see what they exist for), and keep_mask is a sane pure function."""
import math

import pytest
import torch

import layernorm_ref as L


def _shapes():
    """one input set per (dtype, rows, H) of the GPU file, the one with the second output's dropout where there is one"""
    pick = {}
    for c in L.all_cases():
        key = (c.dtype, c.rows, c.H)
        if key not in pick or (c.p2 > 0 and pick[key].p2 == 0):
            pick[key] = c
    return list(pick.values())


def _outside(pert, c, kind, out_dtype, ref=None):
    ref = L.case_reference(c) if ref is None else ref
    bnd = L.bound(ref.v[kind], ref.A[kind], L.k_for(kind, c.rows, c.H), out_dtype)
    return (pert - ref.v[kind]).abs() > bnd


def test_constants_are_capped_per_shape():
    assert L.k_for("mean", 13, 4) == 12 and L.k_for("dbeta", 1, 4) == 16 and L.k_for("dx", 8205, 256) == L.K["dx"]
    assert set(L.RATIO) == set(L.ROW_KINDS + L.COL_KINDS)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_nan_or_an_inf_is_outside_every_bound(bad):
    """the comparison is (|got - ref| <= bound).all(): an element that is not a number cannot pass it"""
    ref = torch.linspace(-1, 1, 12, dtype=torch.float64).reshape(3, 4)
    bnd = torch.full_like(ref, 0.5)
    got = ref.clone()
    assert L.worst(got, ref, bnd)[0] == 0.0
    got[1, 2] = bad
    ratio, at = L.worst(got, ref, bnd)
    assert ratio > 1.0 and at == (1, 2)
    assert L.worst(got.float(), ref, torch.full_like(ref, float("inf")))[0] > 1.0      # not even an infinite bound admits it
    got = ref.clone()
    got[2, 3] += 0.6
    ratio, at = L.worst(got, ref, bnd)
    assert ratio == pytest.approx(1.2) and at == (2, 3)
    got[2, 3] = ref[2, 3] + 0.25
    assert L.worst(got, ref, bnd)[0] == pytest.approx(0.5)
    got[2, 3] = ref[2, 3] + 2.0 ** -40
    ratio, at = L.worst(got, ref, torch.zeros_like(ref))                                # any difference off a zero bound
    assert ratio > 1e100 and at == (2, 3)


@pytest.mark.parametrize("c", L.all_cases(), ids=L.case_id)
def test_fp32_statement_is_inside_the_bounds_at_an_eighth_of_k(c):
    """native_layer_norm in fp32, its autograd and .sum(0), rounded to the stored format, against the float64 reference; and its
    unrounded error is no more than RATIO says, the figure the constants are derived from."""
    ref, st = L.case_reference(c), L.case_statement(c)
    for kind, r in L.statement_ratios(c, st).items():
        assert r <= L.RATIO[kind], f"{kind}: the fp32 statement needs a ratio of {r:.4g}, RATIO says {L.RATIO[kind]}"
    x = L.inputs(c.dtype, c.rows, c.H)[0].double()
    assert bool((x.mean(1).abs() <= 2 * x.std(1, unbiased=False)).all()), "the relative bound on rstd needs |mean| <= 2 std"
    for kind in L.ROW_KINDS + L.COL_KINDS:
        stored = kind in ("y", "dx", "dxd")
        got = st[kind].to(L.TORCH_DTYPE[c.dtype]) if stored else st[kind]
        bnd = L.bound(ref.v[kind], ref.A[kind], L.k_for(kind, c.rows, c.H) / 8, c.dtype if stored else None)
        ratio, at = L.worst(got, ref.v[kind], bnd)
        assert ratio <= 1.0, f"{kind}: worst |fp32 - ref| / bound(k / 8) = {ratio:.4g} at {at}"


@pytest.mark.parametrize("c", L.mask_cases(), ids=L.case_id)
def test_mask_inputs_have_no_kept_element_near_zero(c):
    """what test_dropout_masks_equal_the_host_restatement asserts before it reads a mask off y == 0 and dx_dropped == 0"""
    ref = L.case_reference(c)
    for kind, keep in zip(("y", "dxd"), L.case_masks(c)):
        bnd = L.bound(ref.v[kind], ref.A[kind], L.k_for(kind, c.rows, c.H), c.dtype)
        assert bool((ref.v[kind].abs()[keep] > 2 * bnd[keep]).all())


def _wrong_row_statistic(c):
    x = L.inputs(c.dtype, c.rows, c.H)[0].double()
    ref = L.case_reference(c)
    H = c.H
    # one term missing from the row mean (the term of median magnitude): shows in mean, in both dtypes
    j = x.abs().sort(1).indices[:, H // 2]
    lost = x.gather(1, j[:, None])[:, 0]
    assert bool(_outside(ref.v["mean"] - lost / H, c, "mean", None).all())
    # 1 / (H + 1) instead of 1 / H: rstd moves by 1 / (2H) of itself and shows at EVERY row; mean moves by |mean| / (H + 1), which a
    # row whose mean happens to sit near zero cannot show: 0.05 / 2049 = 2.4e-5 is still 7 times 16 2^-23 mean|x|
    mean = x.sum(1, keepdim=True) / (H + 1)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).sum(1) / (H + 1) + L.EPS)
    assert bool(_outside(rstd, c, "rstd", None).all())
    big = ref.v["mean"].abs() > 0.05
    assert bool(_outside(mean[:, 0], c, "mean", None)[big].all())


def _short_second_reduction(c):
    """the last 8 columns of every row excluded from s2 = mean(g xh): dx_i moves by rstd |xh_i| |delta|, delta = sum8(g xh) / H, of
    typical size sqrt(8) mean|g xh| / H >= 1e-3 mean|g| at H <= 2048.  fp32: that is hundreds of times k 2^-23 A unless |xh_i| is
    tiny, so three quarters of all elements must show.  bf16: the element's own rounding 2^-8 |dx_i| hides it where |dx_i| is
    large, so the elements that must show are those with |dx_i| <= 0.05 rstd mean|g| (rounding <= 2e-4 rstd mean|g|) and |xh_i| >=
    0.5 (shift >= 0.5 rstd |delta|): all of them except in rows whose delta fell under a third of its typical size, a quarter
    of a normal distribution, hence three quarters.  A case too small to hold such an element must still show somewhere."""
    ref = L.case_reference(c)
    delta = (ref.g * ref.xh)[:, -8:].sum(1, keepdim=True) / c.H
    out = _outside(ref.v["dx"] + ref.v["rstd"][:, None] * ref.xh * delta, c, "dx", c.dtype)
    assert bool(out.any())
    if c.dtype == "f32":
        assert float(out.double().mean()) >= 0.75
    else:
        small = (ref.v["dx"].abs() <= 0.05 * ref.v["rstd"][:, None] * ref.g.abs().mean(1, keepdim=True)) & (ref.xh.abs() >= 0.5)
        if int(small.sum()) >= 8:
            assert float(out[small].double().mean()) >= 0.75, (float(out[small].double().mean()), int(small.sum()))


def _lost_or_doubled_row(c):
    """dgamma, dbeta and dcol with one row left out or added twice: the first row of a second grid-stride pass (1024 generic, 2048
    fast atomic, 8192 fast partial) and the last row.  At least nine in ten of the columns whose term is not zero fall outside."""
    ref = L.case_reference(c)
    for r in sorted({r for r in (1024, 2048, 8192) if r < c.rows} | {c.rows - 1}):
        for kind, term in (("dgamma", ref.dd[r] * ref.xh[r]), ("dbeta", ref.dd[r]), ("dcol", ref.v["dxd"][r])):
            nz = term != 0
            assert bool(nz.any())
            for sign in (-1.0, 1.0):
                out = _outside(ref.v[kind] + sign * term, c, kind, None)
                assert int(out[nz].sum()) >= math.floor(0.9 * int(nz.sum())), (kind, r, sign, int(out[nz].sum()), int(nz.sum()))


def _keep_scale_applied_twice(c):
    ref = L.case_reference(c)
    kept = ref.v["dxd"] != 0
    out = _outside(ref.v["dxd"] * L.keep_scale(c.p2), c, "dxd", c.dtype)
    assert int(out[kept].sum()) >= math.floor(0.999 * int(kept.sum()))


@pytest.mark.parametrize("c", _shapes(), ids=L.case_id)
def test_bounds_see_the_faults_they_exist_for(c):
    """The float64 reference perturbed the way a wrong kernel would be falls outside the bound at the affected elements, at every
    shape of the GPU file (one test per shape, so that the reference of a shape is computed once)."""
    _wrong_row_statistic(c)
    _short_second_reduction(c)
    _lost_or_doubled_row(c)
    if c.p2 > 0:
        _keep_scale_applied_twice(c)


def _keep_scalar(seed, idx, p):
    """common.h dropout_keep in plain Python integers, one element"""
    def mix(v):
        v ^= v >> 16; v = (v * 0x7FEB352D) & 0xFFFFFFFF; v ^= v >> 15; v = (v * 0x846CA68B) & 0xFFFFFFFF; v ^= v >> 16
        return v
    return mix((idx & 0xFFFFFFFF) ^ mix((seed ^ ((idx >> 32) * 0x9E3779B9)) & 0xFFFFFFFF)) >= L.drop_threshold(p)


@pytest.mark.parametrize("p", [0.1, 0.2, 0.3])
def test_keep_mask(p):
    rows, H = 60, 640
    keep = L.keep_mask(11, rows, H, p)
    n = rows * H
    pf = L.drop_threshold(p) / 2.0 ** 32
    assert abs(pf - p) < 2.0 ** -24
    assert abs(float(keep.double().mean()) - (1 - pf)) <= 4 * math.sqrt(pf * (1 - pf) / n)
    # a pure function of (seed, r * H + c): the same bits however the flat range is cut into rows, or seen as [B, R, H]
    assert torch.equal(keep.flatten(), L.keep_mask(11, 150, 256, p).flatten())
    assert torch.equal(keep.view(3, 20, H)[2, 5], keep[45])
    for idx in (0, 1, 255, 256, 639, 640, n - 1):
        assert bool(keep.flatten()[idx]) == _keep_scalar(11, idx, p)
    assert not torch.equal(keep, L.keep_mask(12, rows, H, p))
    assert bool(L.keep_mask(11, 4, 8, 0.0).all())


def test_threshold_is_computed_in_float32():
    assert L.drop_threshold(0.1) == int(torch.tensor(0.1, dtype=torch.float32) * torch.tensor(4294967296.0, dtype=torch.float32))
    assert L.drop_threshold(0.1) != int(0.1 * 2 ** 32)
    assert L.drop_threshold(0.9999999999) == 4294967040
