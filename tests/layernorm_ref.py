"""Float64 reference, per-element error bounds and the host restatement of the dropout mask for the LayerNorm kernels
(peneo_amd/csrc/layernorm.hip), with the input sets that tests/test_gpu_layernorm_edges.py runs and tests/test_layernorm_ref_host.py
re-checks on the CPU.  Test infrastructure, not a conftest.

Bounds.  Every output element is compared as |got - ref| <= bound(ref, A, k, out_dtype) = u_out |ref| + k 2^-23 A, where A is the sum
of the magnitudes of the terms that make up the element (so a cancelling sum is held to the size of what was added, not of what is
left), u_out the unit roundoff of the stored format (2^-8 bf16, 2^-24 fp32, 0 for the fp32 statistics and column sums, whose rounding
the k term already holds) and 2^-23 the unit of sum_bound in tests/test_gpu_deterministic_kernels.py.

The constants k are measured against the REFERENCE, never against the kernels: K[kind] = max(16, 8 * ratio) with ratio the largest
|fp32 torch statement - float64| / (2^-23 A) over every input set below (fp32_statement: torch.native_layer_norm in fp32, its autograd
and .sum(0) on the CPU), capped per shape by what any summation order can reach (H + 8 for row quantities, rows + H + 16 for column
sums).  The factor 8: the kernels sum in another order (lane-strided partial sums, a butterfly, atomics across workgroups in any
order), rsqrtf and 1 / (1 - p) are not correctly rounded, and the error is otherwise the same random walk.  `python
tests/layernorm_ref.py` prints the ratios; RATIO holds what it printed.

keep_mask leaves out logical indices past 2^32 (the hi32 word of dropout_keep): a tensor that large does not fit a test.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

EPS = 1e-5
UNIT = 2.0 ** -23
U_OUT = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24, None: 0.0}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}

ROW_KINDS = ("mean", "rstd", "y", "dx", "dxd")
COL_KINDS = ("dgamma", "dbeta", "dcol")

# largest |fp32 statement - float64| / (2^-23 A) over all_cases(), as printed by `python tests/layernorm_ref.py`
#   mean 0.913 (f32 2059x20)   rstd 1.508 (bf16 4101x192)   y 1.827 (bf16 513x520)   dx 2.309, dxd 2.825 (bf16 6x640, p 0.1)
#   dgamma 1.387, dcol 1.268 (bf16 6x640, p 0.3)   dbeta 1.184 (f32 3x640)
RATIO = {"mean": 0.92, "rstd": 1.51, "y": 1.83, "dx": 2.31, "dxd": 2.83, "dgamma": 1.39, "dbeta": 1.19, "dcol": 1.27}
# k = max(16, 8 * RATIO): 16 for all but dx (18.5) and dxd (22.6), whose A takes xh as exact while the fp32 xh of an element with
# x near the row mean carries the absolute error of the mean.  None has been raised for a kernel.
K = {kind: max(16.0, 8.0 * r) for kind, r in RATIO.items()}
# dgamma's A is NOT sum_r |dd xh|: at one or a few rows an element with x ~ mean has |dd xh| -> 0 while the fp32 xh is off by
# 2^-24 (|x| + mean|x|) rstd, and the fp32 torch statement itself then misses 2^-23 sum_r |dd xh| by a factor of 7530 (f32 1x1020).
# A = sum_r |dd| (|x| + mean|x|) rstd counts x and the mean as the two terms of xh, as the scale of y does; it is 2 to 3 times larger
# at many rows and still sees one lost row of 8205 (tests/test_layernorm_ref_host.py).


def k_for(kind, rows, H):
    """The constant of an output kind at one shape: K[kind], capped by the worst case of any summation order."""
    cap = H + 8 if kind in ROW_KINDS else rows + H + 16
    return min(K[kind], float(cap))


def bound(ref, A, k, out_dtype):
    """u_out |ref| + k 2^-23 A, float64.  out_dtype: 'bf16' / 'f32' for an output stored in that format, None for fp32 statistics and sums."""
    return U_OUT[out_dtype] * ref.double().abs() + k * UNIT * A.double()


def worst(got, ref, bnd):
    """-> (largest |got - ref| / bound, its index tuple).  An element counts as inside only where |got - ref| <= bound holds with a
    finite difference: a NaN or an inf in got gives inf, a difference off a zero bound a huge ratio."""
    diff = (got.double() - ref.double()).abs()
    raw = torch.where(diff == 0, torch.zeros_like(diff), diff / bnd.double().clamp_min(1e-300))
    inside = (diff <= bnd) & torch.isfinite(diff)
    outside = torch.where(torch.isfinite(raw) & (raw > 1), raw, torch.full_like(raw, float("inf")))
    ratio = torch.where(inside, raw, outside)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))


# ---------------------------------------------------------------------------------------------- dropout mask
_M = np.uint64(0xFFFFFFFF)
_u = np.uint64


def _mix32(x):
    """common.h: mix32, on uint64 arrays masked to 32 bits"""
    x = x.astype(np.uint64) & _M
    x ^= x >> _u(16); x = (x * _u(0x7FEB352D)) & _M; x ^= x >> _u(15); x = (x * _u(0x846CA68B)) & _M; x ^= x >> _u(16)
    return x


def drop_threshold(p):
    """uint32(min(float32(p) * 2^32, 4294967040)), the product rounded to float32 as in the kernels"""
    return int(min(np.float32(p) * np.float32(4294967296.0), np.float32(4294967040.0)))


def keep_scale(p):
    """1 / (1 - p) of the float32 p that the kernels read, in float64"""
    return 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0


def keep_mask(seed, rows, H, p):
    """bool [rows, H]: common.h dropout_keep(seed, idx = r * H + c, thresh) over LOGICAL rows (what a sliced [B, R, H] map numbers
    b * R + j).  keep = mix32(lo32(idx) ^ mix32(seed ^ (hi32(idx) * 0x9e3779b9))) >= thresh.  rows * H < 2^32 only."""
    if p <= 0:
        return torch.ones(rows, H, dtype=torch.bool)
    assert rows * H < 2 ** 32, "indices past 2^32 are left out (module docstring)"
    idx = np.arange(rows * H, dtype=np.uint64)
    lo, hi = idx & _M, idx >> _u(32)
    base = _mix32((_u(seed & 0xFFFFFFFF) ^ ((hi * _u(0x9E3779B9)) & _M)) & _M)
    h = _mix32(lo ^ base)
    return torch.from_numpy((h >= _u(drop_threshold(p))).reshape(rows, H))


# ---------------------------------------------------------------------------------------------- reference
def reference(x, dy, gamma, beta, eps, keep_in=None, p_in=0.0, keep2=None, p2=0.0):
    """Float64 LayerNorm forward and backward of the values the kernel reads (bf16 inputs are widened).  keep_in / p_in: the dropout
    on the forward's output, applied to dy on the way back; keep2 / p2: the mask of the second backward output dx_dropped.
    -> namespace with .v[name] (mean, rstd, y, dx, dxd = dx_dropped, dgamma, dbeta, dcol = column sums of dxd, dcol_dx = of dx) and
    .A[name], the sum of the magnitudes of the terms of each element:
      mean sum|x| / H;  rstd itself (relative: needs |mean| <= 2 std per row, see inputs());
      y (|x| + mean|x|) rstd |gamma| + |beta|, times 1 / (1 - p);  dx, with g = dd gamma: rstd (|g| + mean|g| + |xh| mean|g xh|);
      dgamma sum_r |dd| (|x| + mean|x|) rstd;  dbeta sum_r |dd|;  dcol sum_r A(dx)."""
    x, dy, gamma, beta = x.double(), dy.double(), gamma.double(), beta.double()
    H = x.shape[-1]
    s_in, s2 = keep_scale(p_in), keep_scale(p2)
    kin = torch.ones_like(x, dtype=torch.bool) if keep_in is None else keep_in
    k2 = torch.ones_like(x, dtype=torch.bool) if keep2 is None else keep2
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    ax = x.abs().mean(-1, keepdim=True)
    y = torch.where(kin, (xh * gamma + beta) * s_in, torch.zeros_like(x))
    A_y = torch.where(kin, ((x.abs() + ax) * rstd * gamma.abs() + beta.abs()) * s_in, torch.zeros_like(x))
    dd = torch.where(kin, dy * s_in, torch.zeros_like(x))
    g = dd * gamma
    s1 = g.mean(-1, keepdim=True)
    s2m = (g * xh).mean(-1, keepdim=True)
    dx = rstd * (g - s1 - xh * s2m)
    A_dx = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    dxd = torch.where(k2, dx * s2, torch.zeros_like(x))
    A_dxd = torch.where(k2, A_dx * s2, torch.zeros_like(x))
    v = dict(mean=mean[:, 0], rstd=rstd[:, 0], y=y, dx=dx, dxd=dxd, dgamma=(dd * xh).sum(0), dbeta=dd.sum(0), dcol=dxd.sum(0),
             dcol_dx=dx.sum(0))
    A = dict(mean=ax[:, 0], rstd=rstd[:, 0], y=A_y, dx=A_dx, dxd=A_dxd, dgamma=(dd.abs() * (x.abs() + ax) * rstd).sum(0), dbeta=dd.abs().sum(0),
             dcol=A_dxd.sum(0), dcol_dx=A_dx.sum(0))
    return SimpleNamespace(v=v, A=A, xh=xh, dd=dd, g=g, rows=x.shape[0], H=H)


def fp32_statement(x, dy, gamma, beta, eps, keep_in=None, p_in=0.0, keep2=None, p2=0.0):
    """The same operation as plain fp32 torch on the CPU: native_layer_norm, its autograd, .sum(0).  -> dict of fp32 tensors."""
    H = x.shape[-1]
    xf = x.float().clone().requires_grad_(True)
    gr, br = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(xf, (H,), gr, br, eps)
    s_in = torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(p_in, dtype=torch.float32))
    s2 = torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(p2, dtype=torch.float32))
    dd, yo = dy.float(), y.detach()
    if keep_in is not None:
        dd = torch.where(keep_in, dd * s_in, torch.zeros_like(dd))
        yo = torch.where(keep_in, yo * s_in, torch.zeros_like(yo))
    y.backward(dd)
    dx = xf.grad
    dxd = dx if keep2 is None else torch.where(keep2, dx * s2, torch.zeros_like(dx))
    return dict(mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1), y=yo, dx=dx, dxd=dxd, dgamma=gr.grad, dbeta=br.grad,
                dcol=dxd.sum(0), dcol_dx=dx.sum(0))


# ---------------------------------------------------------------------------------------------- input sets
# H lists per dtype: the half-wave fast instantiations (32 and 24 data lanes) and row lengths only the generic kernels hold
FAST_H = {"bf16": (256, 512, 768, 1024, 192, 384), "f32": (128, 256, 384, 512, 768, 1024, 96, 192)}
GENERIC_H = {"bf16": (8, 24, 520, 640, 1280, 2048), "f32": (4, 20, 260, 640, 1020)}
DTYPES = ("f32", "bf16")
GRID_H = {"bf16": (768, 192), "f32": (128, 768)}          # fast backward, atomic form: a second pass from row 2048
GRID_ROWS = (2059, 4101)
PARTIAL = {"bf16": (8205, 256), "f32": (8205, 128)}       # partial form: 1024 workgroups, a second pass from row 8192
GENERIC_ROWS = (1030, 2053)                               # generic backward: 256 workgroups of 4 rows, a second pass from row 1024
DET_ROWS = {"bf16": (129, 513, 2059), "f32": (65, 257, 2059)}
DET_H = {"bf16": (24, 520, 768), "f32": (20, 260, 768)}
MASK_P = (0.1, 0.3)
MASK_FAST = {"bf16": (15, 256), "f32": (15, 128)}         # the same flat index range as the generic [., 640] below
MASK_GENERIC = {"bf16": (6, 640), "f32": (3, 640)}
SLICED = (3, 50, 20)                                      # a [3, 50, H] buffer, slices of 20 rows per batch
SLICED_H = (256, 640)
SEED_IN, SEED2 = 11, 9

# one input set: x, dy of `dtype` [rows, H]; the forward's output dropout (p_in, seed_in); the second backward output's (p2, seed2)
Case = namedtuple("Case", "dtype rows H p_in seed_in p2 seed2")


def plain(dt, rows, H):
    return Case(dt, rows, H, 0.0, 0, 0.0, 0)


def fwd_cases():
    return [plain(dt, rows, H) for dt in DTYPES for H in FAST_H[dt] + GENERIC_H[dt] for rows in (1, 13)]


def bwd_cases():
    return [plain(dt, 13, H) for dt in DTYPES for H in FAST_H[dt] + GENERIC_H[dt]]


def grid_cases():
    return [Case(dt, rows, H, 0.0, 0, 0.2, SEED2) for dt in DTYPES for H in GRID_H[dt] for rows in GRID_ROWS]


def partial_cases():
    return [plain(dt, *PARTIAL[dt]) for dt in DTYPES]


def generic_cases():
    return [Case(dt, rows, 640, 0.0, 0, 0.2, SEED2) for dt in DTYPES for rows in GENERIC_ROWS]


def det_cases():
    return [Case(dt, rows, H, 0.1, SEED_IN, 0.2, SEED2) for dt in DTYPES for rows in DET_ROWS[dt] for H in DET_H[dt]]


def mask_cases():
    return [Case(dt, rows, H, p, seed, p, seed + 66) for dt in DTYPES for (rows, H) in (MASK_FAST[dt], MASK_GENERIC[dt])
            for p in MASK_P for seed in (SEED_IN, SEED_IN + 1)]


def sliced_cases():
    B, _, S = SLICED
    return [Case(dt, B * S, H, 0.1, SEED_IN, 0.0, 0) for dt in DTYPES for H in SLICED_H]


def all_cases():
    seen, out = set(), []
    for c in fwd_cases() + bwd_cases() + grid_cases() + partial_cases() + generic_cases() + det_cases() + mask_cases() + sliced_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def case_id(c):
    s = f"{c.dtype}-{c.rows}x{c.H}"
    if c.p_in > 0:
        s += f"-in{c.p_in}s{c.seed_in}"
    if c.p2 > 0:
        s += f"-two{c.p2}s{c.seed2}"
    return s


@functools.lru_cache(maxsize=4)
def inputs(dtype, rows, H):
    """CPU tensors x, dy ([rows, H], `dtype`) and gamma, beta (fp32 [H]) as the existing LayerNorm tests draw them: x = randn * 2 +
    0.3, gamma near 1, beta = 0.5 + 0.1 randn (a mask can be read off y == 0).  A row whose |mean| exceeds 1.5 times its standard
    deviation (possible at H = 4 or 8) is drawn again: the bound on rstd is relative, which needs |mean| <= 2 std per row."""
    g = torch.Generator().manual_seed(rows * 10007 + H * 3 + (1 if dtype == "bf16" else 0))
    td = TORCH_DTYPE[dtype]
    x = (torch.randn(rows, H, generator=g) * 2 + 0.3).to(td)
    for _ in range(64):
        xd = x.double()
        bad = xd.mean(1).abs() > 1.5 * xd.std(1, unbiased=False)
        if not bool(bad.any()):
            break
        x[bad] = (torch.randn(int(bad.sum()), H, generator=g) * 2 + 0.3).to(td)
    gamma = 1 + 0.1 * torch.randn(H, generator=g)
    beta = 0.5 + 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(rows, H, generator=g).to(td)
    return x, dy, gamma, beta


def case_masks(c):
    keep_in = keep_mask(c.seed_in, c.rows, c.H, c.p_in) if c.p_in > 0 else None
    keep2 = keep_mask(c.seed2, c.rows, c.H, c.p2) if c.p2 > 0 else None
    return keep_in, keep2


@functools.lru_cache(maxsize=2)
def case_reference(c):
    """reference() of one input set, computed once and shared; nobody writes to it."""
    x, dy, gamma, beta = inputs(c.dtype, c.rows, c.H)
    keep_in, keep2 = case_masks(c)
    return reference(x, dy, gamma, beta, EPS, keep_in, c.p_in, keep2, c.p2)


def case_statement(c):
    x, dy, gamma, beta = inputs(c.dtype, c.rows, c.H)
    keep_in, keep2 = case_masks(c)
    return fp32_statement(x, dy, gamma, beta, EPS, keep_in, c.p_in, keep2, c.p2)


def statement_ratios(c, st=None):
    """{kind: largest |fp32 statement - float64| / (2^-23 A)} of one input set"""
    ref = case_reference(c)
    st = case_statement(c) if st is None else st
    out = {}
    for kind in ROW_KINDS + COL_KINDS:
        diff = (st[kind].double() - ref.v[kind]).abs()
        assert bool(torch.isfinite(diff).all())
        out[kind] = float(torch.where(diff > 0, diff / (UNIT * ref.A[kind]).clamp_min(1e-300), torch.zeros_like(diff)).max())
    return out


if __name__ == "__main__":
    top = {}
    for case in all_cases():
        for kind, r in statement_ratios(case).items():
            if r > top.get(kind, (0.0, None))[0]:
                top[kind] = (r, case_id(case))
    for kind, (r, where) in top.items():
        print(f"{kind:7s} ratio {r:.3f} at {where}  ->  k = {max(16.0, 8.0 * r):.1f}")
