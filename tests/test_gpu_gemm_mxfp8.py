"""peneo_gemm_mxfp8 and peneo_mxfp8_quantize_rows_bf16 (gemm_mx.hip, pair_heads_mx.hip): the bf16 quantizer bit for bit, an exact-integer
GEMM that pins the lane map and the scale ownership, random data against the fp64 product of the dequantized operands within a
DERIVED bound, the epilogues, the MX output, refusals and repeatability."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BASE = [(5672, 2304, 768), (5672, 768, 768), (5672, 3072, 768), (5672, 768, 3072)]
LARGE = [(2442, 3072, 1024), (2442, 1024, 1024), (2442, 4096, 1024), (2442, 1024, 4096)]
SMALL = [(1, 768, 768), (31, 768, 768), (129, 768, 768), (200, 32, 768), (200, 768, 128), (1, 32, 128)]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


# ---- torch emulation of the contract (include/peneo_hip.h) ---------------------------------------------------------------------
def mx_emulate(v: torch.Tensor):
    """[..., K] -> (e4m3 bytes, E8M0 bytes, dequantized fp64 values) per OCP MX block of 32 along the last dim."""
    vb = v.float().reshape(*v.shape[:-1], v.shape[-1] // 32, 32)
    amax = vb.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(amax)                                  # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex - 9, torch.full_like(ex, -127)).clamp(-127, 127)
    scaled = (vb.double() * torch.pow(2.0, -e.double())).float()   # exact power-of-two division
    q = scaled.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    deq = q.double() * torch.pow(2.0, e.double())
    return (q.view(torch.uint8).reshape(v.shape), (e + 127).to(torch.uint8).squeeze(-1), deq.reshape(v.shape))


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes [R, K] and E8M0 bytes [R, K / 32] -> fp64 values."""
    v = q.view(torch.float8_e4m3fn).double().reshape(q.shape[0], -1, 32)
    return (v * torch.pow(2.0, s.double() - 127.0).unsqueeze(-1)).reshape(q.shape)


def operands(M, N, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn((M, K), device=DEV, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), device=DEV, generator=g).float())
    w = torch.randn((N, K), device=DEV, generator=g) * 0.05
    aq, as_, ad = mx_emulate(a)
    wq, ws, wd = mx_emulate(w)
    return aq, as_, ad, wq, ws, wd


def bound(K, absum, want, bf16_out):
    """fp32 accumulation of K exact products in unknown order is within K 2^-24 sum|.| for round-to-nearest; a factor 4 covers a
    truncating adder inside the MFMA.  A bf16 C adds one rounding, |want| 2^-8."""
    b = K * 2.0 ** -22 * absum
    return b + want.abs() * 2.0 ** -8 if bf16_out else b


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def report(tag, got, want, tol):
    err = (got.double() - want).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{tag}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    return worst


# ---- 1. the bf16 quantizer -----------------------------------------------------------------------------------------------------
def quantizer_inputs():
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((257, 768), device=DEV, generator=g)
    x[3, 64:96] = 0.0                                                   # an all-zero block
    x[5] = 0.0
    mag = torch.exp(torch.empty((300, 256), device=DEV).uniform_(math.log(1e-3), math.log(1e2), generator=g))
    sign = torch.where(torch.rand((300, 256), device=DEV, generator=g) < 0.5, -1.0, 1.0)
    p2 = torch.randn((64, 128), device=DEV, generator=g).clamp(-0.99, 0.99)
    p2[:, ::32] = 1.0                                                   # amax exactly a power of two ...
    p2 = p2 * torch.exp2(torch.randint(-20, 20, (64, 1), device=DEV, generator=g).float())   # ... of many sizes
    tiny = torch.randn((16, 64), device=DEV, generator=g) * 1e-37      # scale clamp at the small end
    return [x, mag * sign, p2, tiny]


def test_bf16_quantizer_is_bit_identical_to_the_emulation_and_to_the_fp32_quantizer(ops):
    for v in quantizer_inputs():
        vb = v.to(torch.bfloat16)
        q, s = ops.mxfp8_quantize_rows_bf16(vb)
        eq, es, _ = mx_emulate(vb.float())
        assert torch.equal(q, eq) and torch.equal(s, es)
        q32, s32 = ops.mxfp8_quantize_rows(vb.float())
        assert torch.equal(q, q32) and torch.equal(s, s32)
    # a strided source (row stride > cols)
    wide = torch.randn((40, 512), device=DEV).to(torch.bfloat16)
    q, s = ops.mxfp8_quantize_rows_bf16(wide[:, 128:384])
    eq, es, _ = mx_emulate(wide[:, 128:384].float())
    assert torch.equal(q, eq) and torch.equal(s, es)


# ---- 2. exact arithmetic: lane map and scale ownership --------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(160, 96, 256), (129, 160, 384)])
def test_exact_integer_gemm_pins_the_lane_map_and_the_scales(ops, M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    ai = torch.randint(-4, 5, (M, K), device=DEV, generator=g).float()
    wi = torch.randint(-4, 5, (N, K), device=DEV, generator=g).float()
    # every row and every K block its own scale 2^e, e in 0..3 (a) and 0..3 (w), arranged so that neighbours differ in row AND block;
    # |product| <= 16 * 64, a row sum <= 2^10 K < 2^24: every partial sum is an integer below 2^24, exact in fp32 in any order
    ae = (torch.arange(M, device=DEV)[:, None] * 3 + torch.arange(K // 32, device=DEV)[None, :] * 5) % 4
    we = (torch.arange(N, device=DEV)[:, None] * 7 + torch.arange(K // 32, device=DEV)[None, :] * 3 + 1) % 4
    aq = ai.to(torch.float8_e4m3fn).view(torch.uint8)
    wq = wi.to(torch.float8_e4m3fn).view(torch.uint8)
    as_ = (ae + 127).to(torch.uint8).contiguous()
    ws = (we + 127).to(torch.uint8).contiguous()
    want = (dequant(aq, as_) @ dequant(wq, ws).t())
    assert float(want.abs().max()) < 2 ** 24
    got = ops.gemm_mxfp8(aq, as_, wq, ws, out_dtype=torch.float32)
    assert torch.equal(got.double(), want)


# ---- 3. random data, derived bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", BASE + LARGE + SMALL)
def test_random_gemm_against_the_fp64_product_of_the_dequantized_operands(ops, M, N, K):
    assert ops.gemm_mxfp8_supported(M, N, K)
    aq, as_, ad, wq, ws, wd = operands(M, N, K, seed=M + 3 * N + 7 * K)
    want = ad @ wd.t()
    absum = ad.abs() @ wd.abs().t()
    for dt in (torch.float32, torch.bfloat16):
        guard = torch.full((M + 2, N), 7.0, dtype=dt, device=DEV)          # rows past M must not be written
        got = ops.gemm_mxfp8(aq, as_, wq, ws, out=guard[:M])
        tol = bound(K, absum, want, dt == torch.bfloat16)
        worst = report(f"M={M} N={N} K={K} {dt}", got, want, tol)
        assert worst <= 1.0
        assert bool((guard[M:] == 7.0).all())


# ---- 4. the epilogues ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bias", "bias_gelu", "bias_residual", "alpha"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_epilogues(ops, case, dt):
    from peneo_amd.hip import ACT_GELU, ACT_NONE
    M, N, K = 300, 768, 768
    aq, as_, ad, wq, ws, wd = operands(M, N, K, seed=5)
    g = torch.Generator(device=DEV).manual_seed(6)
    bias = torch.randn(N, device=DEV, generator=g)
    res = torch.randn((M, N), device=DEV, generator=g).to(dt)
    acc = ad @ wd.t()
    absum = ad.abs() @ wd.abs().t()
    kw = {}
    if case == "alpha":
        kw["alpha"] = 0.375
        want, absum = 0.375 * acc, 0.375 * absum
    else:
        kw["bias"] = bias
        want, absum = acc + bias.double(), absum + bias.abs().double()
    tol = K * 2.0 ** -22 * absum
    if case == "bias_gelu":
        kw["act"] = ACT_GELU
        want = gelu64(want)
        tol = 1.13 * tol + 5e-5         # GELU's largest slope; the documented error of the polynomial erf (csrc/common.h gelu_fast_f)
    if case == "bias_residual":
        kw["residual"] = res
        want = want + res.double()
        tol = tol + K * 2.0 ** -22 * res.double().abs()
    if dt == torch.bfloat16:
        tol = tol + want.abs() * 2.0 ** -8
    got = ops.gemm_mxfp8(aq, as_, wq, ws, out_dtype=dt, **kw)
    assert report(f"{case} {dt}", got, want, tol) <= 1.0


# ---- 5. MX output -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(300, 3072, 768), (129, 96, 128)])
def test_mx_output_equals_the_quantizer_on_the_bf16_result(ops, M, N, K):
    from peneo_amd.hip import ACT_GELU
    aq, as_, ad, wq, ws, wd = operands(M, N, K, seed=9)
    bias = torch.randn(N, device=DEV)
    c, cq, cs = ops.gemm_mxfp8(aq, as_, wq, ws, bias=bias, act=ACT_GELU, mx_out=True)
    assert c.dtype == torch.bfloat16
    q, s = ops.mxfp8_quantize_rows_bf16(c)
    assert torch.equal(cq, q) and torch.equal(cs, s)
    none, cq2, cs2 = ops.gemm_mxfp8(aq, as_, wq, ws, bias=bias, act=ACT_GELU, mx_out=True, store_c=False)
    assert none is None
    assert torch.equal(cq2, q) and torch.equal(cs2, s)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ops):
    from peneo_amd import hip
    lib = hip.lib()
    M, N, K = 64, 64, 128
    aq, as_, ad, wq, ws, wd = operands(M, N, K, seed=2)
    out = torch.full((M, N), 3.0, dtype=torch.float32, device=DEV)
    cq = torch.zeros((M, N), dtype=torch.uint8, device=DEV)
    cs = torch.zeros((M, N // 32), dtype=torch.uint8, device=DEV)
    other = torch.zeros((M, N), dtype=torch.float32, device=DEV)

    def call(ep=None, a=aq, c=out, n=N, k=K, c_q=None, c_s=None):
        return lib.peneo_gemm_mxfp8(M, n, k, a.data_ptr() if hasattr(a, "data_ptr") else a, as_.data_ptr(), wq.data_ptr(), ws.data_ptr(),
                                    c.data_ptr() if hasattr(c, "data_ptr") else c, n, hip.F32, C.byref(ep) if ep is not None else None,
                                    c_q, c_s, hip.stream())

    def ep_with(**kw):
        e = hip.GemmEpilogue()
        for k_, v in kw.items():
            setattr(e, k_, v)
        return e
    bad = [ep_with(preact=other.data_ptr(), ld_preact=N), ep_with(grad_src=other.data_ptr(), ld_grad=N, grad_act=hip.ACT_GELU),
           ep_with(drop_p=0.1), ep_with(accumulate=1), ep_with(pair_dz=other.data_ptr()), ep_with(a_colsum=other.data_ptr()),
           ep_with(act=hip.ACT_SILU)]
    for e in bad:
        assert call(e) == -1
    assert call(a=aq.data_ptr() + 4) == -1                                # misaligned A_q
    assert call(c=out.data_ptr() + 4) == -1                               # misaligned C
    assert call(ep_with(bias=other.data_ptr() + 4)) == -1                 # misaligned bias
    assert call(ep_with(residual=other.data_ptr() + 8, ld_res=N)) == -1   # misaligned residual
    assert call(n=48, c_q=cq.data_ptr(), c_s=cs.data_ptr()) == -1         # MX output with N % 32 != 0
    assert call(k=96) == -1                                               # unsupported K
    assert call(c_q=cq.data_ptr()) == -1                                  # C_q without C_s
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and int(cq.sum()) == 0 and int(cs.sum()) == 0
    assert call() == 0                                                    # ... and the plain call runs
    torch.cuda.synchronize()
    assert not bool((out == 3.0).all())


# ---- 7. repeatability ---------------------------------------------------------------------------------------------------------
def test_three_launches_are_bit_identical(ops):
    from peneo_amd.hip import ACT_GELU
    M, N, K = 5672, 3072, 768
    aq, as_, ad, wq, ws, wd = operands(M, N, K, seed=4)
    bias = torch.randn(N, device=DEV)
    runs = [ops.gemm_mxfp8(aq, as_, wq, ws, bias=bias, act=ACT_GELU, mx_out=True) for _ in range(3)]
    for r in runs[1:]:
        for x, y in zip(r, runs[0]):
            assert torch.equal(x, y)
