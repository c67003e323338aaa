"""Weight-gradient GEMM C[M][N] = A[K][M]^T B[K][N] on 384 x 192 one-per-CU tiles with split-k (gemm_big.hip, launch_gemm_big_nn):
the path the pair heads' dW1 = dz^T x takes.  Forced on with peneo_gemm_set_nn384_mode(2) (the rule without its bound on K) and
compared with the same call under mode 0 (the 128 x 128 kernel).

Exact cases use small integers in [-4, 4] as bf16 and K <= 448: every product is an integer of magnitude <= 16, every partial sum
one of magnitude <= 7168 < 2^24, so every fp32 sum is exact in ANY order and the result must equal the float64 matmul bit for
bit; a dropped, doubled or misplaced k-tile or output tile fails outright.

Which kernel ran is read from peneo_gemm_nn384_launches (the calls that took the path): with the same split both kernels add the
same 16-deep MFMA steps in the same order, so their results are equal bit for bit and cannot tell."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


@pytest.fixture()
def nn(ops):
    """Setter of the path's mode; back to the mode the test found when it ends."""
    from peneo_amd import hip
    lib = hip.lib()
    before = lib.peneo_gemm_nn384_mode()
    yield lib.peneo_gemm_set_nn384_mode
    lib.peneo_gemm_set_nn384_mode(before)


def launches():
    from peneo_amd import hip
    return hip.lib().peneo_gemm_nn384_launches()


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).to(BF)


def exact(a, b):
    """fp32 image of the float64 product of the (integer) operands: a is [K, M], b is [K, N]."""
    return (a.double().t() @ b.double()).float()


@pytest.mark.parametrize("M,N", [(384, 192), (768, 384), (1920, 384)])
def test_exact_placement(ops, nn, M, N):
    """K = 64: one k-tile (split clamped to 1); 128: the ring without wrap-around; 192: the wrap at 2 stages; 448 with split 3:
    ranges of 3, 3 and 1 k-tiles, the last one shorter than the ring.  Every K with split 1, 2 and 3."""
    g = torch.Generator().manual_seed(M + N)
    nn(2)
    for K in (64, 128, 192, 448):
        a, b = ints(g, K, M), ints(g, K, N)
        want = exact(a, b)
        a, b = a.to(DEV), b.to(DEV)
        for split in (1, 2, 3):
            out = torch.full((M, N), float("nan"), device=DEV)
            n0 = launches()
            ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out=out, split_k=split)
            assert launches() == n0 + 1
            assert torch.equal(out.cpu(), want), (K, split)


def test_strided_operands_and_output(ops, nn):
    """A is a 384-column block at a column offset inside a [K, 1920] buffer (lda = 1920, as one head of dz), B a block inside a
    wider buffer, C a block inside a wider fp32 buffer whose other columns must stay as they were."""
    g = torch.Generator().manual_seed(11)
    nn(2)
    K, M, N = 448, 384, 192
    abuf, bbuf = ints(g, K, 1920), ints(g, K, 448)
    want = exact(abuf[:, 768:768 + M], bbuf[:, 64:64 + N])
    abuf, bbuf = abuf.to(DEV), bbuf.to(DEV)
    for split in (1, 3):
        cbuf = torch.full((M, N + 128), 7.0, device=DEV)
        n0 = launches()
        ops.gemm(abuf[:, 768:768 + M], bbuf[:, 64:64 + N], a_kmajor=False, b_kmajor=False, out=cbuf[:, 64:64 + N], split_k=split)
        assert launches() == n0 + 1
        c = cbuf.cpu()
        assert torch.equal(c[:, 64:64 + N], want), split
        assert bool((c[:, :64] == 7.0).all()) and bool((c[:, 64 + N:] == 7.0).all()), split


def test_accumulate_into_nonzero_c(ops, nn):
    g = torch.Generator().manual_seed(12)
    nn(2)
    K, M, N = 448, 768, 384
    a, b = ints(g, K, M), ints(g, K, N)
    c0 = torch.randint(-1000, 1000, (M, N), generator=g).float()
    want = exact(a, b) + c0
    a, b = a.to(DEV), b.to(DEV)
    for split in (1, 3):
        out = c0.to(DEV)
        n0 = launches()
        ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out=out, split_k=split, accumulate=True)
        assert launches() == n0 + 1
        assert torch.equal(out.cpu(), want), split


@pytest.mark.parametrize("M,N,K,split", [(1920, 384, 64 * 37, 3), (768, 192, 64 * 5, 1)])
def test_random_operands_match_fp32_matmul_and_the_128_kernel(ops, nn, M, N, K, split):
    """rel_err < 2e-3: the bound test_gemm_big_tiles_match_fp32_matmul holds the fp32 output of the big tiles to."""
    g = torch.Generator().manual_seed(K)
    a = torch.randn(K, M, generator=g).to(DEV).to(BF)
    b = torch.randn(K, N, generator=g).to(DEV).to(BF)
    z = a.float().t() @ b.float()
    outs = {}
    for mode in (2, 0):
        nn(mode)
        n0 = launches()
        outs[mode] = ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out_dtype=torch.float32, split_k=split)
        assert launches() == n0 + (1 if mode else 0)
    e_ref, e_old = rel_err(outs[2], z), rel_err(outs[2], outs[0])
    print(f"nn384 {M}x{N}x{K} split {split}: rel_err vs fp32 matmul {e_ref:.3e}, vs 128 x 128 kernel {e_old:.3e}")
    assert e_ref < 2e-3
    assert e_old < 2e-3


def test_other_callers_keep_their_kernel(ops, nn):
    """Problems outside the rule (M or N no multiple of the tile, a bf16 C, a_colsum) never reach the path, and give the same
    bits with it forced and with it off.  (The column sums are fp32 atomics whose order is free: integer A makes them exact.)"""
    g = torch.Generator().manual_seed(13)
    K = 64 * 9

    def run(M, N, **kw):
        a = torch.randn(K, M, generator=g).to(DEV).to(BF)
        b = torch.randn(K, N, generator=g).to(DEV).to(BF)
        if "a_colsum" in kw:
            a = ints(g, K, M).to(DEV)
        res = {}
        n0 = launches()
        for mode in (2, 0):
            nn(mode)
            k2 = dict(kw)
            if "a_colsum" in kw:
                k2["a_colsum"] = torch.zeros(M, device=DEV)
            res[mode] = (ops.gemm(a, b, a_kmajor=False, b_kmajor=False, split_k=3, **k2), k2.get("a_colsum"))
        assert launches() == n0, (M, N, kw)
        assert torch.equal(res[2][0], res[0][0]), (M, N, kw)
        if "a_colsum" in kw:
            assert torch.equal(res[2][1], res[0][1]) and torch.equal(res[2][1].cpu(), a.float().sum(0).cpu())

    run(1920 + 8, 384, out_dtype=torch.float32)
    run(1920, 200, out_dtype=torch.float32)
    run(1920, 384, out_dtype=BF)
    run(768, 384, out_dtype=torch.float32, a_colsum=True)


def test_big_tiles_off_switches_the_path_off(ops, nn):
    """peneo_gemm_set_big_mode(0) (PENEO_GEMM_BIG=0) takes this path with it; the rule's bound on K holds in mode 1."""
    from peneo_amd import hip
    lib = hip.lib()
    big = lib.peneo_gemm_big_mode()
    try:
        nn(2)
        lib.peneo_gemm_set_big_mode(1)
        assert lib.peneo_gemm_nn384_mode() == 2 and lib.peneo_gemm_nn384_shape_ok(768, 192, 64) == 1
        lib.peneo_gemm_set_big_mode(0)
        assert lib.peneo_gemm_nn384_mode() == 0 and lib.peneo_gemm_nn384_shape_ok(768, 192, 64) == 0
    finally:
        lib.peneo_gemm_set_big_mode(big)
    g = torch.Generator().manual_seed(14)
    a = torch.randn(64 * 9, 768, generator=g).to(DEV).to(BF)
    b = torch.randn(64 * 9, 192, generator=g).to(DEV).to(BF)
    outs = {}
    n0 = launches()
    for mode in (1, 0):       # K = 576 is below the bound: mode 1 leaves it on the 128 x 128 kernel
        nn(mode)
        outs[mode] = ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out_dtype=torch.float32, split_k=3)
    assert launches() == n0
    assert torch.equal(outs[1], outs[0])


def test_default_rule_takes_deep_problems_only(ops, nn):
    """Mode 1, the rule as shipped: K = 65536 takes the path (with the split ops.gemm picks for it when the caller names none, and
    with a named one), K = 65536 - 64 keeps the 128 x 128 kernel.  Integer operands: every sum stays below 16 x 65536 = 2^20, exact."""
    from peneo_amd import hip
    lib = hip.lib()
    big = lib.peneo_gemm_big_mode()
    g = torch.Generator().manual_seed(15)
    M, N = 384, 192
    try:
        lib.peneo_gemm_set_big_mode(1)
        nn(1)
        for K, taken in ((65536, 1), (65536 - 64, 0)):
            assert lib.peneo_gemm_nn384_shape_ok(M, N, K) == taken
            assert ops.gemm_nn384_takes(M, N, K, BF) == bool(taken)
            a, b = ints(g, K, M), ints(g, K, N)
            want = exact(a, b)
            a, b = a.to(DEV), b.to(DEV)
            for split in (None, 6):
                out = torch.full((M, N), float("nan"), device=DEV)
                n0 = launches()
                ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out=out, split_k=split)
                assert launches() == n0 + taken, (K, split)
                assert torch.equal(out.cpu(), want), (K, split)
        assert ops.choose_split_k_nn384(1920, 384, 1081344) == 25 and ops.choose_split_k_nn384(384, 192, 65536) == 128
    finally:
        lib.peneo_gemm_set_big_mode(big)


def test_short_workspace_is_refused(ops, nn):
    """split_k = 3 with a null workspace or one a byte short: the existing error, nothing launched (C keeps its sentinel)."""
    from peneo_amd import hip
    lib = hip.lib()
    nn(2)
    M, N, K = 768, 384, 448
    a = torch.ones(K, M, dtype=BF, device=DEV)
    b = torch.ones(K, N, dtype=BF, device=DEV)
    c = torch.full((M, N), 7.0, device=DEV)
    ep = hip.GemmEpilogue()
    need = lib.peneo_gemm_workspace_bytes(M, N, K, 3)
    assert need >= 3 * M * N * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    n0 = launches()
    for ws_ptr, ws_bytes in [(None, 0), (ws.data_ptr(), need - 1)]:
        rc = lib.peneo_gemm(hip.BF16, 0, 0, M, N, K, a.data_ptr(), M, b.data_ptr(), N, c.data_ptr(), N, hip.F32, ctypes.byref(ep),
                            3, ws_ptr, ws_bytes, hip.stream())
        assert rc == -1
        assert b"split-k workspace too small" in lib.peneo_last_error()
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()) and launches() == n0
