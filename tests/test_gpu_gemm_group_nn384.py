"""Encoder weight gradients on 384 x 192 one-per-CU tiles (gemm_big.hip): the ragged last k-tile of the (mn, mn) kernel
(K % 8 == 0 in place of K % 64 == 0) and the grouped launch peneo_gemm_group routes to under PENEO_WGRAD_NN384 /
peneo_gemm_group_set_nn384_mode.

The integer scheme of test_gpu_gemm_nn384.py: operands are integers in [-4, 4] as bf16 and K <= 232, so every product is an
integer of magnitude <= 16 and every partial sum one of magnitude <= 3712 < 2^24: every fp32 sum is exact in ANY order and the
result must equal the float64 product bit for bit.  A dropped, doubled or misplaced piece, k-tile or output tile fails outright,
and so does a row at or beyond K that enters the product (those rows hold NaN).

Which kernel ran is read from the launch counters: with the same k order both kernels give the same bits."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


@pytest.fixture()
def modes(ops):
    """(single-call setter, group setter); both modes go back to what the test found."""
    from peneo_amd import hip
    lib = hip.lib()
    nn, grp = lib.peneo_gemm_nn384_mode(), lib.peneo_gemm_group_nn384_mode()
    yield lib.peneo_gemm_set_nn384_mode, lib.peneo_gemm_group_set_nn384_mode
    lib.peneo_gemm_set_nn384_mode(nn)
    lib.peneo_gemm_group_set_nn384_mode(grp)


def single_launches():
    from peneo_amd import hip
    return hip.lib().peneo_gemm_nn384_launches()


def group_launches():
    from peneo_amd import hip
    return hip.lib().peneo_gemm_group_nn384_launches()


def ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).to(BF)


def exact(a, b):
    """fp32 image of the float64 product of the (integer) operands: a is [K, M], b is [K, N]."""
    return (a.double().t() @ b.double()).float()


def with_nan_rows(x, rows=64):
    """x as the first rows of a device tensor that goes on for `rows` rows of NaN."""
    buf = torch.cat([x, torch.full((rows, x.shape[1]), NAN, dtype=x.dtype)]).to(DEV)
    return buf[:x.shape[0]]


def at_allocation_end(x):
    """x as the LAST bytes of a device allocation of its own: the operand ends exactly at row K."""
    n = x.numel()
    buf = torch.empty(n + 4096, dtype=x.dtype, device=DEV)
    view = buf[4096:].view(x.shape)
    view.copy_(x)
    return view


# K: 8 one piece; 40 a tail and nothing else; 64 one full k-tile, no tail; 104 one full k-tile + tail; 168 the ring wraps at two
# stages, then the tail; 232 three full k-tiles + tail
RAGGED_K = (8, 40, 64, 104, 168, 232)


@pytest.mark.parametrize("M,N", [(384, 192), (768, 384)])
@pytest.mark.parametrize("place", ["nan_rows_behind", "allocation_end"])
def test_ragged_k_single_call(ops, modes, M, N, place):
    """Every K with split 1, 2 and 3.  The operands' rows at and beyond K are NaN (or do not exist: the kernel requests no piece
    whose rows lie there - read in gemm_big_body's tail; only the NaN case can fail).  C sits inside a wider NaN-filled buffer: every
    element of C is written, nothing outside it is."""
    set_nn, _ = modes
    set_nn(2)
    g = torch.Generator().manual_seed(M + N + len(place))
    put = with_nan_rows if place == "nan_rows_behind" else at_allocation_end
    for K in RAGGED_K:
        a, b = ints(g, K, M), ints(g, K, N)
        want = exact(a, b)
        a, b = put(a), put(b)
        for split in (1, 2, 3):
            cbuf = torch.full((M, N + 64), NAN, device=DEV)
            n0 = single_launches()
            ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out=cbuf[:, :N], split_k=split)
            assert single_launches() == n0 + 1, (K, split)
            c = cbuf.cpu()
            assert torch.equal(c[:, :N], want), (K, split)
            assert bool(c[:, N:].isnan().all()), (K, split)


def test_ragged_k_shape_rule(ops, modes):
    from peneo_amd import hip
    lib = hip.lib()
    set_nn, _ = modes
    set_nn(2)
    assert lib.peneo_gemm_nn384_shape_ok(384, 192, 8) == 1 and lib.peneo_gemm_nn384_shape_ok(768, 384, 5672) == 1
    assert lib.peneo_gemm_nn384_shape_ok(384, 192, 12) == 0 and lib.peneo_gemm_nn384_shape_ok(384, 192, 0) == 0
    set_nn(1)      # the bound on K of single calls stays
    assert lib.peneo_gemm_nn384_shape_ok(768, 384, 5672) == 0 and lib.peneo_gemm_nn384_shape_ok(384, 192, 65536 + 8) == 1


GROUP_SHAPES = [(384, 192), (768, 192), (384, 576), (768, 384)]


def run_group(problems, accumulate):
    """problems: (A view [K, M], B view [K, N], C view [M, N]); accumulate: one flag per problem.  The C call itself."""
    from peneo_amd import hip
    lib = hip.lib()
    n = len(problems)
    arr = (hip.GemmProblem * n)()
    for q, (a, b, c), acc in zip(arr, problems, accumulate):
        q.M, q.N, q.K = a.shape[1], b.shape[1], a.shape[0]
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0)
        q.accumulate = int(acc)
    rc = lib.peneo_gemm_group(hip.BF16, 0, 0, hip.F32, arr, n, hip.stream())
    assert rc == 0, lib.peneo_last_error()


def group_case(g, shapes, K):
    """Operands as column blocks of wider buffers (lda > M, ldb > N) whose rows beyond K are NaN; the second problem accumulates."""
    ops_, wants, c0s = [], [], []
    for i, (M, N) in enumerate(shapes):
        abuf, bbuf = ints(g, K, M + 64), ints(g, K, N + 128)
        a, b = abuf[:, 64:], bbuf[:, 64:64 + N]
        c0 = torch.randint(-1000, 1000, (M, N), generator=g).float() if i == 1 else torch.full((M, N), NAN)
        wants.append(exact(a, b) + (c0 if i == 1 else 0))
        ops_.append((with_nan_rows(abuf)[:, 64:], with_nan_rows(bbuf)[:, 64:64 + N]))
        c0s.append(c0)
    return ops_, wants, c0s


@pytest.mark.parametrize("K", [104, 168])
def test_group_exact_and_equal_to_the_128_group(ops, modes, K):
    """Four problems with 1, 2, 3 and 4 tiles in one call.  Each C is exact and bit-equal to the same call under mode 0; the counter
    rises by one per call under mode 1 and by zero under mode 0."""
    _, set_grp = modes
    g = torch.Generator().manual_seed(K)
    operands, wants, c0s = group_case(g, GROUP_SHAPES, K)
    outs = {}
    for mode in (1, 0):
        set_grp(mode)
        cbufs = [torch.full((c0.shape[0], c0.shape[1] + 64), NAN, device=DEV) for c0 in c0s]
        for cb, c0 in zip(cbufs, c0s):
            cb[:, :c0.shape[1]] = c0.to(DEV)
        n0 = group_launches()
        run_group([(a, b, cb[:, :c0.shape[1]]) for (a, b), cb, c0 in zip(operands, cbufs, c0s)], [i == 1 for i in range(4)])
        assert group_launches() == n0 + mode
        outs[mode] = [cb.cpu() for cb in cbufs]
    for i, ((M, N), want) in enumerate(zip(GROUP_SHAPES, wants)):
        for mode in (1, 0):
            assert torch.equal(outs[mode][i][:, :N], want), (mode, i)
            assert bool(outs[mode][i][:, N:].isnan().all()), (mode, i)


def test_group_falls_back_as_a_whole(ops, modes):
    """One problem outside the rule (M = 256): the whole call keeps the 128 x 128 group - the counter does not move - and stays exact."""
    _, set_grp = modes
    set_grp(1)
    g = torch.Generator().manual_seed(3)
    shapes = [(384, 192), (256, 192), (768, 384)]
    operands, wants, c0s = group_case(g, shapes, 104)
    cs = [c0.to(DEV) for c0 in c0s]
    n0 = group_launches()
    run_group([(a, b, c) for (a, b), c in zip(operands, cs)], [i == 1 for i in range(3)])
    assert group_launches() == n0
    for c, want in zip(cs, wants):
        assert torch.equal(c.cpu(), want)


def test_group_mode_follows_the_big_tile_switch(ops, modes):
    from peneo_amd import hip
    lib = hip.lib()
    _, set_grp = modes
    big = lib.peneo_gemm_big_mode()
    try:
        set_grp(2)
        lib.peneo_gemm_set_big_mode(1)
        assert lib.peneo_gemm_group_nn384_mode() == 2
        lib.peneo_gemm_set_big_mode(0)
        assert lib.peneo_gemm_group_nn384_mode() == 0
    finally:
        lib.peneo_gemm_set_big_mode(big)


# ---- the layer stage ----------------------------------------------------------------------------------------------------------
class Layer:
    """One encoder layer's buffers for the C stage calls at H = 384 (6 heads of 64), I = 768, B = 1, T = 104: the contraction of its
    weight gradients is R = 104 = one full k-tile + a tail of 40, and each of their shapes is whole 384 x 192 tiles."""

    def __init__(self, ops, wgrad_last):
        from peneo_amd import hip
        self.hip, self.lib = hip, hip.lib()
        B, T, H, nh, I = 1, 104, 384, 6, 768
        R, Tp = B * T, ops.attn_padded_len(T)
        self.dims = (B, T, H, nh, I, R)
        g = torch.Generator().manual_seed(5)
        self.t = t = {}

        def bf(name, *shape, scale=1.0):
            t[name] = (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)

        def f32(name, *shape, scale=1.0, shift=0.0):
            t[name] = (torch.randn(*shape, generator=g) * scale + shift).to(DEV)

        bf("Wqkv", 3 * H, H, scale=0.05); bf("Wo", H, H, scale=0.05); bf("Wi", I, H, scale=0.05); bf("Wo2", H, I, scale=0.05)
        f32("bqkv", 3 * H, scale=0.1); f32("bo", H, scale=0.1); f32("bi", I, scale=0.1); f32("bo2", H, scale=0.1)
        f32("g1", H, scale=0.1, shift=1.0); f32("b1", H, scale=0.1); f32("g2", H, scale=0.1, shift=1.0); f32("b2", H, scale=0.1)
        bf("x", R, H)
        bf("d_out", R, H)
        bias = torch.zeros(B, nh, T, Tp)
        bias[..., T:] = -1e30
        t["bias"] = bias.to(BF).to(DEV)
        p_attn = 0.1
        t["words"] = ops.attn_drop_words(B, nh, T, p_attn, 1234, torch.device(DEV))
        for name, n in (("qkv", 3 * H), ("att", H), ("h1", H), ("a", H), ("h2", H), ("inter", I), ("zi", I), ("out", H)):
            t[name] = torch.zeros(R, n, dtype=BF, device=DEV)
        for name, n in (("lse", B * nh * T), ("m1", R), ("r1", R), ("m2", R), ("r2", R)):
            t[name] = torch.zeros(n, device=DEV)
        L = hip.EncoderLayer()
        for name in ("Wqkv", "bqkv", "Wo", "bo", "g1", "b1", "Wi", "bi", "Wo2", "bo2", "g2", "b2", "bias", "x", "qkv", "att", "lse", "h1",
                     "m1", "r1", "a", "zi", "inter", "h2", "m2", "r2"):
            setattr(L, name, t[name].data_ptr())
        L.bias_ld = Tp
        L.drop_words = t["words"].data_ptr()
        L.B, L.T, L.H, L.nh, L.I, L.wgrad_last = B, T, H, nh, I, int(wgrad_last)
        L.eps, L.attn_scale, L.p_hidden, L.p_attn = 1e-5, 0.125, 0.1, p_attn
        L.seed_o, L.seed_o2 = 77, 78
        self.L = L
        wsb = int(self.lib.peneo_encoder_layer_workspace_bytes(R, H, I, 0))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
        rc = self.lib.peneo_encoder_layer_fwd(ctypes.byref(L), t["out"].data_ptr(), ws.data_ptr() if wsb else None, wsb, hip.stream())
        assert rc == 0, self.lib.peneo_last_error()
        torch.cuda.synchronize()

    def backward(self, side):
        """-> {name: CPU tensor} of everything the backward writes (fresh zero- / NaN-filled outputs for every call)."""
        hip, lib = self.hip, self.lib
        B, T, H, nh, I, R = self.dims
        Tp = (T + 63) // 64 * 64
        o = {}
        for name, n in (("d_x", H), ("d_h2", H), ("d_dense2", H), ("d_a", H), ("d_h1", H), ("d_dense1", H), ("d_att", H), ("d_zi", I),
                        ("dqkv", 3 * H)):
            o[name] = torch.zeros(R, n, dtype=BF, device=DEV)
        o["delta"] = torch.zeros(B * nh * T, device=DEV)
        o["ds_out"] = torch.zeros(B, nh, T, Tp, dtype=BF, device=DEV)
        for name, shape in (("dwqkv", (3 * H, H)), ("dwo", (H, H)), ("dwi", (I, H)), ("dwo2", (H, I))):
            o[name] = torch.full(shape, NAN, device=DEV)       # overwritten: an unwritten tile stays NaN
        for name, n in (("dbqkv", 3 * H), ("dbo", H), ("dg1", H), ("db1", H), ("dbi", I), ("dbo2", H), ("dg2", H), ("db2", H)):
            o[name] = torch.zeros(n, device=DEV)               # accumulated into
        G = hip.EncoderLayerGrads()
        G.d_out = self.t["d_out"].data_ptr()
        for name, v in o.items():
            setattr(G, name, v.data_ptr())
        wmb, wsb = (int(lib.peneo_encoder_layer_workspace_bytes(R, H, I, w)) for w in (1, 2))
        wm = torch.empty(max(wmb, 16), dtype=torch.uint8, device=DEV)
        wsd = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        rc = lib.peneo_encoder_layer_bwd(ctypes.byref(self.L), ctypes.byref(G), wm.data_ptr() if wmb else None, wmb,
                                         wsd.data_ptr() if wsb else None, wsb, main.cuda_stream, side.cuda_stream)
        assert rc == 0, lib.peneo_last_error()
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items()}


def test_layer_backward_is_bit_equal_and_routed(ops, modes):
    """peneo_encoder_layer_bwd with a side stream and dropout on: every output is bit-equal between modes 0 and 1, the grouped
    384 x 192 launch ran once under mode 1, and not at all under mode 2 when the layer is marked as the backward's last."""
    from peneo_amd import hip
    with hip.deterministic(1):             # single-writer column sums and LayerNorm parameter gradients: runs can be compared bit for bit
        _layer_backward_modes(ops, modes)


def _layer_backward_modes(ops, modes):
    _, set_grp = modes
    side = torch.cuda.Stream()
    layer = Layer(ops, wgrad_last=False)
    res, ran = {}, {}
    for mode in (0, 1, 2):
        set_grp(mode)
        n0 = group_launches()
        res[mode] = layer.backward(side)
        ran[mode] = group_launches() - n0
    assert ran == {0: 0, 1: 1, 2: 1}       # mode 2, layer not marked: as mode 1
    for name, want in res[0].items():
        assert not bool(want.isnan().any()), name
        assert torch.equal(res[1][name], want), name
        assert torch.equal(res[2][name], want), name
    last = Layer(ops, wgrad_last=True)
    set_grp(2)
    n0 = group_launches()
    out = last.backward(side)
    assert group_launches() == n0
    for name, want in res[0].items():
        assert torch.equal(out[name], want), name
    set_grp(1)                             # the mark is read under mode 2 alone
    n0 = group_launches()
    last.backward(side)
    assert group_launches() == n0 + 1
