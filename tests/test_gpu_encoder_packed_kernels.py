"""Packed encoder for inference, the device code: peneo_pack_plan / peneo_rows_pack / peneo_rows_unpack against a torch
reference with sentinel-filled destinations, peneo_attn_fwd_varlen bit for bit against peneo_attn_fwd on each document alone, and
peneo_encoder_layer_fwd_packed at full lengths bit for bit against peneo_encoder_layer_fwd."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    return o


# ---- plan / pack / unpack -------------------------------------------------------------------------------------------------------
B, T = 5, 70


def _mask(kind):
    m = torch.ones((B, T), dtype=torch.int32)
    if kind == "ones":
        pass
    elif kind == "zeros":
        m.zero_()
    elif kind == "tail1":
        m[:, 1:] = 0
    elif kind == "tail33":
        m[:, 33:] = 0
    else:                                               # holes: another pattern per document, an empty one and a full one among them
        g = torch.Generator().manual_seed(11)
        m = (torch.rand((B, T), generator=g) < 0.6).to(torch.int32)
        m[1] = 0
        m[2] = 1
        m[3, 0], m[3, T - 1] = 0, 1
        m[4, :40] = 0
        m = m * torch.tensor([1, 1, 1, 1, 7])[:, None].to(torch.int32)    # (any non-zero value is "live")
    return m


def _plan_ref(m):
    lens = (m != 0).sum(1).to(torch.int32)
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    live = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        idx = (m[b] != 0).nonzero()[:, 0].to(torch.int32)
        live[b, :len(idx)] = idx
    return lens, cu, live


def _rows(row_bytes, seed):
    """src [B, T, row_bytes] as raw bytes with no zero byte anywhere, viewed as the dtype a row of that size has in the model"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(1, 256, (B, T, row_bytes), generator=g, dtype=torch.int16).to(torch.uint8)
    if row_bytes == 4:
        return raw.view(torch.int32).reshape(B, T)      # the int32 pos / xs / ys arrays
    return raw.view(BF16)                               # activations [B, T, row_bytes / 2]


@pytest.mark.parametrize("kind", ["ones", "zeros", "tail1", "tail33", "holes"])
def test_plan_pack_unpack(ops, kind):
    m = _mask(kind)
    lens_r, cu_r, live_r = _plan_ref(m)
    lens, cu, live = ops.pack_plan(m.to(DEV))
    assert torch.equal(lens.cpu(), lens_r) and torch.equal(cu.cpu(), cu_r) and torch.equal(live.cpu(), live_r)
    R, Tm = int(cu_r[B]), max(int(lens_r.max()), 1)
    SENT = 0x5A
    for row_bytes in (4, 48, 2 * 768):
        src = _rows(row_bytes, row_bytes)
        src_d = src.to(DEV)
        src_b = src.contiguous().view(torch.uint8).reshape(B, T, row_bytes)
        # per-document layout: every row written, zeros from lens[b] on
        want = torch.zeros((B, Tm, row_bytes), dtype=torch.uint8)
        for b in range(B):
            n = int(lens_r[b])
            want[b, :n] = src_b[b, live_r[b, :n].long()]
        out = torch.full((B, Tm) + tuple(src.shape[2:]), 0, dtype=src.dtype, device=DEV)
        out.view(torch.uint8).fill_(SENT)
        got = ops.rows_pack(src_d, live, lens, None, Tm, out=out)
        assert got is out and torch.equal(got.cpu().view(torch.uint8).reshape(B, Tm, row_bytes), want), (kind, row_bytes)
        # cu_rows layout: live rows only, two guard rows behind them keep the sentinel
        packed = torch.empty((R + 2,) + tuple(src.shape[2:]), dtype=src.dtype, device=DEV)
        packed.view(torch.uint8).fill_(SENT)
        want_p = torch.full((R + 2, row_bytes), SENT, dtype=torch.uint8)
        for b in range(B):
            n = int(lens_r[b])
            want_p[int(cu_r[b]):int(cu_r[b]) + n] = src_b[b, live_r[b, :n].long()]
        ops.rows_pack(src_d, live, lens, cu, Tm, out=packed)
        assert torch.equal(packed.cpu().view(torch.uint8).reshape(R + 2, row_bytes), want_p), (kind, row_bytes)
        # unpack: every row of [B, T] written - the live ones restored byte for byte, zeros elsewhere
        back = torch.empty((B, T) + tuple(src.shape[2:]), dtype=src.dtype, device=DEV)
        back.view(torch.uint8).fill_(SENT)
        ops.rows_unpack(packed, live, lens, cu, out=back)
        want_b = src_b * (m != 0).to(torch.uint8)[:, :, None]
        assert torch.equal(back.cpu().view(torch.uint8).reshape(B, T, row_bytes), want_b), (kind, row_bytes)
    if kind == "ones":
        assert R == B * T and Tm == T
    if kind == "zeros":
        assert R == 0


def test_pack_takes_the_dword_path_for_misaligned_bases(ops):
    """48-byte rows from a base that is 4- but not 16-byte aligned: the same bytes"""
    m = _mask("holes")
    lens_r, cu_r, live_r = _plan_ref(m)
    lens, cu, live = ops.pack_plan(m.to(DEV))
    R, Tm = int(cu_r[B]), int(lens_r.max())
    src = _rows(48, 5)
    hold = torch.empty(B * T * 24 + 2, dtype=BF16, device=DEV)
    src_d = hold[2:].view(B, T, 24)
    assert src_d.data_ptr() % 16 == 4
    src_d.copy_(src)
    got = ops.rows_pack(src_d, live, lens, cu, Tm, rows=R)
    want = torch.cat([src[b, live_r[b, :int(lens_r[b])].long()] for b in range(B)])
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    back = ops.rows_unpack(got, live, lens, cu)
    assert torch.equal(back.cpu().view(torch.int16), (src.view(torch.int16) * (m != 0)[:, :, None].to(torch.int16)))


# ---- per-document-length attention ----------------------------------------------------------------------------------------------
LENS = (0, 1, 31, 32, 33, 96, 128, 129, 197)
TM, NH, D = 197, 2, 64


def test_attn_fwd_varlen_is_attn_fwd_on_each_document_alone(ops):
    nb, H = len(LENS), NH * D
    Tp = ops.attn_padded_len(TM)
    g = torch.Generator(device=DEV).manual_seed(7)
    cu = [0]
    for n in LENS:
        cu.append(cu[-1] + n)
    R = cu[-1]
    qkv32 = torch.randn((R, 3 * H), device=DEV, generator=g)
    bias32 = torch.randn((nb, NH, TM, Tp), device=DEV, generator=g) * 2.0
    assert bool(torch.isfinite(qkv32).all()) and bool(torch.isfinite(bias32).all())
    qkv, bias = qkv32.to(BF16), bias32.to(BF16)
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    cu_rows = torch.tensor(cu, dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(D)
    SENT_O, SENT_L = 1234.0, -777.0
    out = torch.full((R + 3, H), SENT_O, dtype=BF16, device=DEV)          # three guard rows behind the last document
    lse = torch.full((nb, NH, TM), SENT_L, dtype=torch.float32, device=DEV)
    assert ops.attn_fwd_varlen_supported(BF16, D)
    ops.attn_fwd_varlen(q, k, v, lens, cu_rows, NH, TM, D, scale, bias, out=out[:R], lse=lse)
    torch.cuda.synchronize()
    assert bool((out[R:] == SENT_O).all())
    for b, n in enumerate(LENS):
        assert bool((lse[b, :, n:] == SENT_L).all()), b                   # rows past the length keep their sentinel
        if n == 0:
            continue                                                       # (nothing to compare; its lse is checked above, it has no out rows)
        rows = slice(cu[b], cu[b] + n)
        one_bias = bias[b:b + 1, :, :n, :].contiguous()                    # the same slice, the same bias_ld
        assert one_bias.shape[-1] == Tp
        o1, l1 = ops.attn_fwd(q[rows], k[rows], v[rows], 1, NH, n, D, scale, one_bias)
        assert torch.equal(out[rows], o1), (b, n)
        assert torch.equal(lse[b, :, :n], l1[0]), (b, n)
        assert bool(torch.isfinite(o1.float()).all()) and float(o1.float().abs().max()) > 1e-3
    # every out row belongs to exactly one document, so none keeps the sentinel
    assert not bool((out[:R] == SENT_O).all(dim=1).any())


def test_attn_fwd_varlen_refuses_what_it_has_no_kernel_for(ops):
    from peneo_amd import hip
    lens = torch.tensor([4], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    qkv = torch.zeros((4, 3 * 32), dtype=BF16, device=DEV)
    bias = torch.zeros((1, 1, 4, 64), dtype=BF16, device=DEV)
    with pytest.raises(hip.PeneoHipError, match="no fallback"):
        ops.attn_fwd_varlen(qkv[:, :32], qkv[:, 32:64], qkv[:, 64:], lens, cu, 1, 4, 32, 1.0, bias)


# ---- the packed layer call at full lengths --------------------------------------------------------------------------------------
def test_packed_layer_at_full_lengths_equals_the_layer_call(ops):
    from peneo_amd import hip
    Bn, Tn, H, nh, I = 2, 160, 768, 12, 3072
    R = Bn * Tn
    g = torch.Generator(device=DEV).manual_seed(3)
    rn = lambda *s, std=1.0: torch.randn(s, device=DEV, generator=g) * std
    x = rn(R, H).to(BF16)
    w = [rn(n, kk, std=0.03).to(BF16) for n, kk in ((3 * H, H), (H, H), (I, H), (H, I))]
    bs = [rn(n, std=0.1) for n in (3 * H, H, I, H)]
    ln = [1.0 + rn(H, std=0.1), rn(H, std=0.1), 1.0 + rn(H, std=0.1), rn(H, std=0.1)]
    Tp = ops.attn_padded_len(Tn)
    bias = (rn(Bn, nh, Tn, Tp) * 2.0).to(BF16)
    bias[..., Tn:] = -1.0e30
    lens = torch.full((Bn,), Tn, dtype=torch.int32, device=DEV)
    cu = torch.arange(Bn + 1, dtype=torch.int32, device=DEV) * Tn

    def run(packed):
        bf = lambda *s: torch.full(s, 3.0, dtype=BF16, device=DEV)
        f32 = lambda *s: torch.full(s, 3.0, dtype=torch.float32, device=DEV)
        keep = dict(qkv=bf(R, 3 * H), att=bf(R, H), h1=bf(R, H), a=bf(R, H), inter=bf(R, I), h2=bf(R, H), lse=f32(Bn, nh, Tn), m1=f32(R),
                    r1=f32(R), m2=f32(R), r2=f32(R), out=bf(R, H))
        L = hip.EncoderLayer()
        L.Wqkv, L.Wo, L.Wi, L.Wo2 = (t.data_ptr() for t in w)
        L.bqkv, L.bo, L.bi, L.bo2 = (t.data_ptr() for t in bs)
        L.g1, L.b1, L.g2, L.b2 = (t.data_ptr() for t in ln)
        L.bias, L.bias_ld = bias.data_ptr(), Tp
        L.x = x.data_ptr()
        for name in ("qkv", "att", "h1", "a", "inter", "h2", "lse", "m1", "r1", "m2", "r2"):
            setattr(L, name, keep[name].data_ptr())
        L.B, L.T, L.H, L.nh, L.I = Bn, Tn, H, nh, I
        L.eps, L.attn_scale, L.p_hidden, L.p_attn = 1e-5, 1.0 / math.sqrt(H // nh), 0.0, 0.0
        wsb = int(hip.lib().peneo_encoder_layer_workspace_bytes(R, H, I, 0))
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
        if packed:
            ops.encoder_layer_fwd_packed(L, lens, cu, R, keep["out"], ws if wsb else None)
        else:
            hip.check(hip.lib().peneo_encoder_layer_fwd(C.byref(L), keep["out"].data_ptr(), ws.data_ptr() if wsb else None, wsb,
                                                        hip.stream()), "peneo_encoder_layer_fwd")
        torch.cuda.synchronize()
        return keep

    got, want = run(True), run(False)
    for name in ("qkv", "att", "lse", "h1", "a", "inter", "h2", "out"):
        assert torch.equal(got[name], want[name]), name
    assert bool(torch.isfinite(got["out"].float()).all()) and float(got["out"].float().abs().max()) > 0.1
    # an incomplete description is refused with the entry point's name, nothing launched
    L = hip.EncoderLayer()
    rc = hip.lib().peneo_encoder_layer_fwd_packed(C.byref(L), lens.data_ptr(), cu.data_ptr(), R, got["out"].data_ptr(), None, 0, hip.stream())
    assert rc == -1 and b"peneo_encoder_layer_fwd_packed" in hip.lib().peneo_last_error()
