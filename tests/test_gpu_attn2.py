"""peneo_attn2_fwd, the two-stream attention forward (LiLT: text head dim 64 + layout head dim 16, one shared softmax):
bit-identical to the path it replaces (head_concat x 2 -> attn_fwd at head dim 80 -> head_split), inside the project's bf16
bound against an fp32 statement of its contract, and strict about what it reads, writes and refuses."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DA, DB = 64, 16
SA, SB = 1.0 / 8.0, 1.0 / 4.0
ERR_INVALID = -1
MASKED = -1.0e30

# (B, nh, T): one ragged tile; exactly one tile; a second tile holding one key (the nt > 1 prologue); two tiles; one full turn of the
# three-buffer ring; the ring wrapping into a ragged tail; a second query block holding one query; the model's shape; the benchmark
# grid (384 workgroups); 528 workgroups, above the resident slots
CASES = [(1, 1, 17), (2, 2, 32), (2, 2, 33), (1, 2, 64), (2, 3, 96), (1, 2, 97), (1, 2, 129), (2, 12, 512), (8, 12, 512), (33, 16, 64)]


@pytest.fixture(scope="module")
def ops():
    from peneo_amd import ops as o
    from peneo_amd import hip
    hip.load_library()
    return o


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _padded_len(T):
    return (T + 63) // 64 * 64


def _inputs(B, nh, T, mask_all_of_doc=None):
    """Seeded bf16 randn fused buffers [B*T, 3*nh*64] and [B*T, 3*nh*16], and the fp32 key bias [B, Tp] (0 / -1e30, zero padding):
    document 0 has keys T//3 .. T//2 masked, the last document of a batch with B > 1 its tail from max(1, T - 40)."""
    g = torch.Generator(device="cpu").manual_seed(1000 * B + 100 * nh + T)
    qkv = torch.randn(B * T, 3 * nh * DA, generator=g).to(torch.bfloat16).to(DEV)
    lqkv = torch.randn(B * T, 3 * nh * DB, generator=g).to(torch.bfloat16).to(DEV)
    kb = torch.zeros(B, _padded_len(T), dtype=torch.float32)
    kb[0, T // 3:T // 2] = MASKED
    if B > 1:
        kb[B - 1, max(1, T - 40):T] = MASKED
    if mask_all_of_doc is not None:
        kb[mask_all_of_doc, :T] = MASKED
    return qkv, lqkv, kb.to(DEV)


def _streams(qkv, lqkv, nh):
    H, Hl = nh * DA, nh * DB
    return (qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]), (lqkv[:, :Hl], lqkv[:, Hl:2 * Hl], lqkv[:, 2 * Hl:])


def _new_path(ops, qkv, lqkv, kb, B, nh, T, **kw):
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    return ops.attn2_fwd(qa, ka, va, qb, kb_, vb, B, nh, T, SA, SB, kb, **kw)


def _parent_path(ops, qkv, lqkv, kb, B, nh, T):
    """What LiLT's layer ran before: two head_concat launches, attn_fwd at head dim 80 with scale 1, head_split."""
    H, Hl, dc = nh * DA, nh * DB, DA + DB
    R = B * T
    cat = torch.empty((R, 3 * nh * dc), dtype=qkv.dtype, device=DEV)
    ops.head_concat(qkv[:, :H], lqkv[:, :Hl], nh, cat[:, :nh * dc], SA, SB)
    ops.head_concat(qkv[:, H:], lqkv[:, Hl:], 2 * nh, cat[:, nh * dc:])
    attc, lse = ops.attn_fwd(cat[:, :nh * dc], cat[:, nh * dc:2 * nh * dc], cat[:, 2 * nh * dc:], B, nh, T, dc, 1.0, None, kb)
    att = torch.empty((R, H), dtype=qkv.dtype, device=DEV)
    latt = torch.empty((R, Hl), dtype=qkv.dtype, device=DEV)
    ops.head_split(attc, nh, att, latt)
    return att, latt, lse


@functools.lru_cache(maxsize=None)
def _case(B, nh, T):
    """Inputs and the kernel's outputs of a case, computed once and shared by the tests (never modified)."""
    from peneo_amd import ops
    qkv, lqkv, kb = _inputs(B, nh, T)
    out_a, out_b, lse = _new_path(ops, qkv, lqkv, kb, B, nh, T)
    torch.cuda.synchronize()
    return qkv, lqkv, kb, out_a, out_b, lse


def _contract_fp32(qkv, lqkv, kb, B, nh, T):
    """fp32 torch statement of the contract from the same bf16 inputs (the scales are powers of two: their rounding is exact)."""
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    heads = lambda x, d: x.float().view(B, T, nh, d).permute(0, 2, 1, 3)
    s = torch.einsum("bhqd,bhkd->bhqk", heads(qa, DA) * SA, heads(ka, DA)) + torch.einsum("bhqd,bhkd->bhqk", heads(qb, DB) * SB, heads(kb_, DB))
    p = torch.softmax(s + kb[:, None, None, :T], -1)
    rows = lambda o, d: o.permute(0, 2, 1, 3).reshape(B * T, nh * d)
    return rows(torch.einsum("bhqk,bhkd->bhqd", p, heads(va, DA)), DA), rows(torch.einsum("bhqk,bhkd->bhqd", p, heads(vb, DB)), DB)


@pytest.mark.parametrize("B,nh,T", CASES)
def test_bit_identical_to_the_concat_path(ops, B, nh, T):
    qkv, lqkv, kb, out_a, out_b, lse = _case(B, nh, T)
    att, latt, lse0 = _parent_path(ops, qkv, lqkv, kb, B, nh, T)
    assert torch.isfinite(out_a).all() and torch.isfinite(out_b).all() and torch.isfinite(lse).all()
    assert torch.equal(out_a, att)
    assert torch.equal(out_b, latt)
    assert torch.equal(lse, lse0)


def test_a_document_with_every_key_masked_gives_zeros_on_both_paths(ops):
    B, nh, T = 2, 2, 70
    qkv, lqkv, kb = _inputs(B, nh, T, mask_all_of_doc=1)
    out_a, out_b, lse = _new_path(ops, qkv, lqkv, kb, B, nh, T)
    att, latt, lse0 = _parent_path(ops, qkv, lqkv, kb, B, nh, T)
    assert torch.equal(out_a, att) and torch.equal(out_b, latt) and torch.equal(lse, lse0)
    assert torch.isfinite(out_a).all() and torch.isfinite(out_b).all()
    assert float(out_a[T:].abs().max()) == 0.0 and float(out_b[T:].abs().max()) == 0.0
    assert bool((lse[1] == MASKED).all()) and bool((lse[0] > 0.5 * MASKED).all())
    assert float(out_a[:T].abs().max()) > 0.0 and float(out_b[:T].abs().max()) > 0.0


@pytest.mark.parametrize("B,nh,T", CASES)
def test_inside_the_bf16_bound_of_the_fp32_contract(B, nh, T):
    qkv, lqkv, kb, out_a, out_b, _ = _case(B, nh, T)
    ref_a, ref_b = _contract_fp32(qkv, lqkv, kb, B, nh, T)
    ea, eb = rel_err(out_a, ref_a), rel_err(out_b, ref_b)
    print(f"attn2 {B}x{nh}x{T}: rel_err text {ea:.3e} layout {eb:.3e}")
    assert ea < 2e-2 and eb < 2e-2, (ea, eb)


@pytest.mark.parametrize("B,nh,T", [(1, 1, 17), (2, 2, 33), (1, 2, 97), (1, 2, 129)])
def test_padding_columns_of_key_bias_are_not_read(ops, B, nh, T):
    qkv, lqkv, kb, out_a, out_b, lse = _case(B, nh, T)
    kb2 = kb.clone()
    kb2[:, T:] = float("nan")
    a2, b2, l2 = _new_path(ops, qkv, lqkv, kb2, B, nh, T)
    assert torch.equal(a2, out_a) and torch.equal(b2, out_b) and torch.equal(l2, lse)


def test_documents_do_not_leak(ops):
    B, nh, T = 2, 2, 33
    qkv, lqkv, kb = _inputs(B, nh, T)
    qkv[T:] = float("nan")
    lqkv[T:] = float("nan")
    a2, b2, l2 = _new_path(ops, qkv, lqkv, kb, B, nh, T)
    a1, b1, l1 = _new_path(ops, qkv[:T], lqkv[:T], kb[:1].contiguous(), 1, nh, T)
    assert torch.isfinite(a1).all() and torch.isfinite(b1).all() and torch.isfinite(l1).all()
    assert torch.equal(a2[:T], a1) and torch.equal(b2[:T], b1) and torch.equal(l2[0], l1[0])


def _raw_call(qa, ka, va, ld_a, qb, kb_, vb, ld_b, B, nh, T, d_a, d_b, key_bias, out_a, ld_oa, out_b, ld_ob, lse, dtype=None):
    """peneo_attn2_fwd through the C ABI directly (pointers as integers): (return code, peneo_last_error)"""
    from peneo_amd import hip
    lib = hip.lib()
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    rc = lib.peneo_attn2_fwd(hip.BF16 if dtype is None else dtype, p(qa), p(ka), p(va), ld_a, p(qb), p(kb_), p(vb), ld_b, B, nh, T, d_a, d_b,
                             SA, SB, p(key_bias), p(out_a), ld_oa, p(out_b), ld_ob, p(lse), hip.stream())
    return rc, (lib.peneo_last_error() or b"").decode()


def test_outputs_stay_inside_their_column_slices_and_lse_may_be_null(ops):
    B, nh, T = 2, 2, 33
    qkv, lqkv, kb, out_a, out_b, _ = _case(B, nh, T)
    big_a = torch.full((B * T, nh * DA + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    big_b = torch.full((B * T, nh * DB + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    va_, vb_ = big_a[:, 8:8 + nh * DA], big_b[:, 8:8 + nh * DB]
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    rc, msg = _raw_call(qa, ka, va, qkv.stride(0), qb, kb_, vb, lqkv.stride(0), B, nh, T, DA, DB, kb, va_, big_a.stride(0), vb_,
                        big_b.stride(0), None)
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert torch.equal(va_, out_a) and torch.equal(vb_, out_b)
    for big, w in ((big_a, nh * DA), (big_b, nh * DB)):
        assert bool((big[:, :8] == 7.0).all()) and bool((big[:, 8 + w:] == 7.0).all())
    # the same through ops.attn2_fwd with the slices as outputs, and without a key bias at all (no document is masked then)
    big_a.fill_(7.0)
    big_b.fill_(7.0)
    ops.attn2_fwd(qa, ka, va, qb, kb_, vb, B, nh, T, SA, SB, None, out_a=va_, out_b=vb_)
    ref_a, ref_b = _contract_fp32(qkv, lqkv, torch.zeros_like(kb), B, nh, T)
    assert rel_err(va_, ref_a) < 2e-2 and rel_err(vb_, ref_b) < 2e-2
    for big, w in ((big_a, nh * DA), (big_b, nh * DB)):
        assert bool((big[:, :8] == 7.0).all()) and bool((big[:, 8 + w:] == 7.0).all())


def test_refusals_return_invalid_and_launch_nothing(ops):
    from peneo_amd import hip
    B, nh, T = 1, 1, 17
    qkv, lqkv, kb, _, _, _ = _case(B, nh, T)
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    out_a = torch.full((B * T, nh * DA), 7.0, dtype=torch.bfloat16, device=DEV)
    out_b = torch.full((B * T, nh * DB), 7.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, nh, T), 7.0, dtype=torch.float32, device=DEV)
    lda, ldb = qkv.stride(0), lqkv.stride(0)
    good = dict(qa=qa, ka=ka, va=va, ld_a=lda, qb=qb, kb_=kb_, vb=vb, ld_b=ldb, B=B, nh=nh, T=T, d_a=DA, d_b=DB, key_bias=kb, out_a=out_a,
                ld_oa=out_a.stride(0), out_b=out_b, ld_ob=out_b.stride(0), lse=lse)
    bad = {
        "unsupported dims 48 + 12": dict(d_a=48, d_b=12),
        "unsupported dims 80 + 0": dict(d_a=80, d_b=0),
        "fp32": dict(dtype=hip.F32),
        "T = 0": dict(T=0),
        "B = 0": dict(B=0),
        "nh = 0": dict(nh=0),
        "null operand": dict(kb_=None),
        "null output": dict(out_b=None),
        "q_a offset by one element": dict(qa=qa.data_ptr() + 2),
        "out_b offset by one element": dict(out_b=out_b.data_ptr() + 2),
        "ld_b of 20 elements": dict(ld_b=20),
        "ld_a beyond the 32-bit lane offsets": dict(ld_a=1 << 26),
    }
    for what, change in bad.items():
        rc, msg = _raw_call(**dict(good, **change))
        assert rc == ERR_INVALID, (what, rc)
        assert "peneo_attn2_fwd" in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((out_a == 7.0).all()) and bool((out_b == 7.0).all()) and bool((lse == 7.0).all())
    with pytest.raises(hip.PeneoHipError):           # and through ops: an error, never another path
        ops.attn2_fwd(qkv[:, :48], qkv[:, 48:96], qkv[:, 96:144], lqkv[:, :16], lqkv[:, 16:32], lqkv[:, 32:48], B, 1, T, SA, SB, kb)
    rc, msg = _raw_call(**good)                      # the unchanged call is accepted
    assert rc == 0, msg
