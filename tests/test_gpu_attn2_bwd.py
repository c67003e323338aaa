"""peneo_attn2_fwd_dropout and peneo_attn2_bwd, LiLT's two-stream attention for training (text head dim 64 + layout head dim 16, one
shared softmax, attention dropout): bit-identical to the path they replace (head_concat -> attn_fwd / attn_bwd at head dim 80 with
scale 1 -> head_split), inside the project's bf16 bound against a float64 statement of the contract, and strict about what they
read, write and refuse.  The float64 statement takes its dropout keep matrix from the documented layout of the keep words
(attention.hip's header comment), not from any kernel under test."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DA, DB = 64, 16
SA, SB = 1.0 / 8.0, 1.0 / 4.0
ERR_INVALID = -1
MASKED = -1.0e30
DROP_P = 0.1
NAMES = ("dq_a", "dk_a", "dv_a", "dq_b", "dk_b", "dv_b")

# (B, nh, T): one ragged query tile, one key block; exactly one query tile; the nt > 1 prologue; one turn of the ring; the ring
# wrapping into a ragged tail; exactly one key block; a second key block / dQ query block holding one row (its other three waves
# only serve the DMA); the model's shape; 528 workgroups, above the resident slots
CASES = [(1, 1, 17), (2, 2, 32), (2, 2, 33), (1, 2, 96), (1, 2, 97), (1, 2, 128), (1, 2, 129), (2, 12, 512), (33, 16, 64)]
DROPS = [0.0, DROP_P]


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
    """tests/test_gpu_attn2.py's inputs (seeded bf16 randn fused buffers [B*T, 3*nh*64] and [B*T, 3*nh*16], fp32 key bias [B, Tp]:
    document 0 has keys T//3 .. T//2 masked, the last document of a batch with B > 1 its tail from max(1, T - 40)) plus the seeded
    bf16 output gradients d_out_a [B*T, nh*64] and d_out_b [B*T, nh*16]."""
    g = torch.Generator(device="cpu").manual_seed(1000 * B + 100 * nh + T)
    qkv = torch.randn(B * T, 3 * nh * DA, generator=g).to(torch.bfloat16).to(DEV)
    lqkv = torch.randn(B * T, 3 * nh * DB, generator=g).to(torch.bfloat16).to(DEV)
    kb = torch.zeros(B, _padded_len(T), dtype=torch.float32)
    kb[0, T // 3:T // 2] = MASKED
    if B > 1:
        kb[B - 1, max(1, T - 40):T] = MASKED
    if mask_all_of_doc is not None:
        kb[mask_all_of_doc, :T] = MASKED
    d_a = torch.randn(B * T, nh * DA, generator=g).to(torch.bfloat16).to(DEV)
    d_b = torch.randn(B * T, nh * DB, generator=g).to(torch.bfloat16).to(DEV)
    return qkv, lqkv, kb.to(DEV), d_a, d_b


def _words(ops, B, nh, T, drop_p):
    return ops.attn_drop_words(B, nh, T, drop_p, 4242 + T, DEV)[0] if drop_p > 0 else None


def _streams(qkv, lqkv, nh):
    H, Hl = nh * DA, nh * DB
    return (qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]), (lqkv[:, :Hl], lqkv[:, Hl:2 * Hl], lqkv[:, 2 * Hl:])


def _split(dqkv, dlqkv, nh):
    (a0, a1, a2), (b0, b1, b2) = _streams(dqkv, dlqkv, nh)
    return a0, a1, a2, b0, b1, b2


def _new_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words):
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    out_a, out_b, lse = ops.attn2_fwd(qa, ka, va, qb, kb_, vb, B, nh, T, SA, SB, kb, drop_p=drop_p, drop_words=words)
    dqkv = torch.empty_like(qkv)
    dlqkv = torch.empty_like(lqkv)
    ops.attn2_bwd(qa, ka, va, qb, kb_, vb, out_a, d_a, out_b, d_b, lse, B, nh, T, SA, SB, kb, dqkv, dlqkv, drop_p=drop_p,
                  drop_words=words)
    return out_a, out_b, lse, dqkv, dlqkv


def _parent_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words):
    """What LiLT's layer runs without the switch: head_concat x 2, attn_fwd at head dim 80 with scale 1, head_split; then
    head_concat of the output gradients, attn_bwd (its own dS^T slab), head_split x 2 with the scales on dq."""
    H, Hl, dc = nh * DA, nh * DB, DA + DB
    R = B * T
    cat = torch.empty((R, 3 * nh * dc), dtype=qkv.dtype, device=DEV)
    ops.head_concat(qkv[:, :H], lqkv[:, :Hl], nh, cat[:, :nh * dc], SA, SB)
    ops.head_concat(qkv[:, H:], lqkv[:, Hl:], 2 * nh, cat[:, nh * dc:])
    qc, kc, vc = cat[:, :nh * dc], cat[:, nh * dc:2 * nh * dc], cat[:, 2 * nh * dc:]
    attc, lse = ops.attn_fwd(qc, kc, vc, B, nh, T, dc, 1.0, None, kb, drop_p=drop_p, drop_words=words)
    att = torch.empty((R, H), dtype=qkv.dtype, device=DEV)
    latt = torch.empty((R, Hl), dtype=qkv.dtype, device=DEV)
    ops.head_split(attc, nh, att, latt)
    d_attc = torch.empty((R, nh * dc), dtype=qkv.dtype, device=DEV)
    ops.head_concat(d_a, d_b, nh, d_attc)
    dcat = torch.empty_like(cat)
    ops.attn_bwd(qc, kc, vc, attc, d_attc, lse, B, nh, T, dc, 1.0, None, kb, dcat, None, drop_p=drop_p, drop_words=words)
    dqkv = torch.empty_like(qkv)
    dlqkv = torch.empty_like(lqkv)
    ops.head_split(dcat[:, :nh * dc], nh, dqkv[:, :H], dlqkv[:, :Hl], SA, SB)
    ops.head_split(dcat[:, nh * dc:], 2 * nh, dqkv[:, H:], dlqkv[:, Hl:])
    return att, latt, lse, dqkv, dlqkv


@functools.lru_cache(maxsize=None)
def _case(B, nh, T, drop_p):
    """Inputs, keep words and both paths' outputs of a case, computed once and shared by the tests (never modified)."""
    from peneo_amd import ops
    qkv, lqkv, kb, d_a, d_b = _inputs(B, nh, T)
    words = _words(ops, B, nh, T, drop_p)
    new = _new_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words)
    old = _parent_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words)
    torch.cuda.synchronize()
    return (qkv, lqkv, kb, d_a, d_b, words), new, old


def _keep_matrix(words, B, nh, T, drop_p):
    """[B, nh, T q, T keys] float64 keep / (1 - p) from the keep words: words[bh, q >> 5, attn_kslot(key)] bit (q & 31); p is realised
    as thr16 / 2^16 (common.h: pair_drop_thr16_host, pair_drop_scale_host)."""
    key = torch.arange(T, device=DEV)
    kslot = (key & ~31) | (((key >> 3) & 3) << 3) | ((key & 3) << 1) | ((key >> 2) & 1)
    q = torch.arange(T, device=DEV)
    w = words[:, (q >> 5)[:, None], kslot[None, :]].to(torch.int64)                  # [B*nh, T, T]
    keep = (w >> (q & 31)[None, :, None]) & 1
    thr = int(drop_p * 65536.0 + 0.5)
    return keep.view(B, nh, T, T).to(torch.float64) * (65536.0 / (65536.0 - thr))


def _contract_f64(qkv, lqkv, kb, d_a, d_b, words, B, nh, T, drop_p):
    """float64 torch statement of the contract and autograd through it, from the same bf16 inputs: (out_a, out_b, six gradients)."""
    heads = lambda x, d: x.double().view(B, T, nh, d).permute(0, 2, 1, 3)
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    leaves = [heads(t, d).clone().requires_grad_(True) for t, d in ((qa, DA), (ka, DA), (va, DA), (qb, DB), (kb_, DB), (vb, DB))]
    fqa, fka, fva, fqb, fkb, fvb = leaves
    s = torch.einsum("bhqd,bhkd->bhqk", fqa * SA, fka) + torch.einsum("bhqd,bhkd->bhqk", fqb * SB, fkb)
    p = torch.softmax(s + kb[:, None, None, :T].double(), -1)
    if drop_p > 0:
        p = p * _keep_matrix(words, B, nh, T, drop_p)
    oa, ob = torch.einsum("bhqk,bhkd->bhqd", p, fva), torch.einsum("bhqk,bhkd->bhqd", p, fvb)
    ((oa * heads(d_a, DA)).sum() + (ob * heads(d_b, DB)).sum()).backward()
    rows = lambda o: o.permute(0, 2, 1, 3).reshape(B * T, -1)
    return (rows(oa.detach()), rows(ob.detach())) + tuple(rows(t.grad) for t in leaves)


@pytest.mark.parametrize("drop_p", DROPS)
@pytest.mark.parametrize("B,nh,T", CASES)
def test_bit_identical_to_the_concat_path(B, nh, T, drop_p):
    _, (out_a, out_b, lse, dqkv, dlqkv), (att, latt, lse0, dqkv0, dlqkv0) = _case(B, nh, T, drop_p)
    for t in (out_a, out_b, lse, dqkv, dlqkv):
        assert torch.isfinite(t).all()
    assert torch.equal(out_a, att)
    assert torch.equal(out_b, latt)
    assert torch.equal(lse, lse0)
    for name, new, old in zip(NAMES, _split(dqkv, dlqkv, nh), _split(dqkv0, dlqkv0, nh)):
        assert torch.equal(new, old), (name, rel_err(new, old))


@pytest.mark.parametrize("drop_p", DROPS)
@pytest.mark.parametrize("B,nh,T", CASES)
def test_inside_the_bound_of_the_float64_contract(B, nh, T, drop_p):
    (qkv, lqkv, kb, d_a, d_b, words), (out_a, out_b, _, dqkv, dlqkv), (att, latt, _, dqkv0, dlqkv0) = _case(B, nh, T, drop_p)
    ref = _contract_f64(qkv, lqkv, kb, d_a, d_b, words, B, nh, T, drop_p)
    new = (out_a, out_b) + _split(dqkv, dlqkv, nh)
    old = (att, latt) + _split(dqkv0, dlqkv0, nh)
    errs = []
    for name, n, o, r in zip(("out_a", "out_b") + NAMES, new, old, ref):
        en, eo = rel_err(n, r), rel_err(o, r)
        print(f"attn2 bwd {B}x{nh}x{T} p={drop_p}: {name} rel_err two-stream {en:.3e} concat {eo:.3e}")
        errs.append((name, en))
    for name, en in errs:
        assert en < 2e-2, (name, en)


@pytest.mark.parametrize("drop_p", DROPS)
def test_a_document_with_every_key_masked_gets_zero_gradients(ops, drop_p):
    B, nh, T = 2, 2, 70
    qkv, lqkv, kb, d_a, d_b = _inputs(B, nh, T, mask_all_of_doc=1)
    words = _words(ops, B, nh, T, drop_p)
    new = _new_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words)
    old = _parent_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words)
    for n, o in zip(new, old):
        assert torch.equal(n, o)
    for name, g in zip(NAMES, _split(new[3], new[4], nh)):
        assert torch.isfinite(g).all(), name
        assert float(g[T:].abs().max()) == 0.0, name
        assert float(g[:T].abs().max()) > 0.0, name


@pytest.mark.parametrize("B,nh,T", [(1, 1, 17), (2, 2, 33), (1, 2, 97), (1, 2, 129)])
def test_padding_columns_of_key_bias_are_not_read(ops, B, nh, T):
    (qkv, lqkv, kb, d_a, d_b, words), new, _ = _case(B, nh, T, DROP_P)
    kb2 = kb.clone()
    kb2[:, T:] = float("nan")
    again = _new_path(ops, qkv, lqkv, kb2, d_a, d_b, B, nh, T, DROP_P, words)
    for n, a in zip(new, again):
        assert torch.equal(n, a)


@pytest.mark.parametrize("drop_p", DROPS)
def test_documents_do_not_leak(ops, drop_p):
    B, nh, T = 2, 2, 33
    qkv, lqkv, kb, d_a, d_b = _inputs(B, nh, T)
    words = _words(ops, B, nh, T, drop_p)
    for t in (qkv, lqkv, d_a, d_b):
        t[T:] = float("nan")
    two = _new_path(ops, qkv, lqkv, kb, d_a, d_b, B, nh, T, drop_p, words)          # (out_a, out_b, lse of document 1: NaN as well)
    one = _new_path(ops, qkv[:T], lqkv[:T], kb[:1].contiguous(), d_a[:T], d_b[:T], 1, nh, T, drop_p,
                    None if words is None else words[:nh].contiguous())
    assert torch.equal(two[2][0], one[2][0])
    for i in (0, 1, 3, 4):
        assert torch.isfinite(one[i]).all()
        assert torch.equal(two[i][:T], one[i])


class _Raw:
    """peneo_attn2_bwd through the C ABI directly (pointers as integers), on the outputs of a forward call."""

    def __init__(self, ops, B, nh, T, drop_p, margin=0):
        from peneo_amd import hip
        self.hip, self.lib = hip, hip.lib()
        self.B, self.nh, self.T = B, nh, T
        self.qkv, self.lqkv, self.kb, self.d_a, self.d_b = _inputs(B, nh, T)
        self.words = _words(ops, B, nh, T, drop_p)
        (qa, ka, va), (qb, kb_, vb) = _streams(self.qkv, self.lqkv, nh)
        self.out_a, self.out_b, self.lse = ops.attn2_fwd(qa, ka, va, qb, kb_, vb, B, nh, T, SA, SB, self.kb, drop_p=drop_p,
                                                         drop_words=self.words)
        H, Hl = nh * DA, nh * DB
        self.big_a = torch.full((B * T, 3 * H + 2 * margin), 7.0, dtype=torch.bfloat16, device=DEV)
        self.big_b = torch.full((B * T, 3 * Hl + 2 * margin), 7.0, dtype=torch.bfloat16, device=DEV)
        self.dqkv, self.dlqkv = self.big_a[:, margin:margin + 3 * H], self.big_b[:, margin:margin + 3 * Hl]
        self.ws = torch.zeros(ops.attn2_bwd_workspace_bytes(B, nh, T), dtype=torch.uint8, device=DEV)
        da, db = _streams(self.dqkv, self.dlqkv, nh)
        self.good = dict(dtype=hip.BF16, q_a=qa, k_a=ka, v_a=va, ld_a=self.qkv.stride(0), q_b=qb, k_b=kb_, v_b=vb, ld_b=self.lqkv.stride(0),
                         out_a=self.out_a, d_out_a=self.d_a, ld_out_a=self.out_a.stride(0), out_b=self.out_b, d_out_b=self.d_b,
                         ld_out_b=self.out_b.stride(0), lse=self.lse, B=B, nh=nh, T=T, d_a=DA, d_b=DB, scale_a=SA, scale_b=SB,
                         key_bias=self.kb, dq_a=da[0], dk_a=da[1], dv_a=da[2], ld_da=self.big_a.stride(0), dq_b=db[0], dk_b=db[1],
                         dv_b=db[2], ld_db=self.big_b.stride(0), workspace=self.ws, drop_p=drop_p, drop_words=self.words)

    def call(self, **change):
        a = dict(self.good, **change)
        p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        rc = self.lib.peneo_attn2_bwd(a["dtype"], p(a["q_a"]), p(a["k_a"]), p(a["v_a"]), a["ld_a"], p(a["q_b"]), p(a["k_b"]), p(a["v_b"]),
                                      a["ld_b"], p(a["out_a"]), p(a["d_out_a"]), a["ld_out_a"], p(a["out_b"]), p(a["d_out_b"]),
                                      a["ld_out_b"], p(a["lse"]), a["B"], a["nh"], a["T"], a["d_a"], a["d_b"], a["scale_a"], a["scale_b"],
                                      p(a["key_bias"]), p(a["dq_a"]), p(a["dk_a"]), p(a["dv_a"]), a["ld_da"], p(a["dq_b"]), p(a["dk_b"]),
                                      p(a["dv_b"]), a["ld_db"], p(a["workspace"]), a["drop_p"], p(a["drop_words"]), self.hip.stream())
        return rc, (self.lib.peneo_last_error() or b"").decode()


@pytest.mark.parametrize("B,nh,T", [(2, 2, 33), (1, 2, 129)])
def test_the_workspace_needs_no_initialisation_and_keeps_no_state(ops, B, nh, T):
    (_, _, _, _, _, _), (_, _, _, dqkv, dlqkv), _ = _case(B, nh, T, DROP_P)
    raw = _Raw(ops, B, nh, T, DROP_P)
    n = raw.ws.numel() // 4
    for fill in (0.0, float("nan"), None):              # zeros, NaN, then what the call before left behind
        if fill is not None:
            raw.ws[:4 * n].view(torch.float32).fill_(fill)
        raw.big_a.fill_(7.0)
        raw.big_b.fill_(7.0)
        rc, msg = raw.call()
        torch.cuda.synchronize()
        assert rc == 0, msg
        assert torch.equal(raw.dqkv, dqkv) and torch.equal(raw.dlqkv, dlqkv), fill


def test_outputs_stay_inside_their_column_slices(ops):
    B, nh, T = 2, 2, 33
    _, (_, _, _, dqkv, dlqkv), _ = _case(B, nh, T, DROP_P)
    raw = _Raw(ops, B, nh, T, DROP_P, margin=8)         # 16 columns wider than needed, the gradients in the middle
    rc, msg = raw.call()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert torch.equal(raw.dqkv, dqkv) and torch.equal(raw.dlqkv, dlqkv)
    for big, w in ((raw.big_a, 3 * nh * DA), (raw.big_b, 3 * nh * DB)):
        assert bool((big[:, :8] == 7.0).all()) and bool((big[:, 8 + w:] == 7.0).all())
    # the same through ops.attn2_bwd with the slices as outputs
    raw.big_a.fill_(7.0)
    raw.big_b.fill_(7.0)
    g = raw.good
    ops.attn2_bwd(g["q_a"], g["k_a"], g["v_a"], g["q_b"], g["k_b"], g["v_b"], raw.out_a, raw.d_a, raw.out_b, raw.d_b, raw.lse, B, nh, T,
                  SA, SB, raw.kb, raw.dqkv, raw.dlqkv, drop_p=DROP_P, drop_words=raw.words)
    assert torch.equal(raw.dqkv, dqkv) and torch.equal(raw.dlqkv, dlqkv)
    for big, w in ((raw.big_a, 3 * nh * DA), (raw.big_b, 3 * nh * DB)):
        assert bool((big[:, :8] == 7.0).all()) and bool((big[:, 8 + w:] == 7.0).all())


def test_refusals_return_invalid_and_launch_nothing(ops):
    from peneo_amd import hip
    B, nh, T = 1, 1, 17
    raw = _Raw(ops, B, nh, T, 0.0)
    g = raw.good
    bad = {
        "unsupported dims 48 + 12": dict(d_a=48, d_b=12),
        "unsupported dims 80 + 0": dict(d_a=80, d_b=0),
        "fp32": dict(dtype=hip.F32),
        "T = 0": dict(T=0),
        "B = 0": dict(B=0),
        "nh = -1": dict(nh=-1),
        "null operand": dict(k_b=None),
        "null d_out": dict(d_out_a=None),
        "null lse": dict(lse=None),
        "null output": dict(dv_b=None),
        "null workspace": dict(workspace=None),
        "q_a offset by one element": dict(q_a=g["q_a"].data_ptr() + 2),
        "d_out_b offset by one element": dict(d_out_b=g["d_out_b"].data_ptr() + 2),
        "dq_b offset by one element": dict(dq_b=g["dq_b"].data_ptr() + 2),
        "workspace offset by four bytes": dict(workspace=raw.ws.data_ptr() + 4),
        "ld_b of 20 elements": dict(ld_b=20),
        "ld_out_a too small for nh heads": dict(ld_out_a=nh * DA - 8),
        "ld_db of 20 elements": dict(ld_db=20),
        "ld_a beyond the 32-bit lane offsets": dict(ld_a=1 << 26),
        "drop_p > 0 without words": dict(drop_p=0.1, drop_words=None),
        "drop_p = 1": dict(drop_p=1.0),
    }
    for what, change in bad.items():
        rc, msg = raw.call(**change)
        assert rc == ERR_INVALID, (what, rc)
        assert "peneo_attn2_bwd" in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((raw.big_a == 7.0).all()) and bool((raw.big_b == 7.0).all())
    # the forward with dropout refuses the same way
    lib = hip.lib()
    p = lambda t: None if t is None else t.data_ptr()
    out_a = torch.full((B * T, nh * DA), 7.0, dtype=torch.bfloat16, device=DEV)
    out_b = torch.full((B * T, nh * DB), 7.0, dtype=torch.bfloat16, device=DEV)
    rc = lib.peneo_attn2_fwd_dropout(hip.BF16, p(g["q_a"]), p(g["k_a"]), p(g["v_a"]), g["ld_a"], p(g["q_b"]), p(g["k_b"]), p(g["v_b"]),
                                     g["ld_b"], B, nh, T, DA, DB, SA, SB, p(raw.kb), p(out_a), out_a.stride(0), p(out_b), out_b.stride(0),
                                     None, 0.1, None, hip.stream())
    assert rc == ERR_INVALID and "peneo_attn2_fwd_dropout" in (lib.peneo_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert bool((out_a == 7.0).all()) and bool((out_b == 7.0).all())
    with pytest.raises(hip.PeneoHipError):           # and through ops: an error, never another path
        ops.attn2_bwd(raw.qkv[:, :48], raw.qkv[:, 48:96], raw.qkv[:, 96:144], raw.lqkv[:, :12], raw.lqkv[:, 12:24], raw.lqkv[:, 24:36],
                      raw.out_a[:, :48], raw.d_a[:, :48], raw.out_b[:, :12], raw.d_b[:, :12], raw.lse, B, 1, T, SA, SB, raw.kb,
                      torch.empty((B * T, 144), dtype=torch.bfloat16, device=DEV), torch.empty((B * T, 36), dtype=torch.bfloat16, device=DEV))
    rc, msg = raw.call()                             # the unchanged call is accepted
    torch.cuda.synchronize()
    assert rc == 0, msg


def test_forward_without_dropout_is_the_old_entry_point_bit_for_bit(ops):
    """drop_p == 0 with NULL words through peneo_attn2_fwd_dropout gives the bits of peneo_attn2_fwd."""
    from peneo_amd import hip
    B, nh, T = 2, 2, 33
    (qkv, lqkv, kb, _, _, _), (out_a, out_b, lse, _, _), _ = _case(B, nh, T, 0.0)
    (qa, ka, va), (qb, kb_, vb) = _streams(qkv, lqkv, nh)
    a, b, l = torch.empty_like(out_a), torch.empty_like(out_b), torch.empty_like(lse)
    p = lambda t: t.data_ptr()
    rc = hip.lib().peneo_attn2_fwd_dropout(hip.BF16, p(qa), p(ka), p(va), qkv.stride(0), p(qb), p(kb_), p(vb), lqkv.stride(0), B, nh, T,
                                           DA, DB, SA, SB, p(kb), p(a), a.stride(0), p(b), b.stride(0), p(l), 0.0, None, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(a, out_a) and torch.equal(b, out_b) and torch.equal(l, lse)
