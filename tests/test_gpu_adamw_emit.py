"""peneo_adamw_step_emit against the existing path (peneo_adamw_step_clip, then ops.cast of the result): parameters, both
moments and every emitted working copy bit for bit, and not one element written outside a destination."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD = 8                       # sentinel elements in front of and behind every destination
SENTINEL = {BF: -7.0, F32: -12345.0}
# numel -> [(destination dtype, element offset of the destination inside its buffer)].  Buffers start 256-byte aligned, so
# offset 8 is 16-byte aligned for both dtypes, bf16 offset 9 is odd (2-byte aligned), bf16 offset 10 is 4- but not 8-byte
# aligned, fp32 offset 9 is one float past a 16-byte boundary.  5 has no record; 4 (two aligned records) carries step_offset 3.
PLAN = {1: [(BF, 9), (F32, 9)], 3: [(BF, 8)], 4: [(F32, 8), (BF, 8)], 5: [], 4095: [(BF, 9), (F32, 8)],
        4096: [(BF, 8), (F32, 8)], 4097: [(F32, 9), (BF, 10)], 2 * 4096 + 2: [(BF, 9), (F32, 9)]}
STEP_OFFSET = {4: 3}
MISALIGNED_PARAM = 4097         # this tensor's parameter starts one float past a 16-byte boundary: the kernel's element path


class Tensors:
    """One AdamW table over the PLAN's sizes and its device arrays."""

    def __init__(self, seed):
        from peneo_amd import hip
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.p, self.g, self.m, self.v = [], [], [], []
        for n in PLAN:
            if n == MISALIGNED_PARAM:
                self.p.append(torch.randn(n + 1, device="cuda", generator=g)[1:])
            else:
                self.p.append(torch.randn(n, device="cuda", generator=g))
            self.g.append(torch.randn(n, device="cuda", generator=g))
            self.m.append(torch.randn(n, device="cuda", generator=g) * 0.1)
            self.v.append(torch.rand(n, device="cuda", generator=g) * 0.1)
        chunk = hip.lib().peneo_adamw_chunk_elems()
        assert chunk == 4096                                         # the sizes above sit on both sides of its edges
        ct = [k for k, n in enumerate(PLAN) for _ in range((n + chunk - 1) // chunk)]
        ci = [c for n in PLAN for c in range((n + chunk - 1) // chunk)]
        self.chunk_t = torch.tensor(ct, dtype=torch.int32, device="cuda")
        self.chunk_i = torch.tensor(ci, dtype=torch.int32, device="cuda")
        self.sq = torch.zeros(int(hip.lib().peneo_grad_sqnorm_slots()), dtype=torch.float64, device="cuda")

    def clone(self):
        other = object.__new__(Tensors)
        other.p = [torch.empty(t.numel() + 1, device="cuda")[1:].copy_(t) if t.numel() == MISALIGNED_PARAM else t.clone() for t in self.p]
        other.g, other.m, other.v = ([t.clone() for t in ts] for ts in (self.g, self.m, self.v))
        other.chunk_t, other.chunk_i, other.sq = self.chunk_t, self.chunk_i, self.sq.clone()
        return other

    def table(self):
        from peneo_amd import hip
        host = (hip.AdamwTensor * len(self.p))()
        for k, n in enumerate(PLAN):
            e = host[k]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = (t[k].data_ptr() for t in (self.p, self.g, self.m, self.v))
            e.numel, e.lr, e.weight_decay, e.step_offset = n, 1e-2 * (1 + k % 3), 0.1 * (k % 2), STEP_OFFSET.get(n, 0)
        return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()


def destinations():
    """{tensor index: [(buffer, view)]}: every destination carved out of a larger sentinel-filled buffer"""
    out = {}
    for k, (n, recs) in enumerate(PLAN.items()):
        out[k] = []
        for dt, off in recs:
            buf = torch.full((off + n + GUARD,), SENTINEL[dt], dtype=dt, device="cuda")
            view = buf[off:off + n]
            assert view.data_ptr() == buf.data_ptr() + off * dt.itemsize and off >= GUARD
            out[k].append((buf, view))
    return out


def test_the_plan_covers_the_alignments():
    dst = destinations()
    al = {(v.dtype, v.data_ptr() % 16) for recs in dst.values() for _, v in recs}
    assert {(BF, 0), (BF, 2), (BF, 4), (F32, 0), (F32, 4)} <= al
    assert any(len(r) == 0 for r in dst.values()) and any({v.dtype for _, v in r} == {BF, F32} for r in dst.values())


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_step_emit_equals_step_then_cast(clip):
    from peneo_amd import hip, ops
    lib = hip.lib()
    a = Tensors(11)
    b = a.clone()                                      # the reference's own copies
    ta, tb = a.table(), b.table()
    dst = destinations()
    emit = ops.AdamwEmitTable(a.p)
    emit.update([(a.p[k], v) for k, recs in dst.items() for _, v in recs])
    assert emit.n_records == sum(len(r) for r in PLAN.values())
    max_norm = 1.0 if clip else 0.0
    n_chunks = a.chunk_t.numel()
    gen = torch.Generator(device="cuda").manual_seed(5)
    for step in (1, 2):
        for ga, gb in zip(a.g, b.g):
            ga.copy_(torch.randn(ga.shape, device="cuda", generator=gen))
            gb.copy_(ga)
        sqa = sqb = None
        if clip:
            sqa, sqb = a.sq, b.sq
            for t, tab, sq in ((a, ta, sqa), (b, tb, sqb)):
                hip.check(lib.peneo_grad_sqnorm(hip.ptr(tab), hip.ptr(t.chunk_t), hip.ptr(t.chunk_i), n_chunks, hip.ptr(sq), hip.stream()))
            assert float(sqa.sum().sqrt()) > 1.0        # the gradients are clipped
            sqb.copy_(sqa)                              # (fp64 atomics: the partial sums of two launches may differ in the last bit)
        ops.adamw_step_emit(ta, a.chunk_t, a.chunk_i, 0.9, 0.999, 1e-8, step, emit, sqnorm=sqa, max_grad_norm=max_norm)
        hip.check(lib.peneo_adamw_step_clip(hip.ptr(tb), hip.ptr(b.chunk_t), hip.ptr(b.chunk_i), n_chunks, 0.9, 0.999, 1e-8, step,
                                            hip.ptr(sqb), max_norm, hip.stream()), "peneo_adamw_step_clip")
        torch.cuda.synchronize()
        for k, n in enumerate(PLAN):
            assert torch.equal(a.p[k], b.p[k]), (step, n, "param")
            assert torch.equal(a.m[k], b.m[k]), (step, n, "exp_avg")
            assert torch.equal(a.v[k], b.v[k]), (step, n, "exp_avg_sq")
            for (buf, view), (dt, off) in zip(dst[k], PLAN[n]):
                want = ops.cast(b.p[k].clone(), dt)     # (clone: peneo_cast wants its usual 16-byte aligned source)
                assert torch.equal(view, want), (step, n, dt, off)
                assert bool((buf[:off] == SENTINEL[dt]).all()) and bool((buf[off + n:] == SENTINEL[dt]).all()), (step, n, dt, off, "guard")
                assert buf[off + n:].numel() == GUARD
    # the parameters did move, and by different amounts per step count (step_offset 3 is not step_offset 0)
    assert not torch.equal(a.p[0], Tensors(11).p[0])


def test_no_records_is_the_plain_step():
    from peneo_amd import hip, ops
    a = Tensors(3)
    b = a.clone()
    ops.adamw_step_emit(a.table(), a.chunk_t, a.chunk_i, 0.9, 0.999, 1e-8, 1, None)
    hip.check(hip.lib().peneo_adamw_step_clip(hip.ptr(b.table()), hip.ptr(b.chunk_t), hip.ptr(b.chunk_i), b.chunk_t.numel(), 0.9, 0.999,
                                              1e-8, 1, None, 0.0, hip.stream()))
    torch.cuda.synchronize()
    for k in range(len(PLAN)):
        assert torch.equal(a.p[k], b.p[k]) and torch.equal(a.m[k], b.m[k]) and torch.equal(a.v[k], b.v[k])
