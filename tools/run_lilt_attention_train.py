"""LiLT's attention for TRAINING on one box, interleaved A/B:

  parent   the concat path: ``head_concat`` x 2 -> ``attn_fwd`` at head dim 80 (with the keep words) -> ``head_split``; backward:
           ``head_concat`` of the two output gradients -> ``attn_bwd`` (delta, the single-pass kernel at DP = 96, dQ from its dS^T
           slab) -> ``head_split`` x 2;
  attn2    ``attn2_fwd`` with the keep words, ``attn2_bwd`` (delta; dK / dV / dS^T; dQ) straight into the two dqkv buffers.

(a) One layer's attention forward + backward at B = 8, nh = 12, T = 512 on seeded bf16 operands with a ragged key bias and
    drop_p = 0.1, device events around REPS back-to-back calls of each arm, for the forward, the backward and every op call on
    its own (buffers the ops accept as arguments are allocated once, outside the timing; ``attn_bwd`` and ``attn2_bwd`` allocate
    their slab / workspace themselves, as they do in the model).  Both arms' outputs are compared bit for bit first.  If the
    torch profiler yields device kernel times on this box, one call of each backward is also listed kernel by kernel.
(b) A seeded LiLT-base PEneo train step (12 layers, bf16 compute, forward + loss + backward, 8 synthetic documents of 512 tokens)
    with PENEO_LILT_ATTN2_TRAIN unset (the parent commit's path) and =1: ms per step and the peak device memory of both arms;
    loss and gradients of both settings are compared first (same dropout seeds).
ROUNDS interleaved rounds after a warm-up, every round printed, then medians and spreads (max - min).
Results: profiles/lilt_attention2_train.txt."""
import math, os, subprocess, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from peneo_amd import ops
from seeded import lilt_config, peneo_config, seeded_fill_
from peneo_amd.model import PEneoConfig, PEneoModel
from peneo_amd.model.engine import DropoutSeeds
from peneo_amd.data import synthetic_rfund_batch

ROUNDS = int(os.environ.get("ROUNDS", 5))
REPS = int(os.environ.get("REPS", 20))
B, S, NH, DA, DB = 8, 512, 12, 64, 16
DROP_P = 0.1
SWITCH = "PENEO_LILT_ATTN2_TRAIN"


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip()
    except Exception as e:   # noqa: BLE001
        return f"(rocm-smi unavailable: {e})"


def event_us(fn, reps=REPS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def med_spread(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def ab(name, unit, scale, parent, new, reps=REPS):
    for f in (parent, new):
        event_us(f, 3)
    rows = []
    for _ in range(ROUNDS):
        rows.append((event_us(parent, reps) * scale, event_us(new, reps) * scale))
        print(f"{name}: parent {rows[-1][0]:.3f} {unit}  attn2 {rows[-1][1]:.3f} {unit}")
    (pa, sa), (pb, sb) = med_spread([r[0] for r in rows]), med_spread([r[1] for r in rows])
    print(f"{name} median: parent {pa:.3f} {unit} (spread {sa:.3f})  attn2 {pb:.3f} {unit} (spread {sb:.3f})  ({pa / pb:.2f}x)  "
          f"attn2 below parent in every round: {all(r[1] < r[0] for r in rows)}")
    sys.stdout.flush()


def alone(name, fn):
    event_us(fn, 3)
    ts = [event_us(fn) for _ in range(ROUNDS)]
    md, sp = med_spread(ts)
    print(f"(a)   {name}: {' '.join(f'{t:.1f}' for t in ts)} us; median {md:.1f} us (spread {sp:.1f})")
    sys.stdout.flush()


def kernel_table(name, fn):
    """device kernels of ONE call from the torch profiler (best effort: the A/B numbers above do not depend on it)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn(); torch.cuda.synchronize()
        rows = []
        for e in prof.key_averages():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                us = getattr(e, "self_device_time_total", None)
                rows.append((e.key, float(us if us is not None else e.self_cuda_time_total), e.count))
        if not rows:
            print(f"(a)   {name}: the profiler returned no device kernels")
        for kname, us, cnt in rows:
            print(f"(a)   {name}: {us:8.1f} us x{cnt}  {kname[:110]}")
    except Exception as e:   # noqa: BLE001
        print(f"(a)   {name}: no kernel table ({type(e).__name__}: {e})")
    sys.stdout.flush()


def one_layer():
    H, Hl, dc, R = NH * DA, NH * DB, DA + DB, B * S
    g = torch.Generator(device="cpu").manual_seed(0)
    bf = lambda *shape: torch.randn(*shape, generator=g).to(torch.bfloat16).cuda()
    qkv, lqkv, d_att, d_latt = bf(R, 3 * H), bf(R, 3 * Hl), bf(R, H), bf(R, Hl)
    kb = torch.zeros(B, ops.attn_padded_len(S), dtype=torch.float32)
    for b in range(B):
        kb[b, S - 37 * b:S] = -1.0e30                   # ragged documents
    kb = kb.cuda()
    words = ops.attn_drop_words(B, NH, S, DROP_P, 1234, "cuda")[0]
    sa, sb = 1.0 / math.sqrt(DA), 1.0 / math.sqrt(DB)
    new_bf = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    cat, attc, d_attc, dcat = new_bf(R, 3 * NH * dc), new_bf(R, NH * dc), new_bf(R, NH * dc), new_bf(R, 3 * NH * dc)
    att, latt, att2, latt2 = new_bf(R, H), new_bf(R, Hl), new_bf(R, H), new_bf(R, Hl)
    dqkv, dlqkv, dqkv2, dlqkv2 = new_bf(R, 3 * H), new_bf(R, 3 * Hl), new_bf(R, 3 * H), new_bf(R, 3 * Hl)
    lse, lse2 = (torch.empty((B, NH, S), dtype=torch.float32, device="cuda") for _ in range(2))
    qc, kc, vc = cat[:, :NH * dc], cat[:, NH * dc:2 * NH * dc], cat[:, 2 * NH * dc:]
    qa, ka, va, qb, kb_, vb = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], lqkv[:, :Hl], lqkv[:, Hl:2 * Hl], lqkv[:, 2 * Hl:]

    p_cat_q = lambda: ops.head_concat(qkv[:, :H], lqkv[:, :Hl], NH, cat[:, :NH * dc], sa, sb)
    p_cat_kv = lambda: ops.head_concat(qkv[:, H:], lqkv[:, Hl:], 2 * NH, cat[:, NH * dc:])
    p_fwd = lambda: ops.attn_fwd(qc, kc, vc, B, NH, S, dc, 1.0, None, kb, drop_p=DROP_P, drop_words=words, out=attc, lse=lse)
    p_split = lambda: ops.head_split(attc, NH, att, latt)
    p_cat_d = lambda: ops.head_concat(d_att, d_latt, NH, d_attc)
    p_bwd = lambda: ops.attn_bwd(qc, kc, vc, attc, d_attc, lse, B, NH, S, dc, 1.0, None, kb, dcat, None, drop_p=DROP_P, drop_words=words)
    p_split_q = lambda: ops.head_split(dcat[:, :NH * dc], NH, dqkv[:, :H], dlqkv[:, :Hl], sa, sb)
    p_split_kv = lambda: ops.head_split(dcat[:, NH * dc:], 2 * NH, dqkv[:, H:], dlqkv[:, Hl:])
    n_fwd = lambda: ops.attn2_fwd(qa, ka, va, qb, kb_, vb, B, NH, S, sa, sb, kb, out_a=att2, out_b=latt2, lse=lse2, drop_p=DROP_P,
                                  drop_words=words)
    n_bwd = lambda: ops.attn2_bwd(qa, ka, va, qb, kb_, vb, att2, d_att, latt2, d_latt, lse2, B, NH, S, sa, sb, kb, dqkv2, dlqkv2,
                                  drop_p=DROP_P, drop_words=words)

    def parent_fwd():
        p_cat_q(); p_cat_kv(); p_fwd(); p_split()

    def parent_bwd():
        p_cat_d(); p_bwd(); p_split_q(); p_split_kv()

    parent_fwd(); parent_bwd(); n_fwd(); n_bwd()
    torch.cuda.synchronize()
    same_f = torch.equal(att, att2) and torch.equal(latt, latt2) and torch.equal(lse, lse2)
    same_b = torch.equal(dqkv, dqkv2) and torch.equal(dlqkv, dlqkv2)
    print(f"(a) one layer's attention, B = {B}, nh = {NH}, T = {S}, head dims {DA} + {DB}, drop_p = {DROP_P}: forward outputs "
          f"identical: {same_f}; gradients identical: {same_b}")
    ab("(a) forward", "us", 1.0, parent_fwd, n_fwd)
    ab("(a) backward", "us", 1.0, parent_bwd, n_bwd)
    ab("(a) forward + backward", "us", 1.0, lambda: (parent_fwd(), parent_bwd()), lambda: (n_fwd(), n_bwd()))
    print("(a) every op call on its own:")
    for name, fn in (("parent head_concat q", p_cat_q), ("parent head_concat k | v", p_cat_kv), ("parent attn_fwd (d = 80)", p_fwd),
                     ("parent head_split out", p_split), ("parent head_concat d_out", p_cat_d),
                     ("parent attn_bwd (delta + single pass + dQ, d = 80)", p_bwd), ("parent head_split dq", p_split_q),
                     ("parent head_split dk | dv", p_split_kv), ("attn2_fwd", n_fwd), ("attn2_bwd (delta + dK/dV/dS^T + dQ)", n_bwd)):
        alone(name, fn)
    kernel_table("parent attn_bwd", p_bwd)
    kernel_table("attn2_bwd", n_bwd)


def train_step():
    pcfg = peneo_config("lilt-roberta-en-base", lilt_config("base"))
    m = PEneoModel(PEneoConfig(**{k: v for k, v in pcfg.items() if k != "model_type"}))
    seeded_fill_(m.state_dict(), 13)
    m = m.cuda().set_compute_dtype(torch.bfloat16).train()
    m.backbone.check_inputs = False
    batch = synthetic_rfund_batch(B, S, 128, pcfg["backbone_config"]["vocab_size"], seed=0, ragged=True, with_image=False)
    batch = {k: v.cuda() for k, v in batch.items()}

    def step(switch, seed_step=None):
        def go():
            if switch is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = switch
            if seed_step is not None:
                DropoutSeeds._step, m._step = seed_step, seed_step
            m.zero_grad(set_to_none=True)
            out = m(**batch)
            out["loss"].backward()
            return out["loss"]
        return go

    def grads_of(fn):
        loss = fn().detach().clone()
        torch.cuda.synchronize()
        return loss, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    l0, g0 = grads_of(step(None, 50))
    l0b, g0b = grads_of(step(None, 50))
    print(f"(b) two steps of the parent path with the same seeds repeat bit for bit: "
          f"{torch.equal(l0, l0b) and all(torch.equal(g0[n], g0b[n]) for n in g0)} (the step has fp32 atomics outside the attention)")
    del g0b
    l1, g1 = grads_of(step("1", 50))
    same = torch.equal(l0, l1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    worst = min(float(torch.nn.functional.cosine_similarity(g0[n].double().flatten(), g1[n].double().flatten(), dim=0))
                for n in g0 if float(g0[n].abs().max()) > 0)
    print(f"(b) LiLT-base train step, {B} documents x {S} tokens, bf16, dropout on: loss off {float(l0):.6f} on {float(l1):.6f}; loss and "
          f"all {len(g0)} gradients identical: {same}; worst gradient cosine {worst:.6f}")
    del g0, g1
    ab("(b) train step (forward + loss + backward)", "ms", 1e-3, step(None), step("1"))
    for name, fn in (("parent", step(None)), ("attn2", step("1"))):
        fn(); torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn(); torch.cuda.synchronize()
        print(f"(b) peak device memory of one step, {name}: {torch.cuda.max_memory_allocated() / 2**20:.1f} MiB")
    os.environ.pop(SWITCH, None)


def main():
    print(f"device: {torch.cuda.get_device_name(0)}, {ROUNDS} rounds, {REPS} calls per timing")
    print(clocks())
    one_layer()
    train_step()
    print(clocks())


if __name__ == "__main__":
    main()
