"""An encoder layer's four weight gradients dW = dy^T x alone at the benchmark shape (H = 768, I = 3072, K = 8 x 709 = 5672 rows,
fp32 out) as ONE peneo_gemm_group call: the 128 x 128 group (PENEO_WGRAD_NN384 mode 0, 432 two-per-CU workgroups) against the
384 x 192 group (mode 1, 96 one-per-CU workgroups), interleaved, device events; and, as before the grouped launch existed, four
peneo_gemm calls with split-k and their reductions.  ROUNDS / CALLS / ROWS override the defaults.
CU-ms = CUs held x time: 256 for the old launch (432 workgroups on 512 slots), 96 for the new one."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peneo_amd import ops, hip
lib = hip.load_library()
DEV = "cuda"
H, I, R = 768, 3072, int(os.environ.get("ROWS", 5672))
rounds, calls = int(os.environ.get("ROUNDS", 5)), int(os.environ.get("CALLS", 10))
g = torch.Generator(device=DEV).manual_seed(0)
def rnd(*shape): return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)
shapes = [(3 * H, H), (I, H), (H, I), (H, H)]          # QKV, FFN1, FFN2, output projection: (M, N) of dW [M, N] = dy [R, M]^T x [R, N]
probs = [(rnd(R, M), rnd(R, N), torch.empty(M, N, device=DEV)) for M, N in shapes]
def call(): ops.gemm_group(probs, a_kmajor=False, b_kmajor=False)
def four():
    for a, b, c in probs: ops.gemm(a, b, a_kmajor=False, b_kmajor=False, out=c)
def timeit(fn, n):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
before = lib.peneo_gemm_group_nn384_mode()
times, outs, took = {0: [], 1: [], 4: []}, {}, {}
for r in range(rounds):
    times[4].append(timeit(four, calls))
    for mode in (0, 1):
        lib.peneo_gemm_group_set_nn384_mode(mode)
        n0 = lib.peneo_gemm_group_nn384_launches()
        times[mode].append(timeit(call, calls))
        took[mode] = lib.peneo_gemm_group_nn384_launches() - n0
        if r == 0: outs[mode] = [c.clone() for _, _, c in probs]
lib.peneo_gemm_group_set_nn384_mode(before)
flop = sum(2.0 * M * N * R for M, N in shapes)
print(torch.cuda.get_device_name(0), f"H {H} I {I} rows {R}; us per grouped call, {rounds} interleaved rounds of {calls} calls")
for mode, name, wgs, cus in ((0, "128x128", sum(((M + 127) // 128) * ((N + 127) // 128) for M, N in shapes), 256),
                             (1, "384x192", sum((M // 384) * (N // 192) for M, N in shapes), 96)):
    t = sorted(times[mode])
    med = t[len(t) // 2]
    print(f"{name}: {wgs:3d} workgroups, median {med * 1e3:7.1f} us (min {t[0] * 1e3:.1f} max {t[-1] * 1e3:.1f}), {flop / med / 1e9:5.0f} TF/s, "
          f"{cus} CUs x {med * 1e3:.1f} us = {cus * med:6.2f} CU-ms, calls on the 384 x 192 path {took[mode]} of {calls + 2}", flush=True)
t = sorted(times[4])
print(f"four peneo_gemm calls (split-k + reduce): median {t[len(t) // 2] * 1e3:7.1f} us (min {t[0] * 1e3:.1f} max {t[-1] * 1e3:.1f})")
print("bit-equal outputs:", all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])))
