"""The pair heads' dW1 = dz^T x alone at the benchmark shape (M = 1920, N = 384, K = 1 081 344, fp32 out): the 128 x 128 kernel
(PENEO_GEMM_NN384 mode 0) against the 384 x 192 one-per-CU tiles (mode 1) over a sweep of split-k, interleaved, device events.
SPLITS_OLD / SPLITS_NEW / ROUNDS override the sweep."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peneo_amd import ops, hip
lib = hip.load_library()
DEV = "cuda"
M, N, K = 1920, 384, int(os.environ.get("K", 1081344))
old = [int(s) for s in os.environ.get("SPLITS_OLD", "3,11").split(",")]
new = [int(s) for s in os.environ.get("SPLITS_NEW", "4,6,8,10,12,16,25").split(",")]
rounds = int(os.environ.get("ROUNDS", 5))
g = torch.Generator(device=DEV).manual_seed(0)
dz = torch.randn(K, M, generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)
x = torch.randn(K, N, generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)
out = torch.empty(M, N, device=DEV)
def timeit(fn, n=10):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
outs = {}
times = {}
for r in range(rounds):
    for mode, splits in ((0, old), (1, new)):
        lib.peneo_gemm_set_nn384_mode(mode)
        for s in splits:
            fn = lambda: ops.gemm(dz, x, a_kmajor=False, b_kmajor=False, out=out, split_k=s)
            times.setdefault((mode, s), []).append(timeit(fn))
            if r == 0: outs[(mode, s)] = out.clone()
ref = outs[(0, old[0])]
print(torch.cuda.get_device_name(0), f"M {M} N {N} K {K}; ms per call (GEMM + split-k reduce), {rounds} interleaved rounds of 10 calls")
for (mode, s), t in times.items():
    t = sorted(t)
    err = float((outs[(mode, s)] - ref).abs().max() / ref.abs().max())
    print(f"{'384x192' if mode else '128x128'} split {s:3d}: median {t[len(t) // 2]:.3f} min {t[0]:.3f} max {t[-1]:.3f} ms "
          f"{2.0 * M * N * K / t[len(t) // 2] / 1e9:6.0f} TF/s  rel diff to 128x128 split {old[0]}: {err:.2e}", flush=True)
lib.peneo_gemm_set_nn384_mode(1)
