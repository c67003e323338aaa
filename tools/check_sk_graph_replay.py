"""What test_gemm_stream_k_captured_equals_eager does, N_IT times, beside a second stream that runs a long GEMM in every third
iteration: a stream-k launch captured into a graph, replayed with fresh operands, against two eager launches.  Says what differs
when something does.  MODE = const (operands never change) | syncb (device synchronise after the operand copies) | synca (the
second stream synchronised before the replay); OLD_LIB = 1 with PENEO_HIP_LIB: a library from before the nn384 entry points."""
import ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peneo_amd import ops, hip
if os.environ.get("OLD_LIB"):
    for k in [k for k in hip.SIGNATURES if "nn384" in k or k == "peneo_gemm_big_mode"]: del hip.SIGNATURES[k]
lib = hip.load_library()
DEV = "cuda"
MODE = os.environ.get("MODE", "")
N_IT = int(os.environ.get("N_IT", 150))
g = torch.Generator().manual_seed(31)
M, N, K = 1500, 768, 3072
dt = torch.bfloat16
def operands():
    return (torch.randn(M, K, generator=g).to(DEV).to(dt), (torch.randn(N, K, generator=g) * 0.05).to(DEV).to(dt),
            torch.randn(N, generator=g).to(DEV))
print("lib", hip.LIB_PATH, flush=True)
# what the suite does before: some allocator churn and a side stream with a long GEMM
side = torch.cuda.Stream()
big_a = torch.randn(8192, 4096).to(DEV).to(dt); big_b = torch.randn(4096, 4096).to(DEV).to(dt)
a_s, b_s, bias_s = operands()
lib.peneo_gemm_set_sk_mode(105128)
ops.gemm(a_s, b_s, bias=bias_s, split_k=1)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
    out_s = ops.gemm(a_s, b_s, bias=bias_s, split_k=1)
bad = 0
for it in range(N_IT):
    if MODE != "const" or it == 0:
        a, b, bias = operands()
        a_s.copy_(a); b_s.copy_(b); bias_s.copy_(bias)
    if MODE == "syncb": torch.cuda.synchronize()
    if it % 3 == 1:
        with torch.cuda.stream(side):
            lib.peneo_gemm_set_sk_mode(0); ops.gemm(big_a, big_b, split_k=1); lib.peneo_gemm_set_sk_mode(105128)
    if MODE == "synca": side.synchronize()
    graph.replay()
    e1 = ops.gemm(a, b, bias=bias, split_k=1)
    e2 = ops.gemm(a, b, bias=bias, split_k=1)
    torch.cuda.synchronize()
    for name, x, y in (("graph-vs-eager", out_s, e1), ("eager-vs-eager", e1, e2)):
        if not torch.equal(x, y):
            bad += 1
            d = (x.float() - y.float())
            nz = d.nonzero()
            ref = a.float() @ b.float().t() + bias
            print(f"it {it} {name}: {nz.shape[0]} elements differ, max |d| {float(d.abs().max()):.4g}, rows {int(nz[:,0].min())}..{int(nz[:,0].max())} "
                  f"cols {int(nz[:,1].min())}..{int(nz[:,1].max())}; err of first {float((x.float()-ref).abs().max()):.4g} second {float((y.float()-ref).abs().max()):.4g}", flush=True)
print(f"MODE={MODE}: {bad} mismatches in {N_IT} iterations", flush=True)
lib.peneo_gemm_set_sk_mode(1)
