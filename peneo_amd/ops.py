"""Functional wrappers: torch tensors in, libpeneo_hip.so kernels on the current stream, tensors out.

These are 1:1 with the C entry points of include/peneo_hip.h (no autograd here; the
autograd.Functions in peneo_amd/model compose them).  Nothing falls back to PyTorch math.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import hip
from .hip import ACT_GELU, ACT_NONE, ACT_SILU, BF16, F32, check, dtype_code, lib, ptr, stream

_i64p = C.POINTER(C.c_int64)


class KernelTimer:
    """Optional HIP-event timing of individual launches on the current stream (bench.py's roofline leg).
    ``with ops.kernel_timer("name"):`` brackets a launch with two events; ``durations_ms()`` after a
    device synchronise gives the per-launch times."""

    def __init__(self) -> None:
        self.enabled = False
        self.events = {}

    def reset(self, enabled: bool) -> None:
        self.enabled = enabled
        self.events = {}

    def durations_ms(self, name: str):
        return [a.elapsed_time(b) for a, b in self.events.get(name, [])]


TIMER = KernelTimer()


class kernel_timer:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        if TIMER.enabled:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if TIMER.enabled:
            self.b.record()
            TIMER.events.setdefault(self.name, []).append((self.a, self.b))
        return False


def _c(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        raise hip.PeneoHipError("tensor must be contiguous")
    return t


# ----------------------------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------------------------
def _fill_epilogue(ep, out: torch.Tensor, *, bias=None, act=ACT_NONE, residual=None, preact=None, grad_src=None, grad_act=ACT_NONE,
                   alpha: float = 1.0, accumulate: bool = False, drop_p: float = 0.0, drop_seed: int = 0) -> None:
    ep.bias = ptr(bias)
    ep.act = act
    if preact is not None:
        assert preact.dtype == out.dtype and preact.shape == out.shape
        ep.preact, ep.ld_preact = ptr(preact), preact.stride(0)
    if grad_src is not None:
        assert grad_src.dtype == out.dtype and grad_src.shape == out.shape
        ep.grad_src, ep.ld_grad, ep.grad_act = ptr(grad_src), grad_src.stride(0), grad_act
    if residual is not None:
        assert residual.dtype == out.dtype and residual.shape == out.shape
        ep.residual, ep.ld_res = ptr(residual), residual.stride(0)
    ep.alpha = alpha
    ep.accumulate = 1 if accumulate else 0
    ep.drop_p, ep.drop_seed = drop_p, drop_seed & 0xFFFFFFFF


def gemm_group(problems: Sequence, *, a_kmajor: bool = True, b_kmajor: bool = True, accumulate: bool = False,
               out_dtype: Optional[torch.dtype] = None) -> List[torch.Tensor]:
    """Up to 4 independent bf16 GEMMs out_i = epilogue_i(op(A_i) op(B_i)) (one operand layout) in ONE launch, each tile with its
    full K.  A problem is (A, B, out) or (A, B, out, epilogue-dict) with out = None to allocate [M, N] of `out_dtype` (default
    bf16; all outputs share the dtype) and the epilogue keys of `gemm` (bias, act, residual, preact, grad_src, grad_act, drop_p,
    drop_seed, alpha).  Returns the outputs."""
    n = len(problems)
    arr = (hip.GemmProblem * n)()
    eps, outs = [], []
    for q, prob in zip(arr, problems):
        A, B, out = prob[0], prob[1], prob[2]
        kw = prob[3] if len(prob) > 3 else None
        M = A.shape[0] if a_kmajor else A.shape[1]
        K = A.shape[1] if a_kmajor else A.shape[0]
        N = B.shape[0] if b_kmajor else B.shape[1]
        if out is None:
            out = torch.empty((M, N), dtype=out_dtype or torch.bfloat16, device=A.device)
        assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and out.shape == (M, N)
        q.M, q.N, q.K = M, N, K
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(out), out.stride(0)
        q.accumulate = int(accumulate)
        if kw:
            ep = hip.GemmEpilogue()
            _fill_epilogue(ep, out, **kw)
            eps.append(ep)                            # (alive until the call has returned)
            q.ep = C.cast(C.pointer(ep), C.c_void_p)
        outs.append(out)
    with kernel_timer("gemm_group"):
        check(lib().peneo_gemm_group(dtype_code(torch.bfloat16), int(a_kmajor), int(b_kmajor), dtype_code(outs[0].dtype),
                                     arr, n, stream()), "peneo_gemm_group")
    return outs


def choose_split_k(M: int, N: int, K: int, dtype: torch.dtype) -> int:
    """Split the reduction only when the output grid cannot fill the 256 CUs."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    kt = (K + (63 if dtype == torch.bfloat16 else 31)) // (64 if dtype == torch.bfloat16 else 32)
    if tiles >= 192 or kt < 8:
        return 1
    # 512 = resident workgroups (2 per CU): never spill a few workgroups into a second, almost empty round
    return max(1, min(kt // 4, 512 // tiles, 16))


def gemm_nn384_takes(M: int, N: int, K: int, dtype: torch.dtype) -> bool:
    """Whether peneo_gemm runs C[M, N] = A[K, M]^T B[K, N] (fp32 C, no epilogue option beyond accumulate, aligned operands) on
    its 384 x 192 one-per-CU tiles (the rule of launch_gemm_big_nn, gemm_big.hip): a caller picks its split-k from that."""
    return dtype == torch.bfloat16 and bool(lib().peneo_gemm_nn384_shape_ok(M, N, K))     # (the library holds the rule's numbers)


def choose_split_k_nn384(M: int, N: int, K: int) -> int:
    """Split-k of a launch on the 384 x 192 one-per-CU tiles that has the chip to itself: ONE round of the 256 CUs (10 tiles: split 25,
    1.54 ms at the pair heads' dW1 against 2.50 / 1.94 at split 12 / 16 and 2.01 for the 128 x 128 kernel at ITS stand-alone split 11,
    profiles/r07_dw1_nn384.txt), at least 8 k-tiles per workgroup."""
    tiles = (M // 384) * (N // 192)
    return max(1, min(K // 64 // 8, 256 // tiles))


def gemm(a: torch.Tensor, b: torch.Tensor, *, a_kmajor: bool = True, b_kmajor: bool = True,
         bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
         preact: Optional[torch.Tensor] = None, grad_src: Optional[torch.Tensor] = None, grad_act: int = ACT_NONE,
         out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None, accumulate: bool = False,
         alpha: float = 1.0, drop_p: float = 0.0, drop_seed: int = 0, split_k: Optional[int] = None,
         pair_dz=None, pair_dz_ws: Optional[torch.Tensor] = None, a_colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = epilogue(alpha * A.B^T); a, b are 2-D (row stride may exceed the row length).
    a_colsum (a_kmajor=False only): fp32 [M] that receives += the column sums of a = [K, M] -- the bias gradient beside a
    weight gradient, from the tiles the product holds in LDS anyway."""
    assert a.dim() == 2 and b.dim() == 2 and a.dtype == b.dtype
    assert a.stride(1) == 1 and b.stride(1) == 1
    if a_kmajor:
        M, K = a.shape
    else:
        K, M = a.shape
    if b_kmajor:
        N, Kb = b.shape
    else:
        Kb, N = b.shape
    assert K == Kb, f"inner dims differ: {K} vs {Kb}"
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or a.dtype, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    ep = hip.GemmEpilogue()
    ep.bias = ptr(bias)
    ep.act = act
    if preact is not None:
        assert preact.dtype == out.dtype and preact.shape == out.shape
        ep.preact, ep.ld_preact = ptr(preact), preact.stride(0)
    if grad_src is not None:
        assert grad_src.dtype == out.dtype and grad_src.shape == out.shape
        ep.grad_src, ep.ld_grad, ep.grad_act = ptr(grad_src), grad_src.stride(0), grad_act
    if residual is not None:
        assert residual.dtype == out.dtype and residual.shape == out.shape
        ep.residual, ep.ld_res = ptr(residual), residual.stride(0)
    ep.alpha = alpha
    ep.accumulate = 1 if accumulate else 0
    ep.drop_p, ep.drop_seed = drop_p, drop_seed & 0xFFFFFFFF
    if a_colsum is not None:
        assert not a_kmajor and a_colsum.dtype == torch.float32 and a_colsum.numel() == M and a_colsum.is_contiguous()
        ep.a_colsum = ptr(a_colsum)
    if pair_dz is not None:      # hip.PairDzArgs: the tile is z of the pair heads; store dz, accumulate dW2 / db1 partials
        ep.pair_dz, ep.pair_dz_ws = C.cast(C.pointer(pair_dz), C.c_void_p), ptr(pair_dz_ws)
        split_k = 1
    if split_k is None:
        # (the shape and option part of launch_gemm_big_nn's rule; a misaligned operand keeps the 128 x 128 kernel at a split that is
        # merely not its best)
        plain = (bias is None and act == ACT_NONE and residual is None and preact is None and grad_src is None and alpha == 1.0
                 and drop_p == 0.0 and a_colsum is None and pair_dz is None)
        if not a_kmajor and not b_kmajor and plain and out.dtype == torch.float32 and gemm_nn384_takes(M, N, K, a.dtype):
            split_k = choose_split_k_nn384(M, N, K)
        else:
            split_k = choose_split_k(M, N, K, a.dtype)
    # split-k partials, or the flags and slabs of a stream-k launch (which may need them with split_k == 1)
    ws_bytes = lib().peneo_gemm_workspace_bytes(M, N, K, split_k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device) if ws_bytes else None
    check(lib().peneo_gemm(dtype_code(a.dtype), int(a_kmajor), int(b_kmajor), M, N, K, ptr(a), a.stride(0), ptr(b),
                           b.stride(0), ptr(out), out.stride(0), dtype_code(out.dtype), C.byref(ep), split_k, ptr(ws),
                           ws_bytes, stream()), "peneo_gemm")
    return out


# ----------------------------------------------------------------------------------------------
# element-wise plumbing
# ----------------------------------------------------------------------------------------------
def cast(src: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _c(src)
    if out is None:
        out = torch.empty(src.shape, dtype=dtype, device=src.device)
    check(lib().peneo_cast(ptr(src), dtype_code(src.dtype), ptr(out), dtype_code(out.dtype), src.numel(), stream()),
          "peneo_cast")
    return out


class CastPlan:
    """Device tables of a fixed set of (fp32 source, bf16 destination) pairs for ``peneo_cast_multi``: built once, launched
    whenever the sources have changed."""

    def __init__(self, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]]):
        import numpy as np
        chunk = int(lib().peneo_cast_multi_chunk_elems())
        items = (hip.CastItem * len(pairs))()
        ci, cx = [], []
        for k, (src, dst) in enumerate(pairs):
            assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.is_contiguous() and dst.is_contiguous()
            assert src.numel() == dst.numel()
            items[k].src, items[k].dst, items[k].numel = src.data_ptr(), dst.data_ptr(), src.numel()
            n = (src.numel() + chunk - 1) // chunk
            ci += [k] * n
            cx += list(range(n))
        dev = pairs[0][0].device
        raw = np.frombuffer(bytes(items), dtype=np.uint8).copy()
        self.table = torch.from_numpy(raw).to(dev)
        self.chunk_item = torch.tensor(ci, dtype=torch.int32, device=dev)
        self.chunk_index = torch.tensor(cx, dtype=torch.int32, device=dev)
        self.n_chunks = len(ci)
        self.keep = list(pairs)                     # the tensors whose addresses the table holds

    def run(self) -> None:
        check(lib().peneo_cast_multi(ptr(self.table), ptr(self.chunk_item), ptr(self.chunk_index), self.n_chunks, stream()),
              "peneo_cast_multi")


class AdamwEmitTable:
    """Emission table of ``peneo_adamw_step_emit`` for a fixed list of AdamW tensors (in the order of the ``peneo_adamw_tensor``
    table): ``update(pairs)`` takes ``(parameter, destination view)`` pairs -- the step then also writes the updated parameter,
    in the view's dtype, into the view -- and copies the table to the device only when the pairs differ from the last call's.
    A pair's parameter is matched to the list by address and size, so a full view of a parameter counts as that parameter.
    Any number of pairs may name one parameter.  ``ValueError``: a parameter that is not in the list, a destination that is
    not contiguous, lives on another device, is neither bf16 nor fp32, or whose numel differs from the parameter's."""

    def __init__(self, params: Sequence[torch.Tensor]):
        self.params = list(params)
        self.index = {(p.data_ptr(), p.numel()): k for k, p in enumerate(self.params)}
        self.n_records = 0
        self.keep: list = []                        # the destinations whose addresses the table holds
        self._sig = None
        self._dev = None

    def reindex(self) -> bool:
        """The parameters' storage may have moved (``p.data = ...``): match by their current addresses, rebuild on the next
        update.  True when anything moved."""
        index = {(p.data_ptr(), p.numel()): k for k, p in enumerate(self.params)}
        if index == self.index:
            return False
        self.index, self._sig = index, None
        return True

    def records(self, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> List[Tuple[int, int, int]]:
        """Validated (tensor, destination address, dtype code) records, sorted by tensor (host work only)."""
        out = []
        for p, dst in pairs:
            k = self.index.get((p.data_ptr(), p.numel()))
            if k is None:
                raise ValueError("adamw emission: the parameter is not one of the step's tensors")
            if dst.device != p.device:
                raise ValueError(f"adamw emission: destination on {dst.device}, parameter on {p.device}")
            if dst.dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"adamw emission: destination dtype {dst.dtype} is neither bf16 nor fp32")
            if dst.numel() != p.numel():
                raise ValueError(f"adamw emission: destination has {dst.numel()} elements, the parameter {p.numel()}")
            if not dst.is_contiguous():
                raise ValueError("adamw emission: the destination must be one contiguous run of elements")
            out.append((k, dst.data_ptr(), dtype_code(dst.dtype)))
        out.sort(key=lambda r: r[0])                # stable: a tensor's records keep the order of the pairs
        return out

    def update(self, pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> None:
        sig = tuple((p.data_ptr(), p.numel(), d.data_ptr(), d.dtype, d.numel()) for p, d in pairs)
        if sig == self._sig:
            return
        recs = self.records(pairs)
        n, nt = len(recs), len(self.params)
        host = (hip.AdamwEmit * max(n, 1))()
        first = (C.c_int32 * (nt + 1))()
        for r, (k, addr, code) in enumerate(recs):
            host[r].dst, host[r].tensor, host[r].dtype = addr, k, code
            first[k + 1] += 1
        for k in range(nt):
            first[k + 1] += first[k]
        raw = bytes(host) + bytes(first)            # one buffer, one H2D copy: [records | first]
        if self._dev is None or self._dev.numel() != len(raw):
            self._dev = torch.empty(len(raw), dtype=torch.uint8, device=self.params[0].device)
        self._dev.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        self._first_off = C.sizeof(host)
        self.n_records, self.keep, self._sig = n, [d for _, d in pairs], sig

    @property
    def emits_ptr(self) -> int:
        return self._dev.data_ptr()

    @property
    def first_ptr(self) -> int:
        return self._dev.data_ptr() + self._first_off


def adamw_step_emit(table: torch.Tensor, chunk_tensor: torch.Tensor, chunk_index: torch.Tensor, beta1: float, beta2: float,
                    eps: float, step: int, emit: Optional[AdamwEmitTable], sqnorm: Optional[torch.Tensor] = None,
                    max_grad_norm: float = 0.0) -> None:
    """One fused AdamW step over the device table of ``hip.AdamwTensor`` (chunk maps as for ``peneo_adamw_step``) that also
    writes the working copies named by ``emit``; ``emit`` None or empty: the plain step."""
    if emit is not None and emit.n_records and emit._dev.device != table.device:
        raise ValueError("adamw emission: the emission table lives on another device than the tensor table")
    on = emit is not None and emit.n_records > 0
    check(lib().peneo_adamw_step_emit(ptr(table), ptr(chunk_tensor), ptr(chunk_index), chunk_tensor.numel(), float(beta1),
                                      float(beta2), float(eps), int(step), ptr(sqnorm), float(max_grad_norm),
                                      emit.emits_ptr if on else None, emit.first_ptr if on else None, stream()),
          "peneo_adamw_step_emit")


def copy2d(src: torch.Tensor, out: Optional[torch.Tensor] = None, drop_p: float = 0.0, drop_seed: int = 0) -> torch.Tensor:
    assert src.dim() == 2 and src.stride(1) == 1
    if out is None:
        out = torch.empty(src.shape, dtype=src.dtype, device=src.device)
    assert out.shape == src.shape and out.stride(1) == 1
    check(lib().peneo_copy2d(dtype_code(src.dtype), ptr(src), src.stride(0), ptr(out), out.stride(0), src.shape[0],
                             src.shape[1], drop_p, drop_seed & 0xFFFFFFFF, stream()), "peneo_copy2d")
    return out


def copy_rows(src: torch.Tensor, dst: torch.Tensor, drop_p: float = 0.0, drop_seed: int = 0) -> torch.Tensor:
    """Copy between [B, R, C] views whose last dim is contiguous (either side may be a slice of a larger buffer)."""
    assert src.dim() == 3 and dst.dim() == 3 and src.shape == dst.shape and src.dtype == dst.dtype
    assert src.stride(2) == 1 and dst.stride(2) == 1
    Bn, R, Cn = src.shape
    check(lib().peneo_copy_rows(dtype_code(src.dtype), ptr(src), R, src.stride(0), src.stride(1), ptr(dst), R, dst.stride(0),
                                dst.stride(1), Bn * R, Cn, drop_p, drop_seed & 0xFFFFFFFF, stream()), "peneo_copy_rows")
    return dst


def head_concat(a: torch.Tensor, b: torch.Tensor, nh: int, out: torch.Tensor, scale_a: float = 1.0, scale_b: float = 1.0):
    """out[r, h*(da+db) + c] = [scale_a * a_h | scale_b * b_h]; a, b, out are 2-D views with unit column stride."""
    da, db = a.shape[1] // nh, b.shape[1] // nh
    assert out.shape[1] == nh * (da + db) and a.shape[0] == b.shape[0] == out.shape[0]
    check(lib().peneo_head_concat(dtype_code(a.dtype), ptr(a), a.stride(0), da, scale_a, ptr(b), b.stride(0), db, scale_b,
                                  ptr(out), out.stride(0), a.shape[0], nh, stream()), "peneo_head_concat")
    return out


def head_split(x: torch.Tensor, nh: int, a: torch.Tensor, b: torch.Tensor, scale_a: float = 1.0, scale_b: float = 1.0):
    da, db = a.shape[1] // nh, b.shape[1] // nh
    assert x.shape[1] == nh * (da + db) and a.shape[0] == b.shape[0] == x.shape[0]
    check(lib().peneo_head_split(dtype_code(x.dtype), ptr(x), x.stride(0), ptr(a), a.stride(0), da, scale_a, ptr(b),
                                 b.stride(0), db, scale_b, x.shape[0], nh, stream()), "peneo_head_split")
    return a, b


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    assert x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
        accumulate = False
    check(lib().peneo_colsum(dtype_code(x.dtype), ptr(x), x.stride(0), x.shape[0], x.shape[1], ptr(out), int(accumulate),
                             stream()), "peneo_colsum")
    return out


# ----------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------
def _rowmap(t: torch.Tensor, H: int) -> Tuple[int, int, int]:
    """(rows, rows_per_batch, batch_stride) for a [rows, H] or a sliced [B, R, H] tensor."""
    assert t.stride(-1) == 1 and t.shape[-1] == H
    if t.dim() == 2:
        assert t.stride(0) == H
        return t.shape[0], 0, 0
    assert t.dim() == 3 and t.stride(1) == H
    return t.shape[0] * t.shape[1], t.shape[1], t.stride(0)


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None,
                  drop_p: float = 0.0, drop_seed: int = 0):
    H = x.shape[-1]
    rows, xr, xb = _rowmap(x, H)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    orows, yr, yb = _rowmap(out, H)
    assert orows == rows and out.dtype == x.dtype
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib().peneo_layernorm_fwd(dtype_code(x.dtype), ptr(x), xr, xb, ptr(out), yr, yb, ptr(gamma), ptr(beta), eps,
                                    ptr(mean), ptr(rstd), rows, H, drop_p, drop_seed & 0xFFFFFFFF, stream()),
          "peneo_layernorm_fwd")
    return out, mean, rstd


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                  dgamma: torch.Tensor, dbeta: torch.Tensor, dx: Optional[torch.Tensor] = None, drop_p: float = 0.0,
                  drop_seed: int = 0, dx_dropped: Optional[torch.Tensor] = None, drop2_p: float = 0.0,
                  drop2_seed: int = 0, dx_colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx_colsum (fp32 [H], accumulated into): column sums of dx_dropped (of dx without it) = the bias gradient of the Linear in
    front of this LayerNorm."""
    H = x.shape[-1]
    assert dx_colsum is None or (dx_colsum.dtype == torch.float32 and dx_colsum.numel() == H and dx_colsum.is_contiguous())
    rows, xr, xb = _rowmap(x, H)
    drows, dr, db = _rowmap(dy, H)
    assert drows == rows and dy.dtype == x.dtype
    if dx is None:
        dx = torch.empty(dy.shape, dtype=x.dtype, device=x.device)
    _, gr, gb = _rowmap(dx, H)
    check(lib().peneo_layernorm_bwd(dtype_code(x.dtype), ptr(dy), dr, db, ptr(x), xr, xb, ptr(dx), gr, gb, ptr(gamma),
                                    ptr(mean), ptr(rstd), ptr(dgamma), ptr(dbeta), rows, H, drop_p,
                                    drop_seed & 0xFFFFFFFF, ptr(dx_dropped), drop2_p, drop2_seed & 0xFFFFFFFF, ptr(dx_colsum),
                                    stream()),
          "peneo_layernorm_bwd")
    return dx


def layernorm_bwd_partial(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                          dx: Optional[torch.Tensor] = None, drop_p: float = 0.0, drop_seed: int = 0,
                          dx_dropped: Optional[torch.Tensor] = None, drop2_p: float = 0.0, drop2_seed: int = 0):
    """LayerNorm backward with the parameter gradients left as per-workgroup partial sums: -> (dx, partials [P, 2H] fp32 with
    [dgamma | dbeta] per row) or (None, None) when this dtype / row length has no such form.  ``colsum(partials)`` gives
    [dgamma | dbeta]; the model runs that reduction on its weight-gradient stream."""
    H = x.shape[-1]
    rows, xr, xb = _rowmap(x, H)
    drows, dr, db = _rowmap(dy, H)
    assert drows == rows and dy.dtype == x.dtype
    P = int(lib().peneo_layernorm_bwd_partial_rows(dtype_code(x.dtype), rows, H))
    if P <= 0:
        return None, None
    if dx is None:
        dx = torch.empty(dy.shape, dtype=x.dtype, device=x.device)
    _, gr, gb = _rowmap(dx, H)
    partials = torch.empty((P, 2 * H), dtype=torch.float32, device=x.device)
    check(lib().peneo_layernorm_bwd_partial(dtype_code(x.dtype), ptr(dy), dr, db, ptr(x), xr, xb, ptr(dx), gr, gb, ptr(gamma),
                                            ptr(mean), ptr(rstd), ptr(partials), P, rows, H, drop_p,
                                            drop_seed & 0xFFFFFFFF, ptr(dx_dropped), drop2_p, drop2_seed & 0xFFFFFFFF, stream()),
          "peneo_layernorm_bwd_partial")
    return dx, partials


# ----------------------------------------------------------------------------------------------
# embeddings
# ----------------------------------------------------------------------------------------------
def position_ids(input_ids: torch.Tensor, pad_id: int) -> torch.Tensor:
    _c(input_ids)
    B, S = input_ids.shape
    out = torch.empty((B, S), dtype=torch.int32, device=input_ids.device)
    check(lib().peneo_position_ids(ptr(input_ids), B, S, pad_id, ptr(out), stream()), "peneo_position_ids")
    return out


def embed_fwd(dtype: torch.dtype, out: torch.Tensor, B: int, S: int, H: int, *, input_ids=None, pos_ids=None, bbox=None,
              word=None, type0=None, pos=None, x=None, y=None, h=None, w=None, clip_hw: bool = True,
              status: Optional[torch.Tensor] = None) -> torch.Tensor:
    tab = hip.EmbedTables()
    tab.word, tab.type0, tab.pos = ptr(word), ptr(type0), ptr(pos)
    tab.x, tab.y, tab.h, tab.w = ptr(x), ptr(y), ptr(h), ptr(w)
    if x is not None:
        tab.coord_size, tab.shape_size, tab.max_2d = x.shape[1], h.shape[1], x.shape[0]
    if word is not None:
        tab.vocab, tab.max_pos = word.shape[0], pos.shape[0]
    rows, rpb, bs = _rowmap(out, H)
    assert rows == B * S and out.dtype == dtype
    check(lib().peneo_embed_text_fwd(dtype_code(dtype), ptr(input_ids), ptr(pos_ids), ptr(bbox), C.byref(tab), B, S, H,
                                     int(clip_hw), ptr(out), rpb, bs, ptr(status), stream()), "peneo_embed_text_fwd")
    return out


def embed_bwd(d_out: torch.Tensor, B: int, S: int, H: int, *, input_ids=None, pos_ids=None, bbox=None, g_word=None,
              g_pos=None, g_x=None, g_y=None, g_h=None, g_w=None, clip_hw: bool = True, pad_id: int = 1) -> None:
    g = hip.EmbedGrads()
    g.word, g.pos = ptr(g_word), ptr(g_pos)
    g.x, g.y, g.h, g.w = ptr(g_x), ptr(g_y), ptr(g_h), ptr(g_w)
    cs = g_x.shape[1] if g_x is not None else 0
    ss = g_h.shape[1] if g_h is not None else 0
    m2 = g_x.shape[0] if g_x is not None else 0
    rows, rpb, bs = _rowmap(d_out, H)
    assert rows == B * S
    with kernel_timer("embed_bwd"):
        check(lib().peneo_embed_text_bwd(dtype_code(d_out.dtype), ptr(d_out), rpb, bs, ptr(input_ids), ptr(pos_ids), ptr(bbox),
                                         C.byref(g), cs, ss, m2, B, S, H, int(clip_hw), pad_id, stream()),
              "peneo_embed_text_bwd")


def im2col_patch16(image: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    _c(image)
    assert image.dtype == torch.float32
    B, Cc, Hi, Wi = image.shape
    out = torch.empty((B * (Hi // 16) * (Wi // 16), Cc * 256), dtype=dtype, device=image.device)
    check(lib().peneo_im2col_patch16(dtype_code(dtype), ptr(image), B, Cc, Hi, Wi, ptr(out), stream()),
          "peneo_im2col_patch16")
    return out


def visual_assemble_fwd(proj: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, B: int) -> torch.Tensor:
    npch, H = proj.shape[0] // B, proj.shape[1]
    vis = torch.empty((B, npch + 1, H), dtype=proj.dtype, device=proj.device)
    check(lib().peneo_visual_assemble_fwd(dtype_code(proj.dtype), ptr(_c(proj)), ptr(cls), ptr(pos), B, npch, H, ptr(vis),
                                          stream()), "peneo_visual_assemble_fwd")
    return vis


def visual_assemble_bwd(d_vis: torch.Tensor, d_cls: Optional[torch.Tensor], d_pos: Optional[torch.Tensor]) -> torch.Tensor:
    B, t, H = d_vis.shape
    d_proj = torch.empty((B * (t - 1), H), dtype=d_vis.dtype, device=d_vis.device)
    check(lib().peneo_visual_assemble_bwd(dtype_code(d_vis.dtype), ptr(_c(d_vis)), B, t - 1, H, ptr(d_proj), ptr(d_cls),
                                          ptr(d_pos), stream()), "peneo_visual_assemble_bwd")
    return d_proj


# ----------------------------------------------------------------------------------------------
# relative-position bias
# ----------------------------------------------------------------------------------------------
def relpos_inputs(attention_mask: Optional[torch.Tensor], bbox: Optional[torch.Tensor], vx: Optional[torch.Tensor],
                  vy: Optional[torch.Tensor], B: int, S: int, nv: int, want_pos: bool, want_xy: bool):
    """-> (key_mask, pos, xs, ys): int32 [B, S + nv] each (pos / xs, ys None when not wanted), one launch."""
    dev = (attention_mask if attention_mask is not None else bbox).device
    mk = lambda: torch.empty((B, S + nv), dtype=torch.int32, device=dev)
    km, pos = mk(), (mk() if want_pos else None)
    xs, ys = (mk(), mk()) if want_xy else (None, None)
    if attention_mask is not None:
        assert attention_mask.dtype == torch.int64 and attention_mask.is_contiguous()
    if want_xy:
        assert bbox.dtype == torch.int64 and bbox.is_contiguous()
    check(lib().peneo_relpos_inputs(ptr(attention_mask), ptr(bbox), ptr(vx), ptr(vy), B, S, nv, ptr(km), ptr(pos), ptr(xs), ptr(ys),
                                    stream()), "peneo_relpos_inputs")
    return km, pos, xs, ys


def relpos_buckets(pos: Optional[torch.Tensor], xs: Optional[torch.Tensor], ys: Optional[torch.Tensor], B: int, T: int,
                   lut1: Optional[torch.Tensor], half1: int, lut2: Optional[torch.Tensor], half2: int):
    dev = (pos if pos is not None else xs).device
    mk = lambda: torch.empty((B, T, T), dtype=torch.uint8, device=dev)
    bk1 = mk() if pos is not None else None
    bkx = mk() if xs is not None else None
    bky = mk() if ys is not None else None
    check(lib().peneo_relpos_buckets(ptr(pos), ptr(xs), ptr(ys), B, T, ptr(lut1), lut1.numel() if lut1 is not None else 0,
                                     half1, ptr(lut2), lut2.numel() if lut2 is not None else 0, half2, ptr(bk1), ptr(bkx),
                                     ptr(bky), stream()), "peneo_relpos_buckets")
    return bk1, bkx, bky


def attn_padded_len(T: int) -> int:
    return (T + 63) // 64 * 64


def attn_padded_dim(d: int) -> int:
    return (d + 31) // 32 * 32


def relpos_bias_fwd(dtype: torch.dtype, bk1, bkx, bky, w1, wx, wy, scale: float, B: int, nh: int, T: int,
                    key_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> bias [B, nh, T, Tp] (Tp = T rounded up to 64); padding columns and masked keys hold -1e30."""
    dev = (bk1 if bk1 is not None else bkx).device
    Tp = attn_padded_len(T)
    bias = torch.empty((B, nh, T, Tp), dtype=dtype, device=dev)
    check(lib().peneo_relpos_bias_fwd(dtype_code(dtype), ptr(bk1), ptr(bkx), ptr(bky), ptr(w1),
                                      w1.shape[1] if w1 is not None else 0, ptr(wx), ptr(wy),
                                      wx.shape[1] if wx is not None else 0, scale, B, nh, T, Tp, ptr(key_mask), ptr(bias),
                                      stream()), "peneo_relpos_bias_fwd")
    return bias


def relpos_bias_bwd_layers(ds: torch.Tensor, bk1_t, bkx_t, bky_t, dw1, dwx, dwy, scale: float) -> None:
    """ds: bf16 [L, B, nh, T, Tp] per-layer dS^T (attn_bwd's ds_out); bk*_t: transposed bucket maps, [B, T, T] (padded
    here to the kernel's row stride Tp) or already [B, T, Tp]."""
    L, B, nh, T, Tp = ds.shape

    def padded(t):
        if t is None or t.shape[-1] == Tp:
            return t
        out = torch.zeros((B, T, Tp), dtype=torch.uint8, device=t.device)
        out[:, :, :T] = t
        return out
    bk1_t, bkx_t, bky_t = padded(bk1_t), padded(bkx_t), padded(bky_t)
    bins1, bins2 = dw1.shape[1] if dw1 is not None else 0, dwx.shape[1] if dwx is not None else 0
    ws, ws_bytes = _relpos_bwd_workspace(nh, bins1, bins2, ds.device)
    check(lib().peneo_relpos_bias_bwd_layers_ws(ptr(_c(ds)), L, ds.stride(0), ptr(bk1_t), ptr(bkx_t), ptr(bky_t), ptr(dw1), bins1,
                                                ptr(dwx), ptr(dwy), bins2, scale, B, nh, T, Tp, ptr(ws), ws_bytes, stream()),
          "peneo_relpos_bias_bwd_layers_ws")


def _relpos_bwd_workspace(nh: int, bins1: int, bins2: int, device):
    """The fixed-point accumulators of the deterministic fold (None, 0 while the mode is off: the plain kernels)."""
    need = int(lib().peneo_relpos_bwd_workspace_bytes(nh, bins1, bins2))
    return (torch.empty((need + 7) // 8, dtype=torch.int64, device=device), need) if need else (None, 0)


def relpos_bias_bwd(g: torch.Tensor, bk1, bkx, bky, dw1, dwx, dwy, scale: float) -> None:
    B, nh, T, ldg = g.shape
    bins1, bins2 = dw1.shape[1] if dw1 is not None else 0, dwx.shape[1] if dwx is not None else 0
    ws, ws_bytes = _relpos_bwd_workspace(nh, bins1, bins2, g.device)
    check(lib().peneo_relpos_bias_bwd_ws(ptr(_c(g)), ldg, ptr(bk1), ptr(bkx), ptr(bky), ptr(dw1), bins1, ptr(dwx), ptr(dwy), bins2,
                                         scale, B, nh, T, ptr(ws), ws_bytes, stream()),
          "peneo_relpos_bias_bwd_ws")


# ----------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------
def head_transpose(x: torch.Tensor, B: int, nh: int, T: int, d: int) -> torch.Tensor:
    """x: 2-D view [B*T, nh*d] (row stride may be larger) -> [B, nh, DP, Tp] per-head transposed, zero padded."""
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.empty((B, nh, attn_padded_dim(d), attn_padded_len(T)), dtype=x.dtype, device=x.device)
    check(lib().peneo_head_transpose(dtype_code(x.dtype), ptr(x), x.stride(0), B, nh, T, d, ptr(out), stream()),
          "peneo_head_transpose")
    return out


def attn_drop_words_shape(B: int, nh: int, T: int, sets: int = 1):
    nqb, tk = C.c_int(0), C.c_int(0)
    lib().peneo_attn_drop_words_dims(T, C.byref(nqb), C.byref(tk))
    return (sets, B * nh, nqb.value, tk.value)


def attn_drop_words(B: int, nh: int, T: int, drop_p: float, drop_seed: int, device=None, sets: int = 1,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Keep bits of the attention dropout (peneo_attn_drop_words): int32 [sets, B * nh, query blocks, key slots], one launch for
    `sets` independent calls of the same shape (e.g. all layers of a step); hand set i to attn_fwd / attn_bwd of call i.
    `out`: a buffer of attn_drop_words_shape(...) allocated by the caller (e.g. on another stream than the one that fills it)."""
    shape = attn_drop_words_shape(B, nh, T, sets)
    words = out if out is not None else torch.empty(shape, dtype=torch.int32, device=device or torch.device("cuda"))
    assert tuple(words.shape) == shape and words.dtype == torch.int32 and words.is_contiguous()
    check(lib().peneo_attn_drop_words(ptr(words), sets * B, nh, T, drop_p, drop_seed & 0xFFFFFFFF, stream()), "peneo_attn_drop_words")
    return words


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, nh: int, T: int, d: int, scale: float,
             bias: Optional[torch.Tensor], key_bias: Optional[torch.Tensor] = None, drop_p: float = 0.0, drop_seed: int = 0,
             vt: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
             drop_words: Optional[torch.Tensor] = None):
    """q/k/v: 2-D views [B*T, nh*d] with a common row stride (e.g. slices of a fused QKV buffer).
    bias: [B, nh, T, Tp] from relpos_bias_fwd (masking folded in); key_bias: fp32 [B, Tp] additive (0 / -1e30).
    out [B*T, nh*d] / lse [B, nh, T] may be given (e.g. row slices of larger buffers).
    Dropout: `drop_words` = one set of attn_drop_words (the backward of this call takes the same set); without it the words
    are made here from (drop_p, drop_seed) - attn_bwd with the same pair regenerates the same bits."""
    if drop_p > 0 and drop_words is None:
        drop_words = attn_drop_words(B, nh, T, drop_p, drop_seed, q.device)
    assert q.stride(0) == k.stride(0) == v.stride(0) and q.stride(1) == 1
    if vt is None and q.dtype != torch.bfloat16:   # bf16 reads V in place (transpose reads); fp32 needs the transposed copy
        vt = head_transpose(v, B, nh, T, d)
    if out is None:
        out = torch.empty((B * T, nh * d), dtype=q.dtype, device=q.device)
    if lse is None:
        lse = torch.empty((B, nh, T), dtype=torch.float32, device=q.device)
    assert out.shape == (B * T, nh * d) and out.stride(1) == 1 and lse.is_contiguous() and lse.shape == (B, nh, T)
    check(lib().peneo_attn_fwd(dtype_code(q.dtype), ptr(q), ptr(k), ptr(v), q.stride(0), ptr(vt), B, nh, T, d, scale, ptr(bias),
                               bias.shape[-1] if bias is not None else 0, ptr(key_bias), ptr(out), out.stride(0), ptr(lse),
                               drop_p, ptr(drop_words) if drop_p > 0 else None, stream()), "peneo_attn_fwd")
    return out, lse


# ----------------------------------------------------------------------------------------------
# packed ("varlen") inference: the plan, the row movers, the per-document-length attention (include/peneo_hip.h, version 113)
# ----------------------------------------------------------------------------------------------
def _check_plan(who: str, dev, B: int, lens: torch.Tensor, cu_rows: Optional[torch.Tensor], live_t: Optional[torch.Tensor] = None,
                T: Optional[int] = None) -> None:
    def bad(t, shape):
        return (not torch.is_tensor(t)) or t.dtype != torch.int32 or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous()
    if bad(lens, (B,)):
        raise hip.PeneoHipError(f"{who}: lens must be a contiguous int32 [{B}] tensor on {dev}")
    if cu_rows is not None and bad(cu_rows, (B + 1,)):
        raise hip.PeneoHipError(f"{who}: cu_rows must be a contiguous int32 [{B + 1}] tensor on {dev}")
    if live_t is not None and bad(live_t, (B, T)):
        raise hip.PeneoHipError(f"{who}: live_t must be a contiguous int32 [{B}, {T}] tensor on {dev}")


def pack_plan(key_mask: torch.Tensor):
    """key_mask int32 [B, T] on the device (relpos_inputs' first output; holes allowed) -> (lens [B], cu_rows [B + 1], live_t [B, T]),
    all int32: the number of live tokens per document, their exclusive prefix sum, and the position of the i-th live token of each
    document (-1 from lens[b] on).  One launch, no host synchronisation."""
    if not torch.is_tensor(key_mask) or key_mask.dim() != 2 or key_mask.dtype != torch.int32 or not key_mask.is_cuda \
            or not key_mask.is_contiguous():
        raise hip.PeneoHipError("pack_plan: key_mask must be a contiguous int32 [B, T] device tensor")
    B, T = key_mask.shape
    dev = key_mask.device
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    cu_rows = torch.empty(B + 1, dtype=torch.int32, device=dev)
    live_t = torch.empty((B, T), dtype=torch.int32, device=dev)
    check(lib().peneo_pack_plan(ptr(key_mask), B, T, ptr(lens), ptr(cu_rows), ptr(live_t), stream()), "peneo_pack_plan")
    return lens, cu_rows, live_t


def _row_bytes(who: str, t: torch.Tensor, lead: int) -> int:
    if not t.is_contiguous() or not t.is_cuda:
        raise hip.PeneoHipError(f"{who}: tensors must be contiguous and on the device")
    n = t.numel() // max(lead, 1) * t.element_size()
    if n <= 0 or n % 4:
        raise hip.PeneoHipError(f"{who}: rows of {n} bytes (a positive multiple of 4 is needed)")
    return n


def rows_pack(src: torch.Tensor, live_t: torch.Tensor, lens: torch.Tensor, cu_rows: Optional[torch.Tensor], Tm: int,
              rows: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gather the live rows of src [B, T, ...] (peneo_rows_pack).  cu_rows given: -> [rows, ...], row cu_rows[b] + i = src[b, live_t[b, i]]
    (`rows` = cu_rows[B], known to the caller; rows of `out` that belong to no live token are left as they are).  cu_rows None: the
    per-document layout [B, Tm, ...] with zeros from lens[b] on."""
    if src.dim() < 2:
        raise hip.PeneoHipError("rows_pack: src must be [B, T, ...]")
    B, T = src.shape[:2]
    Tm = int(Tm)
    _check_plan("rows_pack", src.device, B, lens, cu_rows, live_t, T)
    if not 1 <= Tm <= T:
        raise hip.PeneoHipError(f"rows_pack: Tm = {Tm} outside 1 .. T = {T}")
    rb = _row_bytes("rows_pack", src, B * T)
    if cu_rows is not None:
        if out is None:
            if rows is None or not 1 <= int(rows) <= B * T:
                raise hip.PeneoHipError(f"rows_pack: the cu_rows layout needs rows in 1 .. B * T = {B * T}, got {rows}")
            out = torch.empty((int(rows),) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
        n_out = out.shape[0]
    else:
        if out is None:
            out = torch.empty((B, Tm) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
        if tuple(out.shape[:2]) != (B, Tm):
            raise hip.PeneoHipError(f"rows_pack: out must be [{B}, {Tm}, ...], got {tuple(out.shape)}")
        n_out = B * Tm
    if out.dtype != src.dtype or out.device != src.device or _row_bytes("rows_pack", out, n_out) != rb:
        raise hip.PeneoHipError("rows_pack: out must have src's dtype, device and row size")
    check(lib().peneo_rows_pack(ptr(src), ptr(live_t), ptr(lens), ptr(cu_rows), B, T, Tm, rb, ptr(out), n_out, stream()), "peneo_rows_pack")
    return out


def rows_unpack(src: torch.Tensor, live_t: torch.Tensor, lens: torch.Tensor, cu_rows: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inverse of rows_pack's cu_rows layout (peneo_rows_unpack): src [rows, ...] -> [B, T, ...] with EVERY row written - row
    (b, live_t[b, i]) from src row cu_rows[b] + i, all other rows zeros."""
    B, T = live_t.shape
    _check_plan("rows_unpack", src.device, B, lens, cu_rows, live_t, T)
    if src.dim() < 1 or src.shape[0] < 1:
        raise hip.PeneoHipError("rows_unpack: src must be [rows, ...] with rows >= 1")
    rb = _row_bytes("rows_unpack", src, src.shape[0])
    if out is None:
        out = torch.empty((B, T) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if tuple(out.shape[:2]) != (B, T) or out.dtype != src.dtype or out.device != src.device or _row_bytes("rows_unpack", out, B * T) != rb:
        raise hip.PeneoHipError(f"rows_unpack: out must be [{B}, {T}, ...] with src's dtype, device and row size")
    check(lib().peneo_rows_unpack(ptr(src), src.shape[0], ptr(live_t), ptr(lens), ptr(cu_rows), B, T, rb, ptr(out), stream()),
          "peneo_rows_unpack")
    return out


def attn_fwd_varlen_supported(dtype, d: int) -> bool:
    """True for (torch.bfloat16, 64), the one shape attn_fwd_varlen has a kernel for (host-side, no GPU call)."""
    code = dtype_code(dtype) if isinstance(dtype, torch.dtype) else int(dtype)
    return bool(lib().peneo_attn_fwd_varlen_supported(code, int(d)))


def attn_fwd_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, lens: torch.Tensor, cu_rows: torch.Tensor, nh: int, Tm: int,
                    d: int, scale: float, bias: torch.Tensor, out: Optional[torch.Tensor] = None,
                    lse: Optional[torch.Tensor] = None):
    """Per-document-length attention forward (peneo_attn_fwd_varlen).  q/k/v: 2-D views [rows, nh*d] with a common row stride; the
    rows of document b are cu_rows[b] .. + min(lens[b], Tm); bias [B, nh, Tm, bias_ld] bf16.  out [rows, nh*d] / lse [B, nh, Tm] may
    be given; rows past a document's length in lse, and rows of out that belong to no document, are not written.  bf16, d = 64 only:
    anything else raises (there is no fallback)."""
    B = lens.shape[0] if torch.is_tensor(lens) and lens.dim() == 1 else -1
    _check_plan("attn_fwd_varlen", q.device, B, lens, cu_rows)
    if not (q.dim() == k.dim() == v.dim() == 2 and q.shape == k.shape == v.shape and q.stride(0) == k.stride(0) == v.stride(0)
            and q.stride(1) == k.stride(1) == v.stride(1) == 1 and q.shape[1] == nh * d):
        raise hip.PeneoHipError("attn_fwd_varlen: q / k / v must be [rows, nh * d] views with one row stride")
    rows, Tm = q.shape[0], int(Tm)
    if not torch.is_tensor(bias) or bias.dim() != 4 or tuple(bias.shape[:3]) != (B, nh, Tm) or bias.dtype != q.dtype \
            or not bias.is_contiguous() or bias.device != q.device:
        raise hip.PeneoHipError(f"attn_fwd_varlen: bias must be a contiguous {q.dtype} [{B}, {nh}, {Tm}, bias_ld] tensor")
    if out is None:
        out = torch.empty((rows, nh * d), dtype=q.dtype, device=q.device)
    if lse is None:
        lse = torch.empty((B, nh, Tm), dtype=torch.float32, device=q.device)
    if tuple(out.shape) != (rows, nh * d) or out.stride(1) != 1 or out.dtype != q.dtype or tuple(lse.shape) != (B, nh, Tm) \
            or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise hip.PeneoHipError("attn_fwd_varlen: out must be [rows, nh * d], lse a contiguous fp32 [B, nh, Tm]")
    check(lib().peneo_attn_fwd_varlen(dtype_code(q.dtype), ptr(q), ptr(k), ptr(v), q.stride(0), rows, ptr(lens), ptr(cu_rows), B, nh, Tm,
                                      d, scale, ptr(bias), bias.shape[-1], ptr(out), out.stride(0), ptr(lse), stream()),
          "peneo_attn_fwd_varlen")
    return out, lse


def encoder_layer_fwd_packed(layer: "hip.EncoderLayer", lens: torch.Tensor, cu_rows: torch.Tensor, rows: int, out: torch.Tensor,
                             workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One C call for the packed inference forward of an encoder layer (include/peneo_hip.h, peneo_encoder_layer_fwd_packed): `layer`
    holds device pointers of buffers with `rows` rows that the caller keeps alive (layer.T = Tm); out [rows, H] bf16 is written."""
    rows = int(rows)
    _check_plan("encoder_layer_fwd_packed", out.device, int(layer.B), lens, cu_rows)
    if out.dtype != torch.bfloat16 or not out.is_contiguous() or tuple(out.shape) != (rows, int(layer.H)):
        raise hip.PeneoHipError(f"encoder_layer_fwd_packed: out must be a contiguous bf16 [{rows}, {int(layer.H)}] tensor")
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    with kernel_timer("encoder_layer_fwd_packed"):
        check(lib().peneo_encoder_layer_fwd_packed(C.byref(layer), ptr(lens), ptr(cu_rows), rows, ptr(out), ptr(workspace), wsb, stream()),
              "peneo_encoder_layer_fwd_packed")
    return out


def attn2_supported(dtype: torch.dtype, d_a: int, d_b: int) -> bool:
    """Whether attn2_fwd takes this dtype and pair of head dims (peneo_attn2_supported: a host-side question, no GPU call)."""
    return bool(lib().peneo_attn2_supported(dtype_code(dtype), d_a, d_b))


def attn2_fwd(q_a: torch.Tensor, k_a: torch.Tensor, v_a: torch.Tensor, q_b: torch.Tensor, k_b: torch.Tensor, v_b: torch.Tensor,
              B: int, nh: int, T: int, scale_a: float, scale_b: float, key_bias: Optional[torch.Tensor] = None,
              out_a: Optional[torch.Tensor] = None, out_b: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
              drop_p: float = 0.0, drop_words: Optional[torch.Tensor] = None):
    """Two-stream attention forward (LiLT): scores = (scale_a q_a).k_a + (scale_b q_b).k_b + key_bias, one softmax,
    out_a = P v_a and out_b = P v_b.  q_a/k_a/v_a: 2-D views [B*T, nh*d_a] with a common row stride, q_b/k_b/v_b: [B*T, nh*d_b]
    likewise (e.g. column slices of the fused qkv and lqkv buffers); key_bias: fp32 [B, Tp] additive (0 / -1e30).
    out_a [B*T, nh*d_a], out_b [B*T, nh*d_b] (row strides may be larger) and lse [B, nh, T] may be given.
    Attention dropout: `drop_p` with `drop_words` = one set of attn_drop_words (both value streams share the mask; attn2_bwd takes
    the same set); with both unset the call is peneo_attn2_fwd, otherwise peneo_attn2_fwd_dropout.
    Returns (out_a, out_b, lse); equal bit for bit to head_concat x 2 -> attn_fwd(d_a + d_b, scale 1) -> head_split."""
    assert q_a.dim() == 2 and q_b.dim() == 2 and q_a.shape[0] == q_b.shape[0] == B * T
    assert q_a.dtype == k_a.dtype == v_a.dtype == q_b.dtype == k_b.dtype == v_b.dtype
    assert q_a.stride(0) == k_a.stride(0) == v_a.stride(0) and q_a.stride(1) == k_a.stride(1) == v_a.stride(1) == 1
    assert q_b.stride(0) == k_b.stride(0) == v_b.stride(0) and q_b.stride(1) == k_b.stride(1) == v_b.stride(1) == 1
    assert q_a.shape == k_a.shape == v_a.shape and q_b.shape == k_b.shape == v_b.shape
    assert q_a.shape[1] % nh == 0 and q_b.shape[1] % nh == 0
    d_a, d_b = q_a.shape[1] // nh, q_b.shape[1] // nh
    if out_a is None:
        out_a = torch.empty((B * T, nh * d_a), dtype=q_a.dtype, device=q_a.device)
    if out_b is None:
        out_b = torch.empty((B * T, nh * d_b), dtype=q_a.dtype, device=q_a.device)
    if lse is None:
        lse = torch.empty((B, nh, T), dtype=torch.float32, device=q_a.device)
    assert out_a.shape == (B * T, nh * d_a) and out_a.stride(1) == 1 and out_a.dtype == q_a.dtype
    assert out_b.shape == (B * T, nh * d_b) and out_b.stride(1) == 1 and out_b.dtype == q_a.dtype
    assert lse.is_contiguous() and lse.shape == (B, nh, T) and lse.dtype == torch.float32
    if key_bias is not None:
        assert key_bias.dtype == torch.float32 and key_bias.is_contiguous() and key_bias.shape == (B, attn_padded_len(T))
    if drop_p == 0.0 and drop_words is None:
        check(lib().peneo_attn2_fwd(dtype_code(q_a.dtype), ptr(q_a), ptr(k_a), ptr(v_a), q_a.stride(0), ptr(q_b), ptr(k_b), ptr(v_b),
                                    q_b.stride(0), B, nh, T, d_a, d_b, scale_a, scale_b, ptr(key_bias), ptr(out_a), out_a.stride(0),
                                    ptr(out_b), out_b.stride(0), ptr(lse), stream()), "peneo_attn2_fwd")
        return out_a, out_b, lse
    _check_drop_words(drop_words, B, nh, T)
    check(lib().peneo_attn2_fwd_dropout(dtype_code(q_a.dtype), ptr(q_a), ptr(k_a), ptr(v_a), q_a.stride(0), ptr(q_b), ptr(k_b),
                                        ptr(v_b), q_b.stride(0), B, nh, T, d_a, d_b, scale_a, scale_b, ptr(key_bias), ptr(out_a),
                                        out_a.stride(0), ptr(out_b), out_b.stride(0), ptr(lse), drop_p,
                                        ptr(drop_words) if drop_p > 0 else None, stream()), "peneo_attn2_fwd_dropout")
    return out_a, out_b, lse


def _check_drop_words(drop_words: Optional[torch.Tensor], B: int, nh: int, T: int) -> None:
    if drop_words is not None:
        assert drop_words.dtype == torch.int32 and drop_words.is_contiguous()
        assert tuple(drop_words.shape) == attn_drop_words_shape(B, nh, T)[1:], "one set of attn_drop_words for (B, nh, T)"


def attn2_bwd_workspace_bytes(B: int, nh: int, T: int) -> int:
    return int(lib().peneo_attn2_bwd_workspace_bytes(B, nh, T))


def attn2_bwd(q_a: torch.Tensor, k_a: torch.Tensor, v_a: torch.Tensor, q_b: torch.Tensor, k_b: torch.Tensor, v_b: torch.Tensor,
              out_a: torch.Tensor, d_out_a: torch.Tensor, out_b: torch.Tensor, d_out_b: torch.Tensor, lse: torch.Tensor,
              B: int, nh: int, T: int, scale_a: float, scale_b: float, key_bias: Optional[torch.Tensor],
              dqkv_a: torch.Tensor, dqkv_b: torch.Tensor, drop_p: float = 0.0, drop_words: Optional[torch.Tensor] = None):
    """Two-stream attention backward (LiLT): the gradients of attn2_fwd's contract with respect to the unscaled q | k | v of both
    streams, written as dq | dk | dv into dqkv_a [B*T, 3*nh*d_a] and dqkv_b [B*T, 3*nh*d_b] (the fused-QKV layout; row strides may
    be larger).  out_* / lse: what attn2_fwd returned; d_out_*: their gradients (out_a / d_out_a share a row stride, out_b /
    d_out_b likewise); drop_p / drop_words: what the forward took.  The workspace (delta and the dS^T slab) is allocated here from
    peneo_attn2_bwd_workspace_bytes.  Equal bit for bit to head_concat -> attn_bwd(d_a + d_b, scale 1) -> head_split x 2."""
    assert q_a.dim() == 2 and q_b.dim() == 2 and q_a.shape[0] == q_b.shape[0] == B * T
    assert q_a.dtype == k_a.dtype == v_a.dtype == q_b.dtype == k_b.dtype == v_b.dtype
    assert q_a.stride(0) == k_a.stride(0) == v_a.stride(0) and q_a.stride(1) == k_a.stride(1) == v_a.stride(1) == 1
    assert q_b.stride(0) == k_b.stride(0) == v_b.stride(0) and q_b.stride(1) == k_b.stride(1) == v_b.stride(1) == 1
    assert q_a.shape == k_a.shape == v_a.shape and q_b.shape == k_b.shape == v_b.shape
    assert q_a.shape[1] % nh == 0 and q_b.shape[1] % nh == 0
    Ha, Hb = q_a.shape[1], q_b.shape[1]
    d_a, d_b = Ha // nh, Hb // nh
    for o, g, w in ((out_a, d_out_a, Ha), (out_b, d_out_b, Hb)):
        assert o.shape == g.shape == (B * T, w) and o.dtype == g.dtype == q_a.dtype
        assert o.stride(0) == g.stride(0) and o.stride(1) == g.stride(1) == 1
    assert lse.is_contiguous() and lse.shape == (B, nh, T) and lse.dtype == torch.float32
    assert dqkv_a.shape == (B * T, 3 * Ha) and dqkv_a.stride(1) == 1 and dqkv_a.dtype == q_a.dtype
    assert dqkv_b.shape == (B * T, 3 * Hb) and dqkv_b.stride(1) == 1 and dqkv_b.dtype == q_a.dtype
    if key_bias is not None:
        assert key_bias.dtype == torch.float32 and key_bias.is_contiguous() and key_bias.shape == (B, attn_padded_len(T))
    _check_drop_words(drop_words, B, nh, T)
    ws = torch.empty(max(attn2_bwd_workspace_bytes(B, nh, T), 16), dtype=torch.uint8, device=q_a.device)
    check(lib().peneo_attn2_bwd(dtype_code(q_a.dtype), ptr(q_a), ptr(k_a), ptr(v_a), q_a.stride(0), ptr(q_b), ptr(k_b), ptr(v_b),
                                q_b.stride(0), ptr(out_a), ptr(d_out_a), out_a.stride(0), ptr(out_b), ptr(d_out_b), out_b.stride(0),
                                ptr(lse), B, nh, T, d_a, d_b, scale_a, scale_b, ptr(key_bias), ptr(dqkv_a[:, :Ha]),
                                ptr(dqkv_a[:, Ha:2 * Ha]), ptr(dqkv_a[:, 2 * Ha:]), dqkv_a.stride(0), ptr(dqkv_b[:, :Hb]),
                                ptr(dqkv_b[:, Hb:2 * Hb]), ptr(dqkv_b[:, 2 * Hb:]), dqkv_b.stride(0), ptr(ws), drop_p,
                                ptr(drop_words) if drop_p > 0 else None, stream()), "peneo_attn2_bwd")
    return dqkv_a, dqkv_b


def attn_bwd(q, k, v, out, d_out, lse, B: int, nh: int, T: int, d: int, scale: float, bias, key_bias,
             dqkv: torch.Tensor, g_bias: Optional[torch.Tensor], drop_p: float = 0.0, drop_seed: int = 0,
             single_pass: Optional[bool] = None, ds_out: Optional[torch.Tensor] = None,
             dq_atomic: bool = False, drop_words: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dqkv: [B*T, 3*nh*d] buffer receiving dq | dk | dv (same layout as the fused QKV activations).
    bf16 runs the single-pass kernel (fp32 dQ accumulator, no transposed copies); fp32 the dQ + dK/dV pair."""
    H = nh * d
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    delta = torch.empty((B, nh, T), dtype=torch.float32, device=q.device)
    if drop_p > 0 and drop_words is None:
        drop_words = attn_drop_words(B, nh, T, drop_p, drop_seed, q.device)
    assert out.stride(0) == d_out.stride(0)
    if single_pass is None:
        single_pass = (q.dtype == torch.bfloat16 and H % 8 == 0 and dqkv.stride(0) % 8 == 0
                       and dqkv.data_ptr() % 16 == 0)
    kt = qt = dot = dq_acc = None
    if single_pass:
        assert q.dtype == torch.bfloat16, "the single-pass attention backward is bf16 only"
        if dq_atomic:      # dQ through fp32 atomics into an accumulator (kept for comparison: a quarter of the kernel's time)
            dq_acc = torch.empty((B * T, H), dtype=torch.float32, device=q.device)
        elif ds_out is None:   # dQ by a second kernel from the layer's dS^T: needs the slab even when nobody else wants it
            ds_out = torch.empty((B, nh, T, attn_padded_len(T)), dtype=q.dtype, device=q.device)
    else:
        kt = head_transpose(k, B, nh, T, d)
        qt = head_transpose(q, B, nh, T, d)
        dot = head_transpose(d_out, B, nh, T, d)
    check(lib().peneo_attn_bwd(dtype_code(q.dtype), ptr(q), ptr(k), ptr(v), q.stride(0), ptr(kt), ptr(qt), ptr(dot),
                               ptr(out), ptr(d_out), out.stride(0), ptr(lse), B, nh, T, d, scale, ptr(bias),
                               bias.shape[-1] if bias is not None else 0, ptr(key_bias), ptr(dq), ptr(dk), ptr(dv),
                               dqkv.stride(0), ptr(g_bias), ptr(delta), ptr(dq_acc), ptr(ds_out), drop_p,
                               ptr(drop_words) if drop_p > 0 else None, stream()), "peneo_attn_bwd")
    return dqkv


# ----------------------------------------------------------------------------------------------
# pair heads
# ----------------------------------------------------------------------------------------------
def _ptr_list(ts: Sequence[Optional[torch.Tensor]]):
    arr = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = ptr(t)
    return arr


def pair_heads_supported(dtype, D: int, num_heads: int) -> bool:
    """True where pair_heads_pack / pair_heads_fwd have a kernel for this dtype, width and head count (host-side query)."""
    return bool(lib().peneo_pair_heads_supported(dtype_code(dtype), int(D), int(num_heads)))


def pair_heads_pack(dtype: torch.dtype, w1: Sequence[torch.Tensor], w2: Sequence[torch.Tensor]) -> torch.Tensor:
    """w1[h]: [D, D] fp32, w2[h]: [C_h, D] fp32 -> one packed byte buffer (both layers, MFMA fragment order)."""
    nh, D = len(w1), w1[0].shape[1]
    dc = dtype_code(dtype)
    dev = w1[0].device
    if D > 512 and not pair_heads_supported(dtype, D, nh):   # (no packed image exists: peneo_pair_heads_packed_bytes is 0)
        raise hip.PeneoHipError(f"peneo_pair_heads_pack: D={D} not supported for {dtype} with {nh} heads (pair_heads_supported)")
    packed = torch.empty(lib().peneo_pair_heads_packed_bytes(dc, nh, D), dtype=torch.uint8, device=dev)
    classes = (C.c_int * nh)(*[w.shape[0] for w in w2])
    check(lib().peneo_pair_heads_pack(dc, _ptr_list([_c(w) for w in w1]), _ptr_list([_c(w) for w in w2]), classes, nh, D,
                                      ptr(packed), stream()), "peneo_pair_heads_pack")
    return packed


def _pair_heads_launch(entry: str, timer: str, ab: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                       classes: Sequence[int], want_logits: bool, tags, class_weights, *, typed: bool = False,
                       want_dlogits: bool = False, drop_p: float = 0.0, drop_seed: int = 0, save_bytes: Optional[int] = None,
                       save_buffers=None, lens: Optional[torch.Tensor] = None, logits_out=None):
    """The one launch behind pair_heads_fwd / pair_heads_fwd_lens / pair_heads_fwd_mxfp8 / pair_heads_fwd_mxfp8_save: fills
    PairHeadsDesc and PairLoss, allocates what the caller asked for and calls `entry` under kernel_timer(`timer`).  typed: the entry
    point takes the dtype code first.  save_bytes: the entry point is a saving one - loss partials in the saving launch's rows, and
    (act [>= save_bytes] uint8, x_rows) checked (save_buffers) or allocated, passed on and returned as a fourth value.  lens: the
    entry point takes the [B] int32 lengths after N.  logits_out: the caller's [B, P, C_h] fp32 maps instead of fresh ones."""
    B, N, D2 = ab.shape
    D = D2 // 2
    P = N * (N + 1) // 2
    nh = len(classes)
    dev = ab.device
    desc = hip.PairHeadsDesc()
    desc.num_heads, desc.D = nh, D
    for h, c in enumerate(classes):
        desc.classes[h] = c
    desc.w_packed, desc.b1, desc.b2 = ptr(wp), ptr(b1), ptr(b2)
    desc.drop_p, desc.drop_seed = float(drop_p), int(drop_seed) & 0xFFFFFFFF
    logits = [torch.empty((B, P, c), dtype=torch.float32, device=dev) for c in classes] if want_logits else None
    if want_logits and logits_out is not None:
        logits = list(logits_out)
        for lg, c in zip(logits, classes):
            assert lg.shape == (B, P, c) and lg.dtype == torch.float32 and lg.is_contiguous() and lg.device == dev
        assert len(logits) == nh
    loss = partials = dlog = None
    if tags is not None:
        loss = hip.PairLoss()
        nrows = lib().peneo_pair_loss_partials_save(B, N) if save_bytes is not None else lib().peneo_pair_loss_partials(B, N)
        partials = torch.empty((nrows, 32), dtype=torch.float32, device=dev)
        if want_dlogits:
            dlog = [torch.empty((B, P, c), dtype=torch.float32, device=dev) for c in classes]
        for h in range(nh):
            assert tags[h].dtype == torch.int64 and tags[h].shape == (B, P)
            loss.tags[h] = ptr(_c(tags[h]))
            loss.class_weight[h] = ptr(class_weights[h]) if class_weights is not None else None
            if dlog is not None:
                loss.dlogits[h] = ptr(dlog[h])
        loss.partials = ptr(partials)
    args = [dtype_code(ab.dtype)] if typed else []
    args += [ptr(ab), B, N] + ([ptr(lens)] if lens is not None else [])
    args += [C.byref(desc), _ptr_list(logits) if logits is not None else None, C.byref(loss) if loss is not None else None]
    saved = ()
    if save_bytes is not None:
        if save_buffers is not None:
            act, x_rows = save_buffers
            assert act.dtype == torch.uint8 and act.numel() >= save_bytes and act.is_contiguous()
            assert x_rows.shape == (B * pair_bwd_rows(N), D) and x_rows.dtype == ab.dtype and x_rows.is_contiguous()
        else:
            act = torch.empty(save_bytes, dtype=torch.uint8, device=dev)
            x_rows = torch.empty((B * pair_bwd_rows(N), D), dtype=ab.dtype, device=dev)
        args += [ptr(act), ptr(x_rows)]
        saved = ((act, x_rows),)
    with kernel_timer(timer):
        check(getattr(lib(), entry)(*args, stream()), entry)
    return (logits, partials, dlog) + saved


def pair_heads_fwd(ab: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                   classes: Sequence[int], *, want_logits: bool = True, tags: Optional[Sequence[torch.Tensor]] = None,
                   class_weights: Optional[Sequence[Optional[torch.Tensor]]] = None, want_dlogits: bool = False,
                   drop_p: float = 0.0, drop_seed: int = 0, save: bool = False, save_buffers=None, save_format: str = "f16"):
    """ab: [B, N, 2D].  Returns (logits list | None, loss partials [n, 32] | None, dlogits list | None).
    drop_p / drop_seed: the Dropout between the two classifier layers (train mode, model/peneo_decoder.py:261).
    save (pair_save_supported): the launch also leaves the hidden activations the backward needs; returns a fourth value
    (act [bytes] uint8, x_rows [B * pair_bwd_rows(N), D]) for pair_bwd_saved; save_buffers = (act, x_rows) supplies them.
    save_format: "f16" (2 KiB records, pair_save_bytes) or "e4m3" (1 KiB records of e4m3fn bytes, pair_save_e4m3_bytes; the backward
    is then pair_bwd_saved(act_format="e4m3"))."""
    if save_format not in PAIR_ACT_FORMATS:
        raise ValueError(f"save_format must be one of {PAIR_ACT_FORMATS}, got {save_format!r}")
    _c(ab)
    entry, nbytes = "peneo_pair_heads_fwd", None
    if save:
        B, N, D2 = ab.shape
        e4m3 = save_format == "e4m3"
        entry = "peneo_pair_heads_fwd_save_e4m3" if e4m3 else "peneo_pair_heads_fwd_save"
        nbytes = (lib().peneo_pair_save_e4m3_bytes if e4m3 else lib().peneo_pair_save_bytes)(B, N, len(classes), D2 // 2)
    return _pair_heads_launch(entry, "pair_heads_fwd", ab, wp, b1, b2, classes, want_logits, tags, class_weights, typed=True,
                              want_dlogits=want_dlogits, drop_p=drop_p, drop_seed=drop_seed, save_bytes=nbytes,
                              save_buffers=save_buffers)


PAIR_PAD_LOGIT = -1e30                  # include/peneo_hip.h: PENEO_PAIR_PAD_LOGIT (as fp32: torch.tensor(-1e30, dtype=torch.float32))


def pair_lens_from_mask(mask: Optional[torch.Tensor], N: int, *, B: Optional[int] = None, device=None) -> torch.Tensor:
    """Token counts for pair_heads_fwd_lens from an attention mask [B, >= N] (any integer / bool dtype, on the device): int32 [B],
    n_b = 1 + the last index below N whose mask is non-zero, 0 where there is none.  One launch, no host synchronisation.  mask None:
    every length is N (B and device say how many, and where)."""
    N = int(N)
    if mask is None:
        if B is None or device is None:
            raise ValueError("pair_lens_from_mask: without a mask, B and device are needed")
        lens = torch.empty(int(B), dtype=torch.int32, device=device)
        check(lib().peneo_pair_lens_from_mask(None, 0, int(B), N, ptr(lens), stream()), "peneo_pair_lens_from_mask")
        return lens
    if mask.dim() != 2 or mask.shape[1] < N or not mask.is_cuda:
        raise hip.PeneoHipError(f"pair_lens_from_mask: mask must be a device tensor [B, >= {N}], got {tuple(mask.shape)} on {mask.device}")
    if mask.dtype != torch.int64:
        mask = mask.to(torch.int64)
    if mask.stride(1) != 1:
        mask = mask.contiguous()
    lens = torch.empty(mask.shape[0], dtype=torch.int32, device=mask.device)
    check(lib().peneo_pair_lens_from_mask(ptr(mask), mask.stride(0), mask.shape[0], N, ptr(lens), stream()), "peneo_pair_lens_from_mask")
    return lens


def pair_heads_fwd_lens(ab: torch.Tensor, lens: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                        classes: Sequence[int], *, want_logits: bool = True, tags: Optional[Sequence[torch.Tensor]] = None,
                        class_weights: Optional[Sequence[Optional[torch.Tensor]]] = None, logits_out=None):
    """Length-aware inference form of pair_heads_fwd (include/peneo_hip.h: peneo_pair_heads_fwd_lens).  ab [B, N, 2D], wp from
    pair_heads_pack, lens [B] int32 on ab's device (pair_lens_from_mask).  Returns (logits list | None, loss partials [n, 32] | None,
    None) like pair_heads_fwd without dlogits: the logits of pairs with j < lens[b] are pair_heads_fwd's bit for bit, every other pair
    holds (0, PAIR_PAD_LOGIT, ...); the partial rows sum over the live pairs only, so loss_finish over them is the class-weighted
    mean over the pairs of real tokens, not the reference's mean over all P.  logits_out: caller-supplied maps to write into."""
    _c(ab)
    B = ab.shape[0]
    if not torch.is_tensor(lens) or lens.dtype != torch.int32 or lens.device != ab.device or lens.shape != (B,) \
            or not lens.is_contiguous():
        what = f"{lens.dtype} {tuple(lens.shape)} on {lens.device}" if torch.is_tensor(lens) else type(lens).__name__
        raise hip.PeneoHipError(f"pair_heads_fwd_lens: lens must be a contiguous int32 [{B}] tensor on {ab.device}, got {what}")
    return _pair_heads_launch("peneo_pair_heads_fwd_lens", "pair_heads_fwd_lens", ab, wp, b1, b2, classes, want_logits, tags,
                              class_weights, typed=True, lens=lens, logits_out=logits_out)


PAIR_ACT_FORMATS = ("f16", "e4m3")      # record formats of the saved pair activations (include/peneo_hip.h)


def pair_save_e4m3_bytes(B: int, N: int, num_heads: int, D: int) -> int:
    """Bytes of the e4m3 records of pair_heads_fwd(save=True, save_format="e4m3"): half of pair_save_bytes."""
    return int(lib().peneo_pair_save_e4m3_bytes(int(B), int(N), int(num_heads), int(D)))


def pair_save_e4m3_supported(dtype, D: int, num_heads: int) -> bool:
    """True when peneo_pair_heads_fwd_save_e4m3 / peneo_pair_bwd_saved_e4m3 exist for this shape (where pair_save_supported is)."""
    return bool(lib().peneo_pair_save_e4m3_supported(dtype_code(dtype), int(D), int(num_heads)))


def pair_save_bytes(B: int, N: int, num_heads: int, D: int) -> int:
    return int(lib().peneo_pair_save_bytes(int(B), int(N), int(num_heads), int(D)))


def pair_save_supported(dtype, D: int, num_heads: int) -> bool:
    """True when peneo_pair_heads_fwd_save / peneo_pair_bwd_saved exist for this shape (bf16, D = 384)."""
    return bool(lib().peneo_pair_save_supported(dtype_code(dtype), int(D), int(num_heads)))


def mxfp8_quantize_rows(src: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[rows, cols] fp32 (cols % 32 == 0) -> (e4m3 bytes [rows, cols] uint8, E8M0 bytes [rows, cols // 32] uint8): OCP MX
    quantization with the rounding and clamping of the MXFP8 pair-heads path (include/peneo_hip.h)."""
    src = _c(src)
    assert src.dtype == torch.float32 and src.dim() == 2
    rows, cols = src.shape
    q = torch.empty((rows, cols), dtype=torch.uint8, device=src.device)
    sc = torch.empty((rows, cols // 32), dtype=torch.uint8, device=src.device)
    check(lib().peneo_mxfp8_quantize_rows(ptr(src), rows, cols, ptr(q), ptr(sc), stream()), "peneo_mxfp8_quantize_rows")
    return q, sc


def mxfp8_quantize_rows_bf16(src: torch.Tensor, q: Optional[torch.Tensor] = None,
                             scales: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """mxfp8_quantize_rows for a bf16 source [rows, cols] (row stride % 8 == 0): the bytes the fp32 quantizer gives on the same values."""
    assert src.dtype == torch.bfloat16 and src.dim() == 2 and src.stride(1) == 1
    rows, cols = src.shape
    if q is None:
        q = torch.empty((rows, cols), dtype=torch.uint8, device=src.device)
    if scales is None:
        scales = torch.empty((rows, cols // 32), dtype=torch.uint8, device=src.device)
    assert q.dtype == torch.uint8 and q.shape == (rows, cols) and q.is_contiguous()
    assert scales.dtype == torch.uint8 and scales.shape == (rows, cols // 32) and scales.is_contiguous()
    check(lib().peneo_mxfp8_quantize_rows_bf16(ptr(src), rows, cols, src.stride(0), ptr(q), ptr(scales), stream()),
          "peneo_mxfp8_quantize_rows_bf16")
    return q, scales


def layernorm_mxfp8_supported(H: int) -> bool:
    """True when layernorm_fwd_mxfp8 holds this row length (host-side, no GPU call): H % 256 == 0, H <= 1024."""
    return bool(lib().peneo_layernorm_mxfp8_supported(int(H)))


def layernorm_fwd_mxfp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """layernorm_fwd of a contiguous bf16 [rows, H] plus the MX copy of its output in the same launch:
    returns (y, mean, rstd, y_q, y_s) with (y_q, y_s) == mxfp8_quantize_rows_bf16(y)."""
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.is_contiguous()
    rows, H = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    q = torch.empty((rows, H), dtype=torch.uint8, device=x.device)
    sc = torch.empty((rows, H // 32), dtype=torch.uint8, device=x.device)
    check(lib().peneo_layernorm_fwd_mxfp8(ptr(x), ptr(y), ptr(gamma), ptr(beta), eps, ptr(mean), ptr(rstd), rows, H, ptr(q), ptr(sc),
                                          stream()), "peneo_layernorm_fwd_mxfp8")
    return y, mean, rstd, q, sc


def gemm_mxfp8_supported(M: int, N: int, K: int) -> bool:
    """True when peneo_gemm_mxfp8 holds this shape (host-side, no GPU call): M >= 1, N % 32 == 0, K % 128 == 0."""
    return bool(lib().peneo_gemm_mxfp8_supported(int(M), int(N), int(K)))


def gemm_mxfp8(a_q: torch.Tensor, a_s: torch.Tensor, b_q: torch.Tensor, b_s: torch.Tensor, *,
               bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
               alpha: float = 1.0, out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16,
               store_c: bool = True, mx_out: bool = False):
    """C = epilogue(A^ B^^T) on the block-scaled FP8 MFMA: a_q [M, K] / b_q [N, K] e4m3 bytes (uint8) with a_s [M, K / 32] /
    b_s [N, K / 32] E8M0 bytes, as mxfp8_quantize_rows writes them.  Returns C (bf16 or fp32); with mx_out=True returns
    (C, C_q, C_s), the MX quantization of the bf16-rounded result along N, and C is None when store_c=False."""
    for t in (a_q, a_s, b_q, b_s):
        assert t.dtype == torch.uint8 and t.dim() == 2 and t.is_contiguous()
    M, K = a_q.shape
    N, Kb = b_q.shape
    assert K == Kb, f"inner dims differ: {K} vs {Kb}"
    assert a_s.shape == (M, K // 32) and b_s.shape == (N, K // 32)
    assert store_c or mx_out, "gemm_mxfp8: nothing to write"
    c_dtype = out.dtype if out is not None else out_dtype
    if store_c and out is None:
        out = torch.empty((M, N), dtype=c_dtype, device=a_q.device)
    if out is not None:
        assert store_c and out.shape == (M, N) and out.stride(1) == 1
    ep = hip.GemmEpilogue()
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    ep.bias = ptr(bias)
    ep.act = act
    if residual is not None:
        assert residual.dtype == c_dtype and residual.shape == (M, N) and residual.stride(1) == 1
        ep.residual, ep.ld_res = ptr(residual), residual.stride(0)
    ep.alpha = alpha
    c_q = torch.empty((M, N), dtype=torch.uint8, device=a_q.device) if mx_out else None
    c_s = torch.empty((M, N // 32), dtype=torch.uint8, device=a_q.device) if mx_out else None
    check(lib().peneo_gemm_mxfp8(M, N, K, ptr(a_q), ptr(a_s), ptr(b_q), ptr(b_s), ptr(out), out.stride(0) if out is not None else N,
                                 dtype_code(c_dtype), C.byref(ep), ptr(c_q), ptr(c_s), stream()), "peneo_gemm_mxfp8")
    return (out, c_q, c_s) if mx_out else out


def encoder_layer_mxfp8_supported(rows: int, H: int, I: int) -> bool:
    """True when the four products of an encoder layer (rows x 3H x H, rows x H x H, rows x I x H, rows x H x I) all pass
    gemm_mxfp8_supported (host-side, no GPU call)."""
    return bool(lib().peneo_encoder_layer_mxfp8_supported(int(rows), int(H), int(I)))


def encoder_layer_fwd_mxfp8(layer: "hip.EncoderLayer", mx: "hip.EncoderLayerMxfp8", out: torch.Tensor) -> torch.Tensor:
    """One C call for the MXFP8 inference forward of an encoder layer (include/peneo_hip.h, peneo_encoder_layer_fwd_mxfp8):
    `layer` / `mx` hold device pointers of buffers the caller keeps alive; out [rows, H] bf16 is written and returned."""
    assert out.dtype == torch.bfloat16 and out.is_contiguous()
    with kernel_timer("encoder_layer_fwd_mxfp8"):
        check(lib().peneo_encoder_layer_fwd_mxfp8(C.byref(layer), C.byref(mx), ptr(out), stream()), "peneo_encoder_layer_fwd_mxfp8")
    return out


def pair_mxfp8_supported(D: int, num_heads: int) -> bool:
    """True when the MXFP8 pair-heads kernel holds this shape (host-side, no GPU call)."""
    return bool(lib().peneo_pair_mxfp8_supported(int(D), int(num_heads)))


def pair_heads_pack_mxfp8(w1: Sequence[torch.Tensor], w2: Sequence[torch.Tensor]) -> torch.Tensor:
    """w1[h]: [D, D] fp32, w2[h]: [C_h, D] fp32 -> the packed buffer of pair_heads_fwd_mxfp8 (e4m3 + E8M0 first layer, bf16 second)."""
    nh, D = len(w1), w1[0].shape[1]
    nbytes = lib().peneo_pair_heads_mxfp8_packed_bytes(nh, D)
    if nbytes == 0:
        raise ValueError(f"MXFP8 pair heads: D={D} with {nh} heads is not supported")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w1[0].device)
    classes = (C.c_int * nh)(*[w.shape[0] for w in w2])
    check(lib().peneo_pair_heads_pack_mxfp8(_ptr_list([_c(w) for w in w1]), _ptr_list([_c(w) for w in w2]), classes, nh, D,
                                            ptr(packed), stream()), "peneo_pair_heads_pack_mxfp8")
    return packed


def pair_heads_fwd_mxfp8(ab: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                         classes: Sequence[int], *, want_logits: bool = True, tags: Optional[Sequence[torch.Tensor]] = None,
                         class_weights: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """Eval-only MXFP8 form of pair_heads_fwd: ab [B, N, 2D] bf16, wp from pair_heads_pack_mxfp8.
    Returns (logits list | None, loss partials [n, 32] | None, None) like pair_heads_fwd without dlogits."""
    _c(ab)
    assert ab.dtype == torch.bfloat16, "pair_heads_fwd_mxfp8 takes bf16 ab"
    return _pair_heads_launch("peneo_pair_heads_fwd_mxfp8", "pair_heads_fwd_mxfp8", ab, wp, b1, b2, classes, want_logits, tags,
                              class_weights)


def pair_mxfp8_wide_supported(D: int, num_heads: int) -> bool:
    """True when the wide MXFP8 pair-heads kernel holds this shape (host-side, no GPU call): D % 64 == 0, 512 < D <= 1024."""
    return bool(lib().peneo_pair_mxfp8_wide_supported(int(D), int(num_heads)))


def pair_heads_pack_mxfp8_wide(w1: Sequence[torch.Tensor], w2: Sequence[torch.Tensor]) -> torch.Tensor:
    """pair_heads_pack_mxfp8 for 512 < D <= 1024: the packed buffer of pair_heads_fwd_mxfp8_wide (a pack of its own)."""
    nh, D = len(w1), w1[0].shape[1]
    nbytes = lib().peneo_pair_heads_mxfp8_wide_packed_bytes(nh, D)
    if nbytes == 0:
        raise ValueError(f"wide MXFP8 pair heads: D={D} with {nh} heads is not supported")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w1[0].device)
    classes = (C.c_int * nh)(*[w.shape[0] for w in w2])
    check(lib().peneo_pair_heads_pack_mxfp8_wide(_ptr_list([_c(w) for w in w1]), _ptr_list([_c(w) for w in w2]), classes, nh, D,
                                                 ptr(packed), stream()), "peneo_pair_heads_pack_mxfp8_wide")
    return packed


def pair_heads_fwd_mxfp8_wide(ab: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                              classes: Sequence[int], *, want_logits: bool = True, tags: Optional[Sequence[torch.Tensor]] = None,
                              class_weights: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """pair_heads_fwd_mxfp8 for 512 < D <= 1024: ab [B, N, 2D] bf16, wp from pair_heads_pack_mxfp8_wide.
    Returns (logits list | None, loss partials [n, 32] | None, None) like pair_heads_fwd without dlogits."""
    _c(ab)
    assert ab.dtype == torch.bfloat16, "pair_heads_fwd_mxfp8_wide takes bf16 ab"
    D, nh = ab.shape[2] // 2, len(classes)
    if not pair_mxfp8_wide_supported(D, nh):
        raise ValueError(f"wide MXFP8 pair heads: D={D} with {nh} heads is not supported")
    if wp.dtype != torch.uint8 or wp.numel() != lib().peneo_pair_heads_mxfp8_wide_packed_bytes(nh, D):
        raise ValueError("pair_heads_fwd_mxfp8_wide: wp is not a pair_heads_pack_mxfp8_wide buffer for this shape")
    return _pair_heads_launch("peneo_pair_heads_fwd_mxfp8_wide", "pair_heads_fwd_mxfp8_wide", ab, wp, b1, b2, classes, want_logits,
                              tags, class_weights)


def pair_mxfp8_save_supported(D: int, num_heads: int) -> bool:
    """True when pair_heads_fwd_mxfp8_save exists for this shape: the saved backward and the MXFP8 kernel both hold it (D = 384)."""
    return bool(lib().peneo_pair_mxfp8_save_supported(int(D), int(num_heads)))


def pair_heads_fwd_mxfp8_save(ab: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, b2: torch.Tensor,
                              classes: Sequence[int], *, want_logits: bool = True, tags: Optional[Sequence[torch.Tensor]] = None,
                              class_weights: Optional[Sequence[Optional[torch.Tensor]]] = None, want_dlogits: bool = False,
                              drop_p: float = 0.0, drop_seed: int = 0, save_buffers=None):
    """MXFP8 train forward: pair_heads_fwd(save=True) with the first layer of pair_heads_fwd_mxfp8.  ab [B, N, 2D] bf16, wp from
    pair_heads_pack_mxfp8.  Returns (logits list | None, loss partials [n, 32] | None, dlogits list | None, (act, x_rows)); act and
    x_rows feed pair_bwd_saved, whose gradients are then straight-through on the quantizer (include/peneo_hip.h)."""
    _c(ab)
    assert ab.dtype == torch.bfloat16, "pair_heads_fwd_mxfp8_save takes bf16 ab"
    B, N, D2 = ab.shape
    D = D2 // 2
    nh = len(classes)
    if not pair_mxfp8_save_supported(D, nh):
        raise ValueError(f"MXFP8 train forward of the pair heads: D={D} with {nh} heads is not supported")
    # the C entry point takes a pointer without a size: a bf16 pack (twice the bytes) is caught here
    if wp.dtype != torch.uint8 or wp.numel() != lib().peneo_pair_heads_mxfp8_packed_bytes(nh, D):
        raise ValueError("pair_heads_fwd_mxfp8_save: wp is not a pair_heads_pack_mxfp8 buffer for this shape")
    return _pair_heads_launch("peneo_pair_heads_fwd_mxfp8_save", "pair_heads_fwd_mxfp8_save", ab, wp, b1, b2, classes, want_logits,
                              tags, class_weights, want_dlogits=want_dlogits, drop_p=drop_p, drop_seed=drop_seed,
                              save_bytes=lib().peneo_pair_save_bytes(B, N, nh, D), save_buffers=save_buffers)


def pair_x_fwd(ab_doc: torch.Tensor, i0: int, i1: int, out: torch.Tensor, pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x = SiLU(a_i + b_j) for the pairs of rows i0..i1; `pre` (same shape) optionally receives a_i + b_j."""
    N, D2 = ab_doc.shape
    check(lib().peneo_pair_x_fwd(dtype_code(ab_doc.dtype), ptr(_c(ab_doc)), N, D2 // 2, i0, i1, ptr(out), ptr(pre), stream()),
          "peneo_pair_x_fwd")
    return out


def pair_x_bwd(ab_doc: torch.Tensor, i0: int, i1: int, dx: torch.Tensor, d_ab_doc: torch.Tensor,
               premultiplied: bool = False) -> None:
    N, D2 = ab_doc.shape
    assert d_ab_doc.dtype == torch.float32 and d_ab_doc.shape == ab_doc.shape
    check(lib().peneo_pair_x_bwd(dtype_code(ab_doc.dtype), ptr(_c(ab_doc)), N, D2 // 2, i0, i1, ptr(dx), ptr(_c(d_ab_doc)),
                                 int(premultiplied), stream()), "peneo_pair_x_bwd")


def pair_dz_workspace(nh: int, D: int, device, slots: Optional[int] = None) -> torch.Tensor:
    """Zeroed [slots, 4 * nh * D] fp32 accumulator for pair_dz (sum its rows with colsum at the end).  The stand-alone
    peneo_pair_dz needs the full size (default); the GEMM epilogue and peneo_pair_dz_fused only touch the first 256 rows."""
    full = lib().peneo_pair_dz_workspace_bytes(nh, D) // (16 * nh * D)
    return torch.zeros((full if slots is None else min(slots, full), 4 * nh * D), dtype=torch.float32, device=device)


def pair_dz_fused_workspace_rows(npairs: int) -> int:
    """Rows of ``pair_dz_fused``'s workspace for launches of up to `npairs` pairs under the deterministic mode in force (256 when off)."""
    return int(lib().peneo_pair_dz_fused_workspace_rows(int(npairs)))


def pair_dz_fused_supported(dtype, D: int, num_heads: int) -> bool:
    """``pair_dz_fused`` has a kernel for (dtype, D, heads): bf16 at D / 16 in {2, 4, 6, 8, 12, 16, 24, 32} and at 512 < D <= 1024 with
    D % 64 == 0.  Host only."""
    return bool(lib().peneo_pair_dz_fused_supported(dtype_code(dtype), int(D), int(num_heads)))


def pair_dz_args(D: int, classes: Sequence[int], dlogits: Sequence[torch.Tensor], w2: Sequence[torch.Tensor],
                 scale: torch.Tensor, drop_p: float = 0.0, drop_seed: int = 0, drop_doc: int = 0,
                 drop_pair0: int = 0) -> "hip.PairDzArgs":
    """drop_*: the forward's classifier dropout; drop_doc / drop_pair0 locate a chunk (document, packed index of its first pair)."""
    a = hip.PairDzArgs()
    a.drop_p, a.drop_seed, a.drop_doc, a.drop_pair0 = float(drop_p), int(drop_seed) & 0xFFFFFFFF, int(drop_doc), int(drop_pair0)
    a.num_heads, a.D = len(classes), D
    for h, c in enumerate(classes):
        a.classes[h] = c
        a.dlogits[h], a.w2[h] = ptr(dlogits[h]), ptr(w2[h])
    a.scale = ptr(scale)
    return a


def pair_dz(z: torch.Tensor, npairs: int, D: int, classes: Sequence[int], dlogits: Sequence[torch.Tensor],
            w2: Sequence[torch.Tensor], workspace: torch.Tensor, scale: torch.Tensor,
            args: Optional["hip.PairDzArgs"] = None) -> None:
    a = args if args is not None else pair_dz_args(D, classes, dlogits, w2, scale)
    check(lib().peneo_pair_dz(dtype_code(z.dtype), ptr(z), npairs, C.byref(a), ptr(workspace), stream()), "peneo_pair_dz")


def pair_dz_fused(ab_doc: torch.Tensor, i0: int, i1: int, wp: torch.Tensor, b1: torch.Tensor, args: "hip.PairDzArgs",
                  dz: torch.Tensor, workspace: torch.Tensor, x: Optional[torch.Tensor] = None,
                  pre: Optional[torch.Tensor] = None) -> None:
    """dz [npairs, nh*D] of rows i0..i1 of one document straight from ab (bf16): no x / z round trip through memory.
    `x` / `pre` ([npairs, D], together) optionally receive what pair_x_fwd would write."""
    N, D2 = ab_doc.shape
    if hip.deterministic_mode():     # a row per workgroup of the launch: the C call takes no size, a short workspace would be overrun
        npairs = (i1 * N - i1 * (i1 - 1) // 2) - (i0 * N - i0 * (i0 - 1) // 2)
        need = pair_dz_fused_workspace_rows(npairs) * 4 * args.num_heads * args.D
        if not (workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= need):
            raise hip.PeneoHipError(f"pair_dz_fused: the workspace must hold {need} contiguous fp32 values under the deterministic "
                                    f"mode in force (got {workspace.numel()}); size it with pair_dz_fused_workspace_rows")
    with kernel_timer("pair_dz_fused"):
        check(lib().peneo_pair_dz_fused(dtype_code(ab_doc.dtype), ptr(_c(ab_doc)), N, D2 // 2, i0, i1, ptr(wp), ptr(b1),
                                        C.byref(args), ptr(dz), ptr(workspace), ptr(x), ptr(pre), stream()),
              "peneo_pair_dz_fused")


def pair_bwd_supported(dtype: torch.dtype, D: int, num_heads: int = 0) -> bool:
    """The fused pair-space backward exists for (dtype, D) and its LDS image fits `num_heads` heads (0: do not ask)."""
    return dtype == torch.bfloat16 and bool(lib().peneo_pair_bwd_supported(BF16, D, num_heads))


def pair_bwd_rows(N: int) -> int:
    """Rows per document of the dz / x buffers of ``pair_bwd_fused`` (pairs in 8 x 16 blocks of the triangle)."""
    return int(lib().peneo_pair_bwd_rows(N))


def pair_bwd_workspace_rows(B: int, N: int) -> int:
    """Rows of the dW2 / db1 workspace of ``pair_bwd_fused`` / ``pair_bwd_saved`` under the deterministic mode in force: 256 when
    off, one per workgroup of the launch (B x blocks of the pair triangle) when on."""
    return int(lib().peneo_pair_bwd_workspace_rows(B, N))


def pair_bwd_workspace(B: int, N: int, nh: int, D: int, device) -> torch.Tensor:
    """Zeroed [rows, 4 * nh * D] fp32 workspace of the fused pair backward, sized for the mode in force (pair_dz_finish sums it)."""
    return torch.zeros((pair_bwd_workspace_rows(B, N), 4 * nh * D), dtype=torch.float32, device=device)


def _check_pair_bwd_workspace(workspace: torch.Tensor, B: int, N: int, ncol: int) -> None:
    """(the C call takes no size: with the mode on, a workspace sized for the default would be written out of bounds)"""
    if not hip.deterministic_mode():
        return
    rows = pair_bwd_workspace_rows(B, N)
    if not (workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= rows * 4 * ncol):
        raise hip.PeneoHipError(f"pair backward: the workspace must be contiguous fp32 [>= {rows}, {4 * ncol}] under the deterministic "
                            f"mode in force (got {tuple(workspace.shape)} {workspace.dtype}); size it with pair_bwd_workspace")


def pair_bwd_pack(w1: Sequence[torch.Tensor]) -> torch.Tensor:
    """First-layer weights of all heads ([D, D] fp32 each) -> bf16 fragment stream of ``pair_bwd_fused``."""
    nh, D = len(w1), w1[0].shape[0]
    out = torch.empty(lib().peneo_pair_bwd_packed_bytes(nh, D), dtype=torch.uint8, device=w1[0].device)
    check(lib().peneo_pair_bwd_pack(_ptr_list([_c(w) for w in w1]), nh, D, ptr(out), stream()), "peneo_pair_bwd_pack")
    return out


def pair_bwd_fused(ab: torch.Tensor, wp: torch.Tensor, b1: torch.Tensor, args: "hip.PairDzArgs", dz: torch.Tensor,
                   x: torch.Tensor, d_ab: torch.Tensor, workspace: torch.Tensor) -> None:
    """Whole-batch decoder backward through the pair space (see include/peneo_hip.h): ab [B, N, 2D] bf16 ->
    dz [B * rows, nh*D], x [B * rows, D] (bf16, block order), d_ab [B, N, 2D] fp32 (overwritten), dW2 / db1 sums in `workspace`."""
    B, N, D2 = ab.shape
    assert d_ab.dtype == torch.float32 and d_ab.shape == ab.shape and dz.dtype == x.dtype == torch.bfloat16
    rows = pair_bwd_rows(N)
    assert dz.shape[0] == B * rows and x.shape == (B * rows, D2 // 2)
    _check_pair_bwd_workspace(workspace, B, N, args.num_heads * args.D)
    partials = torch.empty(lib().peneo_pair_bwd_partial_bytes(B, N, D2 // 2) // 4, dtype=torch.float32, device=ab.device)
    with kernel_timer("pair_bwd_fused"):
        check(lib().peneo_pair_bwd_fused(dtype_code(ab.dtype), ptr(_c(ab)), B, N, D2 // 2, ptr(wp), ptr(b1), C.byref(args),
                                         ptr(_c(dz)), ptr(_c(x)), ptr(_c(d_ab)), ptr(workspace), ptr(partials), stream()),
              "peneo_pair_bwd_fused")


def pair_bwd_saved(ab: torch.Tensor, wp: torch.Tensor, args: "hip.PairDzArgs", act: torch.Tensor, dz: torch.Tensor,
                   d_ab: torch.Tensor, workspace: torch.Tensor, act_format: str = "f16") -> None:
    """pair_bwd_fused for a forward that saved its hidden activations (pair_heads_fwd(save=True)): same outputs except x, which
    the forward already wrote.  act_format: the save_format the forward ran with."""
    if act_format not in PAIR_ACT_FORMATS:
        raise ValueError(f"act_format must be one of {PAIR_ACT_FORMATS}, got {act_format!r}")
    entry = "peneo_pair_bwd_saved_e4m3" if act_format == "e4m3" else "peneo_pair_bwd_saved"
    B, N, D2 = ab.shape
    assert d_ab.dtype == torch.float32 and d_ab.shape == ab.shape and dz.dtype == torch.bfloat16
    assert dz.shape[0] == B * pair_bwd_rows(N)
    _check_pair_bwd_workspace(workspace, B, N, args.num_heads * args.D)
    partials = torch.empty(lib().peneo_pair_bwd_partial_bytes(B, N, D2 // 2) // 4, dtype=torch.float32, device=ab.device)
    with kernel_timer("pair_bwd_saved"):
        check(getattr(lib(), entry)(dtype_code(ab.dtype), ptr(_c(ab)), B, N, D2 // 2, ptr(wp), C.byref(args), ptr(act),
                                    ptr(_c(dz)), ptr(_c(d_ab)), ptr(workspace), ptr(partials), stream()), entry)


def pair_dz_finish(workspace: torch.Tensor, nh: int, D: int, classes: Sequence[int]):
    """-> (dw2 list of [C_h, D] fp32, db1 [nh * D] fp32) from the accumulated workspace."""
    vec = colsum(workspace)                     # [4 * nh * D]
    ncol = nh * D
    blk = vec.view(4, ncol)
    dw2 = [blk[:c, h * D:(h + 1) * D] for h, c in enumerate(classes)]
    return dw2, blk[3]


def loss_finish(partials: torch.Tensor, ratio: torch.Tensor, total_classes: int):
    """-> (out [nh + 1] per-head losses then total, scale [2, nh] = (ratio_h / den_h, 1 / den_h), dl_sum [total_classes])."""
    nh = ratio.numel()
    out = torch.empty(nh + 1, dtype=torch.float32, device=partials.device)
    scale = torch.empty((2, nh), dtype=torch.float32, device=partials.device)
    dls = torch.empty(total_classes, dtype=torch.float32, device=partials.device)
    check(lib().peneo_loss_finish(ptr(partials), partials.shape[0], ptr(ratio), nh, total_classes, ptr(out), ptr(scale[0]),
                                  ptr(dls), ptr(scale[1]), stream()), "peneo_loss_finish")
    return out, scale, dls


def ohem_ce(logits: torch.Tensor, tags: torch.Tensor, cw: Optional[torch.Tensor], num_hard_positive: int, num_hard_negative: int,
            dlogits: Optional[torch.Tensor] = None, out8: Optional[torch.Tensor] = None, dl_sum: Optional[torch.Tensor] = None,
            workspace: Optional[torch.Tensor] = None):
    """OHEM cross entropy of one head over its flattened pairs (reference custom_loss.py:204-288, as executed).
    -> out8 = [loss, kept sum, k_pos + k_neg, n_pos, n_neg, k_pos, k_neg, 0] (device); `dlogits` is masked in place."""
    _c(logits)
    C_ = logits.shape[-1]
    n = logits.numel() // C_
    assert logits.dtype == torch.float32 and tags.dtype == torch.int64 and tags.numel() == n
    need = lib().peneo_ohem_workspace_bytes(n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=logits.device)
    if out8 is None:
        out8 = torch.empty(8, dtype=torch.float32, device=logits.device)
    if dlogits is not None:
        assert dlogits.dtype == torch.float32 and dlogits.numel() == logits.numel()
        _c(dlogits)
    check(lib().peneo_ohem_ce(ptr(logits), ptr(_c(tags)), ptr(cw), n, C_, int(num_hard_positive), int(num_hard_negative),
                              ptr(dlogits), ptr(out8), ptr(dl_sum), ptr(workspace), workspace.numel(), stream()), "peneo_ohem_ce")
    return out8, workspace


def ohem_finish(out8: torch.Tensor, ratio: torch.Tensor):
    """[nh, 8] per-head OHEM results -> (out [nh + 1], scale [2, nh]) like ``loss_finish``."""
    nh = ratio.numel()
    out = torch.empty(nh + 1, dtype=torch.float32, device=out8.device)
    scale = torch.empty((2, nh), dtype=torch.float32, device=out8.device)
    check(lib().peneo_ohem_finish(ptr(_c(out8)), ptr(ratio), nh, ptr(out), ptr(scale[0]), ptr(scale[1]), stream()),
          "peneo_ohem_finish")
    return out, scale


def weighted_ce(logits: torch.Tensor, tags: torch.Tensor, cw: Optional[torch.Tensor], want_dlogits: bool = False):
    _c(logits)
    C_ = logits.shape[-1]
    rows = logits.numel() // C_
    num = torch.zeros(1, dtype=torch.float32, device=logits.device)
    den = torch.zeros(1, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_dlogits else None
    check(lib().peneo_weighted_ce(ptr(logits), ptr(_c(tags)), ptr(cw), rows, C_, ptr(num), ptr(den), ptr(dl), stream()),
          "peneo_weighted_ce")
    return num, den, dl


def spots_compact(logits: torch.Tensor, N: int, max_spots: int = 4096):
    """[P, C] fp32 logits -> (spots int32 [n, 3] (i, j, tag), scores fp32 [n]) in increasing p order."""
    _c(logits)
    P, C_ = logits.shape
    spots = torch.empty((max_spots, 3), dtype=torch.int32, device=logits.device)
    scores = torch.empty(max_spots, dtype=torch.float32, device=logits.device)
    count = torch.zeros(1, dtype=torch.int32, device=logits.device)
    check(lib().peneo_spots_compact(ptr(logits), P, C_, N, ptr(spots), ptr(scores), ptr(count), max_spots, stream()),
          "peneo_spots_compact")
    n = int(count.item())
    if n > max_spots:
        return spots_compact(logits, N, max_spots=n)
    return spots[:n], scores[:n]


def spots_batch_workspace_bytes(num_maps: int, B: int, N: int) -> int:
    return int(lib().peneo_spots_compact_batch_workspace_bytes(num_maps, B, N))


def spots_compact_batch_launch(maps, N: int, max_spots: int, records: Optional[torch.Tensor] = None,
                               counts: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """The two launches of ``peneo_spots_compact_batch`` on the current stream, no host synchronisation.  ``maps``: fp32
    logits [B, P, C] (C >= 2) and / or int64 label maps [B, P], all of one B and P = N (N + 1) / 2, contiguous.  Returns the
    device tensors (records int32 [M, B, max_spots, 4] = (i, j, tag, score bits), counts int32 [M, B])."""
    M = len(maps)
    if not 1 <= M <= hip.MAX_HEADS:
        raise hip.PeneoHipError(f"spots_compact_batch: {M} maps (1 .. {hip.MAX_HEADS} per call)")
    B, P = maps[0].shape[0], maps[0].shape[1]
    dev = maps[0].device
    desc = hip.SpotsBatchDesc()
    desc.num_maps = M
    for m, t in enumerate(maps):
        label = t.dtype == torch.int64 and t.dim() == 2
        if not (label or (t.dtype == torch.float32 and t.dim() == 3)) or tuple(t.shape[:2]) != (B, P) or t.device != dev:
            raise hip.PeneoHipError(f"spots_compact_batch: map {m} is {t.dtype} {tuple(t.shape)}; want fp32 [{B}, {P}, C] or int64 [{B}, {P}]")
        if P != N * (N + 1) // 2:
            raise hip.PeneoHipError(f"spots_compact_batch: P = {P} is not N (N + 1) / 2 for N = {N}")
        desc.classes[m] = 0 if label else t.shape[2]
        desc.maps[m] = ptr(_c(t))
    max_spots = int(max_spots)
    if records is None:   # (an empty tensor has no storage: max_spots == 0 counts only and hands the library a NULL records)
        records = torch.empty((M, B, max_spots, 4), dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty((M, B), dtype=torch.int32, device=dev)
    need = spots_batch_workspace_bytes(M, B, N)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if records.dtype != torch.int32 or records.numel() < M * B * max_spots * 4 or counts.dtype != torch.int32 or \
            counts.numel() < M * B or records.device != dev or counts.device != dev or workspace.device != dev:
        raise hip.PeneoHipError(f"spots_compact_batch: records / counts must be int32 tensors on {dev} holding "
                                f"{M * B * max_spots} records and {M * B} counts")
    check(lib().peneo_spots_compact_batch(C.byref(desc), B, N, ptr(_c(records)) if max_spots else None, ptr(_c(counts)), max_spots,
                                          ptr(_c(workspace)), workspace.numel() * workspace.element_size(), stream()),
          "peneo_spots_compact_batch")
    return records, counts


def spots_compact_batch(maps, N: int, max_spots: int = 4096):
    """Every map of a batch in one call (``spots_compact_batch_launch``) and two device-to-host copies, whatever B and the
    number of maps: the counts, then the stored records alone, packed on the device.  Returns HOST tensors (records int32
    [total, 4] = (i, j, tag, score bits; view as float32), counts int32 [M, B]): the spots of document b of map m are the
    ``counts[m, b]`` rows behind those of the (map, document)s before it, in increasing p order.  A count above ``max_spots``
    repeats the launches once with the largest count."""
    max_spots = max(int(max_spots), 1)
    records, counts = spots_compact_batch_launch(maps, N, max_spots)
    counts_h = counts.cpu()
    k, total = int(counts_h.max()), int(counts_h.sum())
    if k > max_spots:
        max_spots = k
        records, _ = spots_compact_batch_launch(maps, N, max_spots)
    # packed row r belongs to the (map, document) d whose running total first exceeds r, at slot r - (the total before d)
    c = counts.view(-1).long()
    end = c.cumsum(0)
    r = torch.arange(total, device=records.device)
    d = torch.searchsorted(end, r, right=True)
    return records.view(-1, 4).index_select(0, d * max_spots + r - (end - c)[d]).cpu(), counts_h


def spots_to_tags(batch_spots, N: int, device, B: int = None) -> torch.Tensor:
    """Sparse spots -> dense label maps [B, P] int64 built on the device (K13 input side).  ``batch_spots``: a list with
    one [(i, j, tag), ...] list per document, or an int32 tensor [n, 4] of (b, i, j, tag) rows (then ``B`` is required;
    what ``DataCollatorForPEneo(sparse_tags=True)`` ships)."""
    if torch.is_tensor(batch_spots):
        assert B is not None and batch_spots.dim() == 2 and batch_spots.shape[1] == 4
        n = batch_spots.shape[0]
        sp = batch_spots.to(device=device, dtype=torch.int32).contiguous() if n else None
    else:
        B = len(batch_spots)
        flat = [(b, int(sp[0]), int(sp[1]), int(sp[2])) for b, spots in enumerate(batch_spots) for sp in spots]
        n = len(flat)
        sp = torch.tensor(flat, dtype=torch.int32).view(-1, 4).to(device) if flat else None
    tags = torch.empty((B, N * (N + 1) // 2), dtype=torch.int64, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    check(lib().peneo_spots_to_tags(ptr(sp), n, B, N, ptr(tags), ptr(status), stream()), "peneo_spots_to_tags")
    if n and int(status) != 0:
        raise IndexError("spot outside the [0, N) x [0, N) pair matrix")
    return tags
