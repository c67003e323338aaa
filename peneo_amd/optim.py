"""Optimizer step of the training loop: fused multi-tensor AdamW on the C ABI
(``peneo_adamw_step``; ``peneo_adamw_step_emit`` when the step also writes the weights' working copies) and the reference's
four parameter groups.

Reference: ``PEneoTrainer.create_optimizer`` (pipeline/trainer.py:275-330) — parameters whose name contains
``"peneo_decoder"`` train at ``lr * peneo_downstream_speedup_ratio``; biases and LayerNorm weights get no weight
decay (HF ``Trainer.get_decay_parameter_names``); optimizer = AdamW.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List

import torch
import torch.nn as nn

from . import hip, ops
from .hip import check, lib, ptr, stream
from .model.engine import WeightCache, bump_param_epoch


def decay_parameter_names(model: nn.Module) -> List[str]:
    """Names that receive weight decay: everything except LayerNorm parameters and biases (the HF Trainer rule)."""
    no_decay = set()
    for mod_name, mod in model.named_modules():
        if isinstance(mod, nn.LayerNorm):
            for pn, _ in mod.named_parameters(recurse=False):
                no_decay.add(f"{mod_name}.{pn}" if mod_name else pn)
    return [n for n, _ in model.named_parameters() if n not in no_decay and "bias" not in n]


def peneo_param_groups(model: nn.Module, lr: float, weight_decay: float, speedup_ratio: float) -> List[Dict]:
    """The four groups of pipeline/trainer.py:286-322, in the reference's order."""
    decay = set(decay_parameter_names(model))
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    sel = lambda d, s: [p for n, p in named if (n in decay) == d and ("peneo_decoder" in n) == s]
    return [
        {"params": sel(True, True), "weight_decay": weight_decay, "lr": lr * speedup_ratio},
        {"params": sel(False, True), "weight_decay": 0.0, "lr": lr * speedup_ratio},
        {"params": sel(True, False), "weight_decay": weight_decay, "lr": lr},
        {"params": sel(False, False), "weight_decay": 0.0, "lr": lr},
    ]


class FusedAdamW(torch.optim.Optimizer):
    """AdamW over all groups in one kernel launch per step (fp32 master parameters, contiguous fp32 gradients).
    Learning rates may be changed between steps through ``param_groups`` (schedulers work unchanged).

    State layout is torch.optim.AdamW's (``state[p] = {"step", "exp_avg", "exp_avg_sq"}``), so ``state_dict()`` /
    ``load_state_dict()`` round-trip and a reference ``optimizer.pt`` resumes with its own step counts: the kernel takes
    one global step plus a per-tensor offset (0 unless a checkpoint holds differing counts or a parameter joined late).
    ``state[p]["step"]`` is written back lazily (in ``state_dict()`` and before the device tables are rebuilt), not by
    241 host tensor updates per step.

    ``max_grad_norm`` (None = off): global gradient-norm clipping inside the step, i.e. what HF ``Trainer`` does between
    backward and ``optimizer.step()`` at its default ``max_grad_norm = 1.0`` (the reference trains through it,
    start/run_rfund.py:307-321): ``torch.nn.utils.clip_grad_norm_`` is ~1000 small torch launches over 241 tensors; here
    one more launch sums the squares of all gradients into a device scalar and the AdamW kernel applies
    ``min(1, max_grad_norm / (norm + 1e-6))`` while it reads the gradients (``.grad`` itself is left as it is; a Trainer
    driving this optimizer sets its own ``max_grad_norm`` to 0).  ``last_grad_norm()`` returns the un-clipped norm of the
    last step as a device tensor (no host sync unless the caller reads it).

    ``emit_into`` (a module, None = off): the step also writes the working-precision copies of the weights.  Every
    ``WeightCache`` under that module lists its declarative entries (casts, row stacks of casts, concatenated bias vectors);
    for each entry ALL of whose sources are updated by this step, the kernel stores the new value into the entry's buffer while
    it is in a register (``peneo_adamw_step_emit``) and the entry is stamped current, so the next forward finds it instead of
    re-casting 85 M parameters in a second pass.  Entries come into being lazily as before (the first forward builds them,
    emission starts with the first step after that); an entry with a frozen or gradient-less source, the packed / quantised
    forms and ``dec.ab`` stay lazy; a buffer that a lazy rebuild re-allocated (after a foreign ``.data`` write, a
    ``load_state_dict``, a change of compute dtype) is picked up by the next step.  In-place rule: the working copies are
    OVERWRITTEN by ``step()``, they are not fresh tensors -- a backward must not run after a ``step()`` that followed its
    forward (it would multiply by the new weights)."""

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: float = None, emit_into: nn.Module = None):
        if emit_into is not None and not isinstance(emit_into, nn.Module):
            raise TypeError(f"emit_into must be a torch.nn.Module (the model whose weight caches are written), not {type(emit_into).__name__}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be positive (None switches clipping off)")
        self.max_grad_norm = max_grad_norm
        self._emit_into = emit_into
        self._emit, self._emit_plan, self._emitted = None, None, ()
        self._sqnorm = None
        self._sq_ws = None
        self._tables = None
        self._step = 0
        self._entries = []
        self._offsets = []

    # ---- step bookkeeping -------------------------------------------------------------------------------------------
    def _flush_steps(self) -> None:
        """Write the step counts of the tracked tensors into ``self.state`` (torch's format: a CPU float tensor)."""
        for (p, st, _), off in zip(self._entries, self._offsets):
            st["step"] = torch.tensor(float(self._step + off))

    def state_dict(self):
        self._flush_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        # self.state was replaced: the cached per-parameter dicts and the device table (moment pointers) are stale
        self._tables, self._entries, self._offsets, self._step = None, [], [], 0

    def __setstate__(self, state) -> None:
        super().__setstate__(state)
        self._tables, self._entries, self._offsets = None, [], []
        self._step = getattr(self, "_step", 0)
        self._emit_into = getattr(self, "_emit_into", None)
        self._emit, self._emit_plan, self._emitted = None, None, ()

    def _wanted(self):
        return [(p, gi) for gi, group in enumerate(self.param_groups) for p in group["params"] if p.grad is not None]

    def _build(self):
        self._flush_steps()                          # a rebuild (new parameters with gradients) keeps everyone's count
        chunk = lib().peneo_adamw_chunk_elems()
        entries, chunk_t, chunk_i, steps = [], [], [], []
        for p, gi in self._wanted():
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise hip.PeneoHipError("FusedAdamW needs contiguous fp32 parameters on the GPU")
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            for k in ("exp_avg", "exp_avg_sq"):      # e.g. moments loaded from a checkpoint in another dtype / layout
                if st[k].dtype != torch.float32 or not st[k].is_contiguous() or st[k].device != p.device:
                    st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
            steps.append(int(float(st.get("step", 0))))
            t = len(entries)
            entries.append((p, st, gi))
            for c in range((p.numel() + chunk - 1) // chunk):
                chunk_t.append(t)
                chunk_i.append(c)
        if not entries:
            raise hip.PeneoHipError("FusedAdamW.step(): no parameter has a gradient")
        dev = entries[0][0].device
        # global step = the most common count (all equal in practice), the others ride on per-tensor offsets
        self._step = max(set(steps), key=steps.count)
        self._offsets = [s - self._step for s in steps]
        self._entries = entries
        self._chunk_t = torch.tensor(chunk_t, dtype=torch.int32, device=dev)
        self._chunk_i = torch.tensor(chunk_i, dtype=torch.int32, device=dev)
        self._host = (hip.AdamwTensor * len(entries))()
        self._table = torch.empty(C.sizeof(self._host), dtype=torch.uint8, device=dev)
        self._grads = [None] * len(entries)
        self._emit = ops.AdamwEmitTable([e[0] for e in entries]) if self._emit_into is not None else None
        self._emit_plan = None
        self._tables = True

    def _refresh(self):
        dirty = False
        for k, (p, st, gi) in enumerate(self._entries):
            g = p.grad
            if g is None or not g.is_contiguous() or g.dtype != torch.float32:
                raise hip.PeneoHipError("FusedAdamW: every tracked parameter needs a contiguous fp32 .grad each step")
            group = self.param_groups[gi]
            e = self._host[k]
            vals = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                    float(group["lr"]), float(group["weight_decay"]), self._offsets[k])
            if self._grads[k] != vals:
                e.param, e.grad, e.exp_avg, e.exp_avg_sq = vals[:4]
                e.numel, e.lr, e.weight_decay, e.step_offset = p.numel(), vals[4], vals[5], vals[6]
                self._grads[k] = vals
                dirty = True
        if dirty:   # pointer / lr table changed (new .grad tensors, scheduler step): one small H2D copy
            src = torch.frombuffer(memoryview(self._host).cast("B"), dtype=torch.uint8)
            self._table.copy_(src, non_blocking=False)
            if self._emit is not None and self._emit.reindex():
                self._emit_plan = None

    def emitted_keys(self):
        """[(weight cache, key)] of the entries the last step wrote (empty without ``emit_into``)."""
        return list(self._emitted)

    def _collect_emissions(self):
        """The declarative cache entries under the model whose sources are ALL tensors of this step -> the emission table
        (same dirty check and single H2D copy as the tensor table); returns [(cache, key)] to stamp after the launch."""
        plan = self._emit_plan
        if plan is not None and all(wc.gen == gen and wc._touched == touched for wc, gen, touched in plan[0]):
            return plan[1]       # the steady state of a training loop: same entries, same buffers, same parameters as last step
        index, pairs, emitted, caches = self._emit.index, [], [], []
        for mod in self._emit_into.modules():
            wc = getattr(mod, "weight_cache", None)
            if not isinstance(wc, WeightCache) or any(wc is c[0] for c in caches):
                continue
            caches.append((wc, wc.gen, set(wc._touched)))
            for key, srcs, views in wc.declarative():
                if all((p.data_ptr(), p.numel()) in index for p in srcs):
                    pairs += zip(srcs, views)
                    emitted.append((wc, key))
        self._emit.update(pairs)
        self._emit_plan = (caches, emitted)
        return emitted

    def last_grad_norm(self):
        """Global L2 norm of the gradients the last step saw (before clipping); None without max_grad_norm."""
        return None if self._sqnorm is None else self._sqnorm.sum().sqrt().to(torch.float32).reshape(1)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._tables is not None:                 # the set of parameters with gradients changed: rebuild the tables
            want = self._wanted()
            if len(want) != len(self._entries) or any(a is not b[0] for (a, _), b in zip(want, self._entries)):
                self._tables = None
        if self._tables is None:
            self._build()
        self._refresh()
        self._step += 1
        g0 = self.param_groups[0]
        sq = None
        if self.max_grad_norm is not None:
            if self._sqnorm is None or self._sqnorm.device != self._table.device:
                self._sqnorm = torch.zeros(int(lib().peneo_grad_sqnorm_slots()), dtype=torch.float64, device=self._table.device)
            sq = self._sqnorm
            # deterministic mode: the chunks' sums go to a workspace and are added in chunk order (0 bytes and the plain call when off)
            need = int(lib().peneo_grad_sqnorm_workspace_bytes(self._chunk_t.numel()))
            ws = None
            if need:
                if self._sq_ws is None or self._sq_ws.numel() * 8 < need or self._sq_ws.device != self._table.device:
                    self._sq_ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self._table.device)
                ws = self._sq_ws
            check(lib().peneo_grad_sqnorm_ws(ptr(self._table), ptr(self._chunk_t), ptr(self._chunk_i), self._chunk_t.numel(),
                                             ptr(sq), ptr(ws), need, stream()), "peneo_grad_sqnorm_ws")
        if self._emit is None:
            check(lib().peneo_adamw_step_clip(ptr(self._table), ptr(self._chunk_t), ptr(self._chunk_i), self._chunk_t.numel(),
                                              float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), self._step,
                                              ptr(sq), float(self.max_grad_norm or 0.0), stream()), "peneo_adamw_step_clip")
            bump_param_epoch()   # the parameters changed in place behind torch's version counters: invalidate the working copies
            return loss
        emitted = self._collect_emissions()
        ops.adamw_step_emit(self._table, self._chunk_t, self._chunk_i, float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]),
                            self._step, self._emit, sqnorm=sq, max_grad_norm=float(self.max_grad_norm or 0.0))
        bump_param_epoch()   # every working copy is stale now ...
        for wc, key in emitted:                      # ... except those this launch has just written
            wc.mark_current(key)
        self._emitted = emitted
        return loss
