"""Fused multi-tensor optimizers: Adam, SGD+momentum, LAMB.

Reference workload parity: Adam (CNN), SGD+momentum+wd (ResNet/Inception),
LAMB (BERT, torch_optimizer.Lamb) — SURVEY.md section 2.3 optimizer row.
GPU path: ONE kernel launch per step applies the update across every
parameter chunk (csrc/optim.hip, apex-style chunked multi-tensor apply);
LAMB adds a norm-reduction phase for the per-tensor trust ratio. CPU
path: plain torch math (used by the CPU pipeline tests).

Global-norm gradient clipping (``max_grad_norm``): a multi-tensor
squared-norm reduction writes a device scalar coefficient that the update
kernels multiply into every gradient AS THEY LOAD IT — one extra read of
the gradients and no write, no host synchronisation, capturable in a
hipGraph. The gradients in memory keep their unclipped values.
"""
from __future__ import annotations

import math

import torch
from torch.optim import Optimizer

from ._ext import get_ext


def _on_gpu(params):
    return any(p.is_cuda for p in params)


def _cpu_clip_stats(grads, max_norm, stats):
    """torch.nn.utils.clip_grad_norm_'s formula (L2) on the CPU path:
    fills stats = [norm, coefficient, non-finite count] and returns the
    coefficient as a python float."""
    if grads:
        norm = torch.linalg.vector_norm(torch.stack(
            [torch.linalg.vector_norm(g.detach().float()) for g in grads]))
    else:
        norm = torch.zeros(())
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    stats[0] = norm
    stats[1] = coef
    if not math.isfinite(float(norm)):
        stats[2] += 1
    return float(coef)


def _norm_pass(ext, tables, partials, stats, max_norm, max_norm_buf=None):
    """The GPU norm pass: per-chunk squared norms of every table into
    ``partials`` at running offsets, then one finalize launch fills
    stats = [norm, coefficient, non-finite count]. ``max_norm_buf`` (a
    device scalar) overrides the host ``max_norm`` when given."""
    off = 0
    for table, nchunks, esize in tables:
        ext.grad_sqnorm(table, nchunks, esize, partials, off)
        off += nchunks
    ext.grad_norm_finalize(partials, off, stats, max_norm, max_norm_buf)


class _FusedOptimizer(Optimizer):
    """The step shared by the fused optimizers: collect every group's
    lists, upload ONE chunk table per GPU group, then run the update
    kernel(s) from it — with ``max_grad_norm`` set, after a norm pass over
    all tables whose coefficient the update reads from ``stats``.

    A subclass supplies
      _collect(group) -> lists (params first, grads second) of the params
                         that have a grad, creating their state,
      _table_lists(lists) -> the five lists of ``mt_build_table``,
      _table_fn, the name of its ``fused_*_table`` entry point,
      _update_args(group, lists) -> that call's arguments between the
                         table triple and ``stats``, and
      _cpu_update(group, lists, coef).

    ``max_grad_norm`` is a plain attribute (NOT a param-group default): it
    stays out of ``state_dict`` so old checkpoints load unchanged and the
    owner (Node / ComputeEngine) re-supplies it on resume. The norm spans
    every param group of the optimizer.
    """

    _clip_stats = None      # [norm, coefficient, non-finite count] fp32
    _clip_partials = None   # per-chunk partial sums (GPU path)

    def __init__(self, params, defaults, max_grad_norm=None):
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm

    def _stats_on(self, device):
        st = self._clip_stats
        if st is None or st.device != torch.device(device):
            old = st
            st = torch.zeros(3, dtype=torch.float32, device=device)
            if old is not None:
                st[2] = float(old[2])
            self._clip_stats = st
        return st

    def _partials_on(self, device, n):
        buf = self._clip_partials
        if buf is None or buf.device != torch.device(device) \
                or buf.numel() < n:
            buf = torch.empty(max(n, 1), dtype=torch.float32, device=device)
            self._clip_partials = buf
        return buf

    def grad_norm_stats(self):
        """Device tensor [norm before clipping, clip coefficient, count of
        non-finite-norm steps] of the most recent clipped step (None before
        the first one). Returned without any synchronisation."""
        return self._clip_stats

    def _masters(self, ps):
        return ([self.state[p]["master"] for p in ps]
                if ps and ps[0].dtype == torch.bfloat16 else [])

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        work = []
        for group in self.param_groups:
            lists = self._collect(group)
            if lists[0]:
                work.append((group, lists))
        if not work:
            return loss
        clip = self.max_grad_norm is not None
        if clip:
            # one norm over all groups: GPU or CPU is decided once
            grads = [g for _, lists in work for g in lists[1]]
            gpu_work, cpu_work = (work, []) if _on_gpu(grads) else ([], work)
        else:
            # independent groups, which may sit on different devices
            gpu_work = [w for w in work if _on_gpu(w[1][0])]
            cpu_work = [w for w in work if not _on_gpu(w[1][0])]
        if gpu_work:
            ext = get_ext(required=True)
            update = getattr(ext, self._table_fn)
            # arguments first: nothing but the launch then stands between
            # a table's blocking upload and the kernel that reads it
            args = [self._update_args(group, lists)
                    for group, lists in gpu_work]
            # one table per group, shared by the norm and update kernels
            tables = [ext.mt_build_table(*self._table_lists(lists))
                      for _, lists in gpu_work]
            stats = None
            if clip:
                device = gpu_work[0][1][0][0].device
                stats = self._stats_on(device)
                partials = self._partials_on(device,
                                             sum(t[1] for t in tables))
                _norm_pass(ext, tables, partials, stats,
                           float(self.max_grad_norm))
            for table, a in zip(tables, args):
                update(*table, *a, stats)
        if cpu_work:
            coef = None
            if clip:
                coef = _cpu_clip_stats(grads, float(self.max_grad_norm),
                                       self._stats_on("cpu"))
            for group, lists in cpu_work:
                self._cpu_update(group, lists, coef)
        return loss


class _MomentsOptimizer(_FusedOptimizer):
    """State shared by Adam and LAMB: a step count, two fp32 moments and,
    for bf16 params on the GPU, an fp32 master copy."""

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            st["m"] = torch.zeros_like(p, dtype=torch.float32)
            st["v"] = torch.zeros_like(p, dtype=torch.float32)
            if p.dtype == torch.bfloat16 and p.is_cuda:
                st["master"] = p.detach().float().clone()
        return st

    def _collect(self, group):
        ps, gs, ms, vs = [], [], [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            st = self._init_state(p)
            st["step"] += 1
            ps.append(p)
            gs.append(p.grad)
            ms.append(st["m"])
            vs.append(st["v"])
        return ps, gs, ms, vs

    def _bias_corrections(self, group, ps):
        b1, b2 = group["betas"]
        step = self.state[ps[0]]["step"]
        return 1 - b1 ** step, 1 - b2 ** step

    def _table_lists(self, lists):
        return (*lists, self._masters(lists[0]))


class FusedAdam(_MomentsOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, max_grad_norm=None):
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults, max_grad_norm)
        self._graph = None  # hipGraph-capture buffers (see graph_step)

    # ---- hipGraph capture support (engine/graphstep.py) --------------
    # lr and the bias-correction step live in DEVICE buffers so graph
    # replays see live values; the chunk table is built once at capture
    # (param/grad/state pointers are stable across replays).
    def enable_graph_capture(self, device) -> bool:
        if len(self.param_groups) != 1:
            return False
        self._ensure_state()
        start = 0
        for st in self.state.values():
            if "step" in st:
                start = max(start, st["step"])
        self._graph = {
            "lr": torch.zeros(1, dtype=torch.float32, device=device),
            "step": torch.full((1,), start, dtype=torch.int64,
                               device=device),
            "table": None,
            # clipping is recorded into the capture only when it is on at
            # capture time; max_norm then lives in a device scalar that
            # sync_lr refreshes, like lr
            "clip": self.max_grad_norm is not None,
            "max_norm": torch.zeros(1, dtype=torch.float32, device=device),
        }
        if self._graph["clip"]:
            self._stats_on(device)
        self.sync_lr()
        return True

    def _ensure_state(self):
        for group in self.param_groups:
            for p in group["params"]:
                self._init_state(p)

    def sync_lr(self):
        """Host -> device lr (and max_grad_norm) refresh; call OUTSIDE the
        graph, before each replay (lets lr schedules work under capture).
        ``max_grad_norm = None`` after a clipping capture uploads +inf:
        the recorded kernels then compute a coefficient of exactly 1."""
        self._graph["lr"].fill_(float(self.param_groups[0]["lr"]))
        if self._graph["clip"]:
            mn = self.max_grad_norm
            self._graph["max_norm"].fill_(
                float("inf") if mn is None else float(mn))

    def bump_host_steps(self):
        """Mirror the device step counter into the python state (kept
        consistent for checkpoints); call once per replayed step."""
        for st in self.state.values():
            if "step" in st:
                st["step"] += 1

    @torch.no_grad()
    def build_graph_table(self):
        """Allocate stable grad buffers and prebuild the device chunk
        table. Must run OUTSIDE capture (the table upload is a blocking
        H2D copy); the captured step then zeroes these buffers, lets
        backward ACCUMULATE into them, and applies the one-kernel update.
        Returns the stable grad list (for the capture's zero pass)."""
        ext = get_ext(required=True)
        group = self.param_groups[0]
        grads = []
        ps = []
        for p in group["params"]:
            if not p.requires_grad:
                continue
            p.grad = torch.zeros_like(p)
            ps.append(p)
            grads.append(p.grad)
        ms = [self.state[p]["m"] for p in ps]
        vs = [self.state[p]["v"] for p in ps]
        self._graph["table"] = ext.mt_build_table(ps, grads, ms, vs,
                                                  self._masters(ps))
        self._graph["grads"] = grads
        if self._graph["clip"]:
            # preallocated outside the capture: replays reuse the buffer
            self._graph["partials"] = torch.empty(
                self._graph["table"][1], dtype=torch.float32,
                device=ps[0].device)
        return grads

    @torch.no_grad()
    def graph_step(self):
        """The capturable step body: device step bump + ONE kernel (with
        clipping: sqnorm -> finalize -> update, a serial chain).
        Must run inside the captured region, after backward."""
        ext = get_ext(required=True)
        g = self._graph
        g["step"].add_(1)
        group = self.param_groups[0]
        b1, b2 = group["betas"]
        stats = None
        if g["clip"]:
            stats = self._clip_stats
            _norm_pass(ext, [g["table"]], g["partials"], stats, 0.0,
                       g["max_norm"])
        ext.fused_adam_graph(*g["table"], g["lr"], b1, b2, group["eps"],
                             group["weight_decay"], g["step"], stats)

    _table_fn = "fused_adam_table"

    def _update_args(self, group, lists):
        b1, b2 = group["betas"]
        return (group["lr"], b1, b2, group["eps"], group["weight_decay"],
                *self._bias_corrections(group, lists[0]))

    def _cpu_update(self, group, lists, coef):
        b1, b2 = group["betas"]
        bc1, bc2 = self._bias_corrections(group, lists[0])
        for p, g, m, v in zip(*lists):
            gf = g.float()
            if coef is not None:
                gf = gf * coef
            if group["weight_decay"]:
                gf = gf.add(p.float(), alpha=group["weight_decay"])
            m.mul_(b1).add_(gf, alpha=1 - b1)
            v.mul_(b2).addcmul_(gf, gf, value=1 - b2)
            denom = (v / bc2).sqrt_().add_(group["eps"])
            p.add_(((m / bc1) / denom).to(p.dtype),
                   alpha=-group["lr"])


class FusedSGD(_FusedOptimizer):
    def __init__(self, params, lr=1e-2, momentum=0.0, weight_decay=0.0,
                 nesterov=False, max_grad_norm=None):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                        nesterov=nesterov)
        super().__init__(params, defaults, max_grad_norm)

    def _collect(self, group):
        ps, gs, bufs = [], [], []
        mom = group["momentum"]
        for p in group["params"]:
            if p.grad is None:
                continue
            st = self.state[p]
            if mom and "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(
                    p, dtype=torch.float32)
            if p.dtype == torch.bfloat16 and p.is_cuda and \
                    "master" not in st:
                st["master"] = p.detach().float().clone()
            ps.append(p)
            gs.append(p.grad)
            bufs.append(st["momentum_buffer"] if mom
                        else torch.zeros(0))
        return ps, gs, bufs

    def _table_lists(self, lists):
        ps, gs, bufs = lists
        return ps, gs, bufs, [], self._masters(ps)

    _table_fn = "fused_sgd_table"

    def _update_args(self, group, lists):
        return (group["lr"], group["momentum"], group["weight_decay"],
                bool(group["nesterov"]))

    def _cpu_update(self, group, lists, coef):
        mom = group["momentum"]
        for p, g, b in zip(*lists):
            gf = g.float()
            if coef is not None:
                gf = gf * coef
            if group["weight_decay"]:
                gf = gf.add(p.float(), alpha=group["weight_decay"])
            if mom:
                b.mul_(mom).add_(gf)
                gf = gf.add(b, alpha=mom) if group["nesterov"] else b
            p.add_(gf.to(p.dtype), alpha=-group["lr"])


class FusedLAMB(_MomentsOptimizer):
    """LAMB (You et al.) with the per-tensor trust ratio
    clamp(|w| / |update|). Parity: torch_optimizer.Lamb used by the BERT
    example (examples/bert/provider.py:49-50)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                 weight_decay=0.0, clamp_trust=10.0, max_grad_norm=None):
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay, clamp_trust=clamp_trust)
        super().__init__(params, defaults, max_grad_norm)

    _table_fn = "fused_lamb_table"

    def _update_args(self, group, lists):
        b1, b2 = group["betas"]
        return (len(lists[0]), group["lr"], b1, b2, group["eps"],
                group["weight_decay"],
                *self._bias_corrections(group, lists[0]),
                group["clamp_trust"])

    def _cpu_update(self, group, lists, coef):
        b1, b2 = group["betas"]
        bc1, bc2 = self._bias_corrections(group, lists[0])
        for p, g, m, v in zip(*lists):
            gf = g.float()
            if coef is not None:
                gf = gf * coef
            m.mul_(b1).add_(gf, alpha=1 - b1)
            v.mul_(b2).addcmul_(gf, gf, value=1 - b2)
            upd = (m / bc1) / ((v / bc2).sqrt() + group["eps"])
            if group["weight_decay"]:
                upd = upd.add(p.float(), alpha=group["weight_decay"])
            wn = p.float().norm()
            un = upd.norm()
            trust = torch.where(
                (wn > 0) & (un > 0),
                (wn / un).clamp(max=group["clamp_trust"]),
                torch.ones_like(wn))
            p.add_((trust * upd).to(p.dtype), alpha=-group["lr"])


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm) -> torch.Tensor:
    """Drop-in for ``torch.nn.utils.clip_grad_norm_`` (L2 norm), for use
    with any optimizer. Scales the gradients in place by
    ``min(1, max_norm / (norm + 1e-6))`` and returns the 0-dim total norm
    (a device tensor on GPU: no synchronisation). Params without a grad
    are skipped; with no grads at all the result is 0.

    GPU: grads are grouped by dtype (bf16 and fp32 may be mixed); one
    squared-norm launch per dtype fills one partials buffer, one finalize
    launch produces the coefficient, one scale launch per dtype applies
    it. A non-finite norm behaves as torch with error_if_nonfinite=False.
    """
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    if not _on_gpu(grads):
        return torch.nn.utils.clip_grad_norm_(
            [p for p in parameters if p.grad is not None], max_norm)
    ext = get_ext(required=True)
    by_dtype: dict = {}
    for g in grads:
        if g.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(
                f"clip_grad_norm_: unsupported grad dtype {g.dtype} "
                "(bf16 and fp32 only)")
        by_dtype.setdefault(g.dtype, []).append(g)
    device = grads[0].device
    tables = [t for t in (ext.grad_build_table(gs)
                          for gs in by_dtype.values()) if t[1] > 0]
    total = sum(t[1] for t in tables)
    stats = torch.zeros(3, dtype=torch.float32, device=device)
    partials = torch.empty(max(total, 1), dtype=torch.float32, device=device)
    _norm_pass(ext, tables, partials, stats, float(max_norm))
    for table, nchunks, esize in tables:
        ext.scale_mt(table, nchunks, esize, stats)
    return stats[0]
