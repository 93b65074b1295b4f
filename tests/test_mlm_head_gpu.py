"""Sparse MLM head (csrc/mlm_head.hip, ops/mlm_head.py): decoder +
cross-entropy on the non-ignored rows only, live count on the device.

Tolerances are MEASURED, not fixed: E is the error of the existing dense
GPU path (bf16 F.linear -> ops.cross_entropy -> autograd) against an fp32
torch reference on the same bf16 inputs; the sparse path must stay within
2*E per quantity (both are fp32-accumulate with one bf16 rounding and
differ only in accumulation order and split-K atomics). dh, dW and db get
no floor at all. The loss gets 4 fp32 ulps of the reference loss
(4 * 2**-23 * |loss|): both paths sum the per-row losses with fp32 float
atomics, whose order changes from run to run, so the mean moves by a few
ulps of loss_sum / count whatever the logits are. Where the reference is
all zero (count 0) every bound is 0 and equality is asserted.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from ravnest_amd import set_seed
from ravnest_amd.models import BertConfig, BertForMLM
from ravnest_amd.ops import (CrossEntropyLoss, FusedAdam, cross_entropy,
                             sparse_mlm_head_loss)
from ravnest_amd.ops import mlm_head as mlm_head_mod
from ravnest_amd.ops import rng

pytestmark = pytest.mark.gpu

HD, N = 128, 320
IGN = -100
COUNTS = [0, 1, 63, 64, 65, 256, 257, 320]
QTYS = ("loss", "dh", "dW", "db")


def _inputs(V, seed=0):
    g = torch.Generator().manual_seed(1000 + V + seed)
    h = torch.randn(N, HD, generator=g)
    W = torch.randn(V, HD, generator=g) * 0.05
    b = torch.randn(V, generator=g) * 0.1
    dev = "cuda:0"
    return (h.to(dev).bfloat16(), W.to(dev).bfloat16(), b.to(dev).bfloat16())


_INPUT_CACHE = {}


def _shared_inputs(V):
    if V not in _INPUT_CACHE:
        _INPUT_CACHE[V] = _inputs(V)
    return _INPUT_CACHE[V]


def _labels(V, count, place, seed=0):
    g = torch.Generator().manual_seed(77 + 13 * count + seed)
    t = torch.full((N,), IGN, dtype=torch.int64)
    if place == "front":
        rows = torch.arange(count)
    else:
        rows = torch.randperm(N, generator=g)[:count]
    t[rows] = torch.randint(0, V, (count,), generator=g)
    return t.to("cuda:0")


def _run(kind, h, W, b, t):
    """-> dict(loss, dh, dW, db) as fp32 tensors."""
    if kind == "ref":
        h_, W_, b_ = (x.detach().float().requires_grad_(True)
                      for x in (h, W, b))
        if bool((t != IGN).any()):
            loss = F.cross_entropy(h_ @ W_.T + b_, t, ignore_index=IGN)
        else:  # torch's mean over zero rows is NaN; the contract is 0
            loss = (h_ @ W_.T + b_).sum() * 0.0
    else:
        h_, W_, b_ = (x.detach().clone().requires_grad_(True)
                      for x in (h, W, b))
        if kind == "dense":
            loss = cross_entropy(F.linear(h_, W_, b_), t, IGN)
        else:
            loss = sparse_mlm_head_loss(h_, W_, b_, t, IGN)
    loss.backward()
    return {"loss": loss.detach().float().reshape(1),
            "dh": h_.grad.float(), "dW": W_.grad.float(),
            "db": b_.grad.float()}


def _tolerances(ref, dense):
    """(E, tol) per quantity: tol = 2*E, plus 4 fp32 ulps of the reference
    loss for the loss alone (order of the fp32 atomics that sum the per-row
    losses; see the module docstring). All zero when the reference is."""
    E = {q: float((dense[q] - ref[q]).abs().max()) for q in QTYS}
    tol = {q: 2.0 * E[q] for q in QTYS}
    tol["loss"] += 4.0 * 2.0 ** -23 * float(ref["loss"].abs().max())
    return E, tol


def _check_close(got, want, tol, tag):
    for q in QTYS:
        assert torch.isfinite(got[q]).all(), f"{tag} {q}: non-finite"
        err = float((got[q] - want[q]).abs().max())
        assert err <= tol[q], f"{tag} {q}: err {err:.3e} > tol {tol[q]:.3e}"


@pytest.mark.parametrize("place", ["front", "scattered"])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("V", [1024, 1002])
def test_op_matches_fp32_reference(V, count, place):
    h, W, b = _shared_inputs(V)
    t = _labels(V, count, place)
    ref = _run("ref", h, W, b, t)
    dense = _run("dense", h, W, b, t)
    sparse = _run("sparse", h, W, b, t)
    E, tol = _tolerances(ref, dense)
    errs = {q: float((sparse[q] - ref[q]).abs().max()) for q in QTYS}
    print("MLMHEAD_ERR V=%d count=%d place=%s " % (V, count, place) +
          " ".join("%s:E=%.3e,sparse=%.3e" % (q, E[q], errs[q])
                   for q in QTYS))
    _check_close(sparse, ref, tol, f"V={V} count={count} {place}")
    # exact: ignored rows carry exactly zero hidden-state gradient
    dead = t == IGN
    assert bool((sparse["dh"][dead] == 0).all())
    if count == 0:
        for q in QTYS:
            assert bool((sparse[q] == 0).all()), q


def test_graph_replay_large_then_small_counts():
    """Forward+backward captured once, replayed with all live -> 15 % ->
    0 -> 15 % (other positions): the large-then-small order catches any
    reliance on stale workspace rows of an earlier, larger count."""
    V = 1002
    h0, W0, b0 = _shared_inputs(V)
    dev = h0.device
    hs = h0.clone().requires_grad_(True)
    Ws = W0.clone().requires_grad_(True)
    bs = b0.clone().requires_grad_(True)
    ts = _labels(V, N, "front")

    def step():
        loss = sparse_mlm_head_loss(hs, Ws, bs, ts, IGN)
        loss.backward()
        return loss

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    hs.grad = Ws.grad = bs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss = step()

    n15 = int(round(0.15 * N))
    label_sets = [_labels(V, N, "front"), _labels(V, n15, "scattered", 1),
                  _labels(V, 0, "front"), _labels(V, n15, "scattered", 2)]
    for k, t in enumerate(label_sets):
        ts.copy_(t)
        graph.replay()
        torch.cuda.synchronize(dev)
        got = {"loss": s_loss.detach().float().reshape(1).clone(),
               "dh": hs.grad.float().clone(), "dW": Ws.grad.float().clone(),
               "db": bs.grad.float().clone()}
        count = int((t != IGN).sum())
        ref = _run("ref", h0, W0, b0, t)
        dense = _run("dense", h0, W0, b0, t)
        eager = _run("sparse", h0, W0, b0, t)
        _, tol = _tolerances(ref, dense)
        print("MLMHEAD_GRAPH replay=%d count=%d " % (k, count) + " ".join(
            "%s:tol=%.3e,diff=%.3e" % (
                q, tol[q], float((got[q] - eager[q]).abs().max()))
            for q in QTYS))
        _check_close(got, eager, tol, f"replay {k} (count {count})")
        assert bool((got["dh"][t == IGN] == 0).all())
        if count == 0:
            for q in QTYS:
                assert bool((got[q] == 0).all()), q


def test_engine_graphed_step_flag_on_vs_off():
    """3 GraphedTrainStep steps, sparse head on vs RAVNEST_SPARSE_MLM_HEAD=0,
    same seed: per-step losses agree within the measured loss tolerance of
    the same head shape (hidden 128, vocab 1002), and the fused path is
    asserted through its call counter."""
    from ravnest_amd.engine.compute import ComputeEngine
    device = torch.device("cuda:0")
    V = 1002
    cfg = BertConfig.tiny(max_seq=64, vocab_size=V)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (8, 64), generator=g)
    labels = ids.clone()
    labels[torch.rand(ids.shape, generator=g) > 0.15] = IGN
    ids, labels = ids.to(device), labels.to(device)
    mask = torch.ones_like(ids)

    def run(flag):
        os.environ["RAVNEST_SPARSE_MLM_HEAD"] = flag
        os.environ["RAVNEST_CUDA_GRAPH"] = "1"
        try:
            set_seed(31)
            # the dropout counter is per device and outlives an engine:
            # both runs must start it from the same value
            rng.reset_seed_counter(device)
            model = BertForMLM(cfg).to(device).to(torch.bfloat16)
            opt = FusedAdam(model.parameters(), lr=1e-4)
            eng = ComputeEngine(model, opt, device,
                                criterion=CrossEntropyLoss(IGN),
                                loss_filename=None, versioning=False)
            calls0 = mlm_head_mod.CALLS
            losses = [eng.find_loss(i, [ids, mask], [False, False],
                                    labels)[2] for i in range(3)]
            assert eng._graph_step is not None and eng._graph_step.graphs
            assert not eng._graph_step.failed
            return losses, mlm_head_mod.CALLS - calls0
        finally:
            os.environ.pop("RAVNEST_SPARSE_MLM_HEAD", None)
            os.environ.pop("RAVNEST_CUDA_GRAPH", None)

    on, calls_on = run("1")
    off, calls_off = run("0")
    assert calls_on > 0, "sparse head was not taken with the flag on"
    assert calls_off == 0, "sparse head ran with the flag off"

    # measured loss tolerance of this head shape at a comparable count
    h, W, b = _shared_inputs(V)
    count = int((labels != IGN).sum())
    t = _labels(V, min(count, N), "scattered")
    ref = _run("ref", h, W, b, t)
    dense = _run("dense", h, W, b, t)
    _, tol = _tolerances(ref, dense)
    print("MLMHEAD_ENGINE on=%s off=%s tol=%.3e" % (on, off, tol["loss"]))
    for a, c in zip(on, off):
        assert abs(a - c) <= tol["loss"], (on, off, tol["loss"])
