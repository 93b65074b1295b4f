"""Fused BatchNorm + [residual add] + ReLU (csrc/batchnorm.hip) on the GPU.

The composed path is the reference: F.relu(FusedBatchNorm2d(x)) and
F.relu(FusedBatchNorm2d(x) + r), i.e. the BN kernels, a torch add and a
torch ReLU. The fused modules promise the very same numbers, so the
comparisons are torch.equal. With RAVNEST_FUSED_BN_RELU=0 the modules take
the composed path themselves and the file passes trivially.
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from ravnest_amd import set_seed
from ravnest_amd.models import resnet18_ish
from ravnest_amd.ops import (CrossEntropyLoss, FusedAdam, FusedBatchNorm2d,
                             FusedBatchNormAddReLU2d, FusedBatchNormReLU2d)

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}

# the smallest shapes at which each branch of the kernels can go wrong
SHAPES = {
    "hw35_scalar": (4, 3, 5, 7),     # HW = 35: scalar path, C no power of 2
    "hw16_vector": (2, 8, 4, 4),     # HW = 16: vector path in both dtypes
    "hw4_fp32vec": (16, 64, 2, 2),   # HW = 4: one fp32 vector, bf16 scalar
    "hw1": (3, 5, 1, 1),             # HW = 1
    "second_trip": None,             # sized from the kernel's constants
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


def _shape(name):
    if SHAPES[name] is not None:
        return SHAPES[name]
    # more elements than one trip of the grid-stride loop covers at the
    # widest vector (8 bf16 per lane): N = 8, C = 64, HW a multiple of 8
    from ravnest_amd.ops.batchnorm import bn_relu_launch_constants
    cap, block, lane_bytes = bn_relu_launch_constants()
    one_trip = cap * block * (lane_bytes // 2)
    hw = one_trip // (8 * 64) + 8
    assert hw % 8 == 0 and 8 * 64 * hw > one_trip
    return (8, 64, 8, hw // 8)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype, dev, seed=0, n=1):
    """x, r, dy per step and w, b, drawn on the CPU; channels 0, 1, 2 are
    forced when at least two free channels remain next to them. Shared
    between the cases of a shape: callers leave the tensors unchanged."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    steps = []
    for _ in range(n):
        x = 2 * torch.randn(shape, generator=g) + 0.5
        r = torch.randn(shape, generator=g)
        dy = torch.randn(shape, generator=g)
        steps.append(tuple(t.to(dev).to(dtype) for t in (x, r, dy)))
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    forced = C >= 5
    if forced:
        w[0], b[0] = 0.0, 0.0   # every output exactly 0
        b[1] = -100.0           # all dead
        b[2] = 100.0            # all live
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return steps, w.to(dev), b.to(dev), rm.to(dev), rv.to(dev), forced


def _load(m, w, b, rm, rv, dev):
    m = m.to(dev)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
    return m


def _fused(residual, C):
    return (FusedBatchNormAddReLU2d if residual else FusedBatchNormReLU2d)(C)


def _run(m, composed, x, r, dy, residual, r_grad=True):
    """one forward + backward; returns y, dx, dr, dw, db"""
    x = x.clone().requires_grad_(True)
    r = r.clone().requires_grad_(r_grad)
    m.weight.grad = m.bias.grad = None
    if composed:
        y = m(x)
        y = F.relu(y + r if residual else y)
    else:
        y = m(x, r) if residual else m(x)
    y.backward(dy)
    return (y.detach(), x.grad, r.grad, m.weight.grad.clone(),
            m.bias.grad.clone())


@pytest.mark.parametrize("shape_name", list(SHAPES))
@pytest.mark.parametrize("residual", [False, True], ids=["bn_relu",
                                                         "bn_add_relu"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_equals_composed(dev, dtype, training, residual, shape_name):
    shape = _shape(shape_name)
    C = shape[1]
    steps, w, b, rm, rv, forced = _inputs(shape, DTYPES[dtype], dev, n=2)
    fused = _load(_fused(residual, C), w, b, rm, rv, dev).train(training)
    ref = _load(FusedBatchNorm2d(C), w, b, rm, rv, dev).train(training)
    for x, r, dy in steps:  # two steps: the running statistics accumulate
        y1, dx1, dr1, dw1, db1 = _run(fused, False, x, r, dy, residual)
        y0, dx0, dr0, dw0, db0 = _run(ref, True, x, r, dy, residual)
        assert torch.equal(y1, y0)
        assert torch.equal(dx1, dx0)
        assert torch.equal(dw1, dw0)
        assert torch.equal(db1, db0)
        if residual:
            assert torch.equal(dr1, dr0)
            assert dr1.untyped_storage().data_ptr() != \
                dx1.untyped_storage().data_ptr()
        else:
            assert dr1 is None
        assert torch.equal(fused.running_mean, ref.running_mean)
        assert torch.equal(fused.running_var, ref.running_var)
        assert torch.equal(fused.num_batches_tracked, ref.num_batches_tracked)
        if forced:
            assert not dx1[:, 0].any()  # w = 0: no gradient reaches x
            if not residual:
                assert not y1[:, 0].any() and not y1[:, 1].any()
                assert not dw1[:2].any() and not db1[:2].any()
                assert not dx1[:, 1].any()
            assert (y1[:, 2] > 0).all()
    assert int(fused.num_batches_tracked) == (2 if training else 0)
    if training:
        assert not torch.equal(fused.running_mean, rm)
    else:
        assert torch.equal(fused.running_mean, rm)
    assert (y1 == 0).any() and (y1 > 0).any()


@pytest.mark.parametrize("residual", [False, True], ids=["bn_relu",
                                                         "bn_add_relu"])
def test_nonfinite_input(dev, residual):
    shape = SHAPES["hw16_vector"]
    C = shape[1]
    steps, w, b, rm, rv, _ = _inputs(shape, torch.float32, dev)
    x, r, dy = steps[0]
    x = x.clone()
    x[1, 3, 2, 1] = float("inf")  # a free channel
    fused = _load(_fused(residual, C), w, b, rm, rv, dev)
    ref = _load(FusedBatchNorm2d(C), w, b, rm, rv, dev)
    y1, dx1, _, _, _ = _run(fused, False, x, r, dy, residual)
    y0, dx0, _, _, _ = _run(ref, True, x, r, dy, residual)
    assert torch.isnan(y0).any()
    assert torch.allclose(y1, y0, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(dx1, dx0, rtol=0, atol=0, equal_nan=True)


def test_residual_without_grad(dev):
    shape = SHAPES["hw16_vector"]
    C = shape[1]
    steps, w, b, rm, rv, _ = _inputs(shape, torch.float32, dev)
    x, r, dy = steps[0]
    m = _load(_fused(True, C), w, b, rm, rv, dev)
    y1, dx1, dr1, dw1, db1 = _run(m, False, x, r, dy, True, r_grad=True)
    y0, dx0, dr0, dw0, db0 = _run(m, False, x, r, dy, True, r_grad=False)
    assert dr1 is not None and dr0 is None
    assert torch.equal(y1, y0)
    assert torch.equal(dx1, dx0)
    assert torch.equal(dw1, dw0)
    assert torch.equal(db1, db0)


@pytest.mark.parametrize("residual", [False, True], ids=["bn_relu",
                                                         "bn_add_relu"])
@pytest.mark.parametrize("shape_name", ["hw35_scalar", "hw4_fp32vec"])
def test_against_float64(dev, shape_name, residual):
    """fp32 training against plain torch in float64, at the tolerances of
    test_kernels_gpu.py::test_fused_batchnorm. No element is left out: the
    smallest float64 pre-activation magnitude is asserted to be >= 1e-4, so
    a pre-activation on the other side of the ReLU threshold in fp32 would
    be an error above the tolerance. For these inputs (CPU generator seed 2,
    drawn in the order x, w, b, r, dy) the float64 minima are 5.4e-4 and
    6.3e-4 (with residual) at (4,3,5,7), 5.2e-4 and 1.7e-3 (with residual)
    at (16,64,2,2); 37-44 % of the elements are dead. Measured on the
    MI355X: y and dx within 8.2e-7, dw and db within 3.1e-6, dr exact."""
    shape = SHAPES[shape_name]
    C = shape[1]
    g = torch.Generator().manual_seed(2)
    x = 2 * torch.randn(shape, generator=g) + 0.5
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    r = torch.randn(shape, generator=g)
    dy = torch.randn(shape, generator=g)

    x64, w64, b64, r64 = (t.double().requires_grad_(True)
                          for t in (x, w, b, r))
    pre = F.batch_norm(x64, None, None, w64, b64, True, 0.1, 1e-5)
    if residual:
        pre = pre + r64
    ref = F.relu(pre)
    ref.backward(dy.double())
    print(f"min |pre-activation| {pre.abs().min().item():.3e}, dead "
          f"{(pre <= 0).double().mean().item():.2f}")
    assert pre.abs().min().item() >= 1e-4
    assert (pre <= 0).any() and (pre > 0).any()

    m = _load(_fused(residual, C), w, b, torch.zeros(C), torch.ones(C), dev)
    y, dx, dr, dw, db = _run(m, False, x.to(dev), r.to(dev), dy.to(dev),
                             residual)

    def close(a, ref64, atol):
        a = a.double().cpu()
        print(f"  max abs err {(a - ref64).abs().max().item():.3e}")
        return torch.allclose(a, ref64, atol=atol, rtol=1e-3)

    assert close(y, ref.detach(), 1e-4)
    assert close(dx, x64.grad, 1e-4)
    assert close(dw, w64.grad, 1e-3)
    assert close(db, b64.grad, 1e-3)
    if residual:
        assert close(dr, r64.grad, 1e-4)


def _resnet_batch(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (8,), generator=g)
    return x.to(dev), y.to(dev)


def test_graph_matches_eager_resnet(dev):
    """The fused ops live inside the captured training step."""
    from ravnest_amd.engine.compute import ComputeEngine

    def run(graph):
        set_seed(23)
        model = resnet18_ish().to(dev)
        os.environ["RAVNEST_CUDA_GRAPH"] = "1" if graph else "0"
        try:
            opt = FusedAdam(model.parameters(), lr=1e-3)
            eng = ComputeEngine(model, opt, dev,
                                criterion=CrossEntropyLoss(-100),
                                loss_filename=None, versioning=False)
        finally:
            os.environ.pop("RAVNEST_CUDA_GRAPH", None)
        x, y = _resnet_batch(dev)
        losses = [eng.find_loss(i, [x], [False], y)[2] for i in range(6)]
        return losses, eng

    eager, _ = run(False)
    graphed, eng = run(True)
    assert eng._graph_step is not None and eng._graph_step.graphs, \
        "hipGraph was not captured"
    assert not eng._graph_step.failed
    for a, b in zip(eager, graphed):
        assert abs(a - b) < 5e-2 * max(1.0, abs(a)), (eager, graphed)


def test_whole_model_equals_composed(dev, monkeypatch):
    """resnet18_ish fused against composed from one seed: logits equal; the
    gradients equal too if the composed model reproduces its own, else
    within 4x its own run-to-run difference (library convolutions)."""
    def build(switch):
        monkeypatch.setenv("RAVNEST_FUSED_BN_RELU", switch)
        set_seed(5)
        return resnet18_ish().to(dev)

    default = os.environ.get("RAVNEST_FUSED_BN_RELU", "1")
    x, y = _resnet_batch(dev, seed=1)

    def run(m):
        m.zero_grad(set_to_none=True)
        logits = m(x)
        F.cross_entropy(logits, y).backward()
        return logits.detach(), {k: p.grad.clone()
                                 for k, p in m.named_parameters()}

    composed = build("0")
    fused = build(default)
    assert fused.bn1.fused == (default != "0") and not composed.bn1.fused
    lc1, gc1 = run(composed)
    lc2, gc2 = run(composed)
    lf, gf = run(fused)
    assert torch.equal(lf, lc1)
    self_diff = max((gc1[k] - gc2[k]).abs().max().item() for k in gc1)
    diff = max((gf[k] - gc1[k]).abs().max().item() for k in gc1)
    print(f"composed-to-composed max grad diff {self_diff:.3e}, "
          f"fused-to-composed {diff:.3e}")
    if self_diff == 0.0:
        for k in gc1:
            assert torch.equal(gf[k], gc1[k]), k
    else:
        assert diff <= 4 * self_diff, (diff, self_diff)
