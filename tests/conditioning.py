"""Input builders, float64 references and error bounds for the
ill-conditioned kernel tests (test_kernel_conditioning_gpu.py and its CPU
twin test_kernel_conditioning_cpu.py).

Every reference here is float64 and is computed on the CPU from the exact
values the implementation under test was given (bf16 inputs are upcast,
never regenerated). The `*_run` functions go through the package's public
ops, which dispatch on the device of their input: on a GPU they reach the
HIP kernels, on the CPU torch's native fp32 ops. The CPU twin uses that to
prove that every bound below leaves a correct fp32 implementation room.

The `*_ratios` functions return measured error / bound per quantity; a
test asserts `ratio <= 1` (or `<= 1/4` for the twin) and prints them.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24     # fp32 unit roundoff
BF16_ULP = 2.0 ** -8  # one bf16 ulp, relative


def tol(r):
    """Relative bound for a normalised value whose mean/std ratio is r.

    An fp32 mean carries a few ulp of |mu|; after division by sigma that is
    r * 2^-24 times a small constant. The + 8 covers the ordinary rounding
    of |xhat| <= ~5."""
    return 16 * U32 * (r + 8)


def bf16_ulp_bound(ref):
    return BF16_ULP * ref.abs().clamp(min=1.0)


def _leaf(t, device):
    """A fresh leaf on `device`; the case's own tensor is left untouched
    (on the CPU `.to(device)` alone would return that very tensor)."""
    return t.detach().clone().to(device).requires_grad_()


def _ratio(err, bound):
    """max(err / bound), with 0/0 counting as 0."""
    err, bound = err.double(), torch.as_tensor(bound).double()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max())


# ------------------------------------------------------------ BatchNorm
BN_SHAPES = [(16, 8, 14, 14), (4, 8, 7, 7), (3, 8, 9, 11), (32, 8, 28, 28)]
BN_FAMILIES_FP32 = [(0, 1), (3, 1), (100, 1), (-300, 1), (1000, 1),
                    (3000, 1), (50, 0.05), (0, 1e-3)]
# mean/std ratios that bf16's 8 bits can still resolve
BN_FAMILIES_BF16 = [(0, 1), (2, 1), (8, 1), (32, 1), (-16, 0.5), (1, 0.05),
                    (0, 1), (4, 2)]
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def bn_case(shape, dtype, seed=0):
    fam = BN_FAMILIES_BF16 if dtype == torch.bfloat16 else BN_FAMILIES_FP32
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    assert C == len(fam)
    mu = torch.tensor([f[0] for f in fam], dtype=torch.float32)
    sigma = torch.tensor([f[1] for f in fam], dtype=torch.float32)
    x = mu.view(1, C, 1, 1) + sigma.view(1, C, 1, 1) * torch.randn(
        shape, generator=g)
    return {
        "x": x.to(dtype),
        "dy": torch.randn(shape, generator=g).to(dtype),
        "w": torch.randn(C, generator=g),
        "b": torch.randn(C, generator=g),
        "sigma": sigma.double(),
        # eval mode: non-trivial statistics of the same conditioning
        "running_mean": mu + 0.1 * sigma * torch.randn(C, generator=g),
        "running_var": sigma ** 2 * (0.5 + torch.rand(C, generator=g)),
    }


def bn_reference(case, training):
    x = case["x"].double().requires_grad_()
    w = case["w"].double().requires_grad_()
    b = case["b"].double().requires_grad_()
    dy = case["dy"].double()
    if training:
        rm = torch.zeros_like(w).detach()
        rv = torch.ones_like(w).detach()
    else:
        rm = case["running_mean"].double().clone()
        rv = case["running_var"].double().clone()
    stat_mean = x.detach().mean((0, 2, 3)) if training else rm.clone()
    stat_var = (x.detach().var((0, 2, 3), unbiased=False) if training
                else rv.clone())
    y = F.batch_norm(x, rm, rv, w, b, training, BN_MOMENTUM, BN_EPS)
    y.backward(dy)
    std = (stat_var + BN_EPS).sqrt()
    xhat = (x.detach() - stat_mean.view(1, -1, 1, 1)) / std.view(1, -1, 1, 1)
    return {
        "y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad,
        "running_mean": rm, "running_var": rv,
        "abs_dw": (dy * xhat).abs().sum((0, 2, 3)),
        "abs_db": dy.abs().sum((0, 2, 3)),
        "tol": tol(stat_mean.abs() / std),
    }


def bn_run(case, device, training):
    """FusedBatchNorm2d (fp32 parameters, fresh running stats) forward and
    backward on `device`; everything comes back on the CPU."""
    from ravnest_amd.ops import FusedBatchNorm2d
    C = case["x"].shape[1]
    bn = FusedBatchNorm2d(C, eps=BN_EPS, momentum=BN_MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(case["w"])
        bn.bias.copy_(case["b"])
        if not training:
            bn.running_mean.copy_(case["running_mean"])
            bn.running_var.copy_(case["running_var"])
    bn = bn.to(device)
    bn.train(training)
    x = _leaf(case["x"], device)
    y = bn(x)
    y.backward(case["dy"].to(device))
    return {
        "y": y.detach().cpu(), "dx": x.grad.cpu(),
        "dw": bn.weight.grad.cpu(), "db": bn.bias.grad.cpu(),
        "running_mean": bn.running_mean.cpu(),
        "running_var": bn.running_var.cpu(),
    }


def bn_ratios(got, ref, case, training):
    """error / bound for every BatchNorm quantity, worst channel."""
    bf16 = case["x"].dtype == torch.bfloat16
    t = ref["tol"]
    tc = t.view(1, -1, 1, 1)
    out = {}
    for name, k in (("y", 1.0), ("dx", 4.0)):
        err = (got[name].double() - ref[name]).abs()
        cmax = ref[name].abs().amax((0, 2, 3), keepdim=True)
        if bf16:
            out[name] = _ratio(err, bf16_ulp_bound(ref[name]) + tc * cmax)
        else:
            out[name] = _ratio(err.amax((0, 2, 3), keepdim=True),
                               k * tc * cmax)
    out["dw"] = _ratio((got["dw"].double() - ref["dw"]).abs(),
                       4 * t * ref["abs_dw"])
    out["db"] = _ratio((got["db"].double() - ref["db"]).abs(),
                       4 * t * ref["abs_db"])
    if training:
        out["running_mean"] = _ratio(
            (got["running_mean"].double() - ref["running_mean"]).abs(),
            BN_MOMENTUM * t * case["sigma"])
        out["running_var"] = _ratio(
            (got["running_var"].double() - ref["running_var"]).abs(),
            t * ref["running_var"].abs())
    else:  # eval must leave the statistics alone
        out["running_mean"] = float(
            (got["running_mean"].double() != ref["running_mean"]).any())
        out["running_var"] = float(
            (got["running_var"].double() != ref["running_var"]).any())
    return out


# ------------------------------------------------------------ LayerNorm
LN_HIDDEN = [100, 768, 1000]
LN_ROWS = 64
LN_FAMILIES = [(0, 1), (64, 1), (1000, 1), (100, 0.01), (3, 0.02)]
LN_EPS = [1e-5, 1e-12]


def ln_case(H, dtype, add, seed=0):
    """64 rows, row i drawn from family i % 5. With `add` the row is split
    into a residual pair (a, b) whose sum has the family's conditioning."""
    g = torch.Generator().manual_seed(seed + H)
    fam = [LN_FAMILIES[i % len(LN_FAMILIES)] for i in range(LN_ROWS)]
    mu = torch.tensor([f[0] for f in fam], dtype=torch.float32).view(-1, 1)
    sigma = torch.tensor([f[1] for f in fam], dtype=torch.float32).view(-1, 1)
    x = (mu + sigma * torch.randn(LN_ROWS, H, generator=g)).to(dtype)
    case = {
        "a": x,
        "dy": torch.randn(LN_ROWS, H, generator=g).to(dtype),
        "w": torch.randn(H, generator=g),
        "bias": torch.randn(H, generator=g),
    }
    if add:
        case["b"] = (0.25 * sigma * torch.randn(LN_ROWS, H, generator=g)
                     ).to(dtype)
    return case


def ln_input_sum(case):
    """The float64 rows that get normalised. The fused add rounds a + b to
    the activation dtype (that sum is the saved residual stream, as in the
    unfused `a + b`), so for bf16 the reference rounds it too; in fp32 the
    rounding is left to the bound."""
    if "b" not in case:
        return case["a"].double()
    if case["a"].dtype == torch.bfloat16:
        return (case["a"].float() + case["b"].float()).to(
            torch.bfloat16).double()
    return case["a"].double() + case["b"].double()


def ln_reference(case, eps):
    H = case["a"].shape[-1]
    x = ln_input_sum(case).requires_grad_()
    w = case["w"].double().requires_grad_()
    b = case["bias"].double().requires_grad_()
    dy = case["dy"].double()
    y = F.layer_norm(x, (H,), w, b, eps)
    y.backward(dy)
    xd = x.detach()
    mean = xd.mean(-1, keepdim=True)
    std = (xd.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    xhat = (xd - mean) / std
    t = tol(mean.abs() / std)  # (rows, 1)
    return {
        "y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad,
        "tol": t,
        "bound_dw": (4 * t * (dy * xhat).abs()).sum(0),
        "bound_db": (4 * t * dy.abs()).sum(0),
    }


def ln_run(case, device, eps):
    from ravnest_amd.ops import add_layer_norm, layer_norm
    a = _leaf(case["a"], device)
    w = _leaf(case["w"], device)
    bias = _leaf(case["bias"], device)
    if "b" in case:
        b = _leaf(case["b"], device)
        y = add_layer_norm(a, b, w, bias, eps)
    else:
        b = None
        y = layer_norm(a, w, bias, eps)
    y.backward(case["dy"].to(device))
    out = {"y": y.detach().cpu(), "dx": a.grad.cpu(), "dw": w.grad.cpu(),
           "db": bias.grad.cpu()}
    if b is not None:
        out["dx_b"] = b.grad.cpu()
    return out


def ln_ratios(got, ref):
    """fp32: error / bound, worst row (y, dx) or column (dw, db)."""
    out = {}
    for name, k in (("y", 1.0), ("dx", 4.0), ("dx_b", 4.0)):
        if name not in got:
            continue
        r = ref["dx" if name == "dx_b" else name]
        err = (got[name].double() - r).abs().amax(-1, keepdim=True)
        out[name] = _ratio(err, k * ref["tol"] * r.abs().amax(-1, keepdim=True))
    out["dw"] = _ratio((got["dw"].double() - ref["dw"]).abs(), ref["bound_dw"])
    out["db"] = _ratio((got["db"].double() - ref["db"]).abs(), ref["bound_db"])
    return out


def allclose_ratio(got, ref, atol, rtol):
    """error / (atol + rtol * |ref|), the quantity torch.allclose bounds by
    1; NaN or Inf in `got` gives inf."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return _ratio((got - ref).abs(), atol + rtol * ref.abs())


# -------------------------------------------------------------- softmax
SOFTMAX_D = [200, 1000, 4099]
SOFTMAX_ROWS = 7
SOFTMAX_PATTERNS = ["col5", "first64", "one_finite", "ten_finite", "scaled"]
NEG_INF = float("-inf")


def softmax_case(D, pattern, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + D)
    x = torch.randn(SOFTMAX_ROWS, D, generator=g) * 4
    if pattern == "col5":
        x[:, 5] = NEG_INF
    elif pattern == "first64":
        x[:, :64] = NEG_INF
    elif pattern in ("one_finite", "ten_finite"):
        keep = 1 if pattern == "one_finite" else 10
        masked = torch.full_like(x, NEG_INF)
        for r in range(SOFTMAX_ROWS):
            cols = torch.randperm(D, generator=g)[:keep]
            masked[r, cols] = x[r, cols]
        x = masked
    elif pattern == "scaled":
        x = x / x.abs().max() * 3e4
    else:
        raise ValueError(pattern)
    return {"x": x.to(dtype),
            "dy": torch.randn(SOFTMAX_ROWS, D, generator=g).to(dtype)}


def softmax_reference(case):
    x, dy = case["x"].double(), case["dy"].double()
    y = torch.softmax(x, -1)
    return {"y": y, "dx": y * (dy - (dy * y).sum(-1, keepdim=True))}


def softmax_run(case, device):
    from ravnest_amd.ops import softmax
    x = _leaf(case["x"], device)
    y = softmax(x, -1)
    y.backward(case["dy"].to(device))
    return {"y": y.detach().cpu(), "dx": x.grad.cpu()}


def softmax_check(got, ref, case):
    """Returns the measured figures after asserting the mask contract; the
    tolerances are test_softmax_kernel's."""
    masked = case["x"] == NEG_INF
    tol_ = 1e-5 if case["x"].dtype == torch.float32 else 1e-2
    assert not bool(torch.isnan(got["y"]).any()), "NaN in y"
    assert not bool(torch.isnan(got["dx"]).any()), "NaN in dx"
    assert bool((got["y"][masked] == 0).all()), "y != 0 at a -inf input"
    assert bool((got["dx"][masked] == 0).all()), "dx != 0 at a -inf input"
    return {"y": allclose_ratio(got["y"], ref["y"], tol_, 1e-2),
            "dx": allclose_ratio(got["dx"], ref["dx"], 5 * tol_, 2e-2)}


# -------------------------------------------------------- cross-entropy
CE_SHAPES = [(8, 5), (8, 8), (16, 250), (16, 1003), (8, 50304)]
CE_REAL_VOCAB = 50257  # the (8, 50304) case pads this with -inf columns


def ce_case(N, V, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + V)
    logits = torch.randn(N, V, generator=g) * 4
    hi = V
    if V == 50304:
        logits[:, CE_REAL_VOCAB:] = NEG_INF
        hi = CE_REAL_VOCAB
    targets = torch.randint(0, hi, (N,), generator=g)
    targets[::3] = -100
    return {"logits": logits.to(dtype), "targets": targets}


def ce_masked_head_case(dtype, seed=0):
    """(16, 1003) with columns [0, 300) and [1000, 1003) at -inf, as after
    top-k filtering: every thread's FIRST element is masked, in the fp32
    loop (thread t starts at column t), in the bf16 vector loop (groups 0
    to 36) and in the bf16 scalar tail (columns 1000 to 1002)."""
    g = torch.Generator().manual_seed(seed + 17)
    N, V = 16, 1003
    logits = torch.randn(N, V, generator=g) * 4
    logits[:, :300] = NEG_INF
    logits[:, 1000:] = NEG_INF
    targets = torch.randint(300, 1000, (N,), generator=g)
    targets[::3] = -100
    return {"logits": logits.to(dtype), "targets": targets}


def ce_reference(case):
    l = case["logits"].double().requires_grad_()
    loss = F.cross_entropy(l, case["targets"], ignore_index=-100)
    loss.backward()
    return {"loss": loss.detach(), "grad": l.grad}


def ce_run(case, device, fn=None):
    """fn defaults to the package's cross_entropy; the fp32 yardstick passes
    torch's own."""
    if fn is None:
        from ravnest_amd.ops import cross_entropy as fn
    l = _leaf(case["logits"], device)
    loss = fn(l, case["targets"].to(device), ignore_index=-100)
    loss.backward()
    return {"loss": loss.detach().cpu(), "grad": l.grad.cpu()}


def ce_rel_errors(got, ref):
    """(loss error / |loss|, max grad error / max |grad|)."""
    el = float((got["loss"].double() - ref["loss"]).abs() / ref["loss"].abs())
    eg = float((got["grad"].double() - ref["grad"]).abs().max()
               / ref["grad"].abs().max())
    return el, eg


# -------------------------------------------------------------- pooling
POOL_SHAPE = (3, 5, 17, 17)
MAXPOOL_GEOMS = [(3, 2, 1), (3, 2, 0), (2, 2, 0), (3, 1, 1)]


def pool_input(kind, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "ties":  # post-ReLU-like: every window has repeated maxima
        x = torch.randint(0, 4, POOL_SHAPE, generator=g).float()
    else:
        x = torch.randn(POOL_SHAPE, generator=g)
    if kind == "nan":  # one NaN per (n, c) plane
        N, C, H, W = POOL_SHAPE
        pos = torch.randint(0, H * W, (N * C,), generator=g)
        x.view(N * C, H * W)[torch.arange(N * C), pos] = float("nan")
    if kind == "neg_inf":  # windows that see nothing but -inf
        x[:, :, 4:10, 4:10] = NEG_INF
    return x.to(dtype)


def maxpool_pair(x, k, s, p, device, seed=1):
    """(got, ref): the package's MaxPool2d on `device` and torch's float64
    max_pool2d on the CPU, forward and backward, same dy."""
    from ravnest_amd.ops.pool import MaxPool2d
    xg = _leaf(x, device)
    y = MaxPool2d(k, s, p)(xg)
    g = torch.Generator().manual_seed(seed)
    # multiples of 1/8 below 1: the up to nine dy that meet in one dx sum
    # exactly in fp32 and in bf16, whatever the order of the additions
    dy = (torch.randint(-7, 8, y.shape, generator=g).float() / 8).to(x.dtype)
    y.backward(dy.to(device))
    xr = x.double().requires_grad_()
    yr = F.max_pool2d(xr, k, s, p)
    yr.backward(dy.double())
    return ({"y": y.detach().cpu(), "dx": xg.grad.cpu()},
            {"y": yr.detach(), "dx": xr.grad})
