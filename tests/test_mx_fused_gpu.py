"""Fused MX fp8 quantisation: LayerNorm and bias-GELU that emit (q, s) next
to their bf16 output, the vector mx_quant, the bias epilogue of mx_gemm /
mx_gemm2, and the tag that carries (q, s) from producer to MXLinear.

Every fused piece must reproduce the composed path bit for bit, so all
comparisons are torch.equal (bit patterns where NaN occurs) or the
mismatch counts of gemm_cases.mx_quant_mismatches against the float64
reference quantiser. The one bound is not on the code under test: the
value of ops.cross_entropy is an fp32 atomic sum over the rows and moves in
its last bits between two runs on equal logits, so it is held to the
reordering bound of that sum, and equality of the loss is asserted on a
fixed-order cross-entropy (_det_ce).
"""
import math
import os

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ZERO = {"s": 0, "q": 0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ext(dev):
    from ravnest_amd.ops import get_ext
    return get_ext(required=True)


def _bits(t):
    """Bit patterns, so that NaN compares equal to the same NaN."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2
                               else torch.int32)


def _check_quant(ext, y, q, s, what):
    """(q, s) against the stand-alone kernel on the same y and against the
    float64 reference quantiser."""
    q2, s2 = ext.mx_quant(y)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert q.shape == q2.shape and s.shape == s2.shape, what
    assert torch.equal(q, q2) and torch.equal(s, s2), what
    bad = gc.mx_quant_mismatches(q.cpu(), s.cpu(), y.cpu())
    print(f"{what}: mismatches {bad} of {y.numel()} elements")
    assert bad == ZERO


# ------------------------------------------------------------ 1. LN-MX
LN_SHAPES = [(1, 32), (5, 96), (67, 768), (3, 1056), (4, 2048)]


def _ln_case(N, H, variant, pdt):
    g = torch.Generator().manual_seed(100 * N + H)
    x = (torch.randn(N, H, generator=g) * 3 + 50).to(BF16)
    e = torch.randint(-20, 21, (H // 32,), generator=g)
    w = torch.ldexp(torch.randn(H, generator=g), e.repeat_interleave(32))
    b = torch.randn(H, generator=g)
    if variant == "zero_block":     # amax 0 -> scale byte 0
        blk = (H // 32) // 2
        w[blk * 32:(blk + 1) * 32] = 0
        b[blk * 32:(blk + 1) * 32] = 0
    if variant == "nonfinite":      # one NaN row, one +inf row
        x[0, H // 3] = math.nan
        x[N - 1, H // 2] = math.inf
    return x, w.to(pdt), b.to(pdt)


@pytest.mark.parametrize("pdt", [BF16, torch.float32], ids=["wbf16", "wfp32"])
@pytest.mark.parametrize("variant", ["plain", "zero_block", "nonfinite"])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_mx(dev, ext, shape, variant, pdt):
    x, w, b = (t.to(dev) for t in _ln_case(*shape, variant, pdt))
    y0, mean0, rstd0 = ext.layernorm_fwd(x, w, b, 1e-5)
    y, mean, rstd, q, s = ext.layernorm_mx_fwd(x, w, b, 1e-5)
    assert y.dtype == BF16 and y.shape == x.shape
    assert torch.equal(_bits(y), _bits(y0))
    assert torch.equal(_bits(mean), _bits(mean0))
    assert torch.equal(_bits(rstd), _bits(rstd0))
    _check_quant(ext, y, q, s, f"layernorm_mx {shape} {variant}")
    if variant == "zero_block":
        blk = (shape[1] // 32) // 2
        assert bool((s[:, blk] == 0).all())
    if variant == "nonfinite":
        assert not bool(torch.isfinite(y[0]).any())


def test_layernorm_mx_rejects(dev, ext):
    w = torch.ones(48, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        ext.layernorm_mx_fwd(torch.zeros(4, 48, dtype=BF16, device=dev),
                             w, w, 1e-5)
    w = torch.ones(64, device=dev)
    with pytest.raises(RuntimeError):   # fp32 x
        ext.layernorm_mx_fwd(torch.zeros(4, 64, device=dev), w, w, 1e-5)


# ---------------------------------------------------------- 2. GELU-MX
GELU_MX_SHAPES = [(1, 32), (7, 96), (130, 3072), (3, 2080)]


def _gelu_case(N, H, bdt):
    """x ~ N(0, 1), the bias spreads the pre-activations over [-40, 40]
    (as gc.fused_gelu_case does), and +-1e4 at a few places."""
    g = torch.Generator().manual_seed(7 * N + H)
    x = torch.randn(N, H, generator=g)
    flat = x.view(-1)
    idx = (torch.arange(8) * max(1, flat.numel() // 8) + 3) % flat.numel()
    flat[idx] = torch.tensor([1e4, -1e4] * 4)
    return x.to(BF16), torch.linspace(-40.0, 40.0, H).to(bdt)


@pytest.mark.parametrize("bdt", [torch.float32, BF16], ids=["bfp32", "bbf16"])
@pytest.mark.parametrize("shape", GELU_MX_SHAPES,
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_bias_gelu_mx(dev, ext, shape, bdt):
    x, b = (t.to(dev) for t in _gelu_case(*shape, bdt))
    y0 = ext.bias_gelu_fwd(x, b)
    y, q, s = ext.bias_gelu_mx_fwd(x, b)
    assert y.dtype == BF16 and y.shape == x.shape
    assert torch.equal(_bits(y), _bits(y0))
    _check_quant(ext, y, q, s, f"bias_gelu_mx {shape}")


def test_bias_gelu_mx_rejects(dev, ext):
    with pytest.raises(RuntimeError):
        ext.bias_gelu_mx_fwd(torch.zeros(4, 48, dtype=BF16, device=dev),
                             torch.zeros(48, device=dev))
    with pytest.raises(RuntimeError):   # fp32 x
        ext.bias_gelu_mx_fwd(torch.zeros(4, 64, device=dev),
                             torch.zeros(64, device=dev))


# ------------------------------------------------- 3. vector mx_quant
QUANT_SHAPES = [(1, 32), (3, 96), (129, 192), (2, 5, 64)]


@pytest.mark.parametrize("offset", [0, 1, 4])
@pytest.mark.parametrize("shape", QUANT_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_mx_quant_vector_and_offset_views(dev, ext, shape, offset):
    """Block magnitudes from 2^-120 to 2^120 plus NaN / +-inf elements,
    read through a contiguous view whose storage offset leaves the base
    pointer 2 or 8 bytes off a 16-byte boundary."""
    K = shape[-1]
    R = math.prod(shape[:-1])
    x = gc.wide_blocks(rows=R, kb=K // 32, seed=R + K)
    x[0, 5] = math.nan
    x[R - 1, K - 1] = math.inf
    x[R // 2, K // 2] = -math.inf
    big = torch.zeros(R * K + 8, dtype=BF16, device=dev)
    big[offset:offset + R * K] = x.reshape(-1).to(dev)
    view = big[offset:offset + R * K].view(*shape)
    assert view.is_contiguous() and view.storage_offset() == offset
    q, s = ext.mx_quant(view)
    assert q.shape == view.shape and s.shape == (R, K // 32)
    bad = gc.mx_quant_mismatches(q.cpu().reshape(R, K), s.cpu(), x)
    print(f"mx_quant {shape} offset {offset}: mismatches {bad}")
    assert bad == ZERO


# ------------------------------------------------------- 4. GEMM bias
def _gemm_bias_check(fn, dev, M, K, N, bdt):
    xq, xs, _ = gc.mx_operand(M, K, 1)
    wq, ws, _ = gc.mx_operand(N, K, 2)
    ops = [t.to(dev) for t in (xq, xs, wq, ws)]
    g = torch.Generator().manual_seed(M + N)
    # magnitudes from far below to the size of the products' sums
    bias = torch.ldexp(torch.randn(N, generator=g),
                       torch.randint(-6, 14, (N,), generator=g))
    bias = bias.to(bdt).to(dev)
    base = fn(*ops)
    got = fn(*ops, bias)
    assert got.dtype == BF16 and got.shape == (M, N)
    # bf16 + fp32 promotes to fp32 in torch; its rounding to bf16 is the
    # kernel's second rounding
    want = (base + bias).to(BF16)
    assert torch.equal(got, want)
    assert torch.equal(fn(*ops, None), base)
    # a bias view that starts off a 16-byte boundary
    shifted = torch.zeros(N + 1, dtype=bdt, device=dev)[1:].copy_(bias)
    assert torch.equal(fn(*ops, shifted), want)


@pytest.mark.parametrize("bdt", [BF16, torch.float32], ids=["bbf16", "bfp32"])
@pytest.mark.parametrize("shape", gc.MX_GEMM_SHAPES)
def test_mx_gemm_bias(dev, ext, shape, bdt):
    _gemm_bias_check(ext.mx_gemm, dev, *shape, bdt)


@pytest.mark.parametrize("bdt", [BF16, torch.float32], ids=["bbf16", "bfp32"])
@pytest.mark.parametrize("shape", gc.MX_GEMM2_SHAPES)
def test_mx_gemm2_bias(dev, ext, shape, bdt):
    _gemm_bias_check(ext.mx_gemm2, dev, *shape, bdt)


@pytest.mark.parametrize("name", ["mx_gemm", "mx_gemm2"])
def test_mx_gemm_bias_host_checks(dev, ext, name):
    fn = getattr(ext, name)
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)  # noqa: E731
    ops = (z(64, 256), z(64, 8), z(64, 256), z(64, 8))
    with pytest.raises(RuntimeError):   # wrong length
        fn(*ops, torch.zeros(63, dtype=BF16, device=dev))
    with pytest.raises(RuntimeError):   # wrong dtype
        fn(*ops, torch.zeros(64, dtype=torch.float16, device=dev))


# ------------------------------------------------------ 5. tag safety
def test_tag_safety(dev, ext, monkeypatch):
    from ravnest_amd.ops import FusedLayerNorm, MXLinear
    from ravnest_amd.ops import mx
    torch.manual_seed(5)
    ln = FusedLayerNorm(256, emit_mx=True).to(dev).to(BF16)
    with torch.no_grad():
        ln.weight.normal_()
        ln.bias.normal_()
    lin = MXLinear(256, 64).to(dev).to(BF16)
    with torch.no_grad():
        lin.bias.normal_()
    x = torch.randn(10, 256, device=dev).to(BF16)

    def composed(t):
        monkeypatch.setattr(mx, "FUSED_QUANT", False)
        try:
            return lin(t)
        finally:
            monkeypatch.setattr(mx, "FUSED_QUANT", True)

    monkeypatch.setattr(mx, "FUSED_QUANT", True)
    with torch.no_grad():
        y = ln(x)
        assert hasattr(y, mx._TAG)
        q, s = getattr(y, mx._TAG)[:2]
        _check_quant(ext, y, q, s, "FusedLayerNorm(emit_mx) tag")
        out = lin(y)
        assert not hasattr(y, mx._TAG)      # consumed by the one GEMM
        monkeypatch.setattr(mx, "FUSED_QUANT", False)
        y_off = ln(x)
        assert not hasattr(y_off, mx._TAG)
        assert torch.equal(y_off, y)
        assert torch.equal(lin(y_off), out)
        monkeypatch.setattr(mx, "FUSED_QUANT", True)

        # a second consumer of the same tensor quantises for itself
        assert torch.equal(lin(y), out)

        # in-place edit after the producer: the tag is stale
        y = ln(x)
        y.add_(1)
        assert torch.equal(lin(y), composed(y))
        assert not hasattr(y, mx._TAG)

        # clone, view and reshape are other objects
        y = ln(x)
        assert torch.equal(lin(y.clone()), out)
        assert torch.equal(lin(y.view(2, 5, 256)).view(10, 64), out)
        assert hasattr(y, mx._TAG)
        assert torch.equal(lin(y), out)

    # with autograd: same output and gradients as the composed path
    grads = []
    for flag in (True, False):
        monkeypatch.setattr(mx, "FUSED_QUANT", flag)
        xg = x.clone().requires_grad_()
        o = lin(ln(xg))
        o.float().square().sum().backward()
        grads.append([o.detach(), xg.grad] +
                     [p.grad.clone() for p in (*ln.parameters(),
                                               *lin.parameters())])
        ln.zero_grad()
        lin.zero_grad()
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ------------------------------------------------ 6. block end to end
def _nano_fp8(dev, seed=11):
    from ravnest_amd import set_seed
    from ravnest_amd.models import GPT, GPTConfig
    set_seed(seed)
    # vocab 64 >= batch * seq: the ids below are all distinct, so the
    # embedding gradient's fp32 atomics add one value per row
    cfg = GPTConfig.nano64(vocab_size=64, block_size=16)
    cfg.dropout = 0.0
    cfg.fp8 = True
    model = GPT(cfg).to(dev).to(BF16)
    with torch.no_grad():       # biases start at zero: make them count
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(std=0.1)
    return cfg, model


def _det_ce(logits, targets):
    """Cross-entropy with a fixed summation order. ops.cross_entropy adds
    the rows' terms with fp32 atomics, so its value moves in the last bits
    from one run to the next on identical logits (its gradient does not
    read that sum)."""
    return torch.nn.functional.cross_entropy(
        logits.reshape(-1, logits.size(-1)).float(), targets.reshape(-1))


def _reorder_bound(n):
    """Two fp32 sums of the same n positive terms in different orders
    differ by at most 2 (n - 1) u of the sum."""
    return 2 * (n - 1) * gc.U32


def test_gpt_fp8_fused_equals_composed(dev, ext, monkeypatch):
    """Logits, loss and every gradient, FUSED_QUANT on against off. The
    backward runs from ops.cross_entropy; the loss compared for equality
    is the fixed-order one, ops.cross_entropy's own value is held to the
    reordering bound of its atomic sum."""
    from ravnest_amd.ops import cross_entropy, mx
    cfg, model = _nano_fp8(dev)
    g = torch.Generator().manual_seed(0)
    ids = torch.randperm(64, generator=g)[:48].view(3, 16).to(dev)
    tgt = torch.randint(0, 64, (3, 16), generator=g).to(dev)
    calls = {"n": 0}
    real = ext.mx_quant

    def counted(t):
        calls["n"] += 1
        return real(t)

    monkeypatch.setattr(ext, "mx_quant", counted)

    def run(flag):
        monkeypatch.setattr(mx, "FUSED_QUANT", flag)
        model.train()
        model.zero_grad(set_to_none=True)
        calls["n"] = 0
        logits = model(ids)
        n_fwd = calls["n"]
        loss = cross_entropy(logits.reshape(-1, logits.size(-1)),
                             tgt.reshape(-1), ignore_index=-1)
        loss.backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.eval()
        with torch.no_grad():
            short = model(ids[:, :5])
        return (logits.detach(), (_det_ce(logits.detach(), tgt),
                                  loss.detach()), grads, short, n_fwd)

    lg1, (loss1, ploss1), g1, short1, n1 = run(True)
    lg0, (loss0, ploss0), g0, short0, n0 = run(False)
    # per block: 3 weights + the attention output that feeds proj; the
    # composed path adds ln1 -> qkv and mlp_in -> mlp_out
    assert n1 == 4 * cfg.n_layer, n1
    assert n0 == 6 * cfg.n_layer, n0
    assert torch.equal(lg1, lg0)
    assert torch.equal(loss1, loss0)
    print("ops.cross_entropy:", float(ploss1), float(ploss0))
    assert abs(float(ploss1) - float(ploss0)) <= \
        _reorder_bound(tgt.numel()) * float(ploss0)
    assert g1.keys() == g0.keys()
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n
    assert torch.equal(short1, short0)


# ---------------------------------------------------- 7. captured step
@pytest.mark.parametrize("crit", ["fixed_order", "ops"])
def test_graphed_step_fused_equals_composed(dev, monkeypatch, crit):
    """Three captured steps, FUSED_QUANT on against off. With the
    fixed-order criterion the losses are equal; with ops.CrossEntropyLoss,
    whose value carries the rounding of an atomic sum (see _det_ce), they
    agree to the reordering bound."""
    from ravnest_amd.engine.compute import ComputeEngine
    from ravnest_amd.ops import CrossEntropyLoss, FusedAdam, mx
    criterion = _det_ce if crit == "fixed_order" else CrossEntropyLoss(-100)

    def engine(model):          # as tests/test_graphstep_gpu.py:_engine
        os.environ["RAVNEST_CUDA_GRAPH"] = "1"
        try:
            opt = FusedAdam(model.parameters(), lr=1e-3)
            return ComputeEngine(model, opt, dev, criterion=criterion,
                                 loss_filename=None, versioning=False)
        finally:
            os.environ.pop("RAVNEST_CUDA_GRAPH", None)

    g = torch.Generator().manual_seed(1)
    ids = torch.randperm(64, generator=g)[:48].view(3, 16).to(dev)

    def run(flag):
        monkeypatch.setattr(mx, "FUSED_QUANT", flag)
        _, model = _nano_fp8(dev, seed=23)
        eng = engine(model)
        losses = [eng.find_loss(i, [ids], [False], ids)[2] for i in range(3)]
        assert eng._graph_step is not None and eng._graph_step.graphs, \
            "hipGraph was not captured"
        assert not eng._graph_step.failed
        return losses

    fused, composed = run(True), run(False)
    print(f"graphed fp8 losses ({crit})", fused, composed)
    if crit == "fixed_order":
        assert fused == composed
    else:
        for a, b in zip(fused, composed):
            assert abs(a - b) <= _reorder_bound(ids.numel()) * abs(b)
