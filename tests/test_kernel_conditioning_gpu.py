"""Norm, softmax, loss and pooling kernels on ill-conditioned inputs.

test_kernels_gpu.py draws its inputs from randn: zero mean, unit variance,
no ties, no special values. These cases are the ones reduction kernels get
wrong: a mean far from zero next to a small spread (one-pass variance
cancels), -inf logits (exp(-inf - -inf) is NaN), NaN and tied maxima in
pooling windows, hidden sizes on every lane-count path, and dtypes the
entry points do not implement. Every comparison is against a float64
reference of the same operation on the same values; inputs, references and
bounds live in tests/conditioning.py and test_kernel_conditioning_cpu.py
proves the bounds on torch's own fp32 ops.

All marked @pytest.mark.gpu.
"""
import pytest
import torch
import torch.nn.functional as F

import conditioning as cd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


def _assert_within(ratios, what):
    print(f"{what}: error/bound " +
          ", ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}  # NaN is bad
    assert not bad, (what, bad)


# ------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", cd.BN_SHAPES)
def test_batchnorm_train_conditioning(dev, shape, dtype):
    """Channels with |mean|/std up to 3000 (fp32) or 32 (bf16): y, dx,
    dweight, dbias and both running statistics against float64, per channel
    at tol_c = 16 * 2^-24 * (|mu_c| / sqrt(var_c + eps) + 8).

    Measured on an MI355X, error / bound: shifted sums y <= 0.02,
    running_var <= 0.016 (fp32); the unshifted E[x^2] - E[x]^2 this
    replaced gave y 52 to 1.0e5, dx 13 to 5.4e8, running_var 14 to 36.
    bf16 sits at 0.93 to 0.99 for y and dx either way: that is the final
    rounding, whose half-spacing is the 2^-8 term itself."""
    case = cd.bn_case(shape, dtype)
    ref = cd.bn_reference(case, training=True)
    got = cd.bn_run(case, dev, training=True)
    _assert_within(cd.bn_ratios(got, ref, case, True),
                   f"bn train {shape} {dtype}")


@pytest.mark.parametrize("shape", cd.BN_SHAPES[:2])
def test_batchnorm_eval_gradients(dev, shape):
    """Frozen BN: with loaded running statistics and .eval(), forward and
    dx = dy * w * rstd, dweight, dbias match float64 autograd of
    F.batch_norm(training=False); the statistics are left alone. (The
    training-mode formula applied in eval measured dx error / bound 277
    and 1437 here; dx = dy * w * rstd measures 0.002.)"""
    case = cd.bn_case(shape, torch.float32)
    ref = cd.bn_reference(case, training=False)
    got = cd.bn_run(case, dev, training=False)
    _assert_within(cd.bn_ratios(got, ref, case, False), f"bn eval {shape}")


# ------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("add", [False, True], ids=["ln", "add_ln"])
@pytest.mark.parametrize("eps", cd.LN_EPS)
@pytest.mark.parametrize("H", cd.LN_HIDDEN)
def test_layernorm_fp32_conditioning(dev, H, eps, add):
    """fp32 activations with fp32 weights (dispatched, never run by
    test_kernels_gpu.py), rows with mean/std up to 10^4, per row at the
    same tol formula. Measured error / bound: y <= 0.10, dx <= 0.02 with
    shifted sums; E[x^2] - E[x]^2 gave y 245 to 329 at eps = 1e-5 and
    1e6 at eps = 1e-12 (the variance clamps to 0), dx up to 5.7e12."""
    case = cd.ln_case(H, torch.float32, add)
    ref = cd.ln_reference(case, eps)
    got = cd.ln_run(case, dev, eps)
    _assert_within(cd.ln_ratios(got, ref),
                   f"ln fp32 H={H} eps={eps} add={add}")


@pytest.mark.parametrize("add", [False, True], ids=["ln", "add_ln"])
@pytest.mark.parametrize("eps", cd.LN_EPS)
@pytest.mark.parametrize("H", cd.LN_HIDDEN)
def test_layernorm_bf16_conditioning(dev, H, eps, add):
    """The same row families in bf16, at the tolerances of
    test_layernorm_fwd_bwd / test_add_layer_norm, and nothing non-finite.
    Measured error / tolerance: y <= 0.10 with shifted sums, 1.4 to 4.8
    with E[x^2] - E[x]^2 (the (3, 0.02) rows: their variance of 2e-4 is
    the difference of two sums near 9)."""
    case = cd.ln_case(H, torch.bfloat16, add)
    ref = cd.ln_reference(case, eps)
    got = cd.ln_run(case, dev, eps)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"non-finite {k}"
    ty, tdx, aw, rw = (5e-2, 8e-2, 1.0, 3e-2) if add else \
        (3e-2, 5e-2, 0.5, 2e-2)
    ratios = {
        "y": cd.allclose_ratio(got["y"], ref["y"], ty, ty),
        "dx": cd.allclose_ratio(got["dx"], ref["dx"], tdx, tdx),
        "dw": cd.allclose_ratio(got["dw"], ref["dw"], aw, rw),
        "db": cd.allclose_ratio(got["db"], ref["db"], aw, rw),
    }
    if add:
        ratios["dx_b"] = cd.allclose_ratio(got["dx_b"], ref["dx"], tdx, tdx)
    _assert_within(ratios, f"ln bf16 H={H} eps={eps} add={add}")


# ------------------------------------------------------- Embedding + LN
def _embedding_ln(dev, H, word, pos, eps, seed):
    """embedding_ln forward/backward on the GPU and the float64 reference
    gather + gather + add + LayerNorm on the same bf16 values."""
    from ravnest_amd.ops.embedding import embedding_ln
    g = torch.Generator().manual_seed(seed)
    V, P = word.shape[0], pos.shape[0]
    B, S = 4, 24
    ids = torch.randint(0, V, (B, S), generator=g)
    ids[0, :4] = 7  # forced collisions in the scatter-add
    w = torch.randn(H, generator=g).to(torch.bfloat16)
    b = torch.randn(H, generator=g).to(torch.bfloat16)
    dy = torch.randn(B, S, H, generator=g).to(torch.bfloat16)

    leaves = [t.to(dev).requires_grad_() for t in (word, pos, w, b)]
    y = embedding_ln(ids.to(dev), *leaves, eps)
    y.backward(dy.to(dev))
    got = [y.detach().cpu()] + [t.grad.cpu() for t in leaves]

    refs = [t.double().requires_grad_() for t in (word, pos, w, b)]
    x = F.embedding(ids, refs[0]) + refs[1][:S]
    y2 = F.layer_norm(x, (H,), refs[2], refs[3], eps)
    y2.backward(dy.double())
    return got, [y2.detach()] + [t.grad for t in refs], S


@pytest.mark.parametrize("H", [8, 520, 768, 1024])
def test_embedding_ln_hidden_sizes(dev, H):
    """H = 8 leaves 63 lanes idle, 520 gives lane 0 a second vector, 768 and
    1024 (the limit) are the BERT sizes on the two-vector path;
    test_fused_embedding_ln's tolerances."""
    g = torch.Generator().manual_seed(H)
    word = torch.randn(97, H, generator=g).to(torch.bfloat16)
    pos = torch.randn(40, H, generator=g).to(torch.bfloat16)
    got, ref, S = _embedding_ln(dev, H, word, pos, 1e-12, 3)
    y, dword, dpos, dw, db = got
    assert float(dpos[S:].abs().max()) == 0
    dpos, ref[2] = dpos[:S], ref[2][:S]
    ratios = {
        "y": cd.allclose_ratio(y, ref[0], 5e-2, 5e-2),
        "dword": cd.allclose_ratio(dword, ref[1], 8e-2, 8e-2),
        "dpos": cd.allclose_ratio(dpos, ref[2], 8e-2, 8e-2),
        "dw": cd.allclose_ratio(dw, ref[3], 2e-1, 5e-2),
        "db": cd.allclose_ratio(db, ref[4], 2e-1, 5e-2),
    }
    _assert_within(ratios, f"embedding_ln H={H}")


@pytest.mark.parametrize("H", [8, 520, 768, 1024])
def test_embedding_ln_constant_rows(dev, H):
    """Word rows constant at 100, position rows 0.01 * randn, BERT's
    eps = 1e-12: E[x^2] - mean^2 cancels to a slightly negative number and
    rsqrt turns the whole row into NaN. The output must be finite and
    within the existing tolerance of float64 LN(word + pos); the backward
    re-gathers the sum in bf16, so its gradients only have to be finite."""
    g = torch.Generator().manual_seed(100 + H)
    word = torch.full((97, H), 100.0).to(torch.bfloat16)
    pos = (0.01 * torch.randn(40, H, generator=g)).to(torch.bfloat16)
    got, ref, _ = _embedding_ln(dev, H, word, pos, 1e-12, 5)
    for name, t in zip(("y", "dword", "dpos", "dw", "db"), got):
        assert bool(torch.isfinite(t).all()), f"non-finite {name}"
    _assert_within({"y": cd.allclose_ratio(got[0], ref[0], 5e-2, 5e-2)},
                   f"embedding_ln constant rows H={H}")


# -------------------------------------------------------------- softmax
# finite logits scaled to +-3e4 are an fp32 case only
SOFTMAX_CASES = [(D, pat, dt) for D in cd.SOFTMAX_D
                 for pat in cd.SOFTMAX_PATTERNS for dt in DTYPES
                 if not (pat == "scaled" and dt == torch.bfloat16)]


@pytest.mark.parametrize(
    "D,pattern,dtype", SOFTMAX_CASES,
    ids=[f"{D}-{pat}-{'fp32' if dt == torch.float32 else 'bf16'}"
         for D, pat, dt in SOFTMAX_CASES])
def test_softmax_masked_logits(dev, D, pattern, dtype):
    """-inf logits (top-k filtering, padding): no NaN, exact zeros in y and
    dx at the masked columns, test_softmax_kernel's tolerances elsewhere.
    A fully -inf row is not part of the contract and is left out."""
    case = cd.softmax_case(D, pattern, dtype)
    figs = cd.softmax_check(cd.softmax_run(case, dev),
                            cd.softmax_reference(case), case)
    _assert_within(figs, f"softmax D={D} {pattern} {dtype}")


# -------------------------------------------------------- cross-entropy
@pytest.mark.parametrize("N,V", cd.CE_SHAPES)
def test_cross_entropy_bf16_shapes(dev, N, V):
    """V < 8 (scalar tail only), V = 8 (one vector), V < 256 (idle
    threads), ragged V, and a 50257 vocabulary padded to 50304 with -inf
    columns; test_cross_entropy's tolerances, exact zero gradient at the
    pad columns and in the ignored rows."""
    case = cd.ce_case(N, V, torch.bfloat16)
    ref = cd.ce_reference(case)
    got = cd.ce_run(case, dev)
    dl = abs(float(got["loss"]) - float(ref["loss"]))
    ratios = {"loss": dl / (2e-2 * max(1.0, abs(float(ref["loss"])))),
              "grad": cd.allclose_ratio(got["grad"], ref["grad"], 1e-3, 5e-2)}
    _assert_within(ratios, f"ce bf16 ({N},{V})")
    assert bool((got["grad"][case["logits"] == cd.NEG_INF] == 0).all())
    assert bool((got["grad"][case["targets"] == -100] == 0).all())


@pytest.mark.parametrize("N,V", cd.CE_SHAPES)
def test_cross_entropy_fp32_shapes(dev, N, V):
    """The fp32 instantiation. Yardstick: the error of torch's own fp32
    cross_entropy on the same device against the same float64 reference;
    the kernel may be 8x that (__expf is a few ulp looser than libm), with
    a floor of 2^-20 relative."""
    case = cd.ce_case(N, V, torch.float32)
    ref = cd.ce_reference(case)
    got = cd.ce_run(case, dev)
    yard = cd.ce_run(case, dev, fn=F.cross_entropy)
    el, eg = cd.ce_rel_errors(got, ref)
    yl, yg = cd.ce_rel_errors(yard, ref)
    print(f"ce fp32 ({N},{V}): loss rel err {el:.3g} (torch fp32 {yl:.3g}), "
          f"grad rel err {eg:.3g} (torch fp32 {yg:.3g})")
    floor = 2.0 ** -20
    assert el <= max(8 * yl, floor), (el, yl)
    assert eg <= max(8 * yg, floor), (eg, yg)
    assert bool((got["grad"][case["logits"] == cd.NEG_INF] == 0).all())
    assert bool((got["grad"][case["targets"] == -100] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_cross_entropy_masked_head(dev, dtype):
    """-inf where each thread starts reading (the padded-vocabulary case
    above only masks the end of the row, which no fp32 thread reads
    first). bf16 at test_cross_entropy's tolerances, fp32 against the
    torch-fp32 yardstick as above."""
    case = cd.ce_masked_head_case(dtype)
    ref = cd.ce_reference(case)
    got = cd.ce_run(case, dev)
    assert bool(torch.isfinite(got["loss"])), "non-finite loss"
    el, eg = cd.ce_rel_errors(got, ref)
    if dtype == torch.float32:
        yl, yg = cd.ce_rel_errors(cd.ce_run(case, dev, fn=F.cross_entropy),
                                  ref)
        print(f"ce masked head fp32: loss rel err {el:.3g} (torch fp32 "
              f"{yl:.3g}), grad rel err {eg:.3g} (torch fp32 {yg:.3g})")
        assert el <= max(8 * yl, 2.0 ** -20), (el, yl)
        assert eg <= max(8 * yg, 2.0 ** -20), (eg, yg)
    else:
        dl = abs(float(got["loss"]) - float(ref["loss"]))
        _assert_within(
            {"loss": dl / (2e-2 * max(1.0, abs(float(ref["loss"])))),
             "grad": cd.allclose_ratio(got["grad"], ref["grad"], 1e-3, 5e-2)},
            "ce masked head bf16")
    assert bool((got["grad"][case["logits"] == cd.NEG_INF] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_cross_entropy_all_ignored(dev, dtype):
    """No valid target: loss 0 and an all-zero gradient (the mean divides
    by max(n_valid, 1)), not torch's NaN."""
    from ravnest_amd.ops import cross_entropy
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(6, 1003, generator=g) * 4).to(dtype).to(
        dev).requires_grad_()
    targets = torch.full((6,), -100, device=dev)
    loss = cross_entropy(logits, targets, ignore_index=-100)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert bool((logits.grad == 0).all())


# -------------------------------------------------------------- pooling
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k,s,p", cd.MAXPOOL_GEOMS)
def test_maxpool_ties(dev, k, s, p, dtype):
    """Inputs from {0,1,2,3}: every window has tied maxima, as after a
    ReLU. The forward is exact; the gradient goes to the first maximum in
    scan order, as in torch."""
    x = cd.pool_input("ties", dtype)
    got, ref = cd.maxpool_pair(x, k, s, p, dev)
    assert torch.equal(got["y"].double(), ref["y"])
    err = (got["dx"].double() - ref["dx"]).abs()
    print(f"maxpool ties {(k, s, p)} {dtype}: max dx err {float(err.max())}")
    if dtype == torch.float32:
        assert float(err.max()) <= 1e-6
    else:
        assert bool((err <= cd.bf16_ulp_bound(ref["dx"])).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k,s,p", cd.MAXPOOL_GEOMS)
def test_maxpool_propagates_nan(dev, k, s, p, dtype):
    """One NaN per plane: every window that sees it returns NaN, as in
    torch, and nothing else changes."""
    x = cd.pool_input("nan", dtype)
    got, ref = cd.maxpool_pair(x, k, s, p, dev)
    nan = torch.isnan(ref["y"])
    assert bool(nan.any())
    assert torch.equal(torch.isnan(got["y"]), nan)
    assert torch.equal(got["y"][~nan].double(), ref["y"][~nan])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("k,s,p", cd.MAXPOOL_GEOMS)
def test_maxpool_all_neg_inf_windows(dev, k, s, p, dtype):
    """A 6x6 region of -inf: windows inside it return -inf and send their
    gradient to their first element, as in torch."""
    x = cd.pool_input("neg_inf", dtype)
    got, ref = cd.maxpool_pair(x, k, s, p, dev)
    assert bool((ref["y"] == cd.NEG_INF).any())
    assert torch.equal(got["y"].double(), ref["y"])
    assert bool(torch.isfinite(got["dx"]).all())
    err = (got["dx"].double() - ref["dx"]).abs()
    print(f"maxpool -inf {(k, s, p)} {dtype}: max dx err {float(err.max())}")
    if dtype == torch.float32:
        assert float(err.max()) <= 1e-6
    else:
        assert bool((err <= cd.bf16_ulp_bound(ref["dx"])).all())


def _pool_bf16(dev, module, ref_fn, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).to(torch.bfloat16)
    xg = x.to(dev).requires_grad_()
    y = module(xg)
    dy = torch.randn(y.shape, generator=g).to(torch.bfloat16)
    y.backward(dy.to(dev))
    xr = x.double().requires_grad_()
    yr = ref_fn(xr)
    yr.backward(dy.double())
    return {
        "y": cd._ratio((y.detach().cpu().double() - yr.detach()).abs(),
                       cd.bf16_ulp_bound(yr.detach())),
        "dx": cd._ratio((xg.grad.cpu().double() - xr.grad).abs(),
                        cd.bf16_ulp_bound(xr.grad)),
    }


@pytest.mark.parametrize("inc", [True, False])
@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (3, 2, 1)])
def test_avgpool_bf16(dev, k, s, p, inc):
    """bf16 AvgPool2d (test_avgpool2d_kernel is fp32 only), fp32
    accumulation: one bf16 ulp of the float64 reference."""
    from ravnest_amd.ops.pool import AvgPool2d
    ratios = _pool_bf16(
        dev, AvgPool2d(k, s, p, count_include_pad=inc),
        lambda t: F.avg_pool2d(t, k, s, p, count_include_pad=inc),
        (2, 4, 15, 15), 6)
    _assert_within(ratios, f"avgpool bf16 {(k, s, p)} inc={inc}")


def test_global_avgpool_bf16(dev):
    from ravnest_amd.ops.pool import AdaptiveAvgPool2d
    ratios = _pool_bf16(dev, AdaptiveAvgPool2d((1, 1)),
                        lambda t: F.adaptive_avg_pool2d(t, (1, 1)),
                        (4, 8, 9, 9), 7)
    _assert_within(ratios, "global avgpool bf16")


# ------------------------------------------------------ dtype rejection
def test_batchnorm_fwd_rejects_float64(dev):
    """The entry point implements fp32 and bf16 only and must say so:
    dispatching 'not bf16' as float would read a float64 tensor as fp32
    bits. (float64 is the one safe probe: read as float it stays inside
    its own allocation.)"""
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    x = torch.randn(2, 4, 5, 5, device=dev, dtype=torch.float64)
    w, b = torch.ones(4, device=dev), torch.zeros(4, device=dev)
    rm, rv = torch.zeros(4, device=dev), torch.ones(4, device=dev)
    with pytest.raises(RuntimeError):
        ext.batchnorm_fwd(x, w, b, rm, rv, True, 0.1, 1e-5)
    with pytest.raises(RuntimeError):
        ext.batchnorm_fwd(x, w, b, rm, rv, False, 0.1, 1e-5)


def test_layernorm_fwd_rejects_float64(dev):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    x = torch.randn(8, 64, device=dev, dtype=torch.float64)
    w, b = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    with pytest.raises(RuntimeError):
        ext.layernorm_fwd(x, w, b, 1e-5)
