"""CPU twin of test_gemm_family_gpu.py.

The same cases, float64 references and bounds (tests/gemm_cases.py), run
through torch's own fp32 ops. A bound that a known-good fp32
implementation only just meets would say nothing about a HIP kernel that
misses it, so the unrounded fp32 results have to stay within 1/4 of the
fp32 part of each bound; results rounded to bf16 only have to fit (the
rounding alone can use the whole 2^-8 term). The exact checkers (one-hot
routing, MX quantisation) are shown to accept a correct implementation and
to reject a wrong one.
"""
import pytest
import torch

import gemm_cases as gc

ROOM = 4.0
BF16 = torch.bfloat16


def _report(ratios, what):
    print(f"{what}: error/bound " +
          ", ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def _assert_room(ratios, what, room=ROOM):
    _report(ratios, what)
    for k, v in ratios.items():
        assert v * room <= 1.0, (what, k, v)


# ------------------------------------------------------------------ GELU
def _as_fp32(case):
    return {k: (None if v is None else v.float()) for k, v in case.items()}


@pytest.mark.parametrize("dt,with_bias", gc.GELU_VARIANTS,
                         ids=[f"{d}-{'bias' if w else 'nobias'}"
                              for d, w in gc.GELU_VARIANTS])
@pytest.mark.parametrize("shape", gc.GELU_SHAPES +
                         [(r, gc.GELU_DB_H) for r in gc.GELU_DB_ROWS])
def test_gelu_bounds_have_room(shape, dt, with_bias):
    xdt, bdt = gc.GELU_DTYPES[dt]
    case = gc.gelu_case(*shape, xdt, bdt, with_bias)
    # the grid reaches both ends and the overflow thresholds
    pre = gc.gelu_reference(case)["pre"]
    if shape[0] * shape[1] >= 500:
        assert pre.min() <= -9900 and pre.max() >= 9900
        assert ((pre.abs() > 9.9) & (pre.abs() < 40)).sum() > 100
    # fp32 arithmetic on the same values: a quarter of the fp32 bounds
    c32 = _as_fp32(case)
    _assert_room(gc.gelu_ratios(gc.gelu_torch_fp32(c32), c32,
                                gc.gelu_reference(c32)),
                 f"gelu fp32 {shape} {dt}")
    if xdt == BF16:
        r = gc.gelu_ratios(gc.gelu_torch_fp32(case), case,
                           gc.gelu_reference(case))
        _assert_room(r, f"gelu rounded {shape} {dt}", room=1.0)


def _kernel_formula(pre, dy, quotient):
    """csrc/gelu.hip's arithmetic in fp32 (exp in place of __expf), with
    tanh as the quotient (t-1)/(t+1) or as 1 - 2/(t+1)."""
    k = 0.7978845608028654
    x2 = pre * pre
    t = torch.exp(2.0 * (k * (pre + 0.044715 * pre * x2)))
    th = (t - 1.0) / (t + 1.0) if quotient else 1.0 - 2.0 / (t + 1.0)
    y = 0.5 * pre * (1.0 + th)
    sech2 = 1.0 - th * th
    g = 0.5 * (1.0 + th) + 0.5 * pre * sech2 * k * (1.0 + 3.0 * 0.044715 * x2)
    return {"y": y, "dx": dy * g}


def test_gelu_kernel_formula_survives_exp_overflow():
    """t = exp(2a) is inf in fp32 from a pre-activation of 10.06 on:
    (t-1)/(t+1) is NaN there, 1 - 2/(t+1) is 1 and stays inside the
    bounds everywhere."""
    case = gc.gelu_case(200, 300, torch.float32, torch.float32, False)
    ref = gc.gelu_reference(case)
    pre = case["x"]
    bad = _kernel_formula(pre, case["dy"], quotient=True)
    assert torch.isnan(bad["y"][pre >= 10.0625]).all()
    assert torch.isfinite(bad["y"][pre.abs() < 9.9]).all()
    r = gc.gelu_ratios(_kernel_formula(pre, case["dy"], quotient=False),
                       case, ref)
    _assert_room(r, "gelu kernel formula", room=2.0)


def test_gelu_epilogue_formula_needs_the_clamp():
    """csrc/gemm.hip's x*t/(t+1) unclamped: x*t overflows from 9.9614 on
    (inf), t itself from 10.06 on (inf/inf = NaN)."""
    case = gc.gelu_case(200, 300, torch.float32, torch.float32, False)
    ref = gc.gelu_reference(case)
    x = case["x"]
    k = 0.7978845608028654
    e = 2.0 * k * (x + 0.044715 * x * x * x)
    t = torch.exp(e)
    assert not torch.isfinite((x * t / (t + 1.0))[x >= 9.9614]).any()
    t = torch.exp(e.clamp(max=30.0))
    r = gc.gelu_ratios({"y": x * t / (t + 1.0)}, case, ref)
    _assert_room(r, "gelu epilogue formula, clamped", room=2.0)


# ------------------------------------------------------------ bf16 GEMMs
TWIN_SHAPES = gc.GEMM_SHAPES + [(64, 768, 64), (64, 3072, 64)]


@pytest.mark.parametrize("cancel", [False, True], ids=["randn", "cancel"])
@pytest.mark.parametrize("bias", [False, True], ids=["epi0", "epi1"])
@pytest.mark.parametrize("shape", TWIN_SHAPES)
def test_gemm_bound_has_room(shape, bias, cancel):
    M, K, N = shape
    case = gc.gemm_random_case(M, K, N, bias, cancel)
    ref, S = gc.gemm_reference(case["a"], case["b"], case["bias"])
    y = gc.gemm_torch_fp32(case["a"], case["b"], case["bias"])
    r = {"fp32/e_acc": gc.gemm_ratio(y, ref, S, K, bf16_out=False)}
    _assert_room(r, f"gemm {shape} bias={bias} cancel={cancel}")
    r = {"bf16": gc.gemm_ratio(y.to(BF16), ref, S, K)}
    _assert_room(r, f"gemm rounded {shape}", room=1.0)
    if cancel:  # the case does what it says: the sum cancels
        assert float(ref.abs().max()) < 0.25 * float(S.max())


@pytest.mark.parametrize("K", [128, 768, 3072])
def test_gemm_bound_sees_a_dropped_element(K):
    """A product that leaves out one k element misses the bound at every
    K; the printed max|err| / max|ref| is the figure the older tests put
    under 3e-2."""
    case = gc.gemm_random_case(64, K, 64)
    ref, S = gc.gemm_reference(case["a"], case["b"])
    a = case["a"].clone()
    a[:, K // 3] = 0
    y = gc.gemm_torch_fp32(a, case["b"]).to(BF16)
    r = gc.gemm_ratio(y, ref, S, K)
    old = float((y.double() - ref).abs().max() / ref.abs().max())
    print(f"K={K}: dropped element error/bound {r:.3g}, old metric {old:.3g}")
    assert r > 1.0


@pytest.mark.parametrize("bias", [False, True], ids=["epi0", "epi1"])
@pytest.mark.parametrize("shape", gc.GEMM_SHAPES)
def test_routing_probe_accepts_fp32_and_rejects_a_shift(shape, bias):
    M, K, N = shape
    c = gc.routing_case(M, K, N, bias=bias)
    y = gc.gemm_torch_fp32(c["a"], c["b"], c["bias"]).to(BF16)
    assert gc.routing_mismatches(y, c["want"]) == 0
    if K > 1 and M * N > 1:
        wrong = gc.gemm_torch_fp32(c["a"].roll(1, 1), c["b"],
                                   c["bias"]).to(BF16)
        assert gc.routing_mismatches(wrong, c["want"]) > 0
    assert float(c["want"].float().abs().max()) <= 256


@pytest.mark.parametrize("shape", gc.WGRAD_SHAPES)
def test_wgrad_bound_has_room(shape):
    M, N, K = shape
    case = gc.wgrad_random_case(M, N, K)
    ref, S = gc.gemm_reference(case["dy"].t(), case["x"].t())
    y = case["dy"].float().t() @ case["x"].float()
    _assert_room({"dW": gc.gemm_ratio(y, ref, S, M, bf16_out=False)},
                 f"wgrad {shape}")
    c = gc.wgrad_routing_case(M, N, K)
    assert torch.equal(c["dy"].float().t() @ c["x"].float(), c["want"])


def test_hand_wgrad_predicate():
    """_hand_wgrad sends only shapes gemm_wgrad_bf16 accepts to it: odd N
    or K (2-byte-aligned rows under 16-byte loads) go to the library."""
    from ravnest_amd.ops.linear import _hand_wgrad_ok
    for M, N, K in gc.WGRAD_SHAPES + [gc.WGRAD_ROWS_SHAPE]:
        assert _hand_wgrad_ok(M, N, K), (M, N, K)
    assert not _hand_wgrad_ok(*gc.WGRAD_REJECTED)
    assert not _hand_wgrad_ok(128, 129, 128)
    assert not _hand_wgrad_ok(128, 128, 127)
    assert not _hand_wgrad_ok(100, 128, 128)     # M % 64
    assert not _hand_wgrad_ok(64, 128, 128)      # M < 128
    assert not _hand_wgrad_ok(128, 6, 128)
    assert not _hand_wgrad_ok(128, 4096, 768)    # loses to the library
    # the fallback itself
    from ravnest_amd.ops.linear import _hand_wgrad
    c = gc.wgrad_random_case(*gc.WGRAD_REJECTED)
    want = c["dy"].t() @ c["x"]
    assert torch.equal(_hand_wgrad(c["dy"], c["x"]), want)


# ---------------------------------------------------------------- MX fp8
def test_mx_reference_quantiser():
    """The reference the GPU test compares with bit for bit: scaled amax in
    [224, 448), round-to-nearest (error <= 2^-4 relative or half a
    subnormal step), 0x08 for the values just below 2^-6, 0x7F for
    non-finite elements with the scale from the finite rest."""
    for x in (gc.all_finite_bf16(), gc.bf16_under_fixed_amax(),
              gc.wide_blocks()):
        q, s, _ = gc.mx_quant_ref(x)
        xd = x.double().reshape(-1, 32)
        amax = xd.abs().amax(1)
        scaled = torch.ldexp(amax, -s.reshape(-1))
        inside = (scaled >= 224) & (scaled < 448)
        clamped = (s.reshape(-1).abs() == 127)
        assert bool((inside | clamped).all())
        assert bool((s.reshape(-1)[amax == 0] == -127).all())
        back = gc.mx_dequant(q, (s + 127).to(torch.uint8)).reshape(-1, 32)
        step = torch.ldexp(torch.ones_like(amax), s.reshape(-1) - 10)
        err = (back - xd).abs()
        assert bool((err <= torch.maximum(2.0 ** -4 * xd.abs(),
                                          step.unsqueeze(1))).all())
    # amax = 448 * 2^k takes s = k + 1
    x = torch.zeros(3, 32, dtype=BF16)
    x[0, 0], x[1, 0], x[2, 0] = 448.0, 446.0, 224.0
    assert gc.mx_scale_ref(x).reshape(-1).tolist() == [1, 0, 0]
    # |v| in [7.5 * 2^-9, 2^-6) next to amax 256 (s = 0) rounds to 0x08
    x = torch.zeros(1, 32, dtype=BF16)
    x[0, 0], x[0, 1], x[0, 2] = 256.0, 7.75 * 2.0 ** -9, -7.5 * 2.0 ** -9
    q, s, _ = gc.mx_quant_ref(x)
    assert s.item() == 0 and q[0, :3].tolist() == [0x78, 0x08, 0x88]
    # non-finite elements
    x = gc.nonfinite_blocks()
    q, s, nonfin = gc.mx_quant_ref(x)
    assert bool((q[nonfin] == 0x7F).all()) and int(nonfin.sum()) == 39
    assert bool((q[~nonfin] & 0x7F != 0x7F).all())
    assert s[4, 0].item() == -127              # nothing finite in the block
    assert gc.mx_quant_mismatches(q, (s + 127).to(torch.uint8), x) == \
        {"s": 0, "q": 0}


@pytest.mark.parametrize("shape", gc.MX_GEMM_SHAPES + gc.MX_GEMM2_SHAPES)
def test_mx_gemm_bound_has_room(shape):
    M, K, N = shape
    _, _, xd = gc.mx_operand(M, K, 1)
    _, _, wd = gc.mx_operand(N, K, 2)
    ref = xd @ wd.t()
    S = xd.abs() @ wd.abs().t()
    y = xd.float() @ wd.float().t()
    _assert_room({"fp32/e_acc": gc.gemm_ratio(y, ref, S, K, False)},
                 f"mx gemm {shape}")
    _assert_room({"bf16": gc.gemm_ratio(y.to(BF16), ref, S, K)},
                 f"mx gemm rounded {shape}", room=1.0)
    # block scales really differ along rows and k-blocks
    c = gc.mx_routing_case(M, K, N)
    assert K < 64 or M * N == 1 or len(torch.unique(c["ws"])) > 4
    got = (gc.mx_dequant(c["xq"], c["xs"]).float() @
           gc.mx_dequant(c["wq"], c["ws"]).float().t()).to(BF16)
    assert gc.routing_mismatches(got, c["want"]) == 0
