"""CPU twin of test_kernel_conditioning_gpu.py.

The same inputs, float64 references and bounds (tests/conditioning.py), run
through the package's ops on the CPU, where they are torch's native fp32
kernels. Each BatchNorm / LayerNorm bound must hold for that known-good
fp32 implementation with a factor 4 to spare: a bound torch itself only
just meets would say nothing about a HIP kernel that misses it. The
softmax, cross-entropy and pooling checks are run the same way to prove
that the checkers accept a correct implementation of the -inf / NaN / tie
contracts.
"""
import pytest
import torch

import conditioning as cd

CPU = torch.device("cpu")
ROOM = 4.0


def _assert_room(ratios, what):
    print(f"{what}: error/bound " +
          ", ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v * ROOM <= 1.0, (what, k, v)


@pytest.mark.parametrize("shape", cd.BN_SHAPES)
def test_batchnorm_fp32_bound_has_room(shape):
    case = cd.bn_case(shape, torch.float32)
    ref = cd.bn_reference(case, training=True)
    got = cd.bn_run(case, CPU, training=True)
    _assert_room(cd.bn_ratios(got, ref, case, True), f"bn fp32 {shape}")


@pytest.mark.parametrize("shape", cd.BN_SHAPES)
def test_batchnorm_bf16_bound_has_room(shape):
    """fp32 arithmetic on the upcast bf16 inputs, results rounded to bf16:
    what a correct bf16 kernel with fp32 statistics computes."""
    case = cd.bn_case(shape, torch.bfloat16)
    ref = cd.bn_reference(case, training=True)
    up = dict(case, x=case["x"].float(), dy=case["dy"].float())
    got = cd.bn_run(up, CPU, training=True)
    for k in ("y", "dx"):
        got[k] = got[k].to(torch.bfloat16)
    ratios = cd.bn_ratios(got, ref, case, True)
    # bf16 spacing is 2^-7 relative, so the final rounding alone can use
    # the whole 2^-8 term: y and dx only have to fit, the rest needs room
    rounded = {k: ratios.pop(k) for k in ("y", "dx")}
    print(f"bn bf16 {shape}: error/bound after rounding {rounded}")
    assert max(rounded.values()) <= 1.0
    _assert_room(ratios, f"bn bf16 {shape}")


@pytest.mark.parametrize("shape", cd.BN_SHAPES[:2])
def test_batchnorm_eval_bound_has_room(shape):
    case = cd.bn_case(shape, torch.float32)
    ref = cd.bn_reference(case, training=False)
    got = cd.bn_run(case, CPU, training=False)
    _assert_room(cd.bn_ratios(got, ref, case, False), f"bn eval {shape}")


@pytest.mark.parametrize("add", [False, True], ids=["ln", "add_ln"])
@pytest.mark.parametrize("eps", cd.LN_EPS)
@pytest.mark.parametrize("H", cd.LN_HIDDEN)
def test_layernorm_fp32_bound_has_room(H, eps, add):
    case = cd.ln_case(H, torch.float32, add)
    ref = cd.ln_reference(case, eps)
    got = cd.ln_run(case, CPU, eps)
    _assert_room(cd.ln_ratios(got, ref), f"ln fp32 H={H} eps={eps} add={add}")


@pytest.mark.parametrize("pattern", cd.SOFTMAX_PATTERNS)
@pytest.mark.parametrize("D", cd.SOFTMAX_D)
def test_softmax_checker_accepts_torch(D, pattern):
    case = cd.softmax_case(D, pattern, torch.float32)
    figs = cd.softmax_check(cd.softmax_run(case, CPU),
                            cd.softmax_reference(case), case)
    print(f"softmax D={D} {pattern}: error/tolerance {figs}")
    assert figs["y"] <= 1 and figs["dx"] <= 1


@pytest.mark.parametrize("N,V", cd.CE_SHAPES)
def test_cross_entropy_cpu_path(N, V):
    """The CPU path of cross_entropy (torch fp32) on the same cases: fp32
    roundoff against float64, exact zeros at the -inf columns. The bound
    is a sanity level, not a yardstick: l - lse reaches ~32 in magnitude,
    where fp32 rounds to 2^-20 absolute per operation, and that absolute
    error of the exponent is the relative error of the probability; the
    50304-term sum adds a few more. 2^-16 leaves torch's measured 6.9e-6
    a factor 2."""
    case = cd.ce_case(N, V, torch.float32)
    ref = cd.ce_reference(case)
    got = cd.ce_run(case, CPU)
    el, eg = cd.ce_rel_errors(got, ref)
    print(f"ce fp32 cpu ({N},{V}): loss rel err {el:.3g}, grad rel err "
          f"{eg:.3g}")
    assert el <= 2.0 ** -16 and eg <= 2.0 ** -16
    pad = case["logits"] == cd.NEG_INF
    assert bool((got["grad"][pad] == 0).all())


def test_cross_entropy_all_ignored_is_zero():
    from ravnest_amd.ops import cross_entropy
    logits = torch.randn(6, 11, requires_grad=True)
    targets = torch.full((6,), -100)
    loss = cross_entropy(logits, targets, ignore_index=-100)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert bool((logits.grad == 0).all())


@pytest.mark.parametrize("kind", ["ties", "nan", "neg_inf"])
@pytest.mark.parametrize("k,s,p", cd.MAXPOOL_GEOMS)
def test_maxpool_reference_is_dtype_independent(k, s, p, kind):
    """torch's fp32 max-pool picks the same elements as the float64
    reference (ties, NaN, all -inf windows), so the GPU test's exact
    comparisons ask nothing the reference cannot do."""
    x = cd.pool_input(kind, torch.float32)
    got, ref = cd.maxpool_pair(x, k, s, p, CPU)
    nan = torch.isnan(ref["y"])
    assert kind != "nan" or bool(nan.any())
    assert torch.equal(torch.isnan(got["y"]), nan)
    assert torch.equal(got["y"][~nan].double(), ref["y"][~nan])
    assert bool(torch.isfinite(got["dx"]).all())
    assert float((got["dx"].double() - ref["dx"]).abs().max()) <= 1e-6
