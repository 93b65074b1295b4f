"""CPU twin of test_optim_family_gpu.py.

The same cases, float64 references and bounds (tests/optim_cases.py), run
without a GPU: through a plain fp32 yardstick of each formula, which has to
stay within 1/4 of every bound (the final rounding of p alone may use its
whole u*|p| term, see optim_cases), and through the package's own CPU path,
which has to stay within the bounds. Seeded mistakes in the yardstick show
that the checks can fail. Two host-side properties are tested here as
well: bias corrections follow each parameter's own step count, and a
state_dict round trip keeps the fp32 state of bf16 parameters.
"""
import copy

import pytest
import torch

import optim_cases as oc

ROOM = 4.0
KINDS = ["adam", "sgd", "lamb"]
DTYPES = [torch.float32, torch.bfloat16]


def _report(what, ratios):
    print(f"{what}: error/bound " +
          ", ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_yardstick_has_room(kind, dtype):
    arith, rounded = {}, {}
    for spec in oc.SPECS[kind]:
        case = oc.optim_case(kind, dtype, spec)
        got = oc.optim_yardstick(case)
        ref = oc.optim_reference(case, got["coef"])
        a = oc.optim_ratios(got, ref, case, final_rounding=False)
        r = oc.optim_ratios(got, ref, case)
        for k, v in a.items():
            assert v * ROOM <= 1.0, (oc.spec_id(spec), k, v)
        for k, v in r.items():
            assert v <= 1.0, (oc.spec_id(spec), k, v)
        oc.worst(arith, a)
        oc.worst(rounded, r)
    _report(f"{kind} {dtype} yardstick, before the final rounding", arith)
    _report(f"{kind} {dtype} yardstick, rounded", rounded)


def test_cases_do_what_they_say():
    """The LAMB families reach both sides of each clamp and both trust = 1
    branches; the cancelling family cancels; every shape meets every
    family."""
    seen, met = set(), set()
    for spec in oc.SPECS["lamb"]:
        case = oc.optim_case("lamb", torch.float32, spec)
        clamp = spec[0]["clamp_trust"]
        for t, r in zip(case["tensors"], oc.optim_reference(case)):
            met.add((tuple(t["p"].shape), t["family"]))
            if t["family"] == "ratio_big":
                assert r["trust"] == clamp
                seen.add(("clamped", clamp))
            if t["family"] == "ratio_small" and spec[0]["weight_decay"] == 0:
                assert abs(r["trust"] - 0.3) < 1e-6
                seen.add("below")
            if t["family"] == "p_zero":
                assert r["trust"] == 1.0 and float(r["delta"].abs().max()) > 0
                seen.add("wn0")
            if t["family"] in ("zero", "zero_update") and \
                    spec[0]["weight_decay"] == 0:
                assert r["trust"] == 1.0 and not bool(r["delta"].any())
                seen.add("un0")
    assert seen == {("clamped", 10.0), ("clamped", 0.5), "below", "wn0",
                    "un0"}
    assert len(met) == len(oc.SHAPES) * len(oc.LAMB_FAMILIES)
    case = oc.optim_case("adam", torch.float32, oc.SPECS["adam"][0])
    cl = case["tensors"][oc.CHANNELS_LAST]
    assert cl["p"].stride() == (60, 1, 15, 3) == cl["g"].stride()
    for t, r in zip(case["tensors"], oc.optim_reference(case)):
        if t["family"] == "cancel":
            terms = (0.9 * t["m"].double()).abs()
            assert float((r["m"].abs() / terms).max()) < 0.02


@pytest.mark.parametrize("kind", KINDS)
def test_package_cpu_path(kind):
    w = {}
    for spec in oc.SPECS[kind]:
        case = oc.optim_case(kind, torch.float32, spec)
        got = oc.optim_run(case, "cpu")
        r = oc.optim_ratios(got, oc.optim_reference(case, got["coef"]), case)
        for k, v in r.items():
            assert v <= 1.0, (oc.spec_id(spec), k, v)
        oc.worst(w, r)
    _report(f"{kind} package CPU path", w)


@pytest.mark.parametrize("mistake", oc.MISTAKES)
def test_seeded_mistake_is_rejected(mistake):
    hits = total = 0
    for kind in KINDS:
        for dtype in DTYPES:
            for spec in oc.SPECS[kind]:
                case = oc.optim_case(kind, dtype, spec)
                got = oc.optim_yardstick(case, mistake)
                r = oc.optim_ratios(
                    got, oc.optim_reference(case, got["coef"]), case)
                total += 1
                hits += max(r.values()) > 1.0
    print(f"{mistake}: rejected on {hits} of {total} cases")
    assert hits > 0


@pytest.mark.parametrize("kind", KINDS)
def test_chained_steps_cpu(kind):
    w = {}
    for step, r in enumerate(oc.optim_chain(kind, torch.float32, "cpu")):
        for k, v in r.items():
            assert v <= 1.0, (step + 1, k, v)
        oc.worst(w, r)
    _report(f"{kind} 12 chained steps, package CPU path", w)


@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_per_parameter_steps(kind):
    """One group of three parameters; the second has grad None for steps 1
    to 3, so from step 4 on its bias corrections are those of steps 1, 2,
    3 while its neighbours are at 4, 5, 6."""
    for step, r in enumerate(oc.optim_chain(
            kind, torch.float32, "cpu", steps=6, shapes=oc.CHAIN_SHAPES,
            late=(1, 3))):
        _report(f"{kind} step {step + 1}", r)
        for k, v in r.items():
            assert v <= 1.0, (step + 1, k, v)


def _bf16_optimizer(kind, params):
    from ravnest_amd.ops import FusedAdam, FusedLAMB, FusedSGD
    if kind == "sgd":
        return FusedSGD(params, lr=0.1, momentum=0.9)
    return (FusedAdam if kind == "adam" else FusedLAMB)(params, lr=1e-3)


@pytest.mark.parametrize("kind", KINDS)
def test_state_round_trip_keeps_fp32(kind):
    """state_dict() -> load_state_dict() into a fresh optimizer over bf16
    parameters: every state tensor stays fp32 and bit-identical. The CPU
    path keeps no master, so one is planted, as the GPU path would."""
    g = torch.Generator().manual_seed(0)
    ps = [torch.randn(s, generator=g).to(oc.BF16).requires_grad_()
          for s in oc.CHAIN_SHAPES]
    opt = _bf16_optimizer(kind, ps)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(oc.BF16)
        opt.step()
    for p in ps:
        opt.state[p]["master"] = p.detach().float() + 2.0 ** -12
    saved = copy.deepcopy(opt.state_dict())
    fresh = _bf16_optimizer(kind, [p.detach().clone().requires_grad_()
                                   for p in ps])
    fresh.load_state_dict(saved)
    back = fresh.state_dict()
    assert back["param_groups"] == saved["param_groups"]
    names = {"sgd": {"momentum_buffer", "master"}}.get(
        kind, {"step", "m", "v", "master"})
    for i, st in saved["state"].items():
        assert set(st) == set(back["state"][i]) == names
        for k, v in st.items():
            got = back["state"][i][k]
            if k == "step":
                assert got == v == 2
                continue
            assert got.dtype == torch.float32, (k, got.dtype)
            assert torch.equal(got, v), k
            assert got.data_ptr() != v.data_ptr()
    # an fp32 checkpoint of fp32 parameters loads unchanged
    ps32 = [p.detach().float().requires_grad_() for p in ps]
    opt32 = _bf16_optimizer(kind, ps32)
    for p in ps32:
        p.grad = torch.randn(p.shape, generator=g)
    opt32.step()
    saved = copy.deepcopy(opt32.state_dict())
    fresh = _bf16_optimizer(kind, [p.detach().clone().requires_grad_()
                                   for p in ps32])
    fresh.load_state_dict(saved)
    for i, st in saved["state"].items():
        for k, v in st.items():
            got = fresh.state_dict()["state"][i][k]
            assert got == v if k == "step" else torch.equal(got, v)
