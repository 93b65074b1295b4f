"""The fused Adam / SGD / LAMB update kernels (csrc/optim.hip), element by
element against float64: every case, reference and bound of
tests/optim_cases.py through the public optimizers on the GPU, in fp32 and
in bf16 with fp32 masters. `bf16_exact` in the ratios is the exactness
check: every bf16 parameter equals the round-to-nearest-even bf16 of the
kernel's own new master. No element is excluded anywhere; every tensor a
kernel writes sits between sentinels that must survive.

test_optim_family_cpu.py shows that a plain fp32 implementation uses at
most a quarter of these bounds and that seeded mistakes break them.
"""
import copy

import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu

KINDS = ["adam", "sgd", "lamb"]
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


def _report(what, ratios):
    print(f"{what}: error/bound " +
          ", ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


def _check(ratios, where):
    for k, v in ratios.items():
        assert v <= 1.0, (where, k, v)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_meet_the_bounds(dev, kind, dtype):
    w = {}
    for spec in oc.SPECS[kind]:
        case = oc.optim_case(kind, dtype, spec)
        got = oc.optim_run(case, dev)
        r = oc.optim_ratios(got, oc.optim_reference(case, got["coef"]), case)
        oc.worst(w, r)
        _check(r, oc.spec_id(spec))
    _report(f"{kind} {dtype} worst of {len(oc.SPECS[kind])} cases", w)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_chained_steps(dev, kind, dtype):
    w = {}
    for step, r in enumerate(oc.optim_chain(kind, dtype, dev)):
        oc.worst(w, r)
        _check(r, step + 1)
    _report(f"{kind} {dtype} 12 chained steps", w)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["adam", "lamb"])
def test_per_parameter_steps(dev, kind, dtype):
    """The second of three parameters has grad None for steps 1 to 3."""
    for step, r in enumerate(oc.optim_chain(
            kind, dtype, dev, steps=6, shapes=oc.CHAIN_SHAPES, late=(1, 3))):
        _report(f"{kind} {dtype} step {step + 1}", r)
        _check(r, step + 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_adam_graph_entry_point(dev, dtype):
    """ext.fused_adam_graph called directly: lr and the step number N come
    from device buffers and the kernel derives 1 - b^N itself. Same cases,
    reference and bounds as the eager entry point."""
    from ravnest_amd.ops import get_ext
    from ravnest_amd.ops.optim import _norm_pass
    ext = get_ext(required=True)
    by_n = {}
    failures = []
    for spec in oc.SPECS["adam"]:
        hyper, N, clip, _ = spec
        case = oc.optim_case("adam", dtype, spec)
        s = oc.optim_build(case, dev)
        cols = [[v[k] for v in s.views] for k in ("p", "g", "m", "v")]
        masters = [v["master"] for v in s.views if v["master"] is not None]
        table = ext.mt_build_table(*cols, masters)
        lr = torch.full((1,), hyper["lr"], dtype=torch.float32, device=dev)
        step = torch.full((1,), N, dtype=torch.int64, device=dev)
        stats = None
        if clip:
            stats = s.opt._stats_on(dev)
            partials = torch.empty(table[1], dtype=torch.float32, device=dev)
            _norm_pass(ext, [table], partials, stats, float(case["clip"]))
        b1, b2 = hyper["betas"]
        ext.fused_adam_graph(*table, lr, b1, b2, hyper["eps"],
                             hyper["weight_decay"], step, stats)
        got = oc.optim_read(s)
        r = oc.optim_ratios(got, oc.optim_reference(case, got["coef"]), case)
        oc.worst(by_n.setdefault(N, {}), r)
        failures += [(oc.spec_id(spec), k, v) for k, v in r.items()
                     if not v <= 1.0]
    for N, w in sorted(by_n.items()):
        _report(f"fused_adam_graph {dtype} N={N}", w)
    assert not failures, failures[:5]


def _resume_grads(shapes, step):
    g = torch.Generator().manual_seed(1000 + step)
    return [torch.randn(s, generator=g).to(oc.BF16) for s in shapes]


def _state_tensors(opt, ps):
    return [{k: v for k, v in opt.state[p].items()} for p in ps]


@pytest.mark.parametrize("kind", KINDS)
def test_resume_bf16(dev, kind):
    """3 steps, state_dict, load into a fresh optimizer over cloned
    parameters, 3 more steps == 6 uninterrupted steps, bit for bit for
    Adam and SGD. LAMB sums its norms with float atomics across chunks, so
    there the resumed run is held to the single-step bound of the
    uninterrupted run's last step."""
    from ravnest_amd.ops import FusedAdam, FusedLAMB, FusedSGD
    shapes = oc.CHAIN_SHAPES + [(65536 + 5,)]
    hyper = oc.CHAIN_SPECS[kind][0]
    cls = {"adam": FusedAdam, "sgd": FusedSGD, "lamb": FusedLAMB}[kind]
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=g).to(oc.BF16) for s in shapes]

    def fresh(src):
        ps = [p.detach().clone().to(dev).requires_grad_() for p in src]
        return ps, cls(ps, **hyper)

    def run(ps, opt, steps):
        before = None
        for step in steps:
            for p, gr in zip(ps, _resume_grads(shapes, step)):
                p.grad = gr.to(dev)
            if step == 6:
                before = copy.deepcopy(_state_tensors(opt, ps))
            opt.step()
        return before

    ps_a, opt_a = fresh(init)
    before6 = run(ps_a, opt_a, range(1, 7))
    ps_b, opt_b = fresh(init)
    run(ps_b, opt_b, range(1, 4))
    saved = copy.deepcopy(opt_b.state_dict())
    ps_c, opt_c = fresh(ps_b)
    opt_c.load_state_dict(saved)
    for st in _state_tensors(opt_c, ps_c):
        for k, v in st.items():
            assert k == "step" or v.dtype == torch.float32, (k, v.dtype)
    run(ps_c, opt_c, range(4, 7))
    sa, sc = _state_tensors(opt_a, ps_a), _state_tensors(opt_c, ps_c)
    if kind != "lamb":
        for pa, pc, a, c in zip(ps_a, ps_c, sa, sc):
            assert torch.equal(pa, pc)
            assert set(a) == set(c)
            for k in a:
                assert a[k] == c[k] if k == "step" else \
                    torch.equal(a[k], c[k]), k
        return
    case = {"kind": kind, "dtype": oc.BF16, "hyper": hyper, "clip": None,
            "tensors": [
                {"family": "randn", "N": 6, "g": gr, "p": None,
                 "m": st["m"].cpu(), "v": st["v"].cpu(),
                 "master": st["master"].cpu()}
                for st, gr in zip(before6, _resume_grads(shapes, 6))]}
    ref = oc.optim_reference(case)
    got = {"tensors": [{"p": p.detach().cpu(), "m": st["m"].cpu(),
                        "v": st["v"].cpu(), "master": st["master"].cpu()}
                       for p, st in zip(ps_c, sc)]}
    r = oc.optim_ratios(got, ref, case)
    _report("lamb resumed run against the uninterrupted step 6", r)
    _check(r, "resume")
    assert all(st["step"] == 6 for st in sc)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_views(dev, kind, dtype):
    """p, g and the state are views buf[1:1 + n] of sentinel-filled
    buffers: no base is 8-byte aligned, so the Adam kernel has to take its
    scalar loop for the whole chunk. The clipped case also sends the grads
    through the norm kernel's scalar path."""
    spec = oc.SPECS[kind][-1]
    assert spec[2]  # the clipped case
    case = oc.optim_case(kind, dtype, spec, shapes=[(1000,), (7,)])
    s = oc.optim_build(case, dev, offset=1)
    for v in s.views:
        for k, t in v.items():
            assert t is None or t.data_ptr() % 8 != 0, k
    s.opt.step()
    got = oc.optim_read(s)
    r = oc.optim_ratios(got, oc.optim_reference(case, got["coef"]), case)
    _report(f"{kind} {dtype} misaligned views", r)
    _check(r, "misaligned")
