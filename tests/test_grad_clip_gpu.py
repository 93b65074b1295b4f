"""Global-norm gradient clipping on the GPU: the multi-tensor squared-norm
reduction + finalize kernels, ops.clip_grad_norm_, the clip coefficient
fused into the Adam / SGD / LAMB update kernels, non-finite accounting
and hipGraph capture."""
import pytest
import torch

from ravnest_amd import set_seed

pytestmark = pytest.mark.gpu

SMALL = [(64, 64), (3, 7, 11), (128,), (17,)]
OPT_SHAPES = SMALL + [(65536 + 5,)]
# able-to-fail construction of tests/test_grad_clip_cpu.py: weight decay +
# gradient sizes swinging by 1e4, so a dropped coefficient shows in Adam
SCALES = [1.0, 100.0, 0.01, 1.0, 100.0, 0.01]
# see tests/test_grad_clip_cpu.py: lr=1e-3 keeps the effect of a 1-2 ulp
# difference between two correct fp32 clip coefficients below atol where
# g*coef + wd*p cancels; the unclipped trajectory still differs by ~1e-2
ADAM_LR = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


def _randn(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * scale for s in shapes]


def _ref_norm(grads):
    """fp64 reference on the CPU: sqrt(sum(g.double()**2))."""
    return torch.sqrt(sum((g.detach().cpu().double() ** 2).sum()
                          for g in grads))


def _with_grads(grads):
    ps = []
    for g in grads:
        p = torch.zeros_like(g, requires_grad=True)
        p.grad = g
        ps.append(p)
    return ps


# ---- norm kernels vs fp64 ---------------------------------------------
# rtol 1e-4: at most 256 serial fp32 adds per lane, then tree sums of
# positive terms -> relative error well under 256 * 2^-24 ~ 1.5e-5
GRAD_SETS = {
    "tails": SMALL,
    "chunk_plus5": [(65536 + 5,)],
    "two_chunks_plus3": [(2 * 65536 + 3,)],
    "many_300x5": [(5,)] * 300,  # more chunks than finalize has threads
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(GRAD_SETS))
def test_norm_matches_fp64(dev, name, dtype):
    from ravnest_amd.ops import clip_grad_norm_
    grads = [g.to(dev).to(dtype) for g in _randn(GRAD_SETS[name], 3)]
    ref = _ref_norm(grads)
    ps = _with_grads([g.clone() for g in grads])
    n1 = clip_grad_norm_(ps, 1e30)
    n2 = clip_grad_norm_(ps, 1e30)
    assert n1.dim() == 0 and n1.is_cuda and n1.dtype == torch.float32
    assert torch.allclose(n1.cpu().double(), ref, rtol=1e-4, atol=0), \
        (float(n1), float(ref))
    # fixed summation order, no float atomics: bit-reproducible
    assert torch.equal(n1, n2)
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad, g)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_grads_norm_zero_coef_one(dev, dtype):
    from ravnest_amd.ops import FusedSGD
    ps = [torch.randn(*s, device=dev).to(dtype).requires_grad_(True)
          for s in SMALL]
    before = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt = FusedSGD(ps, lr=0.1, max_grad_norm=1.0)
    opt.step()
    stats = opt.grad_norm_stats().cpu()
    assert stats[0] == 0.0 and stats[1] == 1.0 and stats[2] == 0.0
    for p, b in zip(ps, before):
        assert torch.equal(p, b)


def test_grad_none_is_skipped(dev):
    from ravnest_amd.ops import FusedSGD, clip_grad_norm_
    grads = [g.to(dev) for g in _randn(SMALL, 5)]
    ps = _with_grads([g.clone() for g in grads])
    ps.insert(2, torch.zeros(9, device=dev, requires_grad=True))  # no grad
    ref = _ref_norm(grads)
    n = clip_grad_norm_(ps, 1e30)
    assert torch.allclose(n.cpu().double(), ref, rtol=1e-4, atol=0)
    assert ps[2].grad is None
    opt = FusedSGD(ps, lr=0.0, max_grad_norm=1.0)
    opt.step()
    assert torch.allclose(opt.grad_norm_stats()[0].cpu().double(), ref,
                          rtol=1e-4, atol=0)
    assert float(clip_grad_norm_(
        [torch.zeros(3, device=dev, requires_grad=True)], 1.0)) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_misaligned_view_grad(dev, dtype):
    """A grad that is buf[1:1001]: its base is not 16-byte aligned, so
    both the norm and the scale kernel take their scalar path."""
    from ravnest_amd.ops import clip_grad_norm_
    buf = _randn([(1200,)], 7)[0].to(dev).to(dtype)
    keep = buf.clone()
    p = torch.zeros(1000, device=dev, dtype=dtype, requires_grad=True)
    p.grad = buf[1:1 + 1000]
    assert p.grad.data_ptr() % 16 != 0
    ref = _ref_norm([keep[1:1001]])
    n = clip_grad_norm_([p], 1.0)
    assert torch.allclose(n.cpu().double(), ref, rtol=1e-4, atol=0)
    want = (keep[1:1001].double() * (1.0 / (ref.item() + 1e-6))).cpu()
    rtol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-5
    assert torch.allclose(buf[1:1001].cpu().double(), want, rtol=rtol,
                          atol=0)
    # neighbours of the view are untouched
    assert torch.equal(buf[:1], keep[:1])
    assert torch.equal(buf[1001:], keep[1001:])


# ---- ops.clip_grad_norm_ vs torch ----------------------------------------
def _mixed(dev, seed):
    shapes = OPT_SHAPES + [(33, 5)]
    dts = [torch.bfloat16, torch.float32, torch.bfloat16, torch.float32,
           torch.bfloat16, torch.float32]
    return [g.to(dev).to(dt) for g, dt in zip(_randn(shapes, seed), dts)]


def test_clip_grad_norm_mixed_dtypes_matches_torch(dev):
    from ravnest_amd.ops import clip_grad_norm_
    grads = _mixed(dev, 11)
    ps = _with_grads([g.clone() for g in grads])
    # torch's function on upcast copies (fp64 holds bf16 and fp32 exactly)
    qs = _with_grads([g.detach().cpu().double() for g in grads])
    ref = torch.nn.utils.clip_grad_norm_(qs, 1.0)
    n = clip_grad_norm_(ps, 1.0)
    assert float(ref) > 1.0  # the clip acts
    assert torch.allclose(n.cpu().double(), ref, rtol=1e-5, atol=0)
    for p, q in zip(ps, qs):
        rtol = 2.0 ** -7 if p.dtype == torch.bfloat16 else 1e-5
        assert p.grad.dtype == p.dtype
        assert torch.allclose(p.grad.cpu().double(), q.grad, rtol=rtol,
                              atol=0), p.shape


def test_clip_grad_norm_large_max_norm_is_bit_identical(dev):
    from ravnest_amd.ops import clip_grad_norm_
    grads = _mixed(dev, 12)
    ps = _with_grads([g.clone() for g in grads])
    clip_grad_norm_(ps, 1e6)
    for p, g in zip(ps, grads):
        assert torch.equal(p.grad, g)


# ---- fused optimizers -----------------------------------------------------
def _run(dev, make_opt, dtype=torch.float32, steps=len(SCALES),
         torch_clip=None, device=None, shapes=OPT_SHAPES):
    device = dev if device is None else device
    ps = [p.to(dtype).to(device).requires_grad_(True)
          for p in _randn(shapes, 0)]
    opt = make_opt(ps)
    for step in range(steps):
        gs = _randn(shapes, 100 + step, SCALES[step])
        for p, g in zip(ps, gs):
            p.grad = g.to(p.dtype).to(device)
        if torch_clip is not None:
            torch.nn.utils.clip_grad_norm_(ps, torch_clip)
        opt.step()
    return ps, opt


def _close(a, b, atol, rtol):
    return all(torch.allclose(x.detach().cpu().float(),
                              y.detach().cpu().float(), atol=atol, rtol=rtol)
               for x, y in zip(a, b))


def _report(tag, got, ref):
    for x, y in zip(got, ref):
        x, y = x.detach().cpu().float(), y.detach().cpu().float()
        print(f"{tag} {tuple(x.shape)}: max abs err "
              f"{(x - y).abs().max().item():.3e}")


def test_fused_adam_fp32_clip_matches_torch(dev):
    from ravnest_amd.ops import FusedAdam
    kw = dict(lr=ADAM_LR, weight_decay=0.01)
    ref, _ = _run(dev, lambda ps: torch.optim.Adam(ps, **kw), torch_clip=1.0)
    got, _ = _run(dev, lambda ps: FusedAdam(ps, max_grad_norm=1.0, **kw))
    _report("adam fp32", got, ref)
    assert _close(got, ref, 1e-5, 1e-4)
    unclipped, _ = _run(dev, lambda ps: FusedAdam(ps, **kw))
    assert not _close(unclipped, ref, 1e-4, 1e-3), \
        "construction cannot detect a dropped clip coefficient"


def test_fused_adam_bf16_master_clip(dev):
    from ravnest_amd.ops import FusedAdam
    kw = dict(lr=ADAM_LR, weight_decay=0.01)
    # fp32 torch trajectory from bf16-rounded params and bf16-rounded grads
    ps_ref = [p.to(torch.bfloat16).float().to(dev).requires_grad_(True)
              for p in _randn(OPT_SHAPES, 0)]
    o_ref = torch.optim.Adam(ps_ref, **kw)
    ps = [p.to(torch.bfloat16).to(dev).requires_grad_(True)
          for p in _randn(OPT_SHAPES, 0)]
    opt = FusedAdam(ps, max_grad_norm=1.0, **kw)
    for step in range(len(SCALES)):
        gs = [g.to(torch.bfloat16).to(dev)
              for g in _randn(OPT_SHAPES, 100 + step, SCALES[step])]
        for p, q, g in zip(ps, ps_ref, gs):
            p.grad = g.clone()
            q.grad = g.float()
        torch.nn.utils.clip_grad_norm_(ps_ref, 1.0)
        o_ref.step()
        opt.step()
        for p, g in zip(ps, gs):  # grads in memory keep unclipped values
            assert torch.equal(p.grad, g)
    masters = [opt.state[p]["master"] for p in ps]
    _report("adam bf16 master", masters, ps_ref)
    assert _close(masters, ps_ref, 1e-4, 1e-3)


def test_fused_sgd_clip_matches_torch(dev):
    from ravnest_amd.ops import FusedSGD
    kw = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)
    ref, _ = _run(dev, lambda ps: torch.optim.SGD(ps, **kw), torch_clip=1.0)
    got, _ = _run(dev, lambda ps: FusedSGD(ps, max_grad_norm=1.0, **kw))
    _report("sgd", got, ref)
    assert _close(got, ref, 1e-5, 1e-4)
    unclipped, _ = _run(dev, lambda ps: FusedSGD(ps, **kw))
    assert not _close(unclipped, ref, 1e-4, 1e-3)


def test_fused_lamb_clip_gpu_matches_cpu(dev):
    from ravnest_amd.ops import FusedLAMB
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    cpu, _ = _run(dev, lambda ps: FusedLAMB(ps, **kw), steps=3,
                  device=torch.device("cpu"))
    gpu, _ = _run(dev, lambda ps: FusedLAMB(ps, **kw), steps=3)
    _report("lamb", gpu, cpu)
    assert _close(gpu, cpu, 1e-4, 1e-3)
    unclipped, _ = _run(dev, lambda ps: FusedLAMB(
        ps, lr=1e-2, weight_decay=0.01), steps=3)
    assert not _close(unclipped, cpu, 1e-3, 1e-2)


def test_fused_clip_spans_param_groups(dev):
    from ravnest_amd.ops import FusedSGD

    def groups(ps):
        return [{"params": ps[:2]}, {"params": ps[2:], "lr": 0.02}]

    ref, _ = _run(dev, lambda ps: torch.optim.SGD(groups(ps), lr=0.05),
                  torch_clip=1.0, steps=3)
    got, _ = _run(dev, lambda ps: FusedSGD(groups(ps), lr=0.05,
                                           max_grad_norm=1.0), steps=3)
    assert _close(got, ref, 1e-5, 1e-4)


@pytest.mark.parametrize("which", ["adam", "sgd", "lamb"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_huge_max_norm_is_bit_identical_to_none(dev, which, dtype):
    from ravnest_amd.ops import FusedAdam, FusedLAMB, FusedSGD
    mk = {"adam": lambda ps, **k: FusedAdam(ps, lr=1e-2, weight_decay=0.01,
                                            **k),
          "sgd": lambda ps, **k: FusedSGD(ps, lr=0.01, momentum=0.9,
                                          weight_decay=5e-4, **k),
          "lamb": lambda ps, **k: FusedLAMB(ps, lr=1e-2, weight_decay=0.01,
                                            **k)}[which]
    a, oa = _run(dev, lambda ps: mk(ps), dtype=dtype, steps=3)
    b, ob = _run(dev, lambda ps: mk(ps, max_grad_norm=1e30), dtype=dtype,
                 steps=3)
    assert float(ob.grad_norm_stats()[1]) == 1.0
    assert oa.grad_norm_stats() is None  # nothing new ran
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if dtype == torch.bfloat16:
        for x, y in zip(a, b):
            assert torch.equal(oa.state[x]["master"], ob.state[y]["master"])


# ---- non-finite ------------------------------------------------------------
def test_nonfinite_norm_is_counted(dev):
    from ravnest_amd.ops import FusedSGD
    ps = [p.to(dev).requires_grad_(True) for p in _randn(SMALL, 0)]
    opt = FusedSGD(ps, lr=0.0, max_grad_norm=1.0)

    def step(poison):
        gs = _randn(SMALL, 9)
        if poison:
            gs[1][0, 0, 0] = float("inf")
        for p, g in zip(ps, gs):
            p.grad = g.to(dev)
        opt.step()
        return opt.grad_norm_stats().cpu().clone()

    s0 = step(False)
    assert s0[2] == 0 and torch.isfinite(s0[0])
    s1 = step(True)
    assert s1[2] == 1 and torch.isinf(s1[0]) and s1[1] == 0
    s2 = step(False)
    assert s2[2] == 1 and torch.isfinite(s2[0])
    assert torch.equal(s2[:2], s0[:2])


# ---- hipGraph capture (tests/test_graphstep_gpu.py set-up) -------------------
_EAGER = {}


def _eager_run(monkeypatch):
    # the eager reference is computed once and shared, unchanged
    if "run" not in _EAGER:
        _EAGER["run"] = _graph_run(monkeypatch, graph=False,
                                   graph_opt=False)[:2]
    return _EAGER["run"]


def _coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def _graph_run(monkeypatch, graph, graph_opt, steps=8, change_at=None):
    from ravnest_amd.engine.compute import ComputeEngine
    from ravnest_amd.models import BertConfig, BertForMLM
    from ravnest_amd.ops import CrossEntropyLoss, FusedAdam
    device = torch.device("cuda:0")
    monkeypatch.setenv("RAVNEST_CUDA_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("RAVNEST_GRAPH_OPT", "1" if graph_opt else "0")
    cfg = BertConfig.tiny(max_seq=32)
    cfg.dropout = 0.0
    set_seed(23)
    model = BertForMLM(cfg).to(device).to(torch.bfloat16)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    eng = ComputeEngine(model, opt, device, criterion=CrossEntropyLoss(-100),
                        loss_filename=None, versioning=False,
                        max_grad_norm=1.0)
    assert opt.max_grad_norm == 1.0
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, cfg.vocab_size, (8, 32), generator=g).to(device)
    mask = torch.ones(8, 32, dtype=torch.int64, device=device)
    losses, stats = [], []
    for i in range(steps):
        if change_at is not None and i == change_at:
            opt.max_grad_norm = 1e-3
        losses.append(eng.find_loss(i, [ids, mask], [False, False], ids)[2])
        stats.append(opt.grad_norm_stats().cpu().clone())
        assert abs(eng.last_grad_norm() - float(stats[-1][0])) == 0
    return losses, stats, eng


def _assert_matches(eager, graphed):
    # tolerance of test_graph_matches_eager_without_dropout
    for a, b in zip(eager, graphed):
        assert abs(a - b) < 5e-2 * max(1.0, abs(a)), (eager, graphed)


def test_graph_captured_optimizer_clips(monkeypatch):
    """RAVNEST_GRAPH_OPT=1: sqnorm -> finalize -> Adam recorded in the
    graph; every step of the run is a replay. Compared with eager."""
    eager, st_e = _eager_run(monkeypatch)
    graphed, st_g, eng = _graph_run(monkeypatch, graph=True, graph_opt=True)
    assert eng._graph_step.graphs and not eng._graph_step.failed
    assert eng._graph_step.opt_captured
    _assert_matches(eager, graphed)
    replays = st_g[-4:]
    # live norm: changes from replay to replay, and tracks the eager run
    assert len({float(s[0]) for s in replays}) > 1
    for a, b in zip(st_e[-4:], replays):
        assert abs(float(a[0]) - float(b[0])) < 5e-2 * float(a[0])
        want = _coef(float(b[0]), 1.0)
        assert abs(float(b[1]) - want) <= 1e-5 * want
        assert float(b[2]) == 0


def test_graph_replay_sees_live_max_norm(monkeypatch):
    _, stats, eng = _graph_run(monkeypatch, graph=True, graph_opt=True,
                               change_at=6)
    assert eng._graph_step.opt_captured
    for s in stats[4:6]:
        want = _coef(float(s[0]), 1.0)
        assert abs(float(s[1]) - want) <= 1e-5 * want
    for s in stats[6:]:
        want = _coef(float(s[0]), 1e-3)
        assert want < 0.5 and abs(float(s[1]) - want) <= 1e-5 * want


def test_graph_default_mode_eager_step_clips(monkeypatch):
    """Default mode: graphed fwd+bwd, eager fused step with clipping."""
    eager, st_e = _eager_run(monkeypatch)
    graphed, st_g, eng = _graph_run(monkeypatch, graph=True, graph_opt=False)
    assert eng._graph_step.graphs and not eng._graph_step.opt_captured
    _assert_matches(eager, graphed)
    for a, b in zip(st_e[-4:], st_g[-4:]):
        assert abs(float(a[0]) - float(b[0])) < 5e-2 * float(a[0])
        want = _coef(float(b[0]), 1.0)
        assert abs(float(b[1]) - want) <= 1e-5 * want


def test_engine_external_clip_on_gpu(dev):
    """torch.optim.* on the GPU: the engine calls ops.clip_grad_norm_
    before each step."""
    from ravnest_amd.engine.compute import ComputeEngine

    def model():
        set_seed(0)
        return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(),
                                   torch.nn.Linear(16, 4)).to(dev)

    m1, m2 = model(), model()
    eng = ComputeEngine(m1, torch.optim.SGD(m1.parameters(), lr=0.1), dev,
                        max_grad_norm=0.5)
    assert eng._clip_external
    opt2 = torch.optim.SGD(m2.parameters(), lr=0.1)
    x = _randn([(4, 8)], 1)[0].to(dev)
    g = _randn([(4, 4)], 2, 3.0)[0].to(dev)
    eng.forward(0, [x], [False])
    eng.backward(0, {0: g}, speculative_next=False)
    m2(x).backward(g)
    ref = torch.nn.utils.clip_grad_norm_(m2.parameters(), 0.5)
    opt2.step()
    assert abs(eng.last_grad_norm() - float(ref)) <= 1e-5 * float(ref)
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.allclose(p1, p2, atol=1e-5, rtol=1e-4)
