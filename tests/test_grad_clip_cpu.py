"""Global-norm gradient clipping, CPU paths: the fused optimizers'
``max_grad_norm`` option against torch.nn.utils.clip_grad_norm_ + the
matching torch optimizer, ComputeEngine / Node plumbing, checkpoints."""
import torch

from ravnest_amd import Node, set_seed
from ravnest_amd.engine.compute import ComputeEngine
from ravnest_amd.ops import FusedAdam, FusedLAMB, FusedSGD, clip_grad_norm_

ATOL, RTOL = 1e-5, 1e-4
SHAPES = [(64, 64), (3, 7, 11), (128,), (17,)]
# Adam is nearly invariant to a constant gradient scale; weight decay plus
# gradients whose size swings by 1e4 between steps make a dropped clip
# coefficient visible (see test_fused_adam_cpu_clip_matches_torch)
SCALES = [1.0, 100.0, 0.01, 1.0, 100.0, 0.01]
# Adam's step is lr * m / sqrt(v): where the clipped gradient and the
# weight-decay term cancel (g*coef + wd*p ~ 0) it turns an error of one
# fp32 ulp in the coefficient -- torch's own norm is no more exact than
# that -- into a parameter error of a few 1e-4 * lr per such element
# (measured by perturbing max_norm by 1-2 ulp: 2e-5..6e-5 at lr=1e-2 on
# the 65541-element tensor of the GPU test). lr=1e-3 keeps that below
# atol=1e-5 while the unclipped trajectory still differs by ~1e-2.
ADAM_LR = 1e-3


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in SHAPES]


def _grads(step):
    g = torch.Generator().manual_seed(1000 + step)
    return [torch.randn(*s, generator=g) * SCALES[step] for s in SHAPES]


def _run(make_opt, clip_with_torch=None, steps=len(SCALES)):
    ps = [p.clone().requires_grad_(True) for p in _params()]
    opt = make_opt(ps)
    for step in range(steps):
        for p, g in zip(ps, _grads(step)):
            p.grad = g.clone()
        if clip_with_torch is not None:
            torch.nn.utils.clip_grad_norm_(ps, clip_with_torch)
        opt.step()
    return [p.detach() for p in ps], opt


def _close(a, b, atol=ATOL, rtol=RTOL):
    return all(torch.allclose(x, y, atol=atol, rtol=rtol)
               for x, y in zip(a, b))


def test_fused_adam_cpu_clip_matches_torch():
    kw = dict(lr=ADAM_LR, weight_decay=0.01)
    ref, _ = _run(lambda ps: torch.optim.Adam(ps, **kw), clip_with_torch=1.0)
    got, opt = _run(lambda ps: FusedAdam(ps, max_grad_norm=1.0, **kw))
    assert _close(got, ref)
    # the construction must be able to fail: without the clip the
    # trajectory leaves the reference by far more than the tolerance
    unclipped, _ = _run(lambda ps: FusedAdam(ps, **kw))
    assert not _close(unclipped, ref, atol=10 * ATOL, rtol=10 * RTOL)
    # stats of the last step: norm before clipping and the coefficient
    last = torch.sqrt(sum((g.double() ** 2).sum()
                          for g in _grads(len(SCALES) - 1)))
    stats = opt.grad_norm_stats()
    assert torch.allclose(stats[0].double(), last, rtol=1e-5)
    assert float(stats[1]) == 1.0  # x0.01 grads: below max_norm
    assert float(stats[2]) == 0.0


def test_fused_sgd_cpu_clip_matches_torch():
    kw = dict(lr=0.01, momentum=0.9, weight_decay=5e-4)
    ref, _ = _run(lambda ps: torch.optim.SGD(ps, **kw), clip_with_torch=1.0)
    got, _ = _run(lambda ps: FusedSGD(ps, max_grad_norm=1.0, **kw))
    assert _close(got, ref)
    unclipped, _ = _run(lambda ps: FusedSGD(ps, **kw))
    assert not _close(unclipped, ref, atol=10 * ATOL, rtol=10 * RTOL)


def test_fused_lamb_cpu_clip_matches_preclipped():
    kw = dict(lr=1e-2, weight_decay=0.01)
    ref, _ = _run(lambda ps: FusedLAMB(ps, **kw), clip_with_torch=1.0)
    got, _ = _run(lambda ps: FusedLAMB(ps, max_grad_norm=1.0, **kw))
    assert _close(got, ref)


def test_fused_clip_leaves_grads_unclipped_and_state_dict_clean():
    ps = [p.clone().requires_grad_(True) for p in _params()]
    opt = FusedAdam(ps, lr=1e-2, max_grad_norm=1.0)
    gs = _grads(1)  # x100: certainly clipped
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    opt.step()
    for p, g in zip(ps, gs):
        assert torch.equal(p.grad, g)
    sd = opt.state_dict()
    assert "max_grad_norm" not in sd["param_groups"][0]
    # a state dict from a clipping optimizer loads into a plain one
    ps2 = [p.clone().requires_grad_(True) for p in _params()]
    opt2 = FusedAdam(ps2, lr=1e-2)
    opt2.load_state_dict(sd)
    assert opt2.max_grad_norm is None


def test_clip_spans_param_groups():
    kw = dict(lr=0.05)

    def groups(ps):
        return [{"params": ps[:2]}, {"params": ps[2:], "lr": 0.01}]

    ref, _ = _run(lambda ps: torch.optim.SGD(groups(ps), **kw),
                  clip_with_torch=1.0)
    got, _ = _run(lambda ps: FusedSGD(groups(ps), max_grad_norm=1.0, **kw))
    assert _close(got, ref)


def test_clip_grad_norm_cpu_matches_torch():
    ps = [p.clone().requires_grad_(True) for p in _params()]
    ps.append(torch.zeros(5, requires_grad=True))  # grad stays None
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    for p, q, g in zip(ps, qs, _grads(1)):
        p.grad = g.clone()
        q.grad = g.clone()
    n1 = clip_grad_norm_(ps, 0.5)
    n2 = torch.nn.utils.clip_grad_norm_(qs, 0.5)
    assert torch.allclose(n1, n2, rtol=1e-6)
    for p, q in zip(ps[:-1], qs[:-1]):
        assert torch.allclose(p.grad, q.grad, rtol=1e-6, atol=0)
    assert ps[-1].grad is None
    assert float(clip_grad_norm_([torch.zeros(3, requires_grad=True)],
                                 1.0)) == 0.0


# ---- ComputeEngine (tests/test_engine.py style) ----------------------
def small_model():
    return torch.nn.Sequential(
        torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 4))


def test_engine_clips_accumulated_grad_once_per_step():
    set_seed(0)
    m1 = small_model()
    set_seed(0)
    m2 = small_model()
    opt1 = torch.optim.SGD(m1.parameters(), lr=0.1)
    eng = ComputeEngine(m1, opt1, torch.device("cpu"), update_frequency=2,
                        max_grad_norm=0.5)
    opt2 = torch.optim.SGD(m2.parameters(), lr=0.1)
    assert eng.last_grad_norm() is None

    set_seed(42)
    xs = [torch.randn(4, 8) for _ in range(4)]
    gs = [torch.randn(4, 4) * 3 for _ in range(4)]
    norms = []
    for i, (x, g) in enumerate(zip(xs, gs)):
        eng.forward(i, [x], [False])
        _, stepped = eng.backward(i, {0: g}, speculative_next=False)
        assert stepped == (i % 2 == 1)
        # manual: accumulate two microbatches, clip ONCE, step
        m2(x).backward(g)
        if i % 2 == 1:
            norms.append(torch.nn.utils.clip_grad_norm_(m2.parameters(),
                                                        0.5))
            opt2.step()
            opt2.zero_grad(set_to_none=True)
            assert abs(eng.last_grad_norm() - float(norms[-1])) \
                <= 1e-6 * float(norms[-1])
    assert all(float(n) > 0.5 for n in norms)  # the clip really acted
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.allclose(p1, p2, atol=ATOL, rtol=RTOL)


def test_engine_hands_option_to_fused_optimizer():
    set_seed(0)
    m = small_model()
    opt = FusedSGD(m.parameters(), lr=0.1)
    eng = ComputeEngine(m, opt, torch.device("cpu"), max_grad_norm=0.25)
    assert opt.max_grad_norm == 0.25 and not eng._clip_external
    x, g = torch.randn(4, 8), torch.randn(4, 4) * 5
    eng.forward(0, [x], [False])
    eng.backward(0, {0: g}, speculative_next=False)
    set_seed(0)
    m2 = small_model()
    m2(x).backward(g)
    ref = torch.nn.utils.clip_grad_norm_(m2.parameters(), 0.25)
    assert abs(eng.last_grad_norm() - float(ref)) <= 1e-6 * float(ref)


# ---- Node + checkpoint (tests/test_aux.py style) ----------------------
def _mk_node(tmpdir, max_grad_norm):
    set_seed(0)
    model = small_model()
    cfg = {"rank": 0, "world_size": 1, "cluster_id": 0, "stage": 0,
           "n_stages": 1, "cluster_length": 1, "stage_ranks": [0],
           "dp_ranks": [0], "node_type": "root",
           "model_input_names": ["x"],
           "template_path": str(tmpdir) + "/"}
    labels = [(torch.randn(4, 8), torch.randn(4, 4) * 10) for _ in range(4)]
    return Node(config=cfg, model=model,
                input_template=[{"kind": "model_input", "name": "x",
                                 "dtype": "torch.float32",
                                 "shape": [4, 8]}],
                output_template={0: {"consumers": [], "final": True,
                                     "dtype": "torch.float32"}},
                optimizer=FusedAdam, optimizer_params={"lr": 1e-3},
                criterion=lambda p, t: torch.nn.functional.mse_loss(p, t[1]),
                labels=labels, device=torch.device("cpu"),
                loss_filename=str(tmpdir / "losses.txt"),
                max_grad_norm=max_grad_norm)


def test_node_passes_max_grad_norm_and_checkpoints_interchange(tmp_path):
    clipped = _mk_node(tmp_path, 0.1)
    plain = _mk_node(tmp_path, None)
    assert clipped.engine.max_grad_norm == 0.1
    assert clipped.optimizer.max_grad_norm == 0.1
    assert plain.engine.max_grad_norm is None
    assert plain.optimizer.max_grad_norm is None
    for node in (clipped, plain):
        node.start()
        for _ in range(2):
            node.forward_compute(tensors=torch.randn(4, 8))
        node.wait_for_backwards()
    assert clipped.engine.last_grad_norm() > 0.1
    assert plain.engine.last_grad_norm() is None
    ck_c = clipped.save_checkpoint(tmp_path / "clipped.pt")
    ck_p = plain.save_checkpoint(tmp_path / "plain.pt")
    want_c = [p.detach().clone() for p in clipped.model.parameters()]
    want_p = [p.detach().clone() for p in plain.model.parameters()]
    # with clipping -> without, and the other way round
    plain.load_checkpoint(ck_c)
    clipped.load_checkpoint(ck_p)
    for p, w in zip(plain.model.parameters(), want_c):
        assert torch.equal(p, w)
    for p, w in zip(clipped.model.parameters(), want_p):
        assert torch.equal(p, w)
    # the option is the node's, not the checkpoint's
    assert clipped.optimizer.max_grad_norm == 0.1
    assert plain.optimizer.max_grad_norm is None
    for node in (clipped, plain):
        node.forward_compute(tensors=torch.randn(4, 8))
        node.wait_for_backwards()
        node.stop()
