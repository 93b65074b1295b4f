"""FusedBatchNormReLU2d / FusedBatchNormAddReLU2d on the CPU: they compute
relu(batch_norm(x) [+ r]), keep FusedBatchNorm2d's state-dict keys, and are
wired into ResNet and Inception without losing, doubling or misrouting a
ReLU or a residual.
"""
import pytest
import torch
import torch.nn.functional as F

from ravnest_amd import set_seed
from ravnest_amd.models import resnet18_ish
from ravnest_amd.models.inception import BasicConv2d
from ravnest_amd.ops import (FusedBatchNorm2d, FusedBatchNormAddReLU2d,
                             FusedBatchNormReLU2d)
from ravnest_amd.planner.splitter import split_model_by_proportions

BN_KEYS = ["weight", "bias", "running_mean", "running_var",
           "num_batches_tracked"]


def _module(residual, C):
    cls = FusedBatchNormAddReLU2d if residual else FusedBatchNormReLU2d
    m = cls(C)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        m.weight.copy_(torch.rand(C, generator=g) + 0.5)
        m.bias.copy_(torch.randn(C, generator=g))
    return m


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_module_equals_torch(residual, training):
    N, C, H, W = 4, 3, 5, 7
    g = torch.Generator().manual_seed(0)
    m = _module(residual, C).train(training)
    w = m.weight.detach().clone().requires_grad_(True)
    b = m.bias.detach().clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    for _ in range(2):  # two steps: the running statistics accumulate
        x = 2 * torch.randn(N, C, H, W, generator=g) + 0.5
        r = torch.randn(N, C, H, W, generator=g)
        dy = torch.randn(N, C, H, W, generator=g)
        x1, x2 = (x.clone().requires_grad_(True) for _ in range(2))
        r1, r2 = (r.clone().requires_grad_(True) for _ in range(2))
        for t in (m.weight, m.bias, w, b):
            t.grad = None
        y1 = m(x1, r1) if residual else m(x1)
        y2 = F.batch_norm(x2, rm, rv, w, b, training, m.momentum, m.eps)
        y2 = F.relu(y2 + r2 if residual else y2)
        y1.backward(dy)
        y2.backward(dy)
        assert torch.equal(y1, y2)
        assert torch.equal(x1.grad, x2.grad)
        assert torch.equal(m.weight.grad, w.grad)
        assert torch.equal(m.bias.grad, b.grad)
        if residual:
            assert torch.equal(r1.grad, r2.grad)
        assert torch.equal(m.running_mean, rm)
        assert torch.equal(m.running_var, rv)
    if training:
        assert not torch.equal(m.running_mean, torch.zeros(C))
    assert (y1 == 0).any() and (y1 > 0).any()


@pytest.mark.parametrize("cls", [FusedBatchNormReLU2d,
                                 FusedBatchNormAddReLU2d])
def test_state_dict_is_batchnorms(cls):
    plain = FusedBatchNorm2d(6)
    with torch.no_grad():
        plain.weight.uniform_(0.5, 1.5)
        plain.bias.normal_()
        plain.running_mean.normal_()
        plain.running_var.uniform_(0.5, 2.0)
        plain.num_batches_tracked.fill_(7)
    m = cls(6)
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
    assert list(m.state_dict().keys()) == BN_KEYS
    m.load_state_dict(plain.state_dict(), strict=True)
    for k, v in plain.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert isinstance(m, FusedBatchNorm2d)
    assert m._is_leaf_module


def _bn(prefix):
    return [f"{prefix}.{k}" for k in BN_KEYS]


def test_model_state_dict_keys():
    expect = ["conv1.weight"] + _bn("bn1")
    for layer in ("layer1", "layer2", "layer3", "layer4"):
        p = f"{layer}.0"
        expect += ([f"{p}.conv1.weight"] + _bn(f"{p}.bn1")
                   + [f"{p}.conv2.weight"] + _bn(f"{p}.bn2")
                   + [f"{p}.conv3.weight"] + _bn(f"{p}.bn3")
                   + [f"{p}.downsample.0.weight"] + _bn(f"{p}.downsample.1"))
    expect += ["fc.weight", "fc.bias"]
    keys = list(resnet18_ish().state_dict().keys())
    assert not [k for k in keys if "relu" in k]
    assert keys == expect

    keys = list(BasicConv2d(3, 8, kernel_size=3, padding=1)
                .state_dict().keys())
    assert not [k for k in keys if "relu" in k]
    assert keys == ["conv.weight"] + _bn("bn")


def test_resnet_wiring_fused_equals_composed(monkeypatch):
    """The switch only selects the GPU path, so on the CPU both models run
    the same arithmetic; any difference would be a wiring mistake."""
    def run(switch):
        monkeypatch.setenv("RAVNEST_FUSED_BN_RELU", switch)
        set_seed(3)
        m = resnet18_ish()
        assert m.bn1.fused == (switch != "0")
        g = torch.Generator().manual_seed(4)
        x = torch.randn(4, 3, 32, 32, generator=g)
        logits = m(x)
        logits.square().sum().backward()
        return logits.detach(), {k: p.grad for k, p in m.named_parameters()}

    l1, g1 = run("1")
    l0, g0 = run("0")
    assert torch.equal(l1, l0)
    assert g1.keys() == g0.keys()
    for k in g1:
        assert g1[k] is not None and torch.equal(g1[k], g0[k]), k

    # against the block written out with plain torch ops
    set_seed(3)
    m = resnet18_ish().eval()
    blk = m.layer2[0]
    x = torch.randn(2, 256, 8, 8, generator=torch.Generator().manual_seed(5))

    def bn(mod, t):
        return F.batch_norm(t, mod.running_mean, mod.running_var, mod.weight,
                            mod.bias, False, mod.momentum, mod.eps)

    with torch.no_grad():
        out = F.relu(bn(blk.bn1, blk.conv1(x)))
        out = F.relu(bn(blk.bn2, blk.conv2(out)))
        out = bn(blk.bn3, blk.conv3(out))
        ref = F.relu(out + bn(blk.downsample[1], blk.downsample[0](x)))
        assert torch.equal(blk(x), ref)


def test_resnet_still_splits():
    set_seed(0)
    m = resnet18_ish().eval()
    x = torch.randn(2, 3, 32, 32)
    res = split_model_by_proportions(m, [0.5, 0.5], example_args=(x,))
    assert len(res.stages) == 2
    with torch.no_grad():
        ref = m(x)
        out = res.split_gm(x)
    assert torch.allclose(ref, out, atol=1e-6)
