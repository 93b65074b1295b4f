"""Routing of linear layers through the 256x256 wgrad kernel
(ops/linear.py): the shape predicate, the fall-back where it refuses, the
modules make_linear builds and the BERT bias-downstream wiring. No GPU."""
import os

import pytest
import torch


def _with_env(name, value, fn):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def test_shape_predicate():
    from ravnest_amd.ops.linear import wgrad256_shape_ok
    M = 65536
    for N, K in [(2304, 768), (768, 768), (3072, 768), (768, 3072)]:
        assert wgrad256_shape_ok(M, N, K), (N, K)
    assert wgrad256_shape_ok(128, 256, 256)
    assert wgrad256_shape_ok(192, 256, 512)
    assert not wgrad256_shape_ok(M, 264, 768)      # ragged N
    assert not wgrad256_shape_ok(M, 768, 128)      # ragged K
    assert not wgrad256_shape_ok(M, 30522, 768)    # the MLM decoder
    assert not wgrad256_shape_ok(100, 256, 256)    # M % 64
    assert not wgrad256_shape_ok(64, 256, 256)     # one M-tile only
    assert not wgrad256_shape_ok(0, 256, 256)


@pytest.mark.parametrize("M,N,K", [(128, 256, 256), (100, 264, 128)])
def test_fallback_is_autograds_product(M, N, K):
    """On CPU tensors (and on refused shapes) wgrad256() is dy^T @ x and
    dy.sum(0), bit for bit."""
    from ravnest_amd.ops.linear import wgrad256
    g = torch.Generator().manual_seed(M + N)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    dw, db = wgrad256(dy, x, True)
    assert torch.equal(dw, dy.t() @ x)
    assert torch.equal(db, dy.sum(0))
    dw, db = wgrad256(dy, x, False)
    assert torch.equal(dw, dy.t() @ x) and db is None


def test_linear_on_cpu_is_f_linear():
    from ravnest_amd.ops.linear import (WgradLinear, _wgrad256_applies,
                                        linear)
    lin = WgradLinear(256, 256)
    x = torch.randn(2, 64, 256, requires_grad=True)
    assert not _wgrad256_applies(x, lin.weight)
    assert not _wgrad256_applies(x.to(torch.bfloat16),
                                 lin.weight.to(torch.bfloat16))  # CPU
    y = lin(x)
    assert torch.equal(y, torch.nn.functional.linear(x, lin.weight,
                                                     lin.bias))
    assert "Wgrad256" not in type(y.grad_fn).__name__
    assert torch.equal(linear(x, lin.weight), x @ lin.weight.t())


def test_make_linear_modules_and_keys():
    from ravnest_amd.ops.linear import WgradLinear, make_linear
    on = _with_env("RAVNEST_HAND_WGRAD", None,
                   lambda: make_linear(768, 2304))
    off = _with_env("RAVNEST_HAND_WGRAD", "0",
                    lambda: make_linear(768, 2304))
    ref = torch.nn.Linear(768, 2304)
    assert type(on) is WgradLinear and isinstance(on, torch.nn.Linear)
    assert type(off) is torch.nn.Linear          # today's module
    assert list(on.state_dict()) == list(ref.state_dict()) \
        == list(off.state_dict())
    for k, v in ref.state_dict().items():
        assert on.state_dict()[k].shape == v.shape
    nb = _with_env("RAVNEST_HAND_WGRAD", None,
                   lambda: make_linear(768, 768, bias=False))
    assert list(nb.state_dict()) == ["weight"] and nb.bias is None


def test_bert_layer_keeps_bias_downstream():
    from ravnest_amd.models import bert
    from ravnest_amd.models.bert import BertConfig, BertLayer
    from ravnest_amd.ops.linear import WgradLinear
    for switch, kind in ((None, WgradLinear), ("0", torch.nn.Linear)):
        layer = _with_env("RAVNEST_HAND_WGRAD", switch,
                          lambda: BertLayer(BertConfig.tiny()))
        for lin in (layer.attn.qkv, layer.attn.out, layer.mlp_out):
            assert type(lin) is kind
        assert bert._plain_biased_linear(layer.attn.out)
        assert bert._plain_biased_linear(layer.mlp_out)
        # the detached-bias projection computes what lin computes and
        # leaves the bias without a gradient
        x = torch.randn(2, 8, 128, requires_grad=True)
        z = bert._linear_bias_downstream(layer.attn.out, x)
        assert torch.equal(z, layer.attn.out(x))
        z.sum().backward()
        assert layer.attn.out.bias.grad is None
        assert layer.attn.out.weight.grad is not None
    nb = torch.nn.Linear(8, 8, bias=False)
    assert not bert._plain_biased_linear(nb)


def test_state_dict_keys_of_the_model_do_not_depend_on_the_switch():
    from ravnest_amd.models import BertConfig, BertForMLM
    on = _with_env("RAVNEST_HAND_WGRAD", None,
                   lambda: BertForMLM(BertConfig.tiny()))
    off = _with_env("RAVNEST_HAND_WGRAD", "0",
                    lambda: BertForMLM(BertConfig.tiny()))
    assert list(on.state_dict()) == list(off.state_dict())
