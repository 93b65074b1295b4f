"""Bias gradients of the BERT attn.out and mlp_out projections out of the
dropout + LayerNorm backward that consumes their output
(dropout_add_ln_bwd_dzsum), and the model wiring. The qkv bias gradient was
built into the attention backward kernels as well and left out again: it
measured slower than the reduction it replaced (profiles/bias_grad_gelu.txt),
so there is no test of it here and the qkv bias must come out bit-equal.

Everything the fused calls share with the plain ones (dx, dz, dw, db, the
loss, every other gradient) must be bit-equal: the flag only adds a sum.

The sums are fp32 sums, in some order, of the bf16 values the kernel stores,
written once in the output dtype. Against the float64 column sum of the
RETURNED gradient the error of column c is therefore at most the fp32
summation bound n * 2^-24 * sum_r |g[r, c]| (n terms) plus one ulp of the
output dtype at |ref| for the final rounding.

Model: the two routes produce the same bf16 gradient tensors and differ only
in who sums them (at::sum in fp32 against the kernels' fp32 partials), so a
bias gradient may differ by one flipped bf16 rounding. The bound asserted is
2^-8 * max|ref| over the vector (the convention of test_dropout_ln_gpu), not
one ulp at each element's own magnitude: where a column's terms cancel, the
two fp32 summation orders differ by an amount that does not shrink with the
result, so a per-element ulp cannot hold for either route. The per-column
guard with the per-element bound is test_dropout_add_ln_bwd_dzsum above.

Shapes. LN: N = 1 and 5 leave waves of a block without rows; H = 8 and 128
leave lanes without columns; 776 is the ragged three-trip case; 768 and 1024
are the full three- and four-trip cases (dz sums in LDS rows), 2048 the
register one.
"""
import os

import pytest
import torch

SEED = 0x1D2C3B4A59687766  # < 2**62
EPS = 1e-5

LN_SHAPES = [(1, 768), (5, 768), (33, 8), (512, 128), (512, 776),
             (512, 1024), (1000, 2048)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


def _ulp(ref, dtype):
    """One unit in the last place of dtype at |ref| (0 at ref == 0)."""
    bits = 8 if dtype == torch.bfloat16 else 24
    _, e = torch.frexp(ref.abs())  # |ref| = m * 2^e, m in [0.5, 1)
    return torch.where(ref == 0, torch.zeros_like(ref),
                       torch.ldexp(torch.ones_like(ref), e - bits))


def _check_colsum(got, grad2d, what):
    """got against the float64 column sum of grad2d (n rows), with the
    bound of the module docstring."""
    g64 = grad2d.double()
    ref = g64.sum(0)
    n = grad2d.shape[0]
    bound = n * 2.0 ** -24 * g64.abs().sum(0) + _ulp(ref, got.dtype)
    err = (got.double() - ref).abs()
    worst = int(torch.argmax(err - bound))
    print(f"{what}: max err {float(err.max()):.3e}, at the worst column "
          f"err {float(err[worst]):.3e} bound {float(bound[worst]):.3e}")
    assert bool((err <= bound).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("wdt", ["float32", "bfloat16"])
@pytest.mark.parametrize("N,H", LN_SHAPES)
def test_dropout_add_ln_bwd_dzsum(dev, N, H, wdt, p):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    wdtype = getattr(torch, wdt)
    g = torch.Generator(device=dev).manual_seed(1000 * H + N)
    z, a, dy = (torch.randn(N, H, device=dev, generator=g).to(torch.bfloat16)
                for _ in range(3))
    w = torch.randn(H, device=dev, generator=g).to(wdtype)
    b = torch.randn(H, device=dev, generator=g).to(wdtype)
    _, s, mean, rstd, bits = ext.dropout_add_ln_fwd(z, a, w, b, EPS, p, SEED,
                                                    None)
    plain = ext.dropout_add_ln_bwd(dy, s, w, mean, rstd, bits, p)
    assert len(plain) == 4
    for as_bf16 in (False, True):
        out = ext.dropout_add_ln_bwd_dzsum(dy, s, w, mean, rstd, bits, p,
                                           as_bf16)
        assert len(out) == 5
        for name, x, y in zip(("dx", "dz", "dw", "db"), out, plain):
            assert x.dtype == y.dtype and torch.equal(x, y), name
        dzsum = out[4]
        assert dzsum.shape == (H,)
        assert dzsum.dtype == (torch.bfloat16 if as_bf16 else torch.float32)
        _check_colsum(dzsum, out[1], f"dzsum {dzsum.dtype}")


def _make_layer(switch, dropout, dev, state=None):
    from ravnest_amd.models.bert import BertConfig, BertLayer
    old = os.environ.get("RAVNEST_FUSED_BIAS_GRAD")
    os.environ["RAVNEST_FUSED_BIAS_GRAD"] = switch
    try:
        cfg = BertConfig.tiny(dropout=dropout)
        torch.manual_seed(0)
        layer = BertLayer(cfg)
    finally:
        if old is None:
            del os.environ["RAVNEST_FUSED_BIAS_GRAD"]
        else:
            os.environ["RAVNEST_FUSED_BIAS_GRAD"] = old
    for prm in layer.parameters():  # biases start at zero otherwise
        torch.nn.init.normal_(prm, std=0.05)
    layer = layer.to(dev).to(torch.bfloat16)
    if state is not None:
        layer.load_state_dict(state)
    return layer


def _step(layer, x0, mask, dev):
    from ravnest_amd.ops import rng
    rng.reset_seed_counter(dev)
    torch.manual_seed(99)  # the dropout seeds are drawn on the host
    layer.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    y = layer(x, mask)
    loss = (y.float() * torch.linspace(-1, 1, y.numel(), device=dev)
            .reshape(y.shape)).sum()
    loss.backward()
    grads = {n: p.grad for n, p in layer.named_parameters()}
    return loss.detach(), x.grad, grads


BIASES = ("attn.out.bias", "mlp_out.bias")  # fused; qkv is autograd's


@pytest.mark.gpu
def test_bert_layer_bias_grad_switch(dev):
    on = _make_layer("1", 0.1, dev)
    off = _make_layer("0", 0.1, dev, on.state_dict())
    assert on.fused_bias_grad and not off.fused_bias_grad
    g = torch.Generator(device=dev).manual_seed(5)
    x0 = torch.randn(2, 64, 128, device=dev, generator=g).to(torch.bfloat16)
    mask = torch.zeros(2, 1, 1, 64, device=dev)

    # training: the fused routes are taken (the Linear nodes see no bias)
    loss1, dx1, g1 = _step(on, x0, mask, dev)
    loss0, dx0, g0 = _step(off, x0, mask, dev)
    assert torch.equal(loss1, loss0)
    assert torch.equal(dx1, dx0)
    for name in g0:
        assert g1[name] is not None, name
        if name in BIASES:
            ref = g0[name].double()
            tol = 2.0 ** -8 * float(ref.abs().max())
            err = float((g1[name].double() - ref).abs().max())
            print(f"{name}: max diff {err:.3e}, one bf16 ulp {tol:.3e}")
            assert g1[name].dtype == g0[name].dtype
            assert err <= tol, name
            assert float(ref.abs().max()) > 0
        else:
            assert torch.equal(g1[name], g0[name]), name

    # eval, and p = 0 in training: today's path, which still yields them
    on.eval()
    off.eval()
    _, dxe1, ge1 = _step(on, x0, mask, dev)
    _, dxe0, ge0 = _step(off, x0, mask, dev)
    assert torch.equal(dxe1, dxe0)
    for name in BIASES + ("attn.qkv.bias",):  # composed LN path
        assert ge1[name] is not None and float(ge1[name].abs().max()) > 0
        assert torch.equal(ge1[name], ge0[name]), name
    p0 = _make_layer("1", 0.0, dev, on.state_dict())
    _, _, gp = _step(p0, x0, mask, dev)
    for name in BIASES + ("attn.qkv.bias",):
        assert gp[name] is not None and float(gp[name].abs().max()) > 0


def test_trace_unchanged_by_switch():
    """The pipeline splitter's trace keeps the projection module calls
    whatever the switch says (a stage boundary may fall between a projection
    and its consumer)."""
    from ravnest_amd.models import BertConfig, BertForMLM
    from ravnest_amd.planner.splitter import trace_model

    def nodes(switch):
        old = os.environ.get("RAVNEST_FUSED_BIAS_GRAD")
        os.environ["RAVNEST_FUSED_BIAS_GRAD"] = switch
        try:
            model = BertForMLM(BertConfig.tiny())
        finally:
            if old is None:
                del os.environ["RAVNEST_FUSED_BIAS_GRAD"]
            else:
                os.environ["RAVNEST_FUSED_BIAS_GRAD"] = old
        gm = trace_model(model)
        return [(n.op, str(n.target), tuple(str(a) for a in n.args),
                 tuple(sorted((k, str(v)) for k, v in n.kwargs.items())))
                for n in gm.graph.nodes]

    on, off = nodes("1"), nodes("0")
    assert on == off
    targets = [t for op, t, _, _ in on if op == "call_module"]
    for want in ("layers.0.attn.qkv", "layers.0.attn.out",
                 "layers.0.mlp_out"):
        assert want in targets
