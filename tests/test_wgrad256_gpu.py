"""gemm_wgrad256_bf16 (csrc/gemm_wgrad.hip): dW[N,K] = dy[M,N]^T @ x[M,K]
on 256x256 tiles with the reduction split over M, and the autograd function
that routes linear layers through it (ops/linear.py).

Bounds are gemm_cases.py's with M as the reduction length: the fp32 output
within e_acc = C_ACC * M * 2^-24 * (|dy|^T @ |x|), the bf16 output within
2^-8 |ref| + (1 + 2^-8) e_acc. db is an fp32 sum of M bf16 values per
column, in some fixed order, rounded once to bf16: within
M * 2^-24 * sum|dy| plus one bf16 rounding (2^-8 |ref|) of the reference.

Shapes (M, N, K): one tile with two M-tiles (two slices of one tile each);
an odd M-tile count (3 over 2 K-tiles: slices of 2 and 1... per tile); many
slices with uneven M-tiles per slice (64 M-tiles over 28 slices); 3 K-tiles
(the bias-gradient work is dealt over mt % 3); N wider than K.
"""
import pytest
import torch

import gemm_cases as gc

SHAPES = [(128, 256, 256), (192, 256, 512), (4096, 768, 768),
          (2048, 256, 768), (1024, 1024, 256)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_wgrad256_routing(dev, M, N, K):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    c = gc.wgrad_routing_case(M, N, K, dev)
    (dw32,) = ext.gemm_wgrad256_bf16(c["dy"], c["x"], False, True)
    assert dw32.dtype == torch.float32 and dw32.shape == (N, K)
    assert torch.equal(dw32, c["want"])
    dw16, db = ext.gemm_wgrad256_bf16(c["dy"], c["x"], True, False)
    assert dw16.dtype == torch.bfloat16 and db.dtype == torch.bfloat16
    assert gc.routing_mismatches(dw16, c["want"].to(gc.BF16)) == 0
    # one-hot per column: every column of dy sums to exactly 1
    assert torch.equal(db.float(), torch.ones(N, device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_wgrad256_random(dev, M, N, K):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    c = gc.wgrad_random_case(M, N, K)
    dy, x = c["dy"].to(dev), c["x"].to(dev)
    ref, S = gc.gemm_reference(dy.t(), x.t())   # [N, K], float64
    (dw32,) = ext.gemm_wgrad256_bf16(dy, x, False, True)
    dw16, db = ext.gemm_wgrad256_bf16(dy, x, True, False)
    r32 = gc.gemm_ratio(dw32, ref, S, M, bf16_out=False)
    r16 = gc.gemm_ratio(dw16, ref, S, M, bf16_out=True)
    dyd = dy.double()
    dref = dyd.sum(0)
    dbound = M * gc.U32 * dyd.abs().sum(0) + gc.BF16_U * dref.abs()
    rdb = gc._ratio((db.double() - dref).abs(), dbound)
    print(f"wgrad256 {M}x{N}x{K}: fp32 {r32:.4f} bf16 {r16:.4f} "
          f"db {rdb:.4f} of the bound")
    assert r32 <= 1.0
    assert r16 <= 1.0
    assert rdb <= 1.0
    # a pure function of its inputs: a second call is bit-equal
    dw16b, dbb = ext.gemm_wgrad256_bf16(dy, x, True, False)
    (dw32b,) = ext.gemm_wgrad256_bf16(dy, x, False, True)
    assert torch.equal(dw16.view(torch.int16), dw16b.view(torch.int16))
    assert torch.equal(db.view(torch.int16), dbb.view(torch.int16))
    assert torch.equal(dw32, dw32b)
    # with and without the bias gradient: the same dW
    (dw16c,) = ext.gemm_wgrad256_bf16(dy, x, False, False)
    assert torch.equal(dw16.view(torch.int16), dw16c.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(128, 264, 256), (128, 256, 128),
                                   (100, 256, 256)])
def test_wgrad256_rejects(dev, M, N, K):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    dy = torch.zeros(M, N, dtype=gc.BF16, device=dev)
    x = torch.zeros(M, K, dtype=gc.BF16, device=dev)
    with pytest.raises(RuntimeError):
        ext.gemm_wgrad256_bf16(dy, x, False, False)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
def test_wgrad256_autograd(dev, bias):
    """The routed function against nn.Linear's own backward at
    (M, N, K) = (256, 256, 512): dx is the same library call, dW and db
    are within the kernel's bounds of the float64 reference and within
    one bf16 rounding of autograd's."""
    from ravnest_amd.ops.linear import WgradLinear, _wgrad256_applies
    M, N, K = 256, 256, 512
    g = torch.Generator().manual_seed(11)
    ref_lin = torch.nn.Linear(K, N, bias=bias)
    lin = WgradLinear(K, N, bias=bias)
    lin.load_state_dict(ref_lin.state_dict())
    ref_lin = ref_lin.to(dev).to(gc.BF16)
    lin = lin.to(dev).to(gc.BF16)
    x0 = torch.randn(4, 64, K, generator=g).to(gc.BF16).to(dev)
    dy = (torch.randn(4, 64, N, generator=g) / 16).to(gc.BF16).to(dev)
    assert _wgrad256_applies(x0, lin.weight)
    out = {}
    for name, m in (("ref", ref_lin), ("new", lin)):
        x = x0.clone().requires_grad_(True)
        y = m(x)
        y.backward(dy)
        out[name] = (y.detach(), x.grad, m.weight.grad,
                     m.bias.grad if bias else None)
    assert torch.equal(out["new"][0], out["ref"][0])
    assert torch.equal(out["new"][1], out["ref"][1])       # dx bit-equal
    dy2, x2 = dy.reshape(-1, N), x0.reshape(-1, K)
    ref, S = gc.gemm_reference(dy2.t(), x2.t())
    r = gc.gemm_ratio(out["new"][2], ref, S, M, bf16_out=True)
    print(f"autograd dW: {r:.4f} of the bound")
    assert out["new"][2].dtype == gc.BF16 and r <= 1.0
    if bias:
        dref = dy2.double().sum(0)
        dbound = M * gc.U32 * dy2.double().abs().sum(0) + \
            gc.BF16_U * dref.abs()
        rdb = gc._ratio((out["new"][3].double() - dref).abs(), dbound)
        print(f"autograd db: {rdb:.4f} of the bound")
        assert out["new"][3].dtype == gc.BF16 and rdb <= 1.0
