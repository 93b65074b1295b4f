"""MX fp8 backward of MXLinear: the transposing quantisers, the
split-contraction mx_gemm2 and the fp8_backward switch.

The quantisers are held bit for bit to mx_quant of the zero-padded
transpose and to the float64 reference quantiser; the GEMMs to the float64
product of the dequantised operands under the GEMM family's bound
(gemm_cases.gemm_ratio <= 1, depth = the contraction as the kernel sees it).
"""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
ZERO = {"s": 0, "q": 0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ext(dev):
    from ravnest_amd.ops import get_ext
    return get_ext(required=True)


def _pad(n):
    return max(256, -(-n // 128) * 128)


# ------------------------------------------------------- 1. quantisers
def _quant_case(R, C):
    """(R, C) whose 32-row column blocks span 2^-120..2^120, with the
    non-finite blocks of gemm_cases laid along the rows of 8 columns."""
    R32 = -(-R // 32) * 32
    xt = gc.wide_blocks(rows=C, kb=R32 // 32, seed=R + C)
    n, w = min(8, C), min(64, R32)
    xt[:n, :w] = gc.nonfinite_blocks()[:n, :w]
    return xt[:, :R].t().contiguous()


@pytest.mark.parametrize("op", ["mx_quant_t", "mx_quant_dual"])
@pytest.mark.parametrize("shape", [(32, 32), (130, 96), (257, 320), (33, 5)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_quant_t_exact(dev, ext, shape, op):
    R, C = shape
    if op == "mx_quant_dual" and C % 32:
        with pytest.raises(RuntimeError):
            ext.mx_quant_dual(torch.zeros(R, C, dtype=BF16, device=dev))
        return
    x = _quant_case(R, C)
    Rp = _pad(R)
    padt = torch.zeros(C, Rp, dtype=BF16)
    padt[:, :R] = x.t()
    out = getattr(ext, op)(x.to(dev))
    qt, st = out[-2:]
    assert qt.shape == (C, Rp) and st.shape == (C, Rp // 32)
    wq, ws = ext.mx_quant(padt.to(dev))
    assert torch.equal(qt, wq) and torch.equal(st, ws)
    assert gc.mx_quant_mismatches(qt.cpu(), st.cpu(), padt) == ZERO
    assert not bool(qt[:, R:].any()) and not bool(st[:, -(-R // 32):].any())
    if op == "mx_quant_dual":
        q, s = out[:2]
        q0, s0 = ext.mx_quant(x.to(dev))
        assert torch.equal(q, q0) and torch.equal(s, s0)
        assert gc.mx_quant_mismatches(q.cpu(), s.cpu(), x) == ZERO


# ------------------------------------------------------ 2. split GEMM
@pytest.mark.parametrize("n_split", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(70, 130, 1152), (257, 259, 512)],
                         ids=lambda s: "x".join(map(str, s)))
def test_splitk(dev, ext, shape, n_split):
    """9 K-tiles over 4 splits is the uneven case (3, 2, 2, 2). K = 512
    has 4 K-tiles: 3 or 4 splits would leave one tile to a split, which
    the op refuses."""
    M, N, K = shape
    xq, xs, xd = gc.mx_operand(M, K, 1)
    wq, ws, wd = gc.mx_operand(N, K, 2)
    ops = [t.to(dev) for t in (xq, xs, wq, ws)]
    if (K // 128) // n_split < 2:
        with pytest.raises(RuntimeError):
            ext.mx_gemm2_splitk(*ops, n_split)
        return
    got = ext.mx_gemm2_splitk(*ops, n_split)
    assert got.dtype == BF16 and got.shape == (M, N)
    ref, S = gc.gemm_reference(xd, wd)
    ratio = gc.gemm_ratio(got.cpu(), ref, S, depth=K)
    print(f"splitk {shape} n_split {n_split}: ratio {ratio:.3f}")
    assert ratio <= 1
    assert torch.equal(got, ext.mx_gemm2_splitk(*ops, n_split))
    if n_split == 1:
        assert torch.equal(got, ext.mx_gemm2(*ops))


def test_splitk_auto(dev, ext):
    """n_split=None: one output tile and 9 K-tiles give 4 splits."""
    ops = [t.to(dev) for t in (*gc.mx_operand(70, 1152, 1)[:2],
                               *gc.mx_operand(130, 1152, 2)[:2])]
    assert torch.equal(ext.mx_gemm2_splitk(*ops),
                       ext.mx_gemm2_splitk(*ops, 4))


# ------------------------------------------------------- 3. MXLinear
def _layer(dev, rows, fin, fout, fp8_backward):
    from ravnest_amd.ops import MXLinear
    g = torch.Generator().manual_seed(rows + fin + fout)
    lin = MXLinear(fin, fout, fp8_backward=fp8_backward).to(dev).to(BF16)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(fout, fin, generator=g) * 0.05)
        lin.bias.copy_(torch.randn(fout, generator=g))
    x = torch.randn(rows, fin, generator=g).to(BF16).to(dev).requires_grad_()
    dy = torch.randn(rows, fout, generator=g).to(BF16).to(dev)
    return lin, x, dy


def _grads(lin, x, dy):
    lin.zero_grad()
    x.grad = None
    lin(x).backward(dy)
    return x.grad, lin.weight.grad, lin.bias.grad


def _bf16_grads(lin, x, dy):
    """The bf16 backward as it has always been."""
    w, xd = lin.weight.detach(), x.detach()
    return dy @ w, dy.t() @ xd, dy.sum(0)


@pytest.mark.parametrize("shape", [(130, 256, 384), (64, 192, 320)],
                         ids=lambda s: "x".join(map(str, s)))
def test_mxlinear_fp8_backward(dev, ext, shape, monkeypatch):
    rows, fin, fout = shape
    lin, x, dy = _layer(dev, *shape, fp8_backward=True)
    dx, dw, db = _grads(lin, x, dy)
    assert dx.dtype == BF16 and dw.dtype == BF16
    dyq, dys, dyqt, dyst = (t.cpu() for t in ext.mx_quant_dual(dy))
    wqt, wst = (t.cpu() for t in ext.mx_quant_t(lin.weight.detach()))
    xqt, xst = (t.cpu() for t in ext.mx_quant_t(x.detach()))
    ref, S = gc.gemm_reference(gc.mx_dequant(dyq, dys),
                               gc.mx_dequant(wqt, wst)[:, :fout])
    r_dx = gc.gemm_ratio(dx.cpu(), ref, S, depth=_pad(fout))
    ref, S = gc.gemm_reference(gc.mx_dequant(dyqt, dyst),
                               gc.mx_dequant(xqt, xst))
    r_dw = gc.gemm_ratio(dw.cpu(), ref, S, depth=_pad(rows))
    print(f"fp8 backward {shape}: dx ratio {r_dx:.3f}, dw ratio {r_dw:.3f}")
    assert r_dx <= 1 and r_dw <= 1
    assert torch.equal(db, dy.sum(0))
    # fp8_backward=None follows the module switch
    from ravnest_amd.ops import mx
    lin.fp8_backward = None
    monkeypatch.setattr(mx, "FP8_BACKWARD", True)
    for a, b in zip(_grads(lin, x, dy), (dx, dw, db)):
        assert torch.equal(a, b)
    monkeypatch.setattr(mx, "FP8_BACKWARD", False)
    for a, b in zip(_grads(lin, x, dy), _bf16_grads(lin, x, dy)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape,flag", [((130, 256, 384), False),
                                        ((40, 128, 80), True)])
def test_mxlinear_bf16_backward_kept(dev, shape, flag):
    """Switch off, or an out_features the fp8 path does not serve: every
    gradient is today's bf16 backward bit for bit."""
    lin, x, dy = _layer(dev, *shape, fp8_backward=flag)
    for a, b in zip(_grads(lin, x, dy), _bf16_grads(lin, x, dy)):
        assert torch.equal(a, b)


# ----------------------------------------------------- 4. host checks
def test_host_checks(dev, ext):
    x = torch.zeros(64, 64, dtype=BF16, device=dev)
    for fn in (ext.mx_quant_t, ext.mx_quant_dual):
        with pytest.raises(RuntimeError):
            fn(x.t())                       # non-contiguous
        with pytest.raises(RuntimeError):
            fn(x.float())                   # wrong dtype
    with pytest.raises(RuntimeError):
        ext.mx_quant_dual(x[:, :48].contiguous())
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)  # noqa: E731
    ops = (z(64, 512), z(64, 16), z(64, 512), z(64, 16))
    ext.mx_gemm2_splitk(*ops, 2)
    for bad in (3, 0):
        with pytest.raises(RuntimeError):
            ext.mx_gemm2_splitk(*ops, bad)
    with pytest.raises(RuntimeError):
        ext.mx_gemm2_splitk(z(64, 512).t(), *ops[1:], 2)
