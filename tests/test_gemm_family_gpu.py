"""Bias-GELU and the GEMM family, element-wise against float64.

test_kernels_gpu.py runs these kernels at one or two friendly shapes and
asserts max|err| / max|ref| < 3e-2, which a wrong element or a dropped k
term passes. Here every element is held to a bound built from the number
formats (tests/gemm_cases.py; test_gemm_family_cpu.py proves torch's fp32
ops keep a factor 4 of room), the pre-activations cover [-40, 40] and the
overflow thresholds of exp, the GEMM shapes cover every tile path (K = 128,
M < 256, N < 4, odd N, more than one column tile per block, device row
limits), and one-hot operands check the routing of every element bit for
bit. Every test prints error / bound per quantity.

All marked @pytest.mark.gpu.
"""
import math

import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ext(dev):
    from ravnest_amd.ops import get_ext
    return get_ext(required=True)


def _assert_within(ratios, what):
    print(f"{what}: error/bound " +
          ", ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}  # NaN is bad
    assert not bad, (what, bad)


# ------------------------------------------------------------------ GELU
@pytest.mark.parametrize("dt,with_bias", gc.GELU_VARIANTS,
                         ids=[f"{d}-{'bias' if w else 'nobias'}"
                              for d, w in gc.GELU_VARIANTS])
@pytest.mark.parametrize("shape", gc.GELU_SHAPES +
                         [(r, gc.GELU_DB_H) for r in gc.GELU_DB_ROWS])
def test_gelu_elementwise(dev, ext, shape, dt, with_bias):
    """bias_gelu() / gelu() forward and backward (bias_gelu_fwd,
    bias_gelu_bwd_db for bf16, bias_gelu_bwd otherwise) over pre-activations
    in [-40, 40] plus +-1e4: y, dx, db within the bounds, finite (exp(2a)
    overflows from a pre-activation of 10.06 on), and dx exactly 0 or dy
    in the saturated tails. bf16 with H % 8 != 0 is the scalar path: a
    vector of 8 would straddle a row end and run past the bias."""
    xdt, bdt = gc.GELU_DTYPES[dt]
    case = gc.gelu_case(*shape, xdt, bdt, with_bias)
    ref = gc.gelu_reference(case)
    got = gc.gelu_run(case, dev)
    r = gc.gelu_ratios(got, case, ref)
    if with_bias:
        # bias_gelu_bwd on its own (bf16 autograd goes through bwd_db)
        dx = ext.bias_gelu_bwd(case["dy"].to(dev), case["x"].to(dev),
                               case["b"].to(dev))
        r2 = gc.gelu_ratios({"dx": dx}, case, ref)
        r["bwd.dx"], r["bwd.exact"] = r2["dx"], r2["exact"]
    _assert_within(r, f"gelu {shape} {dt} bias={with_bias}")


def test_gelu_host_checks(dev, ext):
    x = torch.randn(4, 16, device=dev)
    b = torch.zeros(16, device=dev)
    xb, bb = x.to(BF16), b.to(BF16)
    with pytest.raises(RuntimeError):
        ext.bias_gelu_fwd(x.double(), b.double())
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd(x.double(), x.double(), b.double())
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd(x, xb, b)              # dy fp32, x bf16
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd(xb, x, b)              # dy bf16, x fp32
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd(x, x, bb)              # bf16 bias under fp32 x
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd(x, x, b[:8])
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd(xb, xb, torch.zeros(32, device=dev))
    with pytest.raises(RuntimeError):
        ext.bias_gelu_fwd(xb, bb[:8])
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd_db(xb, xb, bb[:8])
    with pytest.raises(RuntimeError):
        ext.bias_gelu_bwd_db(xb[:2], xb, bb)
    torch.cuda.synchronize()


def test_gemm_gelu_epilogue(dev, ext):
    """gemm_nt_bf16(a, b, bias, 2) at (64, 128, 72), pre-activations over
    [-30, 30] (the epilogue's exp overflows from 9.96 on): h under the GEMM
    bound, y under that plus 1.13 bound_h plus the fp32 GELU bound. Then
    _HandLinearGeluFn's backward on the kernel's own h: dh and db from
    bias_gelu_bwd_db under the GELU bounds, and dx = dh @ W, dW = dh^T @ a
    under the GEMM bound plus the dh bound carried through the product."""
    from ravnest_amd.ops.linear import _HandLinearGeluFn
    case = gc.fused_gelu_case()
    a, b, bias = (case[k].to(dev) for k in ("a", "b", "bias"))
    y, h = ext.gemm_nt_bf16(a, b, bias, 2)
    r = gc.fused_gelu_ratios(y, h, case)
    span = h.float()
    assert float(span.min()) < -29 and float(span.max()) > 29
    gcase = {"x": h.cpu(), "b": None, "dy": case["dy"]}
    gref = gc.gelu_reference(gcase)
    gb = gc.gelu_bounds(gcase, gref)
    dy = case["dy"].to(dev)
    dh, _ = ext.bias_gelu_bwd_db(dy, h, torch.zeros_like(bias))
    rg = gc.gelu_ratios({"dx": dh}, gcase, gref)
    r["dh"], r["dh.exact"] = rg["dx"], rg["exact"]
    al, wl, bl = (t.clone().requires_grad_() for t in (a, b, bias))
    out = _HandLinearGeluFn.apply(al, wl, bl)
    assert torch.equal(out, y)
    out.backward(dy)
    bdb = gb["db"] + gc.BF16_U * gref["db"].abs()      # db comes back as bf16
    r["db"] = gc._ratio((bl.grad.double().cpu() - gref["db"]).abs(), bdb)
    dhr, E = gref["dx"], gb["dx"]                      # (M, N) each
    ad, wd = case["a"].double(), case["b"].double()
    M, N = dhr.shape
    ref_dx, S_dx = dhr @ wd, dhr.abs() @ wd.abs()
    r["dx"] = gc._ratio((al.grad.double().cpu() - ref_dx).abs(),
                        gc.gemm_bound(ref_dx, S_dx, N) + E @ wd.abs())
    ref_dw, S_dw = dhr.t() @ ad, dhr.abs().t() @ ad.abs()
    r["dW"] = gc._ratio((wl.grad.double().cpu() - ref_dw).abs(),
                        gc.gemm_bound(ref_dw, S_dw, M) + E.t() @ ad.abs())
    _assert_within(r, "gemm + gelu epilogue (64, 128, 72)")


# ------------------------------------------------------------ bf16 GEMMs
def _library(a, b, ref, S, K, tag):
    """torch's matmuls of the same operands, the yardstick for C_ACC.
    The bf16 product under the full bound is printed, not asserted: its
    final rounding alone reaches the 2^-8 |ref| term (up to 0.98, the same
    as the kernel under test), which no C_ACC changes. What C_ACC governs
    is the accumulation, and that is held to 1/2: `2*lib32.*` is twice the
    fp32 product's error / e_acc at C_ACC = 2 (measured <= 0.02)."""
    ref, S = ref.to(a.device), S.to(a.device)
    print(f"torch bf16 matmul {tag}: error/bound "
          f"{gc.gemm_ratio(a @ b.t(), ref, S, K):.3g}")
    lib32 = a.float() @ b.float().t()
    return {"2*lib32." + tag: 2.0 * gc.gemm_ratio(lib32, ref, S, K, False)}


def _routing(ext, dev, M, K, N, bias):
    c = gc.routing_case(M, K, N, dev, bias)
    (y,) = ext.gemm_nt_bf16(c["a"], c["b"], c["bias"], 1 if bias else 0)
    return gc.routing_mismatches(y, c["want"])


@pytest.mark.parametrize("bias", [False, True], ids=["epi0", "epi1"])
@pytest.mark.parametrize("shape", gc.GEMM_SHAPES)
def test_gemm_nt_small(dev, ext, shape, bias):
    """Routing probe (bit for bit) and random / cancelling operands under
    the per-element bound, next to torch's own matmuls (see _library)."""
    M, K, N = shape
    assert _routing(ext, dev, M, K, N, bias) == 0
    r = {}
    for cancel in (False, True):
        case = gc.gemm_random_case(M, K, N, bias, cancel)
        ref, S = gc.gemm_reference(case["a"], case["b"], case["bias"])
        a, b = case["a"].to(dev), case["b"].to(dev)
        bv = case["bias"].to(dev) if bias else None
        (y,) = ext.gemm_nt_bf16(a, b, bv, 1 if bias else 0)
        tag = "cancel" if cancel else "randn"
        r[tag] = gc.gemm_ratio(y.cpu(), ref, S, K)
        r.update(_library(a, b, *gc.gemm_reference(case["a"], case["b"]),
                          K, tag))
    _assert_within(r, f"gemm_nt {shape} bias={bias}")


@pytest.mark.parametrize("shape", gc.GEMM_SHAPES_LARGE)
def test_gemm_nt_multi_column_tile(dev, ext, shape):
    """tpb = 2 (ragged last row tile, ragged second column tile) and
    tpb = 3 (odd K-tile count: the LDS buffer parity flips between column
    tiles): the routing probe on every element, random and cancelling
    operands on the rows of the first and last row tile plus 4096 others
    (float64 product on the GPU), each with both epilogues."""
    M, K, N = shape
    rows = gc.sample_rows(M, dev)
    r = {}
    for bias in (False, True):
        assert _routing(ext, dev, M, K, N, bias) == 0
        for cancel in (False, True):
            c = gc.gemm_random_case(M, K, N, bias, cancel, device=dev)
            a, b, bv = c["a"], c["b"], c["bias"]
            ref, S = gc.gemm_reference(a[rows], b, bv)
            (y,) = ext.gemm_nt_bf16(a, b, bv, int(bias))
            tag = f"epi{int(bias)}." + ("cancel" if cancel else "randn")
            r[tag] = gc.gemm_ratio(y[rows], ref, S, K)
            if not bias:
                r.update(_library(a[rows], b, ref, S, K, tag))
    _assert_within(r, f"gemm_nt {shape}")


def _sentinel_c(rows, width, dev):
    return torch.full((rows, width), gc.SENTINEL, dtype=torch.int16,
                      device=dev).view(BF16)


def _untouched(c):
    return bool((c.view(torch.int16) == gc.SENTINEL).all())


@pytest.mark.parametrize("limit", gc.GEMM_ROWS_LIMITS)
def test_gemm_nt_rows(dev, ext, limit):
    """gemm_nt_bf16_rows into a sentinel-filled C of width 264: rows below
    the device limit satisfy the routing probe and the bound, rows from the
    limit on and the pad columns keep the sentinel bits."""
    M, K, N, W = gc.GEMM_ROWS_SHAPE
    live = min(max(limit, 0), M)
    lim = torch.tensor([limit], dtype=torch.int32, device=dev)
    r = {}
    for bias in (False, True):
        c = gc.routing_case(M, K, N, dev, bias)
        C = _sentinel_c(M, W, dev)
        ext.gemm_nt_bf16_rows(c["a"], c["b"], c["bias"], int(bias), C, lim)
        assert gc.routing_mismatches(C[:live, :N], c["want"][:live]) == 0
        assert _untouched(C[live:]) and _untouched(C[:, N:])
        case = gc.gemm_random_case(M, K, N, bias)
        ref, S = gc.gemm_reference(case["a"], case["b"], case["bias"])
        C = _sentinel_c(M, W, dev)
        ext.gemm_nt_bf16_rows(case["a"].to(dev), case["b"].to(dev),
                              case["bias"].to(dev) if bias else None,
                              int(bias), C, lim)
        assert _untouched(C[live:]) and _untouched(C[:, N:])
        r[f"epi{int(bias)}"] = gc.gemm_ratio(C[:live, :N].cpu(), ref[:live],
                                             S[:live], K)
    _assert_within(r, f"gemm_nt_rows limit={limit}")


def test_gemm_nt_rows_benchmark_geometry(dev, ext):
    """(131072, 128, 826) under a row limit of 15 %: four column tiles per
    block with a device row limit, the sparse MLM head's configuration."""
    M, K, N, limit = gc.GEMM_ROWS_LARGE
    lim = torch.tensor([limit], dtype=torch.int32, device=dev)
    c = gc.routing_case(M, K, N, dev, True)
    C = _sentinel_c(M, N, dev)
    ext.gemm_nt_bf16_rows(c["a"], c["b"], c["bias"], 1, C, lim)
    assert gc.routing_mismatches(C[:limit], c["want"][:limit]) == 0
    assert _untouched(C[limit:])


@pytest.mark.parametrize("shape", gc.WGRAD_SHAPES)
def test_gemm_wgrad(dev, ext, shape):
    M, N, K = shape
    c = gc.wgrad_routing_case(M, N, K, dev)
    dw = ext.gemm_wgrad_bf16(c["dy"], c["x"])
    assert dw.dtype == torch.float32 and torch.equal(dw, c["want"])
    case = gc.wgrad_random_case(M, N, K)
    ref, S = gc.gemm_reference(case["dy"].t(), case["x"].t())
    dy, x = case["dy"].to(dev), case["x"].to(dev)
    r = {"dW": gc.gemm_ratio(ext.gemm_wgrad_bf16(dy, x).cpu(), ref, S, M,
                             False)}
    r.update(_library(dy.t().contiguous(), x.t().contiguous(), ref, S, M,
                      "dW"))
    _assert_within(r, f"gemm_wgrad {shape}")


def test_gemm_wgrad_rejects_odd(dev, ext):
    M, N, K = gc.WGRAD_REJECTED
    dy = torch.zeros(M, N, dtype=BF16, device=dev)
    x = torch.zeros(M, K, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        ext.gemm_wgrad_bf16(dy, x)
    with pytest.raises(RuntimeError):
        ext.gemm_wgrad_bf16(dy[:, :128].contiguous(), x)   # odd K alone
    with pytest.raises(RuntimeError):
        ext.gemm_wgrad_bf16(dy, x[:, :126].contiguous())   # odd N alone
    torch.cuda.synchronize()


@pytest.mark.parametrize("bound", gc.WGRAD_ROWS_BOUNDS)
def test_gemm_wgrad_rows(dev, ext, bound):
    """gemm_wgrad_bf16_rows sums rows [0, round_up(min(bound, M), 64)).
    dy is zero in [bound, round_up), as the contract asks, and non-zero
    from round_up on: a kernel that ignored the bound would add those."""
    M, N, K = gc.WGRAD_ROWS_SHAPE
    live = min(max(bound, 0), M)
    top = min((live + 63) // 64 * 64, M)
    bnd = torch.tensor([bound], dtype=torch.int32, device=dev)
    c = gc.wgrad_routing_case(M, N, K, dev)
    dy = c["dy"].clone()
    dy[live:top] = 0
    want = dy[:top].float().t() @ c["x"][:top].float()     # exact
    full = dy.float().t() @ c["x"].float()
    assert top == M or not torch.equal(full, want)     # the tail counts
    assert torch.equal(ext.gemm_wgrad_bf16_rows(dy, c["x"], bnd), want)
    case = gc.wgrad_random_case(M, N, K)
    case["dy"][live:top] = 0
    ref, S = gc.gemm_reference(case["dy"][:top].t(), case["x"][:top].t())
    got = ext.gemm_wgrad_bf16_rows(case["dy"].to(dev), case["x"].to(dev),
                                   bnd)
    _assert_within({"dW": gc.gemm_ratio(got.cpu(), ref, S, max(top, 1),
                                        False)},
                   f"gemm_wgrad_rows bound={bound}")


# ---------------------------------------------------------------- MX fp8
@pytest.mark.parametrize("which", ["all_finite_bf16",
                                   "bf16_under_fixed_amax", "wide_blocks",
                                   "nonfinite_blocks"])
def test_mx_quant_exact(dev, ext, which):
    """Scale exponent and e4m3 bytes bit for bit: every finite bf16 value
    alone in its block and under a fixed amax, blocks from 2^-120 to
    2^120, and blocks with NaN / +-inf (0x7F, scale from the finite
    elements). The fixed amax is what reaches e4m3's subnormals and the
    round-up from 0x07 to 0x08 just below 2^-6."""
    x = getattr(gc, which)()
    q, s = ext.mx_quant(x.to(dev))
    bad = gc.mx_quant_mismatches(q.cpu(), s.cpu(), x)
    print(f"mx_quant {which}: mismatches {bad} of {x.numel()} elements")
    assert bad == {"s": 0, "q": 0}


@pytest.mark.parametrize("K", [192, 256], ids=["mx_gemm", "mx_gemm2"])
def test_mx_linear_keeps_nonfinite(dev, K):
    """An output element whose float64 reference is non-finite is
    non-finite; the other rows stay finite."""
    from ravnest_amd.ops.mx import mx_linear
    g = torch.Generator().manual_seed(K)
    x = torch.randn(6, K, generator=g).to(BF16)
    w = torch.randn(70, K, generator=g).to(BF16)
    x[1, 7] = math.inf
    x[2, 100] = math.nan
    x[4, K - 1] = -math.inf
    ref = x.double() @ w.double().t()
    y = mx_linear(x.to(dev), w.to(dev)).cpu()
    assert not bool(torch.isfinite(ref[[1, 2, 4]]).any())
    assert not bool(torch.isfinite(y[~torch.isfinite(ref)]).any())
    assert bool(torch.isfinite(y[[0, 3, 5]]).all())


def _mx_check(fn, dev, M, K, N):
    xq, xs, xd = gc.mx_operand(M, K, 1)
    wq, ws, wd = gc.mx_operand(N, K, 2)
    ref, S = xd @ wd.t(), xd.abs() @ wd.abs().t()
    y = fn(xq.to(dev), xs.to(dev), wq.to(dev), ws.to(dev))
    lib = (xd.float().to(dev) @ wd.float().to(dev).t()).cpu()
    r = {"y": gc.gemm_ratio(y.cpu(), ref, S, K),
         "2*lib": 2.0 * gc.gemm_ratio(lib, ref, S, K, False)}
    c = gc.mx_routing_case(M, K, N, dev)
    got = fn(c["xq"], c["xs"], c["wq"], c["ws"])
    assert gc.routing_mismatches(got, c["want"]) == 0
    return r, y.cpu(), gc.gemm_bound(ref, S, K)


@pytest.mark.parametrize("shape", gc.MX_GEMM_SHAPES)
def test_mx_gemm(dev, ext, shape):
    """Block exponents drawn per (row, k-block) from [-12, 12]: a kernel
    reading another row's or block's scale is off by powers of two."""
    r, _, _ = _mx_check(ext.mx_gemm, dev, *shape)
    _assert_within(r, f"mx_gemm {shape}")


@pytest.mark.parametrize("shape", gc.MX_GEMM2_SHAPES)
def test_mx_gemm2(dev, ext, shape):
    r, y2, bound = _mx_check(ext.mx_gemm2, dev, *shape)
    M, K, N = shape
    xq, xs, _ = gc.mx_operand(M, K, 1)
    wq, ws, _ = gc.mx_operand(N, K, 2)
    y1 = ext.mx_gemm(xq.to(dev), xs.to(dev), wq.to(dev), ws.to(dev)).cpu()
    r["gemm2-gemm"] = gc._ratio((y2.double() - y1.double()).abs(), 2 * bound)
    _assert_within(r, f"mx_gemm2 {shape}")


def test_mx_gemm2_multi_column_tile(dev, ext):
    """(130817, 256, 259): two column tiles per block, ragged in M and N.
    Routing probe on every element, through mx_gemm as well; random
    operands on sampled rows, where mx_gemm2 and mx_gemm also have to
    agree to within the two bounds."""
    M, K, N = gc.MX_GEMM2_LARGE
    c = gc.mx_routing_case(M, K, N, dev)
    for fn in (ext.mx_gemm2, ext.mx_gemm):
        got = fn(c["xq"], c["xs"], c["wq"], c["ws"])
        assert gc.routing_mismatches(got, c["want"]) == 0
    xq, xs, xd = gc.mx_operand(M, K, 1, dev)
    wq, ws, wd = gc.mx_operand(N, K, 2, dev)
    y2 = ext.mx_gemm2(xq, xs, wq, ws)
    y1 = ext.mx_gemm(xq, xs, wq, ws)
    rows = gc.sample_rows(M, dev)
    ref, S = xd[rows] @ wd.t(), xd[rows].abs() @ wd.abs().t()
    bound = gc.gemm_bound(ref, S, K)
    d = (y2[rows].double() - y1[rows].double()).abs()
    _assert_within({"rows": gc.gemm_ratio(y2[rows], ref, S, K),
                    "mx_gemm.rows": gc.gemm_ratio(y1[rows], ref, S, K),
                    "gemm2-gemm": gc._ratio(d, 2 * bound)},
                   f"mx_gemm2 {gc.MX_GEMM2_LARGE}")


@pytest.mark.parametrize("name", ["mx_gemm", "mx_gemm2"])
def test_mx_gemm_host_checks(dev, ext, name):
    fn = getattr(ext, name)
    M, K, N = 64, 256, 64
    xq = torch.zeros(M, K, dtype=torch.uint8, device=dev)
    wq = torch.zeros(N, K, dtype=torch.uint8, device=dev)
    xs = torch.full((M, K // 32), 127, dtype=torch.uint8, device=dev)
    ws = torch.full((N, K // 32), 127, dtype=torch.uint8, device=dev)
    assert float(fn(xq, xs, wq, ws).float().abs().max()) == 0.0
    bad = [
        (xq, xs.to(torch.int32), wq, ws),            # scale dtype
        (xq, xs, wq, ws.to(torch.int8)),
        (xq, xs[:, :4].contiguous(), wq, ws),        # scale size
        (xq, xs, wq, ws[:32].contiguous()),
        (xq, xs.t().contiguous().t(), wq, ws),       # scale contiguity
        (xq, xs, wq, ws.t().contiguous().t()),
        (xq.t().contiguous().t(), xs, wq, ws),       # operand contiguity
        (xq, xs, wq.t().contiguous().t(), ws),
        (xq.to(torch.int8), xs, wq, ws),             # operand dtype
        (xq, xs, wq[:, :128].contiguous(), ws),      # K mismatch
        (xq, xs, wq.reshape(-1), ws),                # 1-d weight
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            fn(*args)
    torch.cuda.synchronize()
