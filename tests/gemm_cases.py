"""Input builders, float64 references and error bounds for the bias-GELU
kernels and the GEMM family (test_gemm_family_gpu.py and its CPU twin
test_gemm_family_cpu.py).

Every reference is float64 and is computed from the exact bf16 / fp8 values
the implementation under test was given. The `*_ratios` functions return
measured error / bound per quantity; a test prints them and asserts
`ratio <= 1` (the twin: the stated share of the bound).

Bounds, with u = 2^-24 (fp32 unit roundoff) and 2^-8 (bf16 unit roundoff):

GELU, a = max(1, |x + b|):
    fp32 y   16 u a                fp32 dx   32 u a |dy|
    bf16 tensors add 2^-8 |ref|.
    db: sum over rows of the dx bound + rows u sum|dx_ref|
        (+ 2^-8 |ref| for a bf16 bias).
GEMM, S = |a| @ |b|^T (+ |bias|) in float64, e_acc = C_ACC K u S:
    bf16 out  2^-8 |ref| + (1 + 2^-8) e_acc
    fp32 out  e_acc (wgrad: the reduction length M in place of K).
    A textbook fp32 dot product of length K is within K u S, i.e. C_ACC = 1;
    C_ACC = 2 leaves room for the MFMA's undocumented internal summation
    order and for split-K partial sums meeting in fp32 atomics. Measured
    on an MI355X: torch's fp32 matmul of the same operands uses <= 0.01 of
    e_acc, the fp32-output wgrad kernel <= 0.002, so 2 stands. A bf16
    result reaches 0.98 to 0.99 of its bound for torch's bf16 matmul and
    for the kernels alike: that is the final rounding, whose worst case is
    the 2^-8 |ref| term itself, and no C_ACC would move it. The GPU tests
    therefore print the library's bf16 ratio and assert the part C_ACC
    governs: torch's fp32 product of the same operands within 1/2 of e_acc.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24      # fp32 unit roundoff
BF16_U = 2.0 ** -8    # bf16 unit roundoff
C_ACC = 2.0
BF16 = torch.bfloat16


def _ratio(err, bound):
    """max(err / bound), 0/0 counting as 0 and NaN/inf errors as inf."""
    err, bound = err.double(), torch.as_tensor(bound).double()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, math.inf))
    return float(q.max()) if q.numel() else 0.0


def bits16(t):
    """bf16 -> int16 bit patterns with -0 folded into +0 (a sum of exact
    zeros may carry either sign; that is not a routing error)."""
    return (t + 0.0).contiguous().view(torch.int16)


# ================================================================== GELU
GELU_SHAPES = [(3, 8), (3, 5), (5, 100), (7, 264), (65, 300), (200, 300)]
GELU_DB_ROWS = [1, 63, 64, 65]   # at H = 300: bwd_db's row chunking
GELU_DB_H = 300
GELU_DTYPES = {"bf16_fp32": (BF16, torch.float32),
               "bf16_bf16": (BF16, BF16),
               "fp32_fp32": (torch.float32, torch.float32)}
# (dtypes, with_bias): gelu() builds its zero bias in x's dtype, so without
# a bias there is one bf16 and one fp32 case
GELU_VARIANTS = [("bf16_fp32", True), ("bf16_bf16", True), ("fp32_fp32", True),
                 ("bf16_bf16", False), ("fp32_fp32", False)]
GELU_SPECIALS = [0.0, -0.0, 1e-20, -1e-20, 9.96, -9.96, 10.0625, -10.0625,
                 11.0, -11.0, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4]


def gelu_case(rows, H, xdt, bdt, with_bias=True, seed=0):
    """Pre-activations x + b: a linspace over [-40, 40] laid through the
    tensor, the specials spread over it, and one block of 3 * randn."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + H)
    n = rows * H
    pre = torch.linspace(-40.0, 40.0, n)
    lo, ln = n // 2, max(1, n // 8)
    pre[lo:lo + ln] = 3.0 * torch.randn(ln, generator=g)
    sp = torch.tensor(GELU_SPECIALS)
    idx = (torch.arange(len(sp)) * max(1, n // len(sp)) + 1) % n
    pre[idx] = sp
    pre = pre.view(rows, H)
    if with_bias:
        b = torch.randn(H, generator=g).to(bdt)
        x = (pre - b.float()).to(xdt)
    else:
        b = None
        x = pre.to(xdt)
    dy = torch.randn(rows, H, generator=g).to(xdt)
    return {"x": x, "b": b, "dy": dy}


def gelu_reference(case):
    x, b, dy = case["x"], case["b"], case["dy"]
    pre = x.double() if b is None else x.double() + b.double()
    pre = pre.detach().requires_grad_()
    y = F.gelu(pre, approximate="tanh")
    (deriv,) = torch.autograd.grad(y.sum(), pre)
    dx = deriv * dy.double()
    return {"pre": pre.detach(), "y": y.detach(), "deriv": deriv, "dx": dx,
            "db": dx.sum(0)}


def gelu_bounds(case, ref):
    a = ref["pre"].abs().clamp(min=1.0)
    bf = case["x"].dtype == BF16
    by = 16 * U32 * a + (BF16_U * ref["y"].abs() if bf else 0.0)
    bdx = 32 * U32 * a * case["dy"].double().abs() + \
        (BF16_U * ref["dx"].abs() if bf else 0.0)
    rows = case["x"].shape[0]
    bdb = bdx.sum(0) + rows * U32 * ref["dx"].abs().sum(0)
    if case["b"] is not None and case["b"].dtype == BF16:
        bdb = bdb + BF16_U * ref["db"].abs()
    return {"y": by, "dx": bdx, "db": bdb}


def gelu_ratios(got, case, ref):
    """got: dict with any of y, dx, db. Also `exact`: the number of
    elements with |x+b| >= 20 whose float64 derivative rounds to 0 or 1 in
    the output dtype but whose dx is not exactly 0 or dy (as a ratio: 0
    when there are none, inf otherwise)."""
    bounds = gelu_bounds(case, ref)
    out = {}
    for k in ("y", "dx", "db"):
        if k in got:
            out[k] = _ratio((got[k].double().cpu() - ref[k]).abs(),
                            bounds[k])
    if "dx" in got:
        dt = case["x"].dtype
        far = ref["pre"].abs() >= 20.0
        d = ref["deriv"].to(dt)
        dx, dy = got["dx"].cpu(), case["dy"]
        bad = (far & (d == 1) & (dx != dy)) | (far & (d == 0) & (dx != 0))
        out["exact"] = math.inf if bool(bad.any()) else 0.0
    return out


def gelu_torch_fp32(case):
    """torch's fp32 tanh-GELU and its autograd on the upcast inputs,
    results rounded to the case's dtypes: the known-good implementation."""
    x, b, dy = case["x"], case["b"], case["dy"]
    # fresh leaves: .float() alone would hand back the case's own tensor
    xf = x.detach().clone().float().requires_grad_()
    bf = None if b is None else b.detach().clone().float().requires_grad_()
    y = F.gelu(xf if bf is None else xf + bf, approximate="tanh")
    y.backward(dy.float())
    got = {"y": y.detach().to(x.dtype), "dx": xf.grad.to(x.dtype)}
    if bf is not None:
        got["db"] = bf.grad.to(b.dtype)
    return got


def gelu_run(case, device):
    """Through ops.activation on `device` (the HIP kernels on a GPU)."""
    from ravnest_amd.ops.activation import bias_gelu, gelu
    x = case["x"].detach().clone().to(device).requires_grad_()
    dy = case["dy"].to(device)
    if case["b"] is None:
        y = gelu(x)
        y.backward(dy)
        return {"y": y.detach(), "dx": x.grad}
    b = case["b"].detach().clone().to(device).requires_grad_()
    y = bias_gelu(x, b)
    y.backward(dy)
    return {"y": y.detach(), "dx": x.grad, "db": b.grad}


# ============================================================= bf16 GEMMs
GEMM_SHAPES = [(1, 128, 1), (37, 128, 5), (256, 128, 256), (257, 192, 259),
               (300, 192, 301)]
# the smallest shapes with tpb > 1 (MT * (NT / tpb) >= 512 row x column
# blocks): tpb = 2 with a ragged last row tile and a ragged second column
# tile; tpb = 3 with an odd number of K-tiles
GEMM_SHAPES_LARGE = [(130817, 128, 259), (131072, 192, 517)]
GEMM_ROWS_LIMITS = [-3, 0, 1, 255, 256, 257, 600, 605]
GEMM_ROWS_SHAPE = (600, 128, 259, 264)          # M, K, N, width of C
GEMM_ROWS_LARGE = (131072, 128, 826, 19661)     # M, K, N, limit: tpb = 4
SENTINEL = 0x5A5A                               # bf16 bit pattern
WGRAD_SHAPES = [(128, 8, 8), (192, 130, 72), (2048, 256, 136),
                (4096, 128, 128)]               # (M, N, K)
WGRAD_REJECTED = (128, 129, 127)
WGRAD_ROWS_SHAPE = (512, 136, 136)   # one full tile (LDS-DMA) + three tails
WGRAD_ROWS_BOUNDS = [-1, 0, 1, 63, 64, 65, 511, 512, 600]


def code_matrix(R, C, device="cpu"):
    """Integer code of (r, c) in [-127, 127]: exact in bf16, and different
    between neighbouring rows, columns, 64-column K-tiles and 256-row
    tiles, so a misrouted element shows."""
    r = torch.arange(R, device=device).view(-1, 1)
    c = torch.arange(C, device=device).view(1, -1)
    v = (r * 37 + c * 101 + (r // 256) * 7 + (c // 64) * 3 + (r * c) % 11)
    return (v % 255 - 127).to(BF16)


def routing_perm(M, K, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed + 7 * M + K)
    return torch.randint(0, K, (M,), generator=g).to(device)


def int_bias(N, device="cpu"):
    """Integers in [-128, 128]: code + bias stays an integer <= 255."""
    n = torch.arange(N, device=device)
    return ((n * 29 + 5) % 257 - 128).to(BF16)


def routing_case(M, K, N, device="cpu", bias=False):
    """A one-hot per row at column pi(m): C[m, n] must be B[n, pi(m)]
    (+ bias[n]) bit for bit, whatever the summation order."""
    pi = routing_perm(M, K, device)
    a = torch.zeros(M, K, dtype=BF16, device=device)
    a[torch.arange(M, device=device), pi] = 1.0
    b = code_matrix(N, K, device)
    want = b.t().contiguous()[pi]
    bv = None
    if bias:
        bv = int_bias(N, device)
        want = (want.float() + bv.float()).to(BF16)
    return {"a": a, "b": b, "bias": bv, "want": want}


def routing_mismatches(got, want):
    return int((bits16(got) != bits16(want)).sum())


def wgrad_routing_case(M, N, K, device="cpu"):
    """dy one-hot over m per column n: dW[n, :] must be x[sigma(n), :]."""
    sigma = routing_perm(N, M, device, seed=3)
    dy = torch.zeros(M, N, dtype=BF16, device=device)
    dy[sigma, torch.arange(N, device=device)] = 1.0
    x = code_matrix(M, K, device)
    return {"dy": dy, "x": x, "want": x[sigma].float()}


def gemm_random_case(M, K, N, bias=False, cancel=False, seed=0, device="cpu"):
    """Drawn on `device` (the large shapes are drawn on the GPU)."""
    g = torch.Generator(device=device).manual_seed(seed + M + 3 * K + 5 * N)

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=device)
    if cancel:
        # a = [v, -v] + 2^-6 noise against b = [w, w]: the products cancel
        # to ~2^-6 of their magnitude, so e_acc is the whole bound
        v = randn(M, K // 2)
        a = torch.cat([v, -v], 1) + 2.0 ** -6 * randn(M, K)
        w = randn(N, K // 2)
        b = torch.cat([w, w], 1)
    else:
        a = randn(M, K)
        b = randn(N, K)
    a = (a / math.sqrt(K)).to(BF16)
    b = b.to(BF16)
    bv = randn(N).to(BF16) if bias else None
    return {"a": a, "b": b, "bias": bv}


def gemm_reference(a, b, bias=None):
    """float64 product and S = |a| @ |b|^T (+ |bias|), on a's device."""
    ad, bd = a.double(), b.double()
    ref = ad @ bd.t()
    S = ad.abs() @ bd.abs().t()
    if bias is not None:
        ref = ref + bias.double()
        S = S + bias.double().abs()
    return ref, S


def gemm_bound(ref, S, depth, bf16_out=True, c=C_ACC):
    e_acc = c * depth * U32 * S
    if bf16_out:
        return BF16_U * ref.abs() + (1 + BF16_U) * e_acc
    return e_acc


def gemm_ratio(got, ref, S, depth, bf16_out=True):
    return _ratio((got.double() - ref).abs(),
                  gemm_bound(ref, S, depth, bf16_out))


def gemm_torch_fp32(a, b, bias=None):
    y = a.float() @ b.float().t()
    return y if bias is None else y + bias.float()


def wgrad_random_case(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed + M + 3 * N + 5 * K)
    dy = (torch.randn(M, N, generator=g) / math.sqrt(M)).to(BF16)
    x = torch.randn(M, K, generator=g).to(BF16)
    return {"dy": dy, "x": x}


def sample_rows(M, device="cpu", extra=4096, seed=0):
    """Rows of the first and the last 256-row tile plus `extra` random."""
    g = torch.Generator().manual_seed(seed + M)
    last0 = (M - 1) // 256 * 256
    rows = torch.cat([torch.arange(0, min(256, M)),
                      torch.arange(last0, M),
                      torch.randint(0, M, (extra,), generator=g)])
    return torch.unique(rows).to(device)


def fused_gelu_case(seed=0):
    """(64, 128, 72) with a bias that spreads the pre-activations over
    [-30, 30] (the product itself is ~N(0, 1))."""
    c = gemm_random_case(64, 128, 72, seed=seed)
    c["bias"] = torch.linspace(-30.0, 30.0, 72).to(BF16)
    g = torch.Generator().manual_seed(seed + 99)
    c["dy"] = torch.randn(64, 72, generator=g).to(BF16)
    return c


def fused_gelu_ratios(y, h, case):
    """h and y of gemm_nt_bf16(a, b, bias, 2) against float64."""
    ref_h, S = gemm_reference(case["a"], case["b"], case["bias"])
    K = case["a"].shape[1]
    bound_h = gemm_bound(ref_h, S, K)
    ref_y = F.gelu(ref_h, approximate="tanh")
    a = ref_h.abs().clamp(min=1.0)
    bound_y = gemm_bound(ref_y, S, K) + 1.13 * bound_h + 16 * U32 * a
    return {"h": _ratio((h.double().cpu() - ref_h).abs(), bound_h),
            "y": _ratio((y.double().cpu() - ref_y).abs(), bound_y)}


# ================================================================ MX fp8
E4M3 = torch.float8_e4m3fn
MX_GEMM_SHAPES = [(1, 64, 1), (129, 192, 65), (96, 256, 80)]
MX_GEMM2_SHAPES = [(1, 256, 1), (130, 256, 70), (257, 384, 259)]
MX_GEMM2_LARGE = (130817, 256, 259)    # tpb = 2


def mx_scale_ref(x):
    """s = floor(log2(amax / 448)) + 1 per 32-block over the FINITE
    elements, clamped to [-127, 127]; -127 for amax = 0. Exact: amax =
    m 2^ex with m in [0.5, 1) and 448 = 0.875 * 2^9, so the floor is
    ex - 9 for m >= 0.875 and ex - 10 below."""
    xd = x.double().reshape(-1, 32)
    amax = torch.where(torch.isfinite(xd), xd.abs(),
                       torch.zeros_like(xd)).amax(1)
    m, ex = torch.frexp(amax)
    s = ex.long() - 9 + (m >= 0.875).long()
    s = torch.where(amax > 0, s, torch.full_like(s, -127))
    return s.clamp(-127, 127).reshape(*x.shape[:-1], x.shape[-1] // 32)


def mx_quant_ref(x):
    """-> (q uint8, s int64 exponent, nonfinite mask). q is
    (x.double() * 2^-s).float().to(e4m3fn) bit for bit at finite x; at a
    NaN or +-inf element the contract is 0x7F with either sign."""
    s = mx_scale_ref(x)
    xd = x.double().reshape(*s.shape, 32)
    scaled = torch.ldexp(xd, (-s).unsqueeze(-1).expand_as(xd))
    nonfin = ~torch.isfinite(xd)
    scaled = torch.where(nonfin, torch.zeros_like(scaled), scaled)
    q = scaled.float().to(E4M3).view(torch.uint8)
    q = torch.where(nonfin, torch.full_like(q, 0x7F), q)
    return q.reshape(x.shape), s, nonfin.reshape(x.shape)


def mx_quant_mismatches(q, sc, x):
    """q, sc: the implementation's uint8 outputs (CPU) -> mismatch counts."""
    qr, sr, nonfin = mx_quant_ref(x)
    q = torch.where(nonfin, q & 0x7F, q)
    return {"s": int((sc.long() - 127 != sr).sum()),
            "q": int((q != qr).sum())}


def mx_dequant(q, s_u8):
    """e4m3 bytes + biased e8m0 bytes -> float64."""
    v = q.view(E4M3).float().double()
    e = (s_u8.long() - 127).unsqueeze(-1).expand(*s_u8.shape, 32)
    return torch.ldexp(v.reshape(*s_u8.shape, 32), e).reshape(q.shape)


def all_finite_bf16():
    """Every finite bf16 value, each alone (at a varying position) in an
    otherwise zero 32-block."""
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = pat.view(BF16)
    v = v[torch.isfinite(v)]
    x = torch.zeros(v.numel(), 32, dtype=BF16)
    x[torch.arange(v.numel()), (torch.arange(v.numel()) * 7) % 32] = v
    return x


def bf16_under_fixed_amax():
    """Every bf16 value with |v| <= 446 next to an element 446 (s = 0, so
    v itself is what gets encoded): all of e4m3's binades, its subnormals,
    the ties between them and the underflow to zero. A value that is the
    amax of its own block never leaves [224, 448)."""
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = pat.view(BF16)
    v = v[torch.isfinite(v) & (v.float().abs() <= 446)]
    x = torch.zeros(v.numel(), 32, dtype=BF16)
    x[:, 0] = 446.0
    x[torch.arange(v.numel()), 1 + (torch.arange(v.numel()) * 7) % 31] = v
    return x


def wide_blocks(rows=256, kb=4, seed=0):
    """randn blocks scaled by 2^e, e uniform in [-120, 120] per block."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-120, 121, (rows, kb, 1), generator=g)
    x = torch.ldexp(torch.randn(rows, kb, 32, generator=g).double(), e)
    return x.float().to(BF16).reshape(rows, kb * 32)


def nonfinite_blocks(seed=0):
    """Blocks holding NaN, +inf, -inf, or several of them, next to finite
    elements of mixed magnitude; one block is all non-finite."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(8, 64, generator=g) * 37.0).to(BF16)
    x[0, 3] = math.nan
    x[1, 40] = math.inf
    x[2, 0] = -math.inf
    x[3, 5], x[3, 6], x[3, 33] = math.inf, math.nan, -math.inf
    x[4, :32] = math.inf
    x[5, 31] = math.inf
    x[5, :31] *= 2.0 ** -20
    return x


def mx_operand(R, K, seed, device="cpu"):
    """randn * 2^e with e in [-12, 12] drawn per (row, 32-block), then
    quantised by the reference quantiser (on `device`): (q uint8, s uint8,
    dequantised float64)."""
    g = torch.Generator().manual_seed(seed + R + 3 * K)
    e = torch.randint(-12, 13, (R, K // 32, 1), generator=g)
    x = torch.ldexp(torch.randn(R, K // 32, 32, generator=g), e)
    x = x.to(BF16).reshape(R, K).to(device)
    q, s, _ = mx_quant_ref(x)
    s8 = (s + 127).to(torch.uint8)
    return q, s8, mx_dequant(q, s8)


def mx_routing_case(M, K, N, device="cpu", seed=0):
    """One non-zero e4m3 entry per row of x at column pi(m), every finite
    e4m3 code in w, scales in 2^[-10, 10] on both sides. One product of
    two e4m3 values has 8 significant bits: exact in fp32 and in bf16."""
    g = torch.Generator().manual_seed(seed + M + K + N)
    pi = torch.randint(0, K, (M,), generator=g)
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8)
    nz = codes[(codes & 0x7F) != 0]
    xcode = nz[torch.randint(0, len(nz), (M,), generator=g)]
    wq = codes[torch.randint(0, len(codes), (N, K), generator=g)]
    xs = torch.randint(117, 138, (M, K // 32), generator=g).to(torch.uint8)
    ws = torch.randint(117, 138, (N, K // 32), generator=g).to(torch.uint8)
    rows = torch.arange(M)
    xq = torch.zeros(M, K, dtype=torch.uint8)
    xq[rows, pi] = xcode
    xd = torch.ldexp(xcode.view(E4M3).float().double(),
                     xs[rows, pi // 32].long() - 127)          # (M,)
    wd = mx_dequant(wq, ws).t().contiguous().to(device)[pi.to(device)]
    want = (xd.to(device).unsqueeze(1) * wd).to(BF16)          # (M, N)
    return {"xq": xq.to(device), "xs": xs.to(device), "wq": wq.to(device),
            "ws": ws.to(device), "want": want}
