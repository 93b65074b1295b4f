"""Fused dropout + residual add + LayerNorm (csrc/dropout_ln.hip) against the
composed ops it replaces (dropout_fwd + layernorm_add_fwd, layernorm_bwd +
dropout_bwd), on the ext ops with an explicit seed so both see one mask.

Tolerances. An fp64 reference is computed from the composed path's mask and
its bf16-rounded sum s (the fused s must be bit-equal to it). For y, dx, dz
(and dw/db with bf16 weights) the fused path's max-abs error against that
reference may exceed the composed path's error on the same inputs by at most
one bf16 ulp at the largest reference magnitude, 2^-8 * max|ref|: a
different fp32 summation order can flip one rounding and no more. mean and
rstd are fp32 sums of H terms, so the same rule is applied with the fp32
worst-case summation error H * 2^-24 * max|ref| in place of the bf16 ulp.
dw/db with fp32 weights keep test_add_layer_norm's bounds (atol 1.0,
rtol 3e-2), and y/dx additionally keep that test's 5e-2 / 8e-2 bounds
against plain fp32 torch.

Shapes: H = 128 is BertConfig.tiny (half the lanes idle), 768 is three full
8-byte trips per lane, 1024 is four; N = 1 and N = 5 leave waves of a block
without rows; N = 40003 is more rows than the largest grid has waves
(256 CUs x 32 waves), so every wave takes several rows with a ragged last
sweep.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 768), (5, 768), (512, 768), (512, 128), (512, 1024),
          (40003, 128)]
PS = [0.1, 0.5]
WDTYPES = ["float32", "bfloat16"]
SEED = 0x1D2C3B4A59687766  # < 2**62
EPS = 1e-5
ULP = 2.0 ** -8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


def _err(x, ref):
    return float((x.double() - ref).abs().max())


def _unpack(bits, n):
    sh = torch.arange(8, device=bits.device, dtype=torch.uint8)
    return ((bits.unsqueeze(1) >> sh) & 1).reshape(-1)[:n]


@functools.lru_cache(maxsize=None)
def _case(N, H, p, wdt, counter):
    """Runs both paths once per case and keeps only figures and flags."""
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    dev = torch.device("cuda", 0)
    wdtype = getattr(torch, wdt)
    g = torch.Generator(device=dev).manual_seed(1000 * H + N)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    z, a, dy = (rnd(N, H).to(torch.bfloat16) for _ in range(3))
    w, b = rnd(H).to(wdtype), rnd(H).to(wdtype)
    sb = None if counter is None else torch.tensor(
        [counter], dtype=torch.int64, device=dev)

    d, mask = ext.dropout_fwd(z, p, SEED, sb)
    y_c, s_c, mean_c, rstd_c = ext.layernorm_add_fwd(a, d, w, b, EPS)
    dx_c, dw_c, db_c = ext.layernorm_bwd(dy, s_c, w, mean_c, rstd_c)
    dz_c = ext.dropout_bwd(dx_c, mask, p)

    y_f, s_f, mean_f, rstd_f, bits = ext.dropout_add_ln_fwd(
        z, a, w, b, EPS, p, SEED, sb)
    dx_f, dz_f, dw_f, db_f = ext.dropout_add_ln_bwd(
        dy, s_f, w, mean_f, rstd_f, bits, p)
    torch.cuda.synchronize()

    # fp64 reference from the same mask and the same bf16-rounded s
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    s64, w64, b64, dy64 = s_c.double(), w.double(), b.double(), dy.double()
    mean64 = s64.mean(-1, keepdim=True)
    rstd64 = (s64.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xhat = (s64 - mean64) * rstd64
    gg = dy64 * w64
    c1 = (gg * xhat).mean(-1, keepdim=True)
    c2 = gg.mean(-1, keepdim=True)
    ref = {
        "mean": mean64.squeeze(-1), "rstd": rstd64.squeeze(-1),
        "y": xhat * w64 + b64,
        "dx": rstd64 * (gg - xhat * c1 - c2),
        "dw": (dy64 * xhat).sum(0), "db": dy64.sum(0),
    }
    ref["dz"] = ref["dx"] * mask.reshape(N, H).double() * scale
    fused = {"mean": mean_f, "rstd": rstd_f, "y": y_f, "dx": dx_f,
             "dz": dz_f, "dw": dw_f, "db": db_f}
    comp = {"mean": mean_c, "rstd": rstd_c, "y": y_c, "dx": dx_c,
            "dz": dz_c, "dw": dw_c, "db": db_c}
    out = {k: (_err(fused[k], ref[k]), _err(comp[k], ref[k]),
               float(ref[k].abs().max())) for k in ref}

    # plain fp32 torch on the dropped tensor
    a32 = a.float().requires_grad_(True)
    y32 = F.layer_norm(a32 + d.float(), (H,), w.float(), b.float(), EPS)
    y32.backward(dy.float())
    out["y_vs_fp32"] = torch.allclose(y_f.float(), y32, atol=5e-2, rtol=5e-2)
    out["dx_vs_fp32"] = torch.allclose(dx_f.float(), a32.grad, atol=8e-2,
                                       rtol=8e-2)
    out["dwdb_fp32_bounds"] = all(
        torch.allclose(fused[k].float(), ref[k].float(), atol=1.0, rtol=3e-2)
        for k in ("dw", "db"))

    out["s_equal"] = torch.equal(s_f, s_c)
    out["mask_equal"] = torch.equal(_unpack(bits, N * H), mask)
    out["bits_shape"] = (tuple(bits.shape), bits.dtype)
    out["bits"] = bits.cpu()
    out["distinct"] = (
        dx_f.untyped_storage().data_ptr() != dz_f.untyped_storage().data_ptr()
        and dx_f.data_ptr() != dz_f.data_ptr())
    out["dz_zero_where_dropped"] = bool(
        (dz_f.reshape(-1)[mask == 0] == 0).all())
    out["dz_kept_nonzero"] = int(
        (dz_f.reshape(-1)[mask == 1] != 0).sum()) > 0
    out["grad_dtypes"] = (dw_f.dtype, db_f.dtype, tuple(dw_f.shape))
    return out


def _within(c, key, slack, what):
    ef, ec, mx = c[key]
    print(f"{what} {key}: fused err {ef:.3e}  composed err {ec:.3e}  "
          f"max|ref| {mx:.3e}  allowed {ec + slack * mx:.3e}")
    assert ef <= ec + slack * mx, (key, ef, ec, mx)


@pytest.mark.parametrize("counter", [None, 7])
@pytest.mark.parametrize("wdt", WDTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N,H", SHAPES)
def test_forward_matches_composed(dev, N, H, p, wdt, counter):
    c = _case(N, H, p, wdt, counter)
    assert c["s_equal"], "s = bf16(a + bf16(dropout(z))) must be bit-equal"
    assert c["bits_shape"] == ((N * H // 8,), torch.uint8)
    assert c["mask_equal"], "bit mask differs from dropout_fwd's byte mask"
    _within(c, "mean", H * 2.0 ** -24, "fwd")
    _within(c, "rstd", H * 2.0 ** -24, "fwd")
    _within(c, "y", ULP, "fwd")
    assert c["y_vs_fp32"]
    if counter is not None:
        # the device counter is part of the seed: another mask than with 0
        other = _case(N, H, p, wdt, None)
        assert not torch.equal(c["bits"], other["bits"])


@pytest.mark.parametrize("wdt", WDTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N,H", SHAPES)
def test_backward_matches_composed(dev, N, H, p, wdt):
    c = _case(N, H, p, wdt, None)
    assert c["distinct"], "dx and dz must not share storage"
    assert c["dz_zero_where_dropped"]
    assert c["dz_kept_nonzero"]
    assert c["grad_dtypes"] == (getattr(torch, wdt), getattr(torch, wdt), (H,))
    _within(c, "dx", ULP, "bwd")
    _within(c, "dz", ULP, "bwd")
    assert c["dx_vs_fp32"]
    if wdt == "bfloat16":
        _within(c, "dw", ULP, "bwd")
        _within(c, "db", ULP, "bwd")
    else:
        print("bwd dw/db fp32:", c["dw"], c["db"])
        assert c["dwdb_fp32_bounds"]


# ---------------- module level ----------------

def _modules(dev, H, p, wdtype=torch.float32):
    from ravnest_amd.ops import AddLayerNorm, Dropout, DropoutAddLayerNorm
    torch.manual_seed(5)
    fused = DropoutAddLayerNorm(H, EPS, p).to(dev)
    ln = AddLayerNorm(H, EPS).to(dev)
    drop = Dropout(p)
    with torch.no_grad():
        fused.weight.copy_(torch.randn(H))
        fused.bias.copy_(torch.randn(H))
    fused.to(wdtype)
    ln.to(wdtype)
    ln.load_state_dict(fused.state_dict())
    return fused, ln, drop


def _run_pair(fused, ln, drop, a, z, dy):
    """Both paths from one CPU RNG state; returns outputs, grads and the
    dropped tensor of the composed path."""
    st = torch.get_rng_state()
    res = []
    for path in ("fused", "composed"):
        torch.set_rng_state(st)
        a1 = a.clone().requires_grad_(True)
        z1 = z.clone().requires_grad_(True)
        mod = fused if path == "fused" else ln
        mod.zero_grad()
        if path == "fused":
            d = None
            y = fused(a1, z1)
        else:
            d = drop(z1)
            y = ln(a1, d)
        after = torch.get_rng_state()
        if dy is not None:
            y.backward(dy)
        res.append(dict(y=y.detach(), da=a1.grad, dz=z1.grad,
                        dw=mod.weight.grad, db=mod.bias.grad,
                        d=None if d is None else d.detach(), rng=after))
    return res


def test_module_matches_composed_autograd(dev):
    H, p = 768, 0.1
    fused, ln, drop = _modules(dev, H, p)
    fused.train(), ln.train(), drop.train()
    torch.manual_seed(9)
    a = torch.randn(4, 37, H, device=dev).to(torch.bfloat16)
    z = torch.randn(4, 37, H, device=dev).to(torch.bfloat16)
    dy = torch.randn(4, H, 37, device=dev).to(torch.bfloat16).transpose(1, 2)
    assert not dy.is_contiguous()
    f, c = _run_pair(fused, ln, drop, a, z, dy)
    # one host draw per forward on either path
    assert torch.equal(f["rng"], c["rng"])

    # fp64 reference with the composed path's mask and bf16-rounded s
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    mask = ((c["d"] != 0) | (z == 0)).double()
    a64 = a.double().requires_grad_(True)
    z64 = z.double().requires_grad_(True)
    w64 = fused.weight.detach().double().requires_grad_(True)
    b64 = fused.bias.detach().double().requires_grad_(True)
    lin = a64 + z64 * mask * scale
    s_b = (a + c["d"]).double()  # bf16(a + d), as both kernels save it
    s64 = s_b + (lin - lin.detach())
    y64 = F.layer_norm(s64, (H,), w64, b64, EPS)
    y64.backward(dy.double())

    def within(name, xf, xc, ref):
        ef, ec, mx = _err(xf, ref), _err(xc, ref), float(ref.abs().max())
        print(f"module {name}: fused err {ef:.3e} composed err {ec:.3e} "
              f"max|ref| {mx:.3e}")
        assert ef <= ec + ULP * mx, (name, ef, ec, mx)

    within("y", f["y"], c["y"], y64.detach())
    within("da", f["da"], c["da"], a64.grad)
    within("dz", f["dz"], c["dz"], z64.grad)
    assert f["da"].data_ptr() != f["dz"].data_ptr()
    assert torch.allclose(f["dw"].double(), w64.grad, atol=1.0, rtol=3e-2)
    assert torch.allclose(f["db"].double(), b64.grad, atol=1.0, rtol=3e-2)
    assert bool((f["dz"][mask == 0] == 0).all())


def test_module_respects_needs_input_grad(dev):
    H = 128
    fused, _, _ = _modules(dev, H, 0.1)
    fused.train()
    a = torch.randn(6, H, device=dev).to(torch.bfloat16)
    z = torch.randn(6, H, device=dev).to(torch.bfloat16).requires_grad_(True)
    fused.bias.requires_grad_(False)
    y = fused(a, z)
    y.sum().backward()
    assert a.grad is None and fused.bias.grad is None
    assert z.grad is not None and fused.weight.grad is not None


@pytest.mark.parametrize("mode", ["eval", "p0"])
def test_module_eval_and_p0_equal_add_layer_norm(dev, mode):
    from ravnest_amd.ops import add_layer_norm
    H = 768
    fused, _, _ = _modules(dev, H, 0.0 if mode == "p0" else 0.1)
    fused.train(mode == "p0")
    torch.manual_seed(2)
    a = torch.randn(33, H, device=dev).to(torch.bfloat16)
    z = torch.randn(33, H, device=dev).to(torch.bfloat16)
    st = torch.get_rng_state()
    y = fused(a, z)
    assert torch.equal(torch.get_rng_state(), st)  # no mask, no host draw
    assert torch.equal(y, add_layer_norm(a, z, fused.weight, fused.bias, EPS))


@pytest.mark.parametrize("H,dtype", [(100, torch.bfloat16),
                                     (768, torch.float32)])
def test_module_fallback_shapes_match(dev, H, dtype):
    """Ragged H and fp32 activations take the composed path inside the
    module: same ops, same seed, so the results are equal."""
    fused, ln, drop = _modules(dev, H, 0.1)
    fused.train(), ln.train(), drop.train()
    torch.manual_seed(4)
    a = torch.randn(17, H, device=dev).to(dtype)
    z = torch.randn(17, H, device=dev).to(dtype)
    dy = torch.randn(17, H, device=dev).to(dtype)
    f, c = _run_pair(fused, ln, drop, a, z, dy)
    for k in ("y", "da", "dz", "dw", "db"):
        assert torch.equal(f[k], c[k]), k
    assert int((c["d"] == 0).sum()) > 0  # dropout was active
