"""The two-gradient backward of fused dropout + add + LayerNorm
(csrc/dropout_ln.hip, DY2): the upstream gradient arrives as two bf16
addends dy and dy2, and the kernel forms float(dy) + float(dy2) itself
instead of reading a bf16 sum that a separate add kernel wrote.

Reference: float64, from dy.double() + dy2.double(), the saved bf16 sum s
and the saved mask (the formulas of tests/test_dropout_ln_gpu.py).

Bounds, those of tests/test_dropout_ln_gpu.py for the one-gradient kernel,
with the route this one replaces (bf16(dy + dy2), then the one-gradient
kernel) in the composed path's place: for dx and dz (and dw, db with bf16
parameters) err <= err_parent_route + 2^-8 * max|ref|; dw, db with fp32
parameters allclose(atol 1.0, rtol 3e-2). dzsum keeps the per-column bound of
tests/test_bias_grad_fused_gpu.py against the column sum of the returned dz.
On top of that test_no_less_accurate_than_parent_route asserts, case by case
and output by output, that the maximum error is no larger than the parent
route's on the same inputs. Both are printed.

That check is why the two-gradient kernel rounds dz once, from the fp32 dx.
The one-gradient kernel rounds it twice (bf16 dx, then bf16(dx * scale), as
the composed path does); with those two roundings the two-gradient kernel's
maximum dz error was above the parent route's in 2 of the 38 cases (N=1
H=768 float32: 1.769e-02 against 1.621e-02; N=64 H=1024 bfloat16: 4.709e-02
against 4.609e-02), because the parent route's third rounding, of the sum,
moves the maximum of two roundings up in most cases and down in a few. One
rounding of an fp32 value is at most half an ulp, below the maximum of three
roundings over a row: 1.356e-02 and 2.880e-02 in those two cases. dw and db,
which do not end in a rounding of that size with fp32 parameters, are 10^3
times closer to the reference than the parent route.

dy2 = None and dy = None: bit-equal to the one-gradient kernel on the other.

Shapes: N = 1 and 3 leave waves of a block without rows, 257 is one row more
than a multiple of the 8 waves of a block; H = 64 is one ragged trip, 768,
1024 and 2048 the full three-, four- and eight-trip instantiations.

Ill-conditioned case (in the style of tests/conditioning.py): addends that
nearly cancel, dy2 = bf16(-dy + t) with |dy| ~ 64 and |t| ~ 1/8. The sum is
a small multiple of the addends' ulp: always exact in fp32, and exact in
bf16 only where it fits in 8 bits, so the kernel must form the difference
before anything else touches the addends.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 3, 64, 257]
HS = [64, 768, 1024, 2048]
WDTYPES = ["float32", "bfloat16"]
P = 0.1
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


def _ulp_at(ref, dtype):
    """One unit in the last place of dtype at |ref| (0 at ref == 0)."""
    bits = 8 if dtype == torch.bfloat16 else 24
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref),
                       torch.ldexp(torch.ones_like(ref), e - bits))


@functools.lru_cache(maxsize=None)
def _case(N, H, wdt, cancel):
    """Every route once per case; keeps figures and flags only."""
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    dev = torch.device("cuda", 0)
    wdtype = getattr(torch, wdt)
    g = torch.Generator(device=dev).manual_seed(1000 * H + N + 7)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    z, a = rnd(N, H).to(torch.bfloat16), rnd(N, H).to(torch.bfloat16)
    if cancel:
        dy = (64 * rnd(N, H)).to(torch.bfloat16)
        dy2 = (-dy.float() + rnd(N, H) / 8).to(torch.bfloat16)
    else:
        dy, dy2 = rnd(N, H).to(torch.bfloat16), rnd(N, H).to(torch.bfloat16)
    w, b = rnd(H).to(wdtype), rnd(H).to(wdtype)
    _, s, mean, rstd, bits = ext.dropout_add_ln_fwd(z, a, w, b, EPS, P, SEED,
                                                    None)
    args = (s, w, mean, rstd, bits, P)
    names = ("dx", "dz", "dw", "db")
    two = dict(zip(names, ext.dropout_add_ln_bwd(dy, *args, dy2)))
    parent = dict(zip(names, ext.dropout_add_ln_bwd(dy + dy2, *args)))
    one = ext.dropout_add_ln_bwd(dy, *args)
    none2 = ext.dropout_add_ln_bwd(dy, *args, None)
    out = {"none_equal": all(torch.equal(x, y) for x, y in zip(one, none2))}

    # float64 reference from the exact sum, the saved s and the saved mask
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(P)))
    mask = _unpack(bits, N * H).reshape(N, H).double()
    s64, w64 = s.double(), w.double()
    d64 = dy.double() + dy2.double()
    mean64 = s64.mean(-1, keepdim=True)
    rstd64 = (s64.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xhat = (s64 - mean64) * rstd64
    gg = d64 * w64
    c1 = (gg * xhat).mean(-1, keepdim=True)
    c2 = gg.mean(-1, keepdim=True)
    ref = {"dx": rstd64 * (gg - xhat * c1 - c2),
           "dw": (d64 * xhat).sum(0), "db": d64.sum(0)}
    ref["dz"] = ref["dx"] * mask * scale
    for k in names:
        out[k] = (_err(two[k], ref[k]), _err(parent[k], ref[k]),
                  float(ref[k].abs().max()))
    out["dwdb_fp32_bounds"] = all(
        torch.allclose(two[k].double(), ref[k], atol=1.0, rtol=3e-2)
        for k in ("dw", "db"))
    out["dtypes"] = (two["dw"].dtype, two["db"].dtype, tuple(two["dw"].shape))
    out["dz_zero_where_dropped"] = bool((two["dz"][mask == 0] == 0).all())

    # with the dz column sums (zbias): the rest bit-equal, the sums within
    # the fp32 summation bound of the returned dz plus one output ulp
    out["zs"] = []
    for as_bf16 in (False, True):
        r = ext.dropout_add_ln_bwd_dzsum(dy, *args, as_bf16, dy2)
        r1 = ext.dropout_add_ln_bwd_dzsum(dy, *args, as_bf16)
        r1n = ext.dropout_add_ln_bwd_dzsum(dy, *args, as_bf16, None)
        same = all(torch.equal(x, two[k]) for x, k in zip(r, names))
        g64 = r[1].double()
        zref = g64.sum(0)
        bound = N * 2.0 ** -24 * g64.abs().sum(0) + _ulp_at(zref, r[4].dtype)
        zerr = (r[4].double() - zref).abs()
        # against the reference dz as well, next to the parent route's sum
        pz = ext.dropout_add_ln_bwd_dzsum(dy + dy2, *args, as_bf16)[4]
        zr = ref["dz"].sum(0)
        out["zs"].append(dict(
            same=same, ok=bool((zerr <= bound).all()),
            worst=float((zerr - bound).max()), dtype=r[4].dtype,
            err=_err(r[4], zr), perr=_err(pz, zr), mx=float(zr.abs().max()),
            none_equal=all(torch.equal(x, y) for x, y in zip(r1, r1n))))
    return out


def _check(c, key, what):
    e2, ep, mx = c[key]
    print(f"{what} {key}: two-gradient err {e2:.3e}  parent route err "
          f"{ep:.3e}  max|ref| {mx:.3e}")
    assert e2 <= ep + ULP * mx, (key, e2, ep, mx)


@pytest.mark.parametrize("zbias", [False, True], ids=["plain", "zbias"])
@pytest.mark.parametrize("wdt", WDTYPES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", NS)
def test_two_gradients_vs_float64(dev, N, H, wdt, zbias):
    c = _case(N, H, wdt, False)
    what = f"N={N} H={H} {wdt}"
    assert c["dtypes"] == (getattr(torch, wdt), getattr(torch, wdt), (H,))
    assert c["dz_zero_where_dropped"]
    if not zbias:
        _check(c, "dx", what)
        _check(c, "dz", what)
        _check(c, "dw", what)
        _check(c, "db", what)
        if wdt == "float32":
            assert c["dwdb_fp32_bounds"]
        return
    for z in c["zs"]:
        print(f"{what} dzsum {z['dtype']}: err - bound at the worst column "
              f"{z['worst']:.3e}; against the reference dz: two-gradient "
              f"{z['err']:.3e} parent route {z['perr']:.3e} "
              f"max|ref| {z['mx']:.3e}")
        assert z["same"], "dx, dz, dw, db must not depend on the dz sums"
        assert z["ok"], "dzsum outside the fp32 summation bound"
        assert z["err"] <= z["perr"] + ULP * z["mx"]


@pytest.mark.parametrize("cancel,N,H", [(False, N, H) for N in NS for H in HS]
                         + [(True, 257, 768), (True, 64, 2048), (True, 3, 64)])
@pytest.mark.parametrize("wdt", WDTYPES)
def test_no_less_accurate_than_parent_route(dev, wdt, cancel, N, H):
    c = _case(N, H, wdt, cancel)
    for key in ("dx", "dz", "dw", "db"):
        e2, ep, _ = c[key]
        print(f"cancel={cancel} N={N} H={H} {wdt} {key}: two-gradient err "
              f"{e2:.3e}  parent route err {ep:.3e}")
    for key in ("dx", "dz", "dw", "db"):
        e2, ep, _ = c[key]
        assert e2 <= ep, (key, "larger than the parent route's", e2, ep)


@pytest.mark.parametrize("wdt", WDTYPES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", NS)
def test_one_gradient_is_unchanged(dev, N, H, wdt):
    """dy2 = None is the one-gradient kernel, bit for bit."""
    c = _case(N, H, wdt, False)
    assert c["none_equal"]
    assert all(z["none_equal"] for z in c["zs"])


@pytest.mark.parametrize("wdt", WDTYPES)
@pytest.mark.parametrize("N,H", [(257, 768), (64, 2048), (3, 64)])
def test_nearly_cancelling_addends(dev, N, H, wdt):
    c = _case(N, H, wdt, True)
    what = f"cancel N={N} H={H} {wdt}"
    for k in ("dx", "dz", "dw", "db"):
        _check(c, k, what)
    if wdt == "float32":
        assert c["dwdb_fp32_bounds"]
    for z in c["zs"]:
        assert z["same"] and z["ok"]


def _module(dev, H):
    from ravnest_amd.ops import DropoutAddLayerNorm
    torch.manual_seed(5)
    m = DropoutAddLayerNorm(H, EPS, P).to(dev)
    with torch.no_grad():
        m.weight.copy_(torch.randn(H))
        m.bias.copy_(torch.randn(H))
    return m.train()


@pytest.mark.parametrize("which", ["both", "first", "second"])
def test_module_pair_autograd(dev, which):
    """The pair aliases one y; backward gets one gradient per output and
    either may be missing. Against the single-output module on the same
    seed with the gradients it would be handed."""
    H = 768
    m = _module(dev, H)
    torch.manual_seed(3)
    a0 = torch.randn(5, 7, H, device=dev).to(torch.bfloat16)
    z0 = torch.randn(5, 7, H, device=dev).to(torch.bfloat16)
    g1 = torch.randn(5, 7, H, device=dev).to(torch.bfloat16)
    g2 = torch.randn(5, H, 7, device=dev).to(torch.bfloat16).transpose(1, 2)
    assert not g2.is_contiguous()
    st = torch.get_rng_state()

    a, z = a0.clone().requires_grad_(), z0.clone().requires_grad_()
    y1, y2 = m(a, z, pair=True)
    assert y1.data_ptr() == y2.data_ptr() and torch.equal(y1, y2)
    loss = 0.0
    if which in ("both", "first"):
        loss = loss + (y1.float() * g1.float()).sum()
    if which in ("both", "second"):
        loss = loss + (y2.float() * g2.float()).sum()
    loss.backward()
    got = dict(da=a.grad, dz=z.grad, dw=m.weight.grad, db=m.bias.grad)

    # the single-output module with the one gradient, or for "both" the
    # two-gradient ext op on the same seed
    if which == "both":
        from ravnest_amd.ops import get_ext
        ext = get_ext(True)
        torch.set_rng_state(st)
        seed = int(torch.randint(0, 2**62, (1,)).item())
        from ravnest_amd.ops import rng
        _, s, mean, rstd, bits = ext.dropout_add_ln_fwd(
            z0.contiguous(), a0.contiguous(), m.weight, m.bias, EPS, P, seed,
            rng.device_seed_counter(dev))
        dx, dz, dw, db = ext.dropout_add_ln_bwd(
            g1, s, m.weight, mean, rstd, bits, P, g2.contiguous())
        assert torch.equal(z.grad, dz)
        assert torch.equal(m.weight.grad, dw) and torch.equal(m.bias.grad, db)
        assert torch.equal(a.grad, dx)
        return
    g = g1 if which == "first" else g2
    m.zero_grad()
    torch.set_rng_state(st)
    a, z = a0.clone().requires_grad_(), z0.clone().requires_grad_()
    m(a, z).backward(g)
    assert torch.equal(a.grad, got["da"])
    assert torch.equal(z.grad, got["dz"])
    assert torch.equal(m.weight.grad, got["dw"])
    assert torch.equal(m.bias.grad, got["db"])


def test_switch_off_returns_one_tensor(dev, monkeypatch):
    from ravnest_amd.ops import DropoutAddLayerNorm
    monkeypatch.setenv("RAVNEST_LN_BWD_DY2", "0")
    m = DropoutAddLayerNorm(128, EPS, P).to(dev).train()
    a = torch.randn(4, 128, device=dev).to(torch.bfloat16)
    y1, y2 = m(a, a, pair=True)
    assert y1 is y2
