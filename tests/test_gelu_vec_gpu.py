"""Column-group bias-GELU forward (csrc/gelu.hip, bf16 with H % 8 == 0)
against the kernel it replaces, which stays reachable with RAVNEST_GELU_V1=1
(read at every call).

The per-element arithmetic and its rounding points are unchanged, so y and
the MX pair (q, s) must be bit-equal. bias_gelu_bwd_db keeps its kernel (the
column-group rewrite measured no faster, profiles/bias_grad_gelu.txt
section 3), so dx is bit-equal either way and db is the same fp32 sum both
times, up to the order in which its atomics land: the two calls must agree
within twice the fp32 summation bound N * 2^-24 * sum_r |dx[r, c]| plus one
fp32 ulp. No bound of db against the float64 column sum of the returned dx
is asserted for this unchanged kernel: it sums the UNROUNDED products
dy * gelu'(x + b), which lie up to half a bf16 ulp per row from the stored
dx, so the summation bound alone cannot hold for it (the rewrite summed the
stored values and met it). The error against that sum is printed next to
the summation bound; test_gemm_family_gpu bounds db against its float64
reference.

Shapes: (1, 8) is one thread; (3, 40) has fewer column groups than lanes;
(7, 100) has H % 8 != 0 and must take the unchanged scalar path; (65, 768)
and (257, 3072) leave a ragged last sweep in the forward and a ragged last
chunk in the backward, as does (1031, 3072). In all of these the forward
grid still has a thread per 8-element group, so each thread does one row in
the remainder loop. (5700, 3072) is added for the other path: the grid is
capped at 2048 x 256 threads = 1365 rows of 384 groups per sweep, so rows
0..5459 go through one unrolled trip of four sweeps and the last 240 through
the remainder loop.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (3, 40), (7, 100), (65, 768), (257, 3072), (1031, 3072),
          (5700, 3072)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)  # fail loudly if the extension is missing
    return torch.device("cuda", 0)


class _v1:
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        self.old = os.environ.get("RAVNEST_GELU_V1")
        os.environ["RAVNEST_GELU_V1"] = "1" if self.flag else "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["RAVNEST_GELU_V1"]
        else:
            os.environ["RAVNEST_GELU_V1"] = self.old


def _ulp32(ref):
    _, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref),
                       torch.ldexp(torch.ones_like(ref), e - 24))


@pytest.mark.parametrize("bdt", ["float32", "bfloat16"])
@pytest.mark.parametrize("N,H", SHAPES)
def test_gelu_vec_matches_v1(dev, N, H, bdt):
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    g = torch.Generator(device=dev).manual_seed(100 * H + N)
    # pre-activations over the whole range where gelu is not linear yet
    x = (torch.randn(N, H, device=dev, generator=g) * 3).to(torch.bfloat16)
    dy = torch.randn(N, H, device=dev, generator=g).to(torch.bfloat16)
    bias = torch.randn(H, device=dev, generator=g).to(getattr(torch, bdt))

    with _v1(True):
        y0 = ext.bias_gelu_fwd(x, bias)
        dx0, db0 = ext.bias_gelu_bwd_db(dy, x, bias)
        mx0 = ext.bias_gelu_mx_fwd(x, bias) if H % 32 == 0 else None
    with _v1(False):
        y1 = ext.bias_gelu_fwd(x, bias)
        dx1, db1 = ext.bias_gelu_bwd_db(dy, x, bias)
        mx1 = ext.bias_gelu_mx_fwd(x, bias) if H % 32 == 0 else None
    torch.cuda.synchronize()

    assert torch.equal(y1, y0), "y"
    assert torch.equal(dx1, dx0), "dx"
    if mx0 is not None:
        for name, a, b in zip(("y", "q", "s"), mx1, mx0):
            assert torch.equal(a, b), "mx " + name
        assert torch.equal(mx1[0], y1)

    assert db1.dtype == torch.float32 and db1.shape == (H,)
    d64 = dx1.double()
    ref = d64.sum(0)
    asum = d64.abs().sum(0)
    tol = N * 2.0 ** -24 * asum + _ulp32(ref)
    err = (db1.double() - ref).abs()
    worst = int(torch.argmax(err - tol))
    print(f"db against the column sum of the stored dx (not asserted): max "
          f"err {float(err.max()):.3e}; worst column err "
          f"{float(err[worst]):.3e}, summation bound {float(tol[worst]):.3e}")
    # the same backward kernel both times: one sum, two atomic orders
    assert bool(((db1.double() - db0.double()).abs() <= 2 * tol).all())
