"""Cases, inputs, float64 reference and cache check shared by
test_attn_decode_cpu.py and test_attn_decode_gpu.py."""
import math

import torch

B, H = 3, 2

# (S_max, cache_len, n_split, max_len): the smallest shapes that reach
# each way the decode kernel can go wrong.
CASES = [
    # only the new token; a partial tile; the last slot; direct write
    (64, (0, 1, 63), 1, None),
    # the 64-key tile edge, either side
    (256, (63, 64, 65), 1, None),
    # the new row lands in a different split per sequence; whole splits
    # past L give neutral partials; combine
    (256, (5, 130, 255), 4, None),
    # the last sequence violates max_len
    (320, (70, 200, 319), 4, 256),
    # the host heuristic's own split count
    (2048, (2047, 1000, 0), None, None),
]
IDS = [f"S{c[0]}-split{c[2]}" + ("-maxlen" if c[3] else "") for c in CASES]


def make_inputs(D, S_max, lens, dtype):
    """N(0,1) qkv_new and caches (CPU, fixed seed); every cache row at or
    past cache_len[b] is NaN, so a dead key that reaches the result, even
    with weight 0, shows."""
    g = torch.Generator().manual_seed(1234)
    qkv = torch.randn(B, 3, H, D, generator=g).to(dtype)
    kc = torch.randn(B, H, S_max, D, generator=g).to(dtype)
    vc = torch.randn(B, H, S_max, D, generator=g).to(dtype)
    for b, L in enumerate(lens):
        kc[b, :, L:] = float("nan")
        vc[b, :, L:] = float("nan")
    return qkv, kc, vc, torch.tensor(lens, dtype=torch.int32)


def reference(qkv, kc, vc, lens):
    """float64 softmax(q K^T scale) V over rows [0, L], row L taken from
    qkv_new -> (B, H*D)."""
    scale = 1.0 / math.sqrt(qkv.shape[-1])
    out = []
    for b, L in enumerate(lens):
        q, kn, vn = qkv[b].double()
        K = torch.cat([kc[b, :, :L].double(), kn[:, None]], dim=1)
        V = torch.cat([vc[b, :, :L].double(), vn[:, None]], dim=1)
        p = torch.softmax((K @ q[..., None]).squeeze(-1) * scale, dim=-1)
        out.append((p[..., None] * V).sum(1).flatten())
    return torch.stack(out)


def row_errors(o, ref):
    """Per batch row max|o - ref| / max|ref|."""
    o = o.detach().double().cpu()
    return ((o - ref).abs().amax(1) / ref.abs().amax(1)).tolist()


def assert_cache(kc_after, vc_after, kc_before, vc_before, qkv, lens):
    """Row L holds the new token's k and v bit for bit and every other
    row is bitwise unchanged (integer views, because of the NaNs)."""
    bits = torch.int16 if kc_before.element_size() == 2 else torch.int32
    for after, before, which in ((kc_after, kc_before, 1),
                                 (vc_after, vc_before, 2)):
        want = before.clone()
        for b, L in enumerate(lens):
            want[b, :, L] = qkv[b, which]
        assert torch.equal(after.cpu().view(bits), want.view(bits))
