"""Cases, inputs and the per-sequence float64 reference of the varlen
attention tests (tests/test_attn_varlen_{cpu,gpu}.py) and of the --varlen
mode of tools/attn_{fwd,bwd}_round_model.py, which gives the GPU bounds."""
import math

import torch

D = 64
SCALE = 1.0 / math.sqrt(D)

# name -> (sequence lengths in stream order, heads)
CASES = {
    # starts off every tile boundary; one- to three-tile sequences with
    # ragged sub-tiles and stages
    "edges": ((2, 31, 33, 64, 65, 127, 128, 129, 160, 288), 2),
    # crosses the 2048-row lse/Delta switch next to a short sequence
    "long": ((40, 2080), 1),
    # empty sequences get no tile
    "gaps": ((0, 72, 0, 96), 2),
}


def make_inputs(name, tail, dtype=torch.bfloat16):
    """Seeded N(0,1) qkv (T,3,H,D) and dO (T,H,D) with `tail` NaN rows of
    qkv past the last sequence, and cu_seqlens as a list."""
    lens, H = CASES[name]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(cu[-1], 3, H, D, generator=g).to(dtype)
    do = torch.randn(cu[-1], H, D, generator=g).to(dtype)
    # the live rows do not depend on the tail
    qkv = torch.cat([qkv, qkv.new_full((tail, 3, H, D), float("nan"))])
    do = torch.cat([do, torch.randn(tail, H, D, generator=g).to(dtype)])
    return qkv, do, cu


def causal_term(n, causal):
    """(n, n) float64 term added to the scaled scores."""
    add = torch.zeros(n, n, dtype=torch.float64)
    return add.masked_fill_(torch.ones(n, n).triu(1).bool(),
                            float("-inf")) if causal else add


def sequences(qkv, do, cu):
    """(q, k, v, dO), each (H, n, D), of every non-empty sequence."""
    for lo, hi in zip(cu[:-1], cu[1:]):
        if hi > lo:
            yield tuple(x.transpose(0, 1) for x in
                        (*qkv[lo:hi].unbind(1), do[lo:hi]))


def reference(qkv, do, cu, causal):
    """float64 (o, lse, dq, dk, dv) per non-empty sequence, (H, n, ...)."""
    out = []
    for seq in sequences(qkv, do, cu):
        q, k, v, g = (x.double() for x in seq)
        q, k, v = (x.requires_grad_() for x in (q, k, v))
        s = q @ k.transpose(-2, -1) * SCALE + causal_term(q.shape[1], causal)
        o = torch.softmax(s, dim=-1) @ v
        grads = torch.autograd.grad(o, (q, k, v), g)
        out.append((o.detach(), torch.logsumexp(s, dim=-1).detach(), *grads))
    return out


def rel_err(x, ref):
    """max|x - ref| / max|ref|."""
    return float((x.detach().double() - ref).abs().max() / ref.abs().max())
