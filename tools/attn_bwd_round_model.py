#!/usr/bin/env python3
"""CPU model of the roundings of the D=64 flash attention backward kernels,
against float64, on the cases of tests/test_attn_bwd64_gpu.py: where that
test's bound comes from (bound = 3 x the worst figure printed here).

Modelled: fp32 scores and accumulation, o rounded to bf16 by the forward,
Delta from that bf16 o, P and dS rounded to bf16 before their matmuls,
bf16 outputs. Not modelled: __expf and the order of the fp32 sums.

Usage: python tools/attn_bwd_round_model.py   (no GPU needed)
       python tools/attn_bwd_round_model.py --varlen
           the same model per sequence on the cases of
           tests/attn_varlen_cases.py (bound of test_attn_varlen_gpu.py)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))

import torch  # noqa: E402

import test_attn_bwd64_gpu as t  # noqa: E402


def model(name, q, k, v, do, mask):
    return model_add(q, k, v, do,
                     t.additive_terms(name, mask, q.device).float())


def model_add(q, k, v, do, add):
    bf = lambda x: x.to(torch.bfloat16).float()  # noqa: E731
    qf, kf, vf, dof = (x.float() for x in (q, k, v, do))
    s = qf @ kf.transpose(-2, -1) * t.SCALE + add
    lse = torch.logsumexp(s, dim=-1, keepdim=True)
    p = torch.exp(s - lse)
    o = bf(bf(p) @ vf)
    delta = (dof * o).sum(-1, keepdim=True)
    ds = bf(p * (dof @ vf.transpose(-2, -1) - delta) * t.SCALE)
    dv = bf(bf(p).transpose(-2, -1) @ dof)
    return bf(ds @ kf), bf(ds.transpose(-2, -1) @ qf), dv


def main():
    dev = torch.device("cpu")
    worst = 0.0
    for name in t.CASES:
        q, k, v, do, mask, _, _ = t.make_inputs(name, dev)
        ref = t.reference(name, q, k, v, do, mask)[1:]
        errs = t.rel_errors(model(name, q, k, v, do, mask), ref)
        w = max(float(e.max()) for e in errs)
        worst = max(worst, w)
        print(f"{name:20s} " + "  ".join(
            f"{lab} {float(e.max()):.4f}" for lab, e in
            zip(("dq", "dk", "dv"), errs)))
    print(f"worst figure {worst:.4f}; bound = 3 x worst = {3 * worst:.4f}")


def main_varlen():
    import attn_varlen_cases as vc
    worst = 0.0
    for name in vc.CASES:
        for causal in (False, True):
            qkv, do, cu = vc.make_inputs(name, 0)
            errs = [0.0, 0.0, 0.0]
            for (q, k, v, g), ref in zip(vc.sequences(qkv, do, cu),
                                         vc.reference(qkv, do, cu, causal)):
                add = vc.causal_term(q.shape[1], causal).float()
                got = model_add(q, k, v, g, add)
                errs = [max(e, vc.rel_err(x, r))
                        for e, x, r in zip(errs, got, ref[2:])]
            worst = max(worst, *errs)
            print(f"{name:6s} causal={causal:d} " + "  ".join(
                f"{lab} {e:.4f}" for lab, e in zip(("dq", "dk", "dv"), errs)))
    print(f"worst figure {worst:.4f}; bound = 3 x worst = {3 * worst:.4f}")


if __name__ == "__main__":
    main_varlen() if "--varlen" in sys.argv[1:] else main()
