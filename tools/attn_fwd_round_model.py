#!/usr/bin/env python3
"""CPU model of the roundings of the D=64 flash attention forward kernels,
against float64, on the cases of tests/test_attn_fwd64_gpu.py: where that
test's bounds come from (bound = 3 x the worst figure printed here, for O
and for lse).

Modelled: bf16 inputs, fp32 scores, maxima and sums, the unnormalised P
rounded to bf16 before P V, fp32 accumulation, O divided by l and rounded
to bf16, lse = m + ln l in fp32. Not modelled: the hardware exp2/log2,
the defer-max headroom (P up to e^8) and the order of the fp32 sums.

Usage: python tools/attn_fwd_round_model.py   (no GPU needed)
       python tools/attn_fwd_round_model.py --varlen
           the same model per sequence on the cases of
           tests/attn_varlen_cases.py (bounds of test_attn_varlen_gpu.py)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))

import torch  # noqa: E402

import test_attn_fwd64_gpu as t  # noqa: E402


def model(name, q, k, v, mask):
    return model_add(q, k, v, t.additive_terms(name, mask, q.device).float())


def model_add(q, k, v, add):
    bf = lambda x: x.to(torch.bfloat16).float()  # noqa: E731
    s = q.float() @ k.float().transpose(-2, -1) * t.SCALE + add
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = bf(bf(p) @ v.float() / l)
    return o, (m + torch.log(l)).squeeze(-1)


def main():
    dev = torch.device("cpu")
    worst_o = worst_l = 0.0
    for name in t.CASES:
        q, k, v, _, mask, _, _ = t.make_inputs(name, dev)
        ref_o, ref_lse = t.reference(name, q, k, v, mask)
        o, lse = model(name, q, k, v, mask)
        eo = float(t.o_errors(o, ref_o).max())
        el = t.lse_error(lse, ref_lse)
        worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
        print(f"{name:20s} o {eo:.5f}  lse {el:.3g}")
    print(f"worst figures: o {worst_o:.5f}, lse {worst_l:.3g}; bounds = "
          f"3 x worst = {3 * worst_o:.4f}, {3 * worst_l:.3g}")


def main_varlen():
    import attn_varlen_cases as vc
    worst_o = worst_l = 0.0
    for name in vc.CASES:
        for causal in (False, True):
            qkv, do, cu = vc.make_inputs(name, 0)
            eo = el = 0.0
            for (q, k, v, _), ref in zip(vc.sequences(qkv, do, cu),
                                         vc.reference(qkv, do, cu, causal)):
                add = vc.causal_term(q.shape[1], causal).float()
                o, lse = model_add(q, k, v, add)
                eo = max(eo, vc.rel_err(o, ref[0]))
                el = max(el, float((lse.double() - ref[1]).abs().max()))
            worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
            print(f"{name:6s} causal={causal:d} o {eo:.5f}  lse {el:.3g}")
    print(f"worst figures: o {worst_o:.5f}, lse {worst_l:.3g}; bounds = "
          f"3 x worst = {3 * worst_o:.4f}, {3 * worst_l:.3g}")


if __name__ == "__main__":
    main_varlen() if "--varlen" in sys.argv[1:] else main()
