"""The MX fp8 backward of MXLinear against the bf16 one (GPU only).

  quant    mx_quant / mx_quant_t / mx_quant_dual on dy (rows x out), with the
           bytes each moves and the bandwidth that makes
  dgrad    dy @ W            bf16 library matmul | fp8: mx_quant_dual(dy) +
           mx_quant_t(W) + GEMM | the fp8 GEMM alone
  wgrad    dy^T @ x          bf16 library matmul | fp8: mx_quant_t(x) +
           mx_gemm2_splitk (dy^T comes from dgrad's dual pass) | GEMM alone
  layer    MXLinear forward + backward, fp8_backward off | on
  grads    relative L2 distance per parameter of one GPTConfig.nano64(fp8)
           step, switch on against off (a property of e4m3, reported only)

Shapes: GPT-2-small's four projections at 32 x 1024 rows and BERT-base's at
128 x 128 rows. Arms are alternated inside the process round after round and
timed with device events; each line gives the median over the rounds and the
min-max spread.

Run:  python tools/bench_mx_bwd.py [--rounds 7] [--iters 10] [--only PART]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from ravnest_amd.ops import MXLinear, get_ext, mx  # noqa: E402

BF16 = torch.bfloat16
# (name, rows, in_features, out_features)
SHAPES = [("gpt2 qkv", 32768, 768, 2304), ("gpt2 proj", 32768, 768, 768),
          ("gpt2 mlp_in", 32768, 768, 3072), ("gpt2 mlp_out", 32768, 3072, 768),
          ("bert qkvo", 16384, 768, 768), ("bert mlp_in", 16384, 768, 3072),
          ("bert mlp_out", 16384, 3072, 768)]


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def quant_bytes(arm, R, C):
    rp = mx._contraction_pad(R)
    row, col = R * C * (1 + 1 / 32), C * rp * (1 + 1 / 32)
    return 2 * R * C + {"mx_quant": row, "mx_quant_t": col,
                        "mx_quant_dual": row + col}[arm]


def build_arms(ext, dev, only):
    """-> {site: {arm: (callable, bytes or None, flop or None)}}"""
    g = torch.Generator(device=dev).manual_seed(0)

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=dev).to(BF16)

    arms = {}
    for name, R, fin, fout in SHAPES:
        dy, x, w = randn(R, fout), randn(R, fin), randn(fout, fin) * 0.02
        if "quant" in only and name in ("gpt2 proj", "gpt2 mlp_in"):
            arms[f"quant {R}x{fout}"] = {
                a: (lambda a=a, dy=dy: getattr(ext, a)(dy),
                    quant_bytes(a, R, fout), None)
                for a in ("mx_quant", "mx_quant_t", "mx_quant_dual")}
        flop = 2.0 * R * fin * fout
        dyq, dys, dyqt, dyst = ext.mx_quant_dual(dy)
        wqt, wst = ext.mx_quant_t(w)
        xqt, xst = ext.mx_quant_t(x)
        if "dgrad" in only:
            arms[f"dgrad {name} {R}x{fout}x{fin}"] = {
                "bf16": (lambda dy=dy, w=w: dy @ w, None, flop),
                "fp8+quant": (lambda dy=dy, w=w: ext.mx_gemm2(
                    *ext.mx_quant_dual(dy)[:2], *ext.mx_quant_t(w)),
                    None, flop),
                "fp8 gemm": (lambda a=(dyq, dys, wqt, wst): ext.mx_gemm2(*a),
                             None, flop)}
        if "wgrad" in only:
            arms[f"wgrad {name} {fout}x{R}x{fin}"] = {
                "bf16": (lambda dy=dy, x=x: dy.t() @ x, None, flop),
                "fp8+quant": (lambda t=(dyqt, dyst), x=x: ext.mx_gemm2_splitk(
                    *t, *ext.mx_quant_t(x)), None, flop),
                "fp8 gemm": (lambda a=(dyqt, dyst, xqt, xst):
                             ext.mx_gemm2_splitk(*a), None, flop)}
        if "layer" in only:
            site = arms.setdefault(f"layer {name} fwd+bwd", {})
            for flag in (False, True):
                lin = MXLinear(fin, fout, fp8_backward=flag).to(dev).to(BF16)
                xg = x.clone().requires_grad_()

                def step(lin=lin, xg=xg, dy=dy):
                    lin.weight.grad = lin.bias.grad = xg.grad = None
                    lin(xg).backward(dy)
                site["fp8 bwd" if flag else "bf16 bwd"] = (step, None,
                                                           3 * flop)
    return arms


def grad_distance(dev):
    from ravnest_amd import set_seed
    from ravnest_amd.models import GPT, GPTConfig
    from ravnest_amd.ops import cross_entropy
    grads = []
    for flag in (False, True):
        mx.FP8_BACKWARD = flag
        set_seed(11)
        cfg = GPTConfig.nano64(vocab_size=64, block_size=16)
        cfg.dropout, cfg.fp8 = 0.0, True
        model = GPT(cfg).to(dev).to(BF16)
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(0, 64, (8, 16), generator=g).to(dev)
        logits = model(ids)
        cross_entropy(logits.reshape(-1, logits.size(-1)),
                      ids.roll(-1, 1).reshape(-1), ignore_index=-1).backward()
        grads.append({n: p.grad.double() for n, p in model.named_parameters()})
    mx.FP8_BACKWARD = False
    for n in grads[0]:
        d = (grads[1][n] - grads[0][n]).norm() / grads[0][n].norm()
        print(json.dumps({"site": "grads nano64 fp8 on vs off", "param": n,
                          "rel_l2": float(f"{float(d):.3e}")}))


def main():
    ap = argparse.ArgumentParser(description=inspect.cleandoc(__doc__),
                                 formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="quant,dgrad,wgrad,layer,grads")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    only = args.only.split(",")
    arms = build_arms(ext, dev, only)
    times = {(s, a): [] for s, d in arms.items() for a in d}
    for d in arms.values():
        for fn, _, _ in d.values():
            for _ in range(3):
                fn()                                       # warm-up
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for s, d in arms.items():
            for a, (fn, _, _) in d.items():
                times[(s, a)].append(time_ms(fn, args.iters))
    for (s, a), t in times.items():
        med = statistics.median(t)
        rec = {"site": s, "arm": a, "median_us": round(med * 1e3, 1),
               "min_us": round(min(t) * 1e3, 1),
               "max_us": round(max(t) * 1e3, 1)}
        _, nbytes, flop = arms[s][a]
        if nbytes:
            rec["MB"] = round(nbytes / 1e6, 1)
            rec["TB_per_s"] = round(nbytes / med / 1e9, 2)
        if flop:
            rec["TFLOP_per_s"] = round(flop / med / 1e9, 0)
        print(json.dumps(rec), flush=True)
    if "grads" in only:
        grad_distance(dev)


if __name__ == "__main__":
    main()
