"""The Linear bias gradient out of dropout_add_ln_bwd, and the column-group
bias-GELU forward, each against the arm it replaces (GPU only).

At the BERT-base shapes of the flagship benchmark (micro-batch 128 x seq 512:
N = 65536 rows, hidden 768, intermediate 3072), on the ext ops, with the
variants alternated inside one process round after round and timed with
device events:

  ln0   dropout_add_ln_bwd, then dz.sum(0)   (what autograd's addmm backward
        does for the bias of the Linear that produced z)
  ln1   dropout_add_ln_bwd_dzsum             (the sum out of the same kernel)
  lnb   dropout_add_ln_bwd alone             (the kernel both arms start from)

  gf0 / gf1   bias_gelu_fwd, RAVNEST_GELU_V1=1 / column-group kernel
  gb          bias_gelu_bwd_db (one kernel; for its bytes per second)

Bytes are the least each kernel must move, from the shapes; for the arm
with a separate reduction they include its re-read of the gradient. The
spread of a variant over the rounds is printed next to its median.

Run:  python tools/bench_bias_grad.py [--parts ln,gelu] [--rounds 9]
          [--iters 20] [--batch 128] [--seq 512]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from ravnest_amd.ops import get_ext  # noqa: E402

SEED = 1234567890123


def time_calls(fn, iters):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3  # us per call


def v1(flag):
    # read by csrc/gelu.hip at every call
    os.environ["RAVNEST_GELU_V1"] = "1" if flag else "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ln,gelu")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--inter", type=int, default=3072)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bias_grad.py needs a GPU: nothing is measured "
                 "without one")
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    B, S, H, I = args.batch, args.seq, args.hidden, args.inter
    n = B * S
    parts = [p for p in args.parts.split(",") if p]
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, device=dev, generator=g) * scale).to(
            torch.bfloat16)

    fns, nbytes = {}, {}
    if "ln" in parts:
        z, a, dy = rnd(n, H), rnd(n, H), rnd(n, H)
        w, b = rnd(H), rnd(H)
        sb = torch.zeros(1, dtype=torch.int64, device=dev)
        _, s, mean, rstd, bits = ext.dropout_add_ln_fwd(
            z, a, w, b, 1e-12, 0.1, SEED, sb)
        del z, a
        e = n * H
        base = 4 * (2 * e) + e // 8 + 8 * n  # dy, s, bits in; dx, dz out

        def lnb():
            ext.dropout_add_ln_bwd(dy, s, w, mean, rstd, bits, 0.1)

        def ln0():
            ext.dropout_add_ln_bwd(dy, s, w, mean, rstd, bits, 0.1)[1].sum(0)

        def ln1():
            ext.dropout_add_ln_bwd_dzsum(dy, s, w, mean, rstd, bits, 0.1,
                                         True)

        fns.update(lnb=lnb, ln0=ln0, ln1=ln1)
        nbytes.update(lnb=base, ln0=base + 2 * e, ln1=base)
    if "gelu" in parts:
        x, gy = rnd(n, I), rnd(n, I)
        bias = rnd(I, scale=0.1)
        e = n * I

        def gf(flag):
            def f():
                v1(flag)
                ext.bias_gelu_fwd(x, bias)
            return f

        def gb():
            ext.bias_gelu_bwd_db(gy, x, bias)

        fns.update(gf0=gf(True), gf1=gf(False), gb=gb)
        nbytes.update(gf0=4 * e, gf1=4 * e, gb=6 * e)

    kinds = list(fns)
    for k in kinds:
        for _ in range(args.warmup):
            fns[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for r in range(args.rounds):
        order = kinds[r % len(kinds):] + kinds[:r % len(kinds)]
        for k in order:
            times[k].append(time_calls(fns[k], args.iters))
    v1(False)

    print(f"bench_bias_grad: B={B} S={S} hidden={H} inter={I} bf16, "
          f"{args.rounds} rounds x {args.iters} calls per variant")
    result = {"batch": B, "seq": S, "hidden": H, "inter": I,
              "rounds": args.rounds, "iters": args.iters}
    for k in kinds:
        t = times[k]
        med = statistics.median(t)
        print(f"  variant {k}: median {med:8.2f} us  min {min(t):8.2f}  "
              f"max {max(t):8.2f}  spread {(max(t) - min(t)) / med * 100:.1f}%"
              f"  {nbytes[k] / 1e6:.0f} MB -> "
              f"{nbytes[k] / (med * 1e-6) / 1e12:.2f} TB/s")
        result[k] = {"median_us": med, "min_us": min(t), "max_us": max(t),
                     "bytes": nbytes[k]}
    if "ln0" in result:
        mb, mo, mn = (result[k]["median_us"] for k in ("lnb", "ln0", "ln1"))
        print(f"  dropout_add_ln_bwd: alone {mb:.2f} us; with the separate "
              f"reduction {mo:.2f} (+{mo - mb:.2f}); with the sum fused "
              f"{mn:.2f} (+{mn - mb:.2f})")
    if "gf0" in result:
        print(f"  bias_gelu_fwd: V1 {result['gf0']['median_us']:.2f} us -> "
              f"{result['gf1']['median_us']:.2f} us")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
