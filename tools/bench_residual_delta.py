"""Isolated timings of the two passes taken out of the BERT step
(profiles/residual_delta.txt), at the flagship's shapes.

  ln   LayerNorm backward with a two-addend upstream gradient, N = B * S rows:
         add+bwd  dy + dy2 (the stock bf16 add), then dropout_add_ln_bwd_dzsum
         bwd2     dropout_add_ln_bwd_dzsum(dy, ..., dy2): the kernel adds
  attn attention backward, packed (B,S,3,H,D) qkv, D = 64, with
       RAVNEST_ATTN_DELTA_FUSED (read by csrc/attention_bwd64.hip per call):
         delta0   Delta kernel, kv, dq
         delta1   dq (computes and stores Delta), kv
       Per-kernel times come from a rocprofv3 --kernel-trace run of this
       script; here the whole backward is timed with device events.

Variants are alternated round by round; bytes are the ones the algorithm has
to move. Run:  python tools/bench_residual_delta.py [--parts ln,attn]
"""
import argparse
import json
import math
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ln,attn")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_residual_delta.py needs a GPU: nothing is measured "
                 "without one")
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    B, S, H, A = args.batch, args.seq, args.hidden, args.heads
    n = B * S
    parts = [p for p in args.parts.split(",") if p]
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)

    fns, nbytes = {}, {}
    if "ln" in parts:
        z, a, dy, dy2 = rnd(n, H), rnd(n, H), rnd(n, H), rnd(n, H)
        w, b = rnd(H), rnd(H)
        sb = torch.zeros(1, dtype=torch.int64, device=dev)
        _, s, mean, rstd, bits = ext.dropout_add_ln_fwd(
            z, a, w, b, 1e-12, 0.1, SEED, sb)
        del z, a
        e = n * H
        one = 4 * (2 * e) + e // 8 + 8 * n  # dy, s, bits in; dx, dz out

        def add_bwd():
            ext.dropout_add_ln_bwd_dzsum(dy + dy2, s, w, mean, rstd, bits,
                                         0.1, True)

        def bwd2():
            ext.dropout_add_ln_bwd_dzsum(dy, s, w, mean, rstd, bits, 0.1,
                                         True, dy2)

        fns.update({"add+bwd": add_bwd, "bwd2": bwd2})
        nbytes.update({"add+bwd": one + 6 * e, "bwd2": one + 2 * e})
    if "attn" in parts:
        D = H // A
        scale = 1.0 / math.sqrt(D)
        qkv = rnd(B, S, 3, A, D)
        do = rnd(B, S, A, D)
        empty = torch.Tensor()
        o, lse = ext.attn_fwd_qkv(qkv, empty, False, scale, 0.0, 0, None,
                                  None)[:2]

        def attn(flag):
            def f():
                os.environ["RAVNEST_ATTN_DELTA_FUSED"] = flag
                ext.attn_bwd_qkv(qkv, o, do, lse, empty, False, scale)
            return f

        e = B * S * A * D
        fns.update(delta0=attn("0"), delta1=attn("1"))
        # q, k, v, dO in and dq, dk, dv out once per kernel that uses them
        # (kv: 4 in 2 out, dq: 4 in 1 out), O + dO for Delta
        nbytes.update(delta0=2 * e * (6 + 5 + 2), delta1=2 * e * (6 + 5 + 1))

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
    os.environ.pop("RAVNEST_ATTN_DELTA_FUSED", None)  # back to the default

    print(f"bench_residual_delta: B={B} S={S} hidden={H} heads={A} bf16, "
          f"{args.rounds} rounds x {args.iters} calls per variant")
    result = {"batch": B, "seq": S, "hidden": H, "heads": A,
              "rounds": args.rounds, "iters": args.iters}
    for k in kinds:
        t = times[k]
        med = statistics.median(t)
        print(f"  variant {k}: median {med:8.2f} us  min {min(t):8.2f}  "
              f"max {max(t):8.2f}  spread {(max(t) - min(t)) / med * 100:.1f}%"
              f"  {nbytes[k] / 1e6:.0f} MB -> "
              f"{nbytes[k] / (med * 1e-6) / 1e9:.0f} GB/s")
        result[k] = {"median_us": med, "min_us": min(t), "max_us": max(t),
                     "bytes": nbytes[k]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
