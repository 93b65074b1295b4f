#!/usr/bin/env python3
"""Isolated MLM head + loss, forward + backward: the dense path
(F.linear -> ops.cross_entropy -> autograd) against the sparse path
(ops.sparse_mlm_head_loss, live rows only).

    python tools/bench_mlm_head.py [--rows 65536] [--hidden 768]
        [--vocab 30522] [--fractions 0.15,1.0] [--rounds 5] [--calls 5]

Variants alternate round after round in one process; device events time
`calls` consecutive forward+backward calls. Live fraction 1.0 is expected
to be slower than the dense (library GEMM) path: the op then does the same
work on the hand GEMMs.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ravnest_amd.ops import cross_entropy, sparse_mlm_head_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--fractions", default="0.15,1.0")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, Hd, V = args.rows, args.hidden, args.vocab
    h = torch.randn(N, Hd, device=dev).bfloat16().requires_grad_(True)
    W = (torch.randn(V, Hd, device=dev) * 0.02).bfloat16().requires_grad_(True)
    b = torch.zeros(V, device=dev).bfloat16().requires_grad_(True)

    def dense(t):
        return cross_entropy(F.linear(h, W, b), t, -100)

    def sparse(t):
        return sparse_mlm_head_loss(h, W, b, t, -100)

    def timed(fn, t):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            h.grad = W.grad = b.grad = None
            fn(t).backward()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / args.calls

    for frac in [float(f) for f in args.fractions.split(",")]:
        t = torch.randint(0, V, (N,), device=dev)
        if frac < 1.0:
            t[torch.rand(N, device=dev) > frac] = -100
        live = int((t != -100).sum())
        res = {"dense": [], "sparse": []}
        for fn in (dense, sparse):  # warm-up (allocator, library tuning)
            timed(fn, t)
        for _ in range(args.rounds):
            res["dense"].append(timed(dense, t))
            res["sparse"].append(timed(sparse, t))
        print(f"bench_mlm_head: N={N} Hd={Hd} V={V} live fraction {frac} "
              f"({live} rows), {args.rounds} rounds x {args.calls} calls, "
              "fwd+bwd ms per call")
        for k, v in res.items():
            print(f"  {k:6s}: median {statistics.median(v):8.3f}  "
                  f"min {min(v):8.3f}  max {max(v):8.3f}")
        print(f"  sparse / dense = "
              f"{statistics.median(res['sparse']) / statistics.median(res['dense']):.3f}")


if __name__ == "__main__":
    main()
