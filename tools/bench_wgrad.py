#!/usr/bin/env python3
"""Isolated A/B of the BERT-base weight-gradient GEMMs at M = 65536.

    python tools/bench_wgrad.py --out FILE [--rounds 15]

Arms, alternated round by round and timed with device events:
  (a) the library call autograd makes for a linear layer's weight,
      dy2.t().mm(x2), plus dy2.sum(0) where the layer has a bias;
  (b) gemm_wgrad_bf16 (128x128 tiles, fp32 atomics) plus its cast;
  (c) gemm_wgrad256_bf16 (256x256 tiles, finalize kernel), with and
      without the bias gradient.
Prints median (min-max) microseconds and TFLOP/s per arm and writes the
same text to --out; nothing else is written.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_TUNED = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "tunableop_mi355x.csv")
if os.path.exists(_TUNED) and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ:
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = _TUNED

import torch  # noqa: E402

M = 65536
# name, N, K, the layer's bias gradient comes from its own reduction
SHAPES = [("qkv", 2304, 768, True), ("attn.out", 768, 768, False),
          ("mlp_in", 3072, 768, False), ("mlp_out", 768, 3072, False),
          ("head.dense", 768, 768, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wgrad.py needs a GPU")
    from ravnest_amd.ops import get_ext
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; M = {M}; "
             f"{args.rounds} rounds x {args.inner} calls, arms alternated; "
             "us per call: median (min-max)"]

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / args.inner

    for name, N, K, has_db in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N + K)
        dy = (torch.randn(M, N, device=dev, generator=g) / 256).to(
            torch.bfloat16)
        x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        arms = {
            "a lib": lambda: dy.t().mm(x),
            "b hand128+cast": lambda: ext.gemm_wgrad_bf16(dy, x).to(
                torch.bfloat16),
            "c wgrad256": lambda: ext.gemm_wgrad256_bf16(dy, x, False,
                                                         False),
        }
        if has_db:
            arms["a lib+sum"] = lambda: (dy.t().mm(x), dy.sum(0))
            arms["sum alone"] = lambda: dy.sum(0)
            arms["c wgrad256+db"] = lambda: ext.gemm_wgrad256_bf16(
                dy, x, True, False)
        for fn in arms.values():   # warm up: code objects, algorithms
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn))
        flop = 2.0 * M * N * K
        ntiles = (N // 256) * (K // 256)
        split = min(M // 64, max(1, 256 // ntiles))
        lines.append(f"{name}: N={N} K={K}  {flop / 1e9:.0f} GFLOP; "
                     f"wgrad256 split {split}, finalize reads "
                     f"{split * N * K * 4 / 1e6:.1f} MB of partials and "
                     f"writes {N * K * 2 / 1e6:.1f} MB")
        for k, t in times.items():
            med = statistics.median(t)
            tf = "" if k == "sum alone" else \
                f"  {flop / med / 1e6:7.0f} TF at the median"
            lines.append(f"  {k:16s} {med:8.1f} ({min(t):.1f}-{max(t):.1f})"
                         f"{tf}")
        del dy, x
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
