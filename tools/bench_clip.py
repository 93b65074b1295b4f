"""Cost of global-norm gradient clipping on the optimizer step (GPU only).

Model: BertForMLM(BertConfig.base()) in bf16 with fp32-master FusedAdam and
seeded random gradients; only the optimizer step is timed. Variants:

  a  FusedAdam(max_grad_norm=None)                      (no clipping)
  b  FusedAdam(max_grad_norm=1.0)                       (fused clipping)
  c  torch.nn.utils.clip_grad_norm_ + variant a         (stock clipping)

Each variant owns a copy of the parameters and gradients. The variants are
alternated inside one process, round after round, and timed with device
events; the spread of a variant over the rounds is reported next to its
median so that differences can be judged against the noise. Bytes moved
are computed from the shapes (the least each variant has to move).

Run:  python tools/bench_clip.py [--variants a,b,c] [--rounds 9] [--iters 20]
(--variants a runs on a tree without the option, for A/B against it.)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from ravnest_amd.models import BertConfig, BertForMLM  # noqa: E402
from ravnest_amd.ops import FusedAdam, get_ext  # noqa: E402

# bytes per parameter, bf16 param/grad + fp32 master/m/v:
# read g 2 + read m,v,master 12 + write m,v,master 12 + write p 2
ADAM_BYTES = 28
EXTRA_BYTES = {"a": 0,
               "b": 2,   # one more read of g (squared-norm pass)
               "c": 6}   # norm read 2 + in-place scale read 2, write 2


def make_variant(kind, shapes, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    ps = []
    for s in shapes:
        p = (torch.randn(s, device=dev, generator=g) * 0.02).to(
            torch.bfloat16).requires_grad_(True)
        p.grad = (torch.randn(s, device=dev, generator=g) * 0.01).to(
            torch.bfloat16)
        ps.append(p)
    if kind == "b":
        opt = FusedAdam(ps, lr=1e-4, max_grad_norm=1.0)
    else:
        opt = FusedAdam(ps, lr=1e-4)
    if kind == "c":
        def step():
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()
    else:
        step = opt.step
    return step, opt


def time_steps(step, iters):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip.py needs a GPU: nothing is measured without one")
    get_ext(required=True)
    dev = torch.device("cuda", 0)
    kinds = [k for k in args.variants.split(",") if k]
    assert kinds and all(k in EXTRA_BYTES for k in kinds), args.variants

    shapes = [tuple(p.shape) for p in
              BertForMLM(BertConfig.base()).parameters()]
    nparam = sum(torch.Size(s).numel() for s in shapes)
    steps = {k: make_variant(k, shapes, dev) for k in kinds}
    for k in kinds:
        for _ in range(args.warmup):
            steps[k][0]()
    torch.cuda.synchronize()

    times = {k: [] for k in kinds}
    for r in range(args.rounds):
        order = kinds[r % len(kinds):] + kinds[:r % len(kinds)]
        for k in order:
            times[k].append(time_steps(steps[k][0], args.iters))

    print(f"bench_clip: BERT-base bf16 + fp32-master FusedAdam, "
          f"{len(shapes)} tensors, {nparam / 1e6:.1f} M params, "
          f"{args.rounds} rounds x {args.iters} steps per variant")
    result = {"params": nparam, "rounds": args.rounds, "iters": args.iters}
    for k in kinds:
        t = times[k]
        med = statistics.median(t)
        nbytes = nparam * (ADAM_BYTES + EXTRA_BYTES[k])
        print(f"  variant {k}: median {med:.4f} ms/step  "
              f"min {min(t):.4f}  max {max(t):.4f}  "
              f"spread {(max(t) - min(t)) / med * 100:.1f}%  "
              f"{nbytes / 1e6:.0f} MB/step -> "
              f"{nbytes / (med * 1e-3) / 1e12:.2f} TB/s")
        result[k] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t),
                     "bytes": nbytes}
    if "b" in kinds:
        st = steps["b"][1].grad_norm_stats().tolist()
        print(f"  variant b stats: norm {st[0]:.4f}  coef {st[1]:.6f}  "
              f"nonfinite {st[2]:.0f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
