"""Fused dropout + residual add + LayerNorm against the composed ops (GPU only).

y = LN(a + dropout(z)) on an N x H bf16 activation (default 65536 x 768, the
BERT-base layer at micro-batch 128 x seq 512), p = 0.1, fp32 or bf16 LN
parameters. Variants, all on the ext ops with one fixed seed:

  cf  composed forward :  dropout_fwd + layernorm_add_fwd
  ff  fused forward    :  dropout_add_ln_fwd
  cb  composed backward:  layernorm_bwd (+ the two dw/db casts it does) +
                          dx.clone() + dropout_bwd, as autograd runs them
  fb  fused backward   :  dropout_add_ln_bwd

Forward + backward is the sum of a path's two variants; backward is timed on
its own from saved forward results, so each figure is one direction. The
variants are alternated inside one process, round after round, and timed
with device events; the spread of a variant over the rounds is reported
next to its median so that differences can be judged against the noise.
Bytes are the least each variant must move, computed from the shapes.

Run:  python tools/bench_dropout_ln.py [--rows 65536] [--hidden 768]
          [--wdtype float32] [--rounds 9] [--iters 20]
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


def min_bytes(kind, n, h):
    e = n * h          # elements; bf16 = 2 B each
    small = 8 * n      # mean + rstd, fp32
    return {
        # read z, write d + byte mask | read a, d, write s, y
        "cf": 2 * e + 2 * e + e + 4 * (2 * e) + small,
        # read z, a, write s, y, bit mask
        "ff": 4 * (2 * e) + e // 8 + small,
        # dx kernel: read dy, s, write dx | dwdb: read dy, s | clone: read,
        # write | dropout_bwd: read dx, byte mask, write dz
        "cb": 3 * (2 * e) + 2 * (2 * e) + 2 * (2 * e) + 2 * (2 * e) + e
        + 2 * small,
        # read dy, s, bit mask, write dx, dz
        "fb": 4 * (2 * e) + e // 8 + small,
    }[kind]


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
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--wdtype", default="float32",
                    choices=["float32", "bfloat16"])
    ap.add_argument("--variants", default="cf,ff,cb,fb")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dropout_ln.py needs a GPU: nothing is measured "
                 "without one")
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    n, h, p = args.rows, args.hidden, args.p
    kinds = [k for k in args.variants.split(",") if k]
    assert kinds and all(k in ("cf", "ff", "cb", "fb") for k in kinds)

    g = torch.Generator(device=dev).manual_seed(0)
    z, a, dy = (torch.randn(n, h, device=dev, generator=g).to(torch.bfloat16)
                for _ in range(3))
    wdt = getattr(torch, args.wdtype)
    w = torch.randn(h, device=dev, generator=g).to(wdt)
    b = torch.randn(h, device=dev, generator=g).to(wdt)
    sb = torch.zeros(1, dtype=torch.int64, device=dev)
    eps = 1e-12

    d, mask = ext.dropout_fwd(z, p, SEED, sb)
    _, s_c, mean_c, rstd_c = ext.layernorm_add_fwd(a, d, w, b, eps)
    _, s_f, mean_f, rstd_f, bits = ext.dropout_add_ln_fwd(
        z, a, w, b, eps, p, SEED, sb)
    assert torch.equal(s_c, s_f), "fused s differs from the composed path's"
    del d

    def cf():
        d_, _m = ext.dropout_fwd(z, p, SEED, sb)
        ext.layernorm_add_fwd(a, d_, w, b, eps)

    def ff():
        ext.dropout_add_ln_fwd(z, a, w, b, eps, p, SEED, sb)

    def cb():
        dx, _dw, _db = ext.layernorm_bwd(dy, s_c, w, mean_c, rstd_c)
        _da = dx.clone()
        ext.dropout_bwd(dx, mask, p)

    def fb():
        ext.dropout_add_ln_bwd(dy, s_f, w, mean_f, rstd_f, bits, p)

    fns = {"cf": cf, "ff": ff, "cb": cb, "fb": fb}
    for k in kinds:
        for _ in range(args.warmup):
            fns[k]()
    torch.cuda.synchronize()

    times = {k: [] for k in kinds}
    for r in range(args.rounds):
        order = kinds[r % len(kinds):] + kinds[:r % len(kinds)]
        for k in order:
            times[k].append(time_calls(fns[k], args.iters))

    print(f"bench_dropout_ln: N={n} H={h} bf16, p={p}, LN params "
          f"{args.wdtype}, {args.rounds} rounds x {args.iters} calls per "
          f"variant")
    result = {"rows": n, "hidden": h, "p": p, "wdtype": args.wdtype,
              "rounds": args.rounds, "iters": args.iters}
    for k in kinds:
        t = times[k]
        med = statistics.median(t)
        nbytes = min_bytes(k, n, h)
        print(f"  variant {k}: median {med:8.2f} us  min {min(t):8.2f}  "
              f"max {max(t):8.2f}  spread {(max(t) - min(t)) / med * 100:.1f}%"
              f"  {nbytes / 1e6:.0f} MB -> {nbytes / (med * 1e-6) / 1e12:.2f}"
              f" TB/s")
        result[k] = {"median_us": med, "min_us": min(t), "max_us": max(t),
                     "bytes": nbytes}
    for c, f, name in (("cf", "ff", "forward"), ("cb", "fb", "backward")):
        if c in result and f in result:
            print(f"  {name}: composed {result[c]['median_us']:.2f} us -> "
                  f"fused {result[f]['median_us']:.2f} us")
    if all(k in result for k in ("cf", "ff", "cb", "fb")):
        tc = result["cf"]["median_us"] + result["cb"]["median_us"]
        tf = result["ff"]["median_us"] + result["fb"]["median_us"]
        print(f"  forward + backward: composed {tc:.2f} us -> fused "
              f"{tf:.2f} us")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
