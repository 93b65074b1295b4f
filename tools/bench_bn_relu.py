"""Fused BatchNorm + [residual add] + ReLU against the composed ops (GPU only).

Shapes: the BN sites of the benchmark's ResNet-50 (batch 256, 64x64 input),
in fp32 (the benchmark's dtype) and in bf16. A site whose channel count is a
block's expanded width is a block tail, y = relu(bn(x) + r); the others are
y = relu(bn(x)). Training mode. Variants, all on the ext ops and the torch
kernels autograd would run:

  cf  composed forward :  batchnorm_fwd [+ torch add] + torch relu
  ff  fused forward    :  batchnorm_relu_fwd
  cb  composed backward:  torch threshold_backward + batchnorm_bwd
  fb  fused backward   :  batchnorm_relu_bwd

Forward + backward is the sum of a path's two variants; backward is timed on
its own from saved forward results. The variants are alternated inside one
process, round after round, and timed with device events; the spread of a
variant over the rounds is reported next to its median so that differences
can be judged against the noise. Bytes are the least each variant must move,
computed from the shape.

Run:  python tools/bench_bn_relu.py [--dtypes float32,bfloat16]
          [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from ravnest_amd.ops import get_ext  # noqa: E402

# (shape, block tail?) at ResNet-50, batch 256, 64x64 input
SITES = [
    ((256, 64, 32, 32), False),
    ((256, 64, 16, 16), False),
    ((256, 256, 16, 16), True),
    ((256, 128, 8, 8), False),
    ((256, 512, 8, 8), True),
    ((256, 256, 4, 4), False),
    ((256, 1024, 4, 4), True),
    ((256, 512, 2, 2), False),
    ((256, 2048, 2, 2), True),
]
KINDS = ("cf", "ff", "cb", "fb")
EPS, MOMENTUM = 1e-5, 0.1


def min_bytes(kind, numel, esize, residual):
    e = numel * esize
    res = 1 if residual else 0
    return {
        # stats: read x | apply: read x, write y | add: read 2, write 1 |
        # relu: read, write
        "cf": e + 2 * e + 3 * e * res + 2 * e,
        # stats: read x | apply: read x [, r], write y
        "ff": e + (2 + res) * e,
        # threshold_backward: read dy, y, write g | stats: read g, x |
        # apply: read g, x, write dx (g doubles as the residual's gradient)
        "cb": 3 * e + 2 * e + 3 * e,
        # stats: read dy, y, x | apply: read dy, y, x, write dx [, dr]
        "fb": 3 * e + (4 + res) * e,
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


def bench_site(ext, dev, shape, residual, dtype, args):
    g = torch.Generator(device=dev).manual_seed(0)
    C = shape[1]
    x = (2 * torch.randn(shape, device=dev, generator=g) + 0.5).to(dtype)
    dy = torch.randn(shape, device=dev, generator=g).to(dtype)
    r = (torch.randn(shape, device=dev, generator=g).to(dtype)
         if residual else None)
    w = torch.rand(C, device=dev, generator=g) + 0.5
    b = torch.randn(C, device=dev, generator=g)
    rm = torch.zeros(C, device=dev)
    rv = torch.ones(C, device=dev)

    def cf():
        y, mean, rstd = ext.batchnorm_fwd(x, w, b, rm, rv, True, MOMENTUM,
                                          EPS)
        if residual:
            y = y + r
        return torch.relu(y), mean, rstd

    def ff():
        return ext.batchnorm_relu_fwd(x, r, w, b, rm, rv, True, MOMENTUM,
                                      EPS)

    y_c, mean, rstd = cf()
    y_f, mean_f, rstd_f = ff()
    assert torch.equal(y_c, y_f), "fused y differs from the composed path's"

    def cb():
        gm = torch.ops.aten.threshold_backward(dy, y_c, 0)
        return ext.batchnorm_bwd(gm, x, w, mean, rstd, True)

    def fb():
        return ext.batchnorm_relu_bwd(dy, x, y_f, w, mean_f, rstd_f, True,
                                      residual)

    assert torch.equal(cb()[0], fb()[0]), "fused dx differs"

    fns = {"cf": cf, "ff": ff, "cb": cb, "fb": fb}
    for k in KINDS:
        for _ in range(args.warmup):
            fns[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in KINDS}
    for rnd in range(args.rounds):
        order = KINDS[rnd % 4:] + KINDS[:rnd % 4]
        for k in order:
            times[k].append(time_calls(fns[k], args.iters))

    numel = x.numel()
    out = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""),
           "residual": residual}
    print(f"  {tuple(shape)} {out['dtype']} "
          f"{'bn+add+relu' if residual else 'bn+relu'}")
    for k in KINDS:
        t = times[k]
        med = statistics.median(t)
        nbytes = min_bytes(k, numel, x.element_size(), residual)
        print(f"    {k}: median {med:8.2f} us  min {min(t):8.2f}  max "
              f"{max(t):8.2f}  spread {(max(t) - min(t)) / med * 100:5.1f}%"
              f"  {nbytes / 1e6:7.1f} MB -> {nbytes / (med * 1e-6) / 1e9:7.1f}"
              f" GB/s")
        out[k] = {"median_us": med, "min_us": min(t), "max_us": max(t),
                  "bytes": nbytes}
    tc = out["cf"]["median_us"] + out["cb"]["median_us"]
    tf = out["ff"]["median_us"] + out["fb"]["median_us"]
    print(f"    forward: composed {out['cf']['median_us']:.2f} us -> fused "
          f"{out['ff']['median_us']:.2f} us; forward + backward: composed "
          f"{tc:.2f} us -> fused {tf:.2f} us")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bn_relu.py needs a GPU: nothing is measured without "
                 "one")
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    dtypes = [getattr(torch, d) for d in args.dtypes.split(",") if d]
    assert dtypes and all(d in (torch.float32, torch.bfloat16)
                          for d in dtypes)
    print(f"bench_bn_relu: training mode, {args.rounds} rounds x "
          f"{args.iters} calls per variant")
    results = []
    for dtype in dtypes:
        for shape, residual in SITES:
            results.append(bench_site(ext, dev, shape, residual, dtype,
                                      args))
    print(json.dumps({"rounds": args.rounds, "iters": args.iters,
                      "sites": results}))


if __name__ == "__main__":
    main()
