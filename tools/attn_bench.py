#!/usr/bin/env python3
"""Attention kernel micro-bench: fwd/bwd wall time + effective TF/s for
both layouts (separate (B,H,S,D) and packed (B,S,3,H,D)).

Usage (GPU box): python tools/attn_bench.py [--B 32] [--S 512] [--H 12]

--fill F [F ...]: padded-batch mode. For each live share F the packed fwd
and bwd are timed on a right-padded batch (seeded lengths, mean F*S) in
three modes, alternated round after round in one process: additive mask
only (KV_SKIP off), mask with the key horizon derived on the device
(KV_SKIP on, derivation launch included), explicit kv_len without mask.
Medians and min..max spreads per mode; useful FLOPs counted from the
lengths (every query row against the sequence's live keys).
"""
import argparse
import math
import statistics
import sys
import os

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def draw_lengths(B, S, fill, seed=0):
    """Seeded right-padding lengths with mean ~ fill*S: uniform on
    [fill*S - w, fill*S + w], w = min(fill, 1 - fill) * S / 2."""
    g = torch.Generator().manual_seed(seed)
    w = min(fill, 1.0 - fill) * S / 2
    lens = fill * S + (torch.rand(B, generator=g) * 2 - 1) * w
    return lens.round().clamp(1, S).to(torch.int32)


def bench_fill(ext, dev, B, S, H, D, fills, rounds, iters):
    scale = 1.0 / math.sqrt(D)
    empty = torch.Tensor()
    qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16)
    do = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
    cols = torch.arange(S, device=dev)
    full_mm = 2 * B * H * S * S * D
    print(f"packed fwd/bwd, B={B} S={S} H={H} D={D}; {rounds} rounds x "
          f"{iters} iters per mode, modes alternated; ms median [min..max]")
    for fill in fills:
        lens = draw_lengths(B, S, fill).to(dev)
        mask = ((cols[None, :] >= lens[:, None]).float()
                * -10000.0).view(B, 1, 1, S)
        lf = lens.float()
        useful = lf.sum().item() / (B * S)  # live share of the S x S work

        def fwd(mode):
            if mode == "mask":
                return ext.attn_fwd_qkv(qkv, mask, False, scale)
            if mode == "mask+derived":
                kvl = ext.attn_mask_kv_len(mask)
                return ext.attn_fwd_qkv(qkv, mask, False, scale, 0.0, 0,
                                        None, kvl) + [kvl]
            return ext.attn_fwd_qkv(qkv, empty, False, scale, 0.0, 0, None,
                                    lens) + [lens]

        modes = ["mask", "mask+derived", "kv_len"]
        saved = {m: fwd(m) for m in modes}

        def bwd(mode):
            r = saved[mode]
            kvl = r[2] if len(r) > 2 else None
            m = empty if mode == "kv_len" else mask
            return ext.attn_bwd_qkv(qkv, r[0], do, r[1], m, False, scale,
                                    0.0, None, kvl)

        t = {(m, d): [] for m in modes for d in ("fwd", "bwd")}
        for _ in range(rounds):
            for m in modes:
                t[(m, "fwd")].append(timeit(lambda: fwd(m), iters, 2))
                t[(m, "bwd")].append(timeit(lambda: bwd(m), iters, 2))
        print(f"fill {fill:.2f}: lengths mean {lf.mean().item():.1f} "
              f"min {int(lf.min())} max {int(lf.max())} "
              f"std {lf.std().item():.1f}; useful FLOP share {useful:.3f}")
        for m in modes:
            parts = []
            for d, nmm in (("fwd", 2), ("bwd", 7)):
                x = t[(m, d)]
                med = statistics.median(x)
                parts.append(
                    f"{d} {med:7.3f} [{min(x):7.3f}..{max(x):7.3f}] "
                    f"({nmm * full_mm * useful / med / 1e9:6.1f} useful TF/s)")
            print(f"  {m:13s} " + "  ".join(parts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--fill", type=float, nargs="+", default=None,
                    help="live share(s) of a right-padded batch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    dev = torch.device("cuda", 0)
    B, S, H, D = args.B, args.S, args.H, args.D
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    if args.fill:
        bench_fill(ext, dev, B, S, H, D, args.fill, args.rounds, args.iters)
        return

    # FLOPs: fwd 2 matmuls, bwd 7 matmul passes (S,dP twice + dV,dK,dQ)
    mm = 2 * B * H * S * S * D  # one S x S x D matmul pass (x2 flops)
    fwd_fl, bwd_fl = 2 * mm, 7 * mm

    q, k, v = (torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16)
               for _ in range(3))
    empty = torch.Tensor()
    o, lse = ext.attn_fwd(q, k, v, empty, False, scale)
    do = torch.randn_like(o)
    t_f = timeit(lambda: ext.attn_fwd(q, k, v, empty, False, scale))
    t_b = timeit(lambda: ext.attn_bwd(q, k, v, o, do, lse, empty, False,
                                      scale))
    print(f"separate: fwd {t_f:7.3f} ms ({fwd_fl/t_f/1e9:7.1f} TF/s)  "
          f"bwd {t_b:7.3f} ms ({bwd_fl/t_b/1e9:7.1f} TF/s)")

    qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16)
    o2, lse2 = ext.attn_fwd_qkv(qkv, empty, False, scale)
    do2 = torch.randn_like(o2)
    t_f2 = timeit(lambda: ext.attn_fwd_qkv(qkv, empty, False, scale))
    t_b2 = timeit(lambda: ext.attn_bwd_qkv(qkv, o2, do2, lse2, empty, False,
                                           scale))
    print(f"packed:   fwd {t_f2:7.3f} ms ({fwd_fl/t_f2/1e9:7.1f} TF/s)  "
          f"bwd {t_b2:7.3f} ms ({bwd_fl/t_b2/1e9:7.1f} TF/s)")


if __name__ == "__main__":
    main()
