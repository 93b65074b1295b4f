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

--D 128: fwd, then the backward on both arms, alternated round after
round in one process: the flash kernels (BWD_D128 on; separate and packed
layouts) and the composed torch backward (BWD_D128 off, what
RAVNEST_ATTN_BWD_D128=0 selects). --causal for the causal case. Medians
with min..max; TF/s over the 7 matmul passes (halved work when causal).

--D 64 (default): fwd once, then the backward on both arms, alternated
round after round in one process: the 64-row-stage kernels (bwd64: Delta,
dK+dV, dQ = 7 executed matmul passes) and the 32-row kernels (rows32:
Delta, dV, dK, dQ = 8 executed passes), separate and packed layouts.
Medians with min..max; TF/s on the executed passes and on the 5 passes
the result needs (halved work when causal).

--fwd (D = 64): the forward on both arms, alternated round after round in
one process: the 64-key-stage kernel (fwd64) and the 32-key-tile kernel
(keys32, what RAVNEST_ATTN_FWD64=0 selects), separate and packed layouts,
non-causal and causal, with the (B,1,1,S) additive mask BERT passes (all
zeros) on the non-causal runs. Medians with min..max; TF/s over the two
matmul passes (halved work when causal). The flagship shape is
--B 128 --H 12 --S 512.

--varlen (D = 64): variable-length batches, B sequences inside S. The
varlen op on the packed (T,3,H,64) stream of the live tokens (T rounded up
to 64, one tile table per batch) against the packed kernels with kv_len on
the padded (B,S,3,H,64) batch and against the same kernels on the dense
batch, alternated round after round in one process; fwd and fwd+bwd.
Lengths: the seeded uniform [16, S] draw of examples/bert/provider.py
--var-len, a 25 % fill and a 100 % fill. Medians with min..max and the
work ratio sum(len^2) / (B S^2) next to each. A build without the varlen
entry points runs the other two arms only (the parent-commit run). The
flagship shape is --B 128 --H 12 --S 512.

--decode: cached decoding. Kernel alone: attention_decode against its
composed torch twin, alternated round after round, at B = 8, 32 x
(H=12, D=64), (H=16, D=128) x L = 128, 512, 1023 cached keys inside
S_max = 1024, max_len = L + 1 as generate passes it; time per call
(host enqueue included, which is what the small shapes measure), the
chosen n_split and achieved bytes/s over the live cache (2*B*H*(L+1)*D*2
bytes) next to the HBM peak. End to end (--decode-e2e): gpt2_small in
bf16, B = 8, prompt 128, 128 new tokens, then B = 32, prompt 512;
tokens/s of generate(use_cache=True) against use_cache=False, alternated.
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


def bench_varlen(ext, dev, B, S, H, rounds, iters):
    D, empty = 64, torch.Tensor()
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(42)
    draws = {"uniform[16,S]": torch.randint(16, S + 1, (B,), generator=g),
             "fill 0.25": draw_lengths(B, S, 0.25).long(),
             "fill 1.00": torch.full((B,), S)}
    has_varlen = hasattr(ext, "attn_varlen_fwd_qkv")
    print(f"varlen against padded, B={B} S={S} H={H} D={D}; {rounds} rounds "
          f"x {iters} iters per arm, arms alternated; ms median [min..max]")
    for name, lens in draws.items():
        live = int(lens.sum())
        T = -(-live // 64) * 64
        ratio = float((lens.double() ** 2).sum()) / (B * S * S)
        qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16)
        do = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        keep = (torch.arange(S)[None, :] < lens[:, None]).to(dev)
        pqkv = torch.zeros(T, 3, H, D, device=dev, dtype=torch.bfloat16)
        pdo = torch.zeros(T, H, D, device=dev, dtype=torch.bfloat16)
        pqkv[:live], pdo[:live] = qkv[keep], do[keep]
        kvl = lens.to(device=dev, dtype=torch.int32)
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = lens.cumsum(0)
        cu = cu.to(dev)

        def padded(kv, bwd):
            o, lse = ext.attn_fwd_qkv(qkv, empty, False, scale, 0.0, 0, None,
                                      kv)
            if bwd:
                ext.attn_bwd_qkv(qkv, o, do, lse, empty, False, scale, 0.0,
                                 None, kv)

        def varlen(bwd):
            o, lse = ext.attn_varlen_fwd_qkv(pqkv, cu, tiles, False, scale)
            if bwd:
                ext.attn_varlen_bwd_qkv(pqkv, o, pdo, lse, cu, tiles, False,
                                        scale)

        arms = {"dense": lambda b: padded(None, b),
                "kv_len": lambda b: padded(kvl, b)}
        if has_varlen:
            tiles = ext.attn_varlen_tiles(cu, T)
            arms["varlen"] = varlen
        t = {(a, b): [] for a in arms for b in (False, True)}
        for _ in range(rounds):
            for a, fn in arms.items():
                for b in (False, True):
                    t[(a, b)].append(timeit(lambda: fn(b), iters, 3))
        print(f"{name}: live tokens {live} of {B * S} (T = {T}), work ratio "
              f"sum(len^2)/(B S^2) = {ratio:.3f}")
        for a in arms:
            print(f"  {a:7s} " + "  ".join(
                f"{lab} {statistics.median(x):7.3f} "
                f"[{min(x):7.3f}..{max(x):7.3f}]" for lab, x in
                (("fwd", t[(a, False)]), ("fwd+bwd", t[(a, True)]))))


def bench_d128(ext, dev, B, S, H, D, causal, rounds, iters):
    import importlib
    # ops/__init__ exports the attention() function under the same name
    attn_mod = importlib.import_module("ravnest_amd.ops.attention")
    scale = 1.0 / math.sqrt(D)
    empty = torch.Tensor()
    mm = 2 * B * H * S * S * D * (0.5 if causal else 1.0)
    q, k, v = (torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16,
                           requires_grad=True) for _ in range(3))
    o = attn_mod.attention(q, k, v, causal=causal)   # one graph, both arms
    do = torch.randn_like(o)
    qkv = torch.stack([q, k, v], 0).detach().permute(1, 3, 0, 2, 4)
    qkv = qkv.contiguous()
    o_p, lse_p = ext.attn_fwd_qkv(qkv, empty, causal, scale)[:2]
    do_p = do.transpose(1, 2).contiguous()

    def bwd(flag):
        attn_mod.BWD_D128 = flag
        return torch.autograd.grad(o, (q, k, v), do, retain_graph=True)

    arms = {
        "kernel": lambda: bwd(True),
        "kernel packed": lambda: ext.attn_bwd_qkv(
            qkv, o_p, do_p, lse_p, empty, causal, scale, 0.0, None, None),
        "composed": lambda: bwd(False),
    }
    t_f = timeit(lambda: ext.attn_fwd(q, k, v, empty, causal, scale), iters)
    t = {a: [] for a in arms}
    for _ in range(rounds):
        for a, fn in arms.items():
            t[a].append(timeit(fn, iters, 2))
    attn_mod.BWD_D128 = True
    print(f"B={B} H={H} S={S} D={D} causal={causal}: fwd {t_f:7.3f} ms "
          f"({2 * mm / t_f / 1e9:6.1f} TF/s); bwd {rounds} rounds x {iters} "
          f"iters per arm, arms alternated; ms median [min..max]")
    for a, x in t.items():
        med = statistics.median(x)
        print(f"  bwd {a:13s} {med:8.3f} [{min(x):8.3f}..{max(x):8.3f}] "
              f"({7 * mm / med / 1e9:6.1f} TF/s)")


HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def bench_decode(ext, dev, rounds, iters):
    from ravnest_amd.ops.attention import _decode_twin, attention_decode
    S_max = 1024
    print(f"attention_decode, S_max={S_max}, max_len=L+1; {rounds} rounds x "
          f"{iters} iters per arm, arms alternated; us median [min..max]; "
          f"GB/s over the live cache, HBM peak {HBM_PEAK / 1e9:.0f} GB/s")
    for H, D in ((12, 64), (16, 128)):
        scale = 1.0 / math.sqrt(D)
        for B in (8, 32):
            qkv = torch.randn(B, 3, H, D, device=dev, dtype=torch.bfloat16)
            kc = torch.randn(B, H, S_max, D, device=dev,
                             dtype=torch.bfloat16)
            vc = torch.randn_like(kc)
            for L in (128, 512, 1023):
                cl = torch.full((B,), L, dtype=torch.int32, device=dev)
                arms = {
                    "kernel": lambda: attention_decode(qkv, kc, vc, cl,
                                                       max_len=L + 1),
                    "twin": lambda: _decode_twin(qkv, kc, vc, cl, scale),
                }
                t = {a: [] for a in arms}
                for _ in range(rounds):
                    for a, fn in arms.items():
                        t[a].append(timeit(fn, iters, 3) * 1e3)
                nbytes = 2 * B * H * (L + 1) * D * 2
                ns = ext.attn_decode_splits(B * H, L + 1)
                line = f"B={B:2d} H={H} D={D:3d} L={L:4d} n_split={ns:2d}:"
                for a, x in t.items():
                    med = statistics.median(x)
                    line += (f"  {a} {med:8.1f} [{min(x):8.1f}..{max(x):8.1f}]"
                             f" {nbytes / med / 1e3:7.1f} GB/s")
                print(line)


def bench_decode_e2e(dev, rounds):
    import time
    from ravnest_amd.models.gpt import GPT, GPTConfig
    torch.manual_seed(0)
    cfg = GPTConfig.gpt2_small()
    model = GPT(cfg).to(dev).to(torch.bfloat16).eval()
    # the issue's shape, then one with enough work per step to leave the
    # launch-bound regime
    for B, S0, new in ((8, 128, 128), (32, 512, 128)):
        idx = torch.randint(0, cfg.vocab_size, (B, S0), device=dev)

        def run(use_cache):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(idx, new, use_cache=use_cache)
            torch.cuda.synchronize()
            return B * new / (time.perf_counter() - t0)

        t = {True: [], False: []}
        for flag in t:
            run(flag)  # warm-up: every shape of the timed window
        for _ in range(rounds):
            for flag in t:
                t[flag].append(run(flag))
        print(f"gpt2_small bf16 generate, B={B} prompt={S0} new={new}; "
              f"{rounds} rounds, arms alternated; tokens/s median "
              f"[min..max]")
        for flag, x in t.items():
            print(f"  use_cache={flag!s:5s} {statistics.median(x):9.1f} "
                  f"[{min(x):9.1f}..{max(x):9.1f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--H", type=int, default=12)
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--fill", type=float, nargs="+", default=None,
                    help="live share(s) of a right-padded batch")
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--fwd", action="store_true",
                    help="D=64 forward, 64-key stages against 32-key tiles")
    ap.add_argument("--varlen", action="store_true",
                    help="D=64 varlen op against kv_len on the padded batch")
    ap.add_argument("--decode", action="store_true",
                    help="decode attention kernel against its torch twin")
    ap.add_argument("--decode-e2e", action="store_true",
                    help="gpt2_small generate, cached against uncached")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    from ravnest_amd.ops import get_ext
    ext = get_ext(True)
    dev = torch.device("cuda", 0)
    B, S, H, D = args.B, args.S, args.H, args.D
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(0)
    if args.decode or args.decode_e2e:
        if args.decode:
            bench_decode(ext, dev, args.rounds, args.iters)
        if args.decode_e2e:
            bench_decode_e2e(dev, min(args.rounds, 5))
        return
    if args.varlen:
        bench_varlen(ext, dev, B, S, H, args.rounds, args.iters)
        return
    if args.fwd:
        for causal in (False, True):
            bench_fwd64(ext, dev, B, S, H, causal, args.rounds, args.iters)
        return
    if args.fill:
        bench_fill(ext, dev, B, S, H, D, args.fill, args.rounds, args.iters)
        return
    if D == 128:
        bench_d128(ext, dev, B, S, H, D, args.causal, args.rounds,
                   args.iters)
        return

    bench_d64(ext, dev, B, S, H, D, args.causal, args.rounds, args.iters)


def bench_fwd64(ext, dev, B, S, H, causal, rounds, iters):
    D = 64
    scale = 1.0 / math.sqrt(D)
    mm = 2 * B * H * S * S * D * (0.5 if causal else 1.0)  # one matmul pass
    q, k, v = (torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16)
               for _ in range(3))
    qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16)
    mask = (torch.Tensor() if causal
            else torch.zeros(B, 1, 1, S, device=dev))
    arms = {}
    for name, flag in (("keys32", False), ("fwd64", True)):
        arms[f"{name} separate"] = (
            lambda f=flag: ext.attn_fwd(q, k, v, mask, causal, scale, None,
                                        f))
        arms[f"{name} packed"] = (
            lambda f=flag: ext.attn_fwd_qkv(qkv, mask, causal, scale, 0.0, 0,
                                            None, None, f))
    t = {a: [] for a in arms}
    for _ in range(rounds):
        for a, fn in arms.items():
            t[a].append(timeit(fn, iters, 2))
    print(f"fwd B={B} H={H} S={S} D={D} causal={causal} "
          f"mask={'none' if causal else 'zeros'}: {rounds} rounds x {iters} "
          f"iters per arm, arms alternated; ms median [min..max]")
    for a, x in t.items():
        med = statistics.median(x)
        print(f"  fwd {a:16s} {med:8.4f} [{min(x):8.4f}..{max(x):8.4f}] "
              f"({2 * mm / med / 1e9:6.1f} TF/s)")


def bench_d64(ext, dev, B, S, H, D, causal, rounds, iters):
    scale = 1.0 / math.sqrt(D)
    empty = torch.Tensor()
    mm = 2 * B * H * S * S * D * (0.5 if causal else 1.0)  # one matmul pass
    q, k, v = (torch.randn(B, H, S, D, device=dev, dtype=torch.bfloat16)
               for _ in range(3))
    o, lse = ext.attn_fwd(q, k, v, empty, causal, scale)
    do = torch.randn_like(o)
    qkv = torch.randn(B, S, 3, H, D, device=dev, dtype=torch.bfloat16)
    o2, lse2 = ext.attn_fwd_qkv(qkv, empty, causal, scale)[:2]
    do2 = torch.randn_like(o2)
    t_f = timeit(lambda: ext.attn_fwd(q, k, v, empty, causal, scale), iters)
    t_f2 = timeit(lambda: ext.attn_fwd_qkv(qkv, empty, causal, scale), iters)

    def sep(flag):
        return lambda: ext.attn_bwd(q, k, v, o, do, lse, empty, causal,
                                    scale, None, flag)

    def packed(flag):
        return lambda: ext.attn_bwd_qkv(qkv, o2, do2, lse2, empty, causal,
                                        scale, 0.0, None, None, flag)

    # arm -> (callable, executed matmul passes)
    arms = {"rows32 separate": (sep(False), 8),
            "bwd64 separate": (sep(True), 7),
            "rows32 packed": (packed(False), 8),
            "bwd64 packed": (packed(True), 7)}
    t = {a: [] for a in arms}
    for _ in range(rounds):
        for a, (fn, _) in arms.items():
            t[a].append(timeit(fn, iters, 2))
    print(f"B={B} H={H} S={S} D={D} causal={causal}: fwd separate "
          f"{t_f:7.3f} ms ({2 * mm / t_f / 1e9:6.1f} TF/s), packed "
          f"{t_f2:7.3f} ms ({2 * mm / t_f2 / 1e9:6.1f} TF/s); bwd {rounds} "
          f"rounds x {iters} iters per arm, arms alternated; ms median "
          f"[min..max]")
    for a, (_, passes) in arms.items():
        x = t[a]
        med = statistics.median(x)
        print(f"  bwd {a:16s} {med:8.3f} [{min(x):8.3f}..{max(x):8.3f}] "
              f"({passes * mm / med / 1e9:6.1f} TF/s executed, "
              f"{5 * mm / med / 1e9:6.1f} useful)")


if __name__ == "__main__":
    main()
