"""The passes around the MX fp8 GEMMs: composed against fused (GPU only).

Sites (GPT-2-small, micro-batch 32 x seq 1024 = 32768 rows):

  ln      32768 x 768          LayerNorm, then quantise    (ln1 -> qkv)
  gelu    32768 x 3072         bias-GELU, then quantise    (mlp_in -> mlp_out)
  quant   32768 x 768          stand-alone mx_quant        (attn out -> proj)
  quantw  2304 x 768           stand-alone mx_quant        (a weight)
  gemm    32768 x 768 x 2304   mx_gemm2, then + bias       (qkv)
  gemm    32768 x 3072 x 768   mx_gemm2, then + bias       (mlp_out)

Arms: `composed` runs the separate kernels (layernorm_fwd + mx_quant,
bias_gelu_fwd + mx_quant, mx_gemm2 + torch add); `fused` runs
layernorm_mx_fwd, bias_gelu_mx_fwd and mx_gemm2(..., bias). Only the entry
points the built extension has are run, so the tool also runs on a tree
from before the fused kernels and then times the composed arm alone; to
compare two trees, alternate the two checkouts' runs in one session.

The arms are alternated inside one process, round after round, and timed
with device events; each line gives the median over the rounds and the
min-max spread, so a difference can be judged against the noise.

Run:  python tools/bench_mx_quant.py [--rounds 7] [--iters 20] [--tag NAME]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from ravnest_amd.ops import get_ext  # noqa: E402

BF16 = torch.bfloat16
ROWS = 32768


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def build_arms(ext, dev):
    """-> {site: {arm: callable}}"""
    g = torch.Generator(device=dev).manual_seed(0)

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=dev).to(BF16)

    arms = {}
    # LayerNorm + quantise
    x, w, b = randn(ROWS, 768), randn(768), randn(768)
    site = arms.setdefault("ln 32768x768", {})
    site["composed"] = lambda: ext.mx_quant(
        ext.layernorm_fwd(x, w, b, 1e-5)[0])
    if hasattr(ext, "layernorm_mx_fwd"):
        site["fused"] = lambda: ext.layernorm_mx_fwd(x, w, b, 1e-5)
    # bias-GELU + quantise
    h, hb = randn(ROWS, 3072), randn(3072)
    site = arms.setdefault("gelu 32768x3072", {})
    site["composed"] = lambda: ext.mx_quant(ext.bias_gelu_fwd(h, hb))
    if hasattr(ext, "bias_gelu_mx_fwd"):
        site["fused"] = lambda: ext.bias_gelu_mx_fwd(h, hb)
    # stand-alone quantise (same entry point on both trees)
    wt = randn(2304, 768)
    arms["quant 32768x768"] = {"composed": lambda: ext.mx_quant(x)}
    arms["quantw 2304x768"] = {"composed": lambda: ext.mx_quant(wt)}
    # GEMM + bias
    try:
        has_bias = "bias" in (ext.mx_gemm2.__doc__ or "")
    except AttributeError:
        has_bias = False
    for M, K, N in ((ROWS, 768, 2304), (ROWS, 3072, 768)):
        xq, xs = ext.mx_quant(randn(M, K))
        wq, ws = ext.mx_quant(randn(N, K))
        bias = randn(N)
        site = arms.setdefault(f"gemm {M}x{K}x{N}", {})
        site["composed"] = (lambda xq=xq, xs=xs, wq=wq, ws=ws, bias=bias:
                            ext.mx_gemm2(xq, xs, wq, ws) + bias)
        if has_bias:
            site["fused"] = (lambda xq=xq, xs=xs, wq=wq, ws=ws, bias=bias:
                             ext.mx_gemm2(xq, xs, wq, ws, bias))
    return arms


def main():
    ap = argparse.ArgumentParser(description=inspect.cleandoc(__doc__),
                                 formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tag", default="", help="label printed on every line")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = get_ext(required=True)
    dev = torch.device("cuda", 0)
    arms = build_arms(ext, dev)
    times = {(s, a): [] for s, d in arms.items() for a in d}
    for fn in (f for d in arms.values() for f in d.values()):
        for _ in range(3):
            fn()                                       # warm-up
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for s, d in arms.items():
            for a, fn in d.items():
                times[(s, a)].append(time_ms(fn, args.iters))
    for (s, a), t in times.items():
        print(json.dumps({"tag": args.tag, "site": s, "arm": a,
                          "median_us": round(statistics.median(t) * 1e3, 1),
                          "min_us": round(min(t) * 1e3, 1),
                          "max_us": round(max(t) * 1e3, 1),
                          "rounds": args.rounds, "iters": args.iters}))


if __name__ == "__main__":
    main()
