"""Cases, float64 references and error bounds for the fused optimizer
updates (test_optim_family_gpu.py and its CPU twin
test_optim_family_cpu.py).

A case fixes the whole input state of ONE step: per tensor p, g, m, v (SGD:
m is the momentum buffer), for bf16 the fp32 master, and the step number N.
`optim_run` builds the public optimizer on a device, writes that state into
it with step = N - 1, calls step() once and reads everything back. The
reference does the same step in float64 from the same values, written out
below: neither torch.optim nor the package's CPU path is used. It takes the
hyperparameters as the kernels receive them, rounded to fp32 and widened
again (1 - float32(0.999) differs from 0.001 by 1.3e-5 relative), and the
bias corrections 1 - b**N in float64 from those rounded betas.

Formulations pinned here:
  Adam  g' = coef*g + wd*p;  m = b1*m + (1-b1)*g';  v = b2*v + (1-b2)*g'^2;
        p -= lr * (m/bc1) / (sqrt(v/bc2) + eps)
  SGD   g' = coef*g + wd*p;  buf = mom*buf + g';
        p -= lr * (g' + mom*buf  if nesterov  else buf);  no dampening
  LAMB  g' = coef*g;  m, v as Adam;
        upd = (m/bc1) / (sqrt(v/bc2) + eps) + wd*p;
        trust = min(|p|/|upd|, clamp_trust) if |p| > 0 and |upd| > 0 else 1;
        p -= lr * trust * upd

Bounds. u = 2^-24. A value computed in fp32 as a sum of products carries at
most (roundings on the longest path) * u * (sum of the ABSOLUTE terms), to
first order; every bound below is 4 times that count, so that a correct
fp32 implementation stays under a quarter of it, capped at 16:
  g'      4*k*u*(|coef*g| + |wd*p|), k = 0 (neither), 1 (clip only), 2 (wd)
  m, buf  8*u*(|b1*m| + |(1-b1)*g'|) + (1-b1)*bound(g')        [2 roundings]
  v       12*u*(|b2*v| + (1-b2)*g'^2) + (1-b2)*2|g'|*bound(g') [3 roundings]
  delta   the moment bounds carried through lr*mhat/(sqrt(vhat)+eps) (the
          square root exactly, not to first order: v may be 0), plus
          16*u*|delta| for the 7 roundings of the quotient itself
  p       u*|p_ref| for the final rounding, plus bound(delta)
  LAMB    additionally 2 * 1e-4 * |delta| for the two fp32 norms: 1e-4 is
          what test_norm_matches_fp64 allows an fp32 sum of positive terms
None of these figures was chosen by looking at a kernel's error.

The final rounding p = fl(p - delta) alone can use the whole u*|p_ref|
term, so the twin judges the fp32 yardstick twice: its delta against a
quarter of bound(delta), and its rounded p against the whole bound.
"""
import itertools
import struct

import torch

U32 = 2.0 ** -24
NORM_RTOL = 1e-4   # test_grad_clip_gpu.test_norm_matches_fp64
PAD = 32
SENTINEL = -7.0
BF16 = torch.bfloat16
INF = float("inf")

SHAPES = [(1,), (3,), (5,), (7,), (64, 64), (3, 7, 11), (1023,),
          (65536 + 5,), (2, 3, 4, 5)]
CHANNELS_LAST = 8   # index into SHAPES
STEPS = [1, 2, 10, 1000, 100000]

FAMILIES = ["randn", "g_small", "g_big", "v_tiny", "zero", "cancel"]
LAMB_FAMILIES = FAMILIES + ["p_zero", "zero_update", "ratio_big",
                            "ratio_small"]
G_SCALE = {"g_small": 1e-4, "g_big": 1e4}


def f32(x):
    """x rounded to fp32, as a python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


# ------------------------------------------------------------------ cases
def _specs():
    out = {"adam": [], "sgd": [], "lamb": []}
    grid = itertools.product([0.0, 0.01],
                             [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)],
                             [1e-8, 1e-3], STEPS)
    for wd, betas, eps, N in grid:
        out["adam"].append((dict(lr=1e-3, betas=betas, eps=eps,
                                 weight_decay=wd), N, False))
    out["adam"].append((dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                             weight_decay=0.01), 10, True))
    # SGD has no step number: each setting runs once per family rotation
    for (mom, nes), wd, _ in itertools.product(
            [(0.0, False), (0.9, False), (0.9, True)], [0.0, 5e-4],
            range(len(FAMILIES))):
        out["sgd"].append((dict(lr=0.1, momentum=mom, weight_decay=wd,
                                nesterov=nes), 1, False))
    out["sgd"].append((dict(lr=0.1, momentum=0.9, weight_decay=5e-4,
                            nesterov=True), 1, True))
    for wd, clamp, N in itertools.product([0.0, 0.01], [10.0, 0.5], STEPS):
        out["lamb"].append((dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                                 weight_decay=wd, clamp_trust=clamp), N,
                            False))
    out["lamb"].append((dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6,
                             weight_decay=0.01, clamp_trust=10.0), 10, True))
    # (hyperparameters, N, clip, rotation of the families over the tensors)
    return {k: [(h, N, clip, i) for i, (h, N, clip) in enumerate(v)]
            for k, v in out.items()}


SPECS = _specs()


def spec_id(spec):
    h, N, clip, rot = spec
    return f"{h} N={N} clip={clip} rot={rot}"


def _f32_hyper(kind, hyper):
    """The hyperparameters as the kernel sees them, as python floats."""
    h = {"lr": f32(hyper["lr"]), "wd": f32(hyper["weight_decay"])}
    if kind == "sgd":
        h["mom"] = f32(hyper["momentum"])
        h["nesterov"] = bool(hyper["nesterov"])
    else:
        h["b1"], h["b2"] = (f32(b) for b in hyper["betas"])
        h["eps"] = f32(hyper["eps"])
    if kind == "lamb":
        h["clamp"] = f32(hyper["clamp_trust"])
    return h


def _adam_direction(h, g, m, v, N):
    """float64 mhat / (sqrt(vhat) + eps) of the state after the step."""
    m = h["b1"] * m + (1 - h["b1"]) * g
    v = h["b2"] * v + (1 - h["b2"]) * g * g
    return (m / (1 - h["b1"] ** N)) / (
        (v / (1 - h["b2"] ** N)).sqrt() + h["eps"])


def _tensor(kind, fam, shape, cl, dtype, h, N, gen):
    def fmt(x):
        return x.contiguous(memory_format=torch.channels_last) if cl else x

    def randn():
        return fmt(torch.randn(shape, generator=gen))

    p, g, m = randn(), randn(), randn()
    v = fmt(torch.rand(shape, generator=gen)) * 1e-2
    g = g * G_SCALE.get(fam, 1.0)
    if fam == "v_tiny":
        v = torch.full_like(v, 1e-16)
    if fam == "zero":
        g, m, v = (torch.zeros_like(p) for _ in range(3))
    if fam == "zero_update":
        g, m = torch.zeros_like(p), torch.zeros_like(p)
    if fam == "p_zero":
        p = torch.zeros_like(p)
    if dtype == BF16:
        g = g.to(BF16)
    if fam == "cancel":
        # the new first moment (SGD: buffer) nearly cancels; with b1 = 0
        # (mom = 0) there is nothing to cancel against
        keep = h["mom"] if kind == "sgd" else h["b1"]
        if keep:
            lose = 1.0 if kind == "sgd" else 1 - keep
            m = -(lose / keep) * g.float() * (1 + 1e-3 * randn())
    if fam in ("ratio_big", "ratio_small"):
        # |p| = 100 or 0.3 times the norm of the decay-free update
        a = _adam_direction(h, g.double(), m.double(), v.double(), N)
        want = (100.0 if fam == "ratio_big" else 0.3) * a.norm()
        p = (p.double() * (want / p.double().norm())).float()
    t = {"family": fam, "N": N, "g": g, "m": m,
         "v": None if kind == "sgd" else v, "master": None}
    if kind == "sgd" and not h["mom"]:
        t["m"] = None
    if dtype == BF16:
        t["master"] = p
        t["p"] = p.to(BF16)
    else:
        t["p"] = p
    return t


def optim_case(kind, dtype, spec, shapes=None, seed=0):
    """CPU tensors of one step. Tensor i belongs to family (i + rot) of the
    optimizer's list, so over the specs every shape meets every family."""
    hyper, N, clip, rot = spec
    gen = torch.Generator().manual_seed(seed + 1000 * rot)
    fams = LAMB_FAMILIES if kind == "lamb" else FAMILIES
    h = _f32_hyper(kind, hyper)
    shapes = SHAPES if shapes is None else shapes
    tensors = [
        _tensor(kind, fams[(i + rot) % len(fams)], s,
                shapes is SHAPES and i == CHANNELS_LAST, dtype, h, N, gen)
        for i, s in enumerate(shapes)]
    case = {"kind": kind, "dtype": dtype, "hyper": hyper, "clip": None,
            "tensors": tensors}
    if clip:  # a coefficient of about 0.37
        case["clip"] = 0.37 * float(_grad_norm(case))
    return case


def _grad_norm(case):
    return torch.sqrt(sum((t["g"].double() ** 2).sum()
                          for t in case["tensors"] if t["g"] is not None))


def coef_ratio(case, coef):
    """|reported clip coefficient - float64| / (1e-4 * float64)."""
    ref = min(1.0, f32(case["clip"]) / (float(_grad_norm(case)) + 1e-6))
    return abs(coef - ref) / (NORM_RTOL * ref)


# -------------------------------------------------------------- reference
def _start(t):
    p = t["p"] if t["master"] is None else t["master"]
    return p.double()


def _grad_ref(h, t, p, coef, wd_in_grad):
    """g' and its bound (see the module docstring)."""
    g = t["g"].double()
    k = 0
    if coef is not None:
        g, k = g * coef, 1
    G = g.abs()
    if wd_in_grad and h["wd"]:
        g, G, k = g + h["wd"] * p, G + (h["wd"] * p).abs(), 2
    return g, 4 * k * U32 * G


def _moments_ref(h, t, g, bg):
    b1, b2, N = h["b1"], h["b2"], t["N"]
    m0, v0 = t["m"].double(), t["v"].double()
    m = b1 * m0 + (1 - b1) * g
    bm = 8 * U32 * ((b1 * m0).abs() + (1 - b1) * g.abs()) + (1 - b1) * bg
    v = b2 * v0 + (1 - b2) * g * g
    bv = (12 * U32 * ((b2 * v0).abs() + (1 - b2) * g * g)
          + (1 - b2) * 2 * g.abs() * bg)
    bc1, bc2 = 1 - b1 ** N, 1 - b2 ** N
    rt = (v / bc2).sqrt()
    den = rt + h["eps"]
    a = (m / bc1) / den
    # sqrt is concave: the larger deviation is downwards
    d_den = rt - ((v - bv).clamp(min=0) / bc2).sqrt()
    ba = (bm / bc1) / den + a.abs() * d_den / (den - d_den) \
        + 16 * U32 * a.abs()
    return m, bm, v, bv, a, ba


def optim_reference(case, coef=None):
    """Per tensor: the float64 p, m, v after the step and the delta that
    was subtracted from p, their bounds b_m, b_v, b_delta and the
    final-rounding term round_p. `coef` is the clip
    coefficient the optimizer reported (None without clipping). A tensor
    without a grad must come back unchanged: its bounds are 0."""
    kind = case["kind"]
    h = _f32_hyper(kind, case["hyper"])
    out = []
    for t in case["tensors"]:
        p = _start(t)
        if t["g"] is None:
            zero = torch.zeros_like(p)
            out.append({"p": p, "delta": zero, "b_delta": zero,
                        "round_p": zero,
                        "m": None if t["m"] is None else t["m"].double(),
                        "v": None if t["v"] is None else t["v"].double(),
                        "b_m": zero, "b_v": zero})
            continue
        g, bg = _grad_ref(h, t, p, coef, wd_in_grad=kind != "lamb")
        r = {"m": None, "v": None}
        if kind == "sgd":
            d, bd = g, bg
            if h["mom"]:
                b0 = t["m"].double()
                buf = h["mom"] * b0 + g
                bbuf = 8 * U32 * ((h["mom"] * b0).abs() + g.abs()) + bg
                r["m"], r["b_m"] = buf, bbuf
                if h["nesterov"]:
                    d = g + h["mom"] * buf
                    bd = (8 * U32 * (g.abs() + (h["mom"] * buf).abs())
                          + bg + h["mom"] * bbuf)
                else:
                    d, bd = buf, bbuf
            delta = h["lr"] * d
            b_delta = h["lr"] * bd + 4 * U32 * delta.abs()
        else:
            r["m"], r["b_m"], r["v"], r["b_v"], a, ba = \
                _moments_ref(h, t, g, bg)
            if kind == "adam":
                delta, b_delta = h["lr"] * a, h["lr"] * ba
            else:
                upd, bu = a, ba
                if h["wd"]:
                    upd = a + h["wd"] * p
                    bu = ba + 8 * U32 * (a.abs() + (h["wd"] * p).abs())
                wn, un = p.norm(), upd.norm()
                trust = 1.0
                if wn > 0 and un > 0:
                    trust = min(float(wn / un), h["clamp"])
                delta = h["lr"] * trust * upd
                b_delta = (h["lr"] * trust * bu
                           + (2 * NORM_RTOL + 8 * U32) * delta.abs())
                r["trust"] = trust
        r["p"] = p - delta
        r["delta"], r["b_delta"] = delta, b_delta
        r["round_p"] = U32 * r["p"].abs()
        out.append(r)
    return out


def _ratio(got, ref, bound):
    """max(|got - ref| / bound) over ALL elements; 0/0 counts as 0, an
    error above a zero bound and anything non-finite as inf."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return INF
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(q.max())


def optim_ratios(got, ref, case, final_rounding=True):
    """Worst error / bound over the tensors for p (bf16: the master), m
    and v; `bf16_exact` is 0 when every bf16 parameter equals the
    round-to-nearest-even bf16 of the implementation's OWN new master, else
    inf; `sentinels` likewise for the words around every output; `coef`
    judges the reported clip coefficient."""
    out = {"p": 0.0}
    for t, g, r in zip(case["tensors"], got["tensors"], ref):
        if final_rounding:
            pg = g["p"] if t["master"] is None else g["master"]
            q = _ratio(pg, r["p"], r["b_delta"] + r["round_p"])
        else:  # the yardstick's delta, before p - delta is rounded
            q = _ratio(g["delta"], r["delta"], r["b_delta"])
        out["p"] = max(out["p"], q)
        for k in ("m", "v"):
            if r[k] is not None:
                out[k] = max(out.get(k, 0.0),
                             _ratio(g[k], r[k], r["b_" + k]))
        if t["master"] is not None:
            same = torch.equal(g["p"], g["master"].to(BF16))
            out["bf16_exact"] = max(out.get("bf16_exact", 0.0),
                                    0.0 if same else INF)
    if "sentinels" in got:
        out["sentinels"] = 0.0 if got["sentinels"] else INF
    if case["clip"] is not None:
        out["coef"] = coef_ratio(case, got["coef"])
    return out


# ----------------------------------------------------- the fp32 yardstick
MISTAKES = ["bc_next_step", "adamw", "no_nesterov", "clamp_weight_norm",
            "trust0", "bf16_truncate", "clip_dropped"]


def _truncate_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(
        torch.float32).to(BF16)


def optim_yardstick(case, mistake=None):
    """The three formulas in plain torch fp32, independent of the package,
    in the shape of optim_run's result, plus the fp32 `delta` that the last
    operation subtracts from p. `mistake` seeds one of MISTAKES."""
    kind = case["kind"]
    hd = _f32_hyper(kind, case["hyper"])
    h = {k: torch.tensor(x, dtype=torch.float32) for k, x in hd.items()
         if k != "nesterov"}
    coef = None
    if case["clip"] is not None:
        norm = torch.sqrt(sum((t["g"].float() ** 2).sum()
                              for t in case["tensors"]))
        coef = torch.clamp(torch.tensor(case["clip"], dtype=torch.float32)
                           / (norm + 1e-6), max=1.0)
    tensors = []
    for t in case["tensors"]:
        p = (t["p"] if t["master"] is None else t["master"]).clone()
        g = t["g"].float()
        if coef is not None and mistake != "clip_dropped":
            g = g * coef
        wd_late = mistake == "adamw" and kind == "adam"
        if kind != "lamb" and hd["wd"] and not wd_late:
            g = g + h["wd"] * p
        r = {"m": None, "v": None, "master": None}
        if kind == "sgd":
            d = g
            if hd["mom"]:
                r["m"] = h["mom"] * t["m"] + g
                d = r["m"]
                if hd["nesterov"] and mistake != "no_nesterov":
                    d = g + h["mom"] * r["m"]
            delta = h["lr"] * d
        else:
            N = t["N"] + (mistake == "bc_next_step")
            bc1 = torch.tensor(1 - hd["b1"] ** N, dtype=torch.float32)
            bc2 = torch.tensor(1 - hd["b2"] ** N, dtype=torch.float32)
            r["m"] = h["b1"] * t["m"] + (1 - h["b1"]) * g
            r["v"] = h["b2"] * t["v"] + (1 - h["b2"]) * g * g
            if kind == "adam":
                delta = h["lr"] * (r["m"] / bc1) / (
                    (r["v"] / bc2).sqrt() + h["eps"])
                if wd_late and hd["wd"]:
                    delta = delta + h["lr"] * h["wd"] * p
            else:
                upd = (r["m"] / bc1) / ((r["v"] / bc2).sqrt() + h["eps"])
                if hd["wd"]:
                    upd = upd + h["wd"] * p
                wn, un = p.norm(), upd.norm()
                trust = torch.ones(())
                if wn > 0 and un > 0:
                    trust = torch.minimum(wn / un, h["clamp"])
                    if mistake == "clamp_weight_norm":
                        trust = torch.minimum(wn, h["clamp"]) / un
                elif mistake == "trust0" and wn == 0:
                    trust = torch.zeros(())
                delta = (h["lr"] * trust) * upd
        r["delta"] = delta
        r["p"] = p - delta
        if t["master"] is not None:
            r["master"] = r["p"]
            r["p"] = (_truncate_bf16(r["p"]) if mistake == "bf16_truncate"
                      else r["p"].to(BF16))
        tensors.append(r)
    return {"tensors": tensors,
            "coef": None if coef is None else float(coef)}


# ------------------------------------------------ the optimizer under test
class Session:
    """One public optimizer over the tensors of a case. Every tensor the
    step may write (p, m, v, master) is a view `offset` words into a
    sentinel-filled buffer with PAD sentinels after it."""


def _place(x, device, offset):
    n = x.numel()
    buf = torch.full((offset + n + PAD,), SENTINEL, dtype=x.dtype,
                     device=device)
    view = torch.as_strided(buf, x.shape, x.stride(), offset)
    view.copy_(x.to(device))
    return buf, view


def optim_build(case, device, offset=PAD):
    from ravnest_amd.ops import FusedAdam, FusedLAMB, FusedSGD
    s = Session()
    s.case, s.offset = case, offset
    s.bufs, s.views = [], []
    ps = []
    for t in case["tensors"]:
        views = {}
        for k in ("p", "g", "m", "v", "master"):
            if t[k] is None:
                views[k] = None
                continue
            buf, views[k] = _place(t[k], device, offset)
            if k != "g":
                s.bufs.append((buf, t[k].numel()))
        views["p"].requires_grad_(True)
        views["p"].grad = views["g"]
        ps.append(views["p"])
        s.views.append(views)
    cls = {"adam": FusedAdam, "sgd": FusedSGD, "lamb": FusedLAMB}
    s.opt = cls[case["kind"]](ps, max_grad_norm=case["clip"],
                              **case["hyper"])
    for t, v in zip(case["tensors"], s.views):
        st = s.opt.state[v["p"]]
        if case["kind"] == "sgd":
            if v["m"] is not None:
                st["momentum_buffer"] = v["m"]
        else:
            st.update(step=t["N"] - 1, m=v["m"], v=v["v"])
        if v["master"] is not None:
            st["master"] = v["master"]
    return s


def optim_read(s):
    """Everything back on the CPU, as fresh tensors."""
    tensors = []
    for v in s.views:
        r = {k: None if v[k] is None else v[k].detach().cpu().clone()
             for k in ("p", "m", "v", "master")}
        # the optimizer updated the tensors it was given, in place
        st = s.opt.state[v["p"]]
        for key, k in (("m", "m"), ("v", "v"), ("momentum_buffer", "m"),
                       ("master", "master")):
            if key in st and v[k] is not None:
                assert st[key] is v[k], key
        tensors.append(r)
    ok = all(bool((buf[:s.offset] == SENTINEL).all())
             and bool((buf[s.offset + n:] == SENTINEL).all())
             for buf, n in s.bufs)
    stats = s.opt.grad_norm_stats()
    coef = None if s.case["clip"] is None else float(stats[1])
    return {"tensors": tensors, "sentinels": ok, "coef": coef}


def optim_run(case, device, offset=PAD):
    s = optim_build(case, device, offset)
    s.opt.step()
    return optim_read(s)


def worst(into, ratios):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)
    return into


# --------------------------------------------------------- chained steps
CHAIN_SHAPES = [(7,), (1023,), (64, 64)]
CHAIN_SPECS = {
    "adam": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                  weight_decay=0.01), 1, False, 0),
    "sgd": (dict(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True),
            1, False, 0),
    "lamb": (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                  clamp_trust=10.0), 1, False, 0),
}


def optim_chain(kind, dtype, device, steps=12, shapes=None, late=None):
    """Single steps chained on ONE optimizer: before each step the
    reference takes the state the implementation produced at the step
    before, read back, so nothing compounds while the optimizer's own step
    counts evolve. Yields the ratios of each step.

    late = (i, k): tensor i has grad None during the first k steps; it
    must not change then, and afterwards its step count is k behind."""
    case = optim_case(kind, dtype, CHAIN_SPECS[kind],
                      SHAPES if shapes is None else shapes)
    for t in case["tensors"]:
        t["m"] = None if t["m"] is None else torch.zeros_like(t["m"])
        t["v"] = None if t["v"] is None else torch.zeros_like(t["v"])
    gen = torch.Generator().manual_seed(99)
    s = optim_build(case, device)
    for step in range(steps):
        for i, (t, v) in enumerate(zip(case["tensors"], s.views)):
            off = late is not None and i == late[0] and step < late[1]
            if off:
                t["g"], v["p"].grad = None, None
                continue
            g = torch.randn(t["p"].shape, generator=gen)
            g = (g * G_SCALE.get(t["family"], 1.0)).to(dtype)
            t["g"] = g
            v["g"].copy_(g.to(device))
            v["p"].grad = v["g"]
        s.opt.step()
        got = optim_read(s)
        yield optim_ratios(got, optim_reference(case), case)
        for t, g in zip(case["tensors"], got["tensors"]):
            if t["g"] is not None:
                t["N"] += 1
            t.update({k: g[k] for k in ("p", "m", "v", "master")})
