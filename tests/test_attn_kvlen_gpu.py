"""Per-sequence key lengths (kv_len) in the fused attention kernels.

Three properties, per the feature's contract:
  A. deriving the bound from an additive padding mask (KV_SKIP on) leaves
     every output and gradient BIT-identical to the mask-only path;
  B. an explicit kv_len without any mask matches an fp32 torch reference
     that puts -inf on columns >= kv_len[b], at the tolerances of
     tests/test_kernels_gpu.py (o 3e-2, lse 2e-2, grads 8e-2 on the
     (B,H,S,D) path, 5e-2 on the packed path);
  C. the bound is read on the device at run time (graph replay with new
     mask contents).

Shape: S = 288 is a multiple of neither the 128-key dk/dv block nor 64;
the lengths hit a single key, a 32-key tile edge, both sides of the
128-key block edge, and a ragged last tile.

Scale of dO. The gradient tolerances are ABSOLUTE and the kernels return
bf16, whose rounding alone is up to 2^-9 of the value: 5e-2 can only be
met where |grad| stays below ~25. The kv_len = 1 row puts P == 1 on key 0
for all 288 queries, so dv[key 0] is the plain sum of 288 dO rows: with
dO ~ N(0, sigma^2) that is sigma * 17 per element and about sigma * 50-70
at the maximum over the H*D elements. At sigma = 1 the exactly summed,
correctly rounded bf16 result is already off by up to 0.125 (measured at
sigma = 1: dv max err 0.0958 on that row, every other figure under 1e-2).
dO is therefore drawn with sigma = 2^-3 (an exact scaling in bf16): max
|dv| of that row stays under 16, its rounding under 3.2e-2.

Every gradient is linear in dO, so a tolerance `tol` of the yardsticks,
which draw dO at sigma = 1, corresponds to tol * 2^-3 here. dq, dk and dv
are all held to that scaled bound. The one exception is dv of the
kv_len = 1 sequence, whose error is the bf16 rounding above and does not
shrink below half an ulp of the value: it is held to the plain `tol`.
"""
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

attn_mod = importlib.import_module("ravnest_amd.ops.attention")

B, H, S, D = 6, 2, 288, 64
LENS = [1, 33, 128, 129, 287, 288]
SCALE = 1.0 / math.sqrt(D)
DO_SIGMA = 0.125   # see "Scale of dO" above
EMPTY = torch.Tensor()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(required=True)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ext(dev):
    from ravnest_amd.ops import get_ext
    return get_ext(True)


def _inputs(dev, nb=B, d=D, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q, k, v, do = (torch.randn(nb, H, S, d, generator=g).to(
        device=dev, dtype=torch.bfloat16) for _ in range(4))
    return q, k, v, do * DO_SIGMA


def _pack(q, k, v):
    """(B,H,S,D) x3 -> packed (B,S,3,H,D)."""
    return torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).contiguous()


def _unpack_grad(dqkv):
    """packed (B,S,3,H,D) grad -> dq, dk, dv as (B,H,S,D)."""
    return tuple(dqkv[:, :, i].transpose(1, 2) for i in range(3))


def _len_mask(lens, dev, fill):
    """(B,1,1,S) additive mask: 0 on keys < len, `fill` after."""
    cols = torch.arange(S, device=dev)
    lens = torch.as_tensor(lens, device=dev)
    m = torch.zeros(len(lens), S, device=dev)
    m[cols[None, :] >= lens[:, None]] = fill
    return m.view(len(lens), 1, 1, S)


def _reference(q, k, v, do, add_mask, causal):
    """fp32 autograd reference: o, lse, dq, dk, dv."""
    q2, k2, v2 = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    s = (q2 @ k2.transpose(-2, -1)) * (1.0 / math.sqrt(q.shape[-1]))
    if causal:
        s = s + torch.triu(torch.full((S, S), float("-inf"),
                                      device=q.device), 1)
    s = s + add_mask
    o = torch.softmax(s, dim=-1) @ v2
    o.backward(do.float())
    return (o.detach(), torch.logsumexp(s.detach(), dim=-1), q2.grad,
            k2.grad, v2.grad)


_REF = {}


def _ref_for(dev, causal):
    """Reference for the shared inputs; computed once, never modified."""
    if causal not in _REF:
        q, k, v, do = _inputs(dev)
        _REF[causal] = _reference(
            q, k, v, do, _len_mask(LENS, dev, float("-inf")), causal)
    return _REF[causal]


def _run_sep(q, k, v, do, causal, mask=None, kv_len=None):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = attn_mod.attention(q, k, v, mask=mask, causal=causal, kv_len=kv_len)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


def _run_packed(qkv, do_tok, causal, mask=None, kv_len=None, pdrop=0.0):
    qkv = qkv.detach().clone().requires_grad_(True)
    o = attn_mod.attention_qkv(qkv, mask=mask, causal=causal,
                               prob_dropout=pdrop, kv_len=kv_len)
    o.backward(do_tok)
    return o.detach(), qkv.grad


def _check(name, got, want, tol):
    err = (got.float() - want).abs().max().item()
    print(f"{name}: max err {err:.4g} (tol {tol})")
    return err < tol, f"{name} max err {err} >= {tol}"


def _check_per_seq(name, got, want, tol, tol_single_key):
    """One check per sequence: `tol` where kv_len > 1, `tol_single_key`
    on the kv_len = 1 sequence (each caller says why it differs)."""
    return [_check(f"{name}[kv_len={n}]", got[b], want[b],
                   tol_single_key if n == 1 else tol)
            for b, n in enumerate(LENS)]


def _assert_all(results):
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "; ".join(bad)


# ---- 1. explicit kv_len, no mask, vs the fp32 reference -----------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", ["separate", "packed"])
def test_kv_len_matches_reference(dev, ext, layout, causal):
    q, k, v, do = _inputs(dev)
    kv_len = torch.tensor(LENS, device=dev)
    o_ref, lse_ref, dq_ref, dk_ref, dv_ref = _ref_for(dev, causal)
    kv32 = kv_len.to(torch.int32)
    if layout == "separate":
        gtol = 8e-2
        o, dq, dk, dv = _run_sep(q, k, v, do, causal, kv_len=kv_len)
        lse = ext.attn_fwd(q, k, v, EMPTY, causal, SCALE, kv32)[1]
    else:
        gtol = 5e-2
        qkv = _pack(q, k, v)
        do_tok = do.transpose(1, 2).flatten(2).contiguous()
        o_tok, dqkv = _run_packed(qkv, do_tok, causal, kv_len=kv_len)
        o = o_tok.unflatten(2, (H, D)).transpose(1, 2)
        dq, dk, dv = _unpack_grad(dqkv)
        lse = ext.attn_fwd_qkv(qkv, EMPTY, causal, SCALE, 0.0, 0, None,
                               kv32)[1]
    res = [_check("o", o, o_ref, 3e-2), _check("lse", lse, lse_ref, 2e-2),
           _check("dq", dq, dq_ref, gtol * DO_SIGMA),
           _check("dk", dk, dk_ref, gtol * DO_SIGMA)]
    # dv: scaled like dq and dk, except the kv_len = 1 sequence, whose
    # bf16 rounding alone exceeds the scaled bound (module docstring)
    res += _check_per_seq("dv", dv, dv_ref, gtol * DO_SIGMA, gtol)
    for b, n in enumerate(LENS):  # keys past the horizon get no gradient
        res.append((bool((dk[b, :, n:] == 0).all()), f"dk[{b}] tail != 0"))
        res.append((bool((dv[b, :, n:] == 0).all()), f"dv[{b}] tail != 0"))
    _assert_all(res)


# ---- 2. KV_SKIP on == off, bit for bit ----------------------------------
def _masks_with_non_prefix(dev):
    """The six right-padded rows plus one non-prefix row: dead run, live
    keys, dead tail."""
    m = _len_mask(LENS + [200], dev, -10000.0)
    m[6, 0, 0, :40] = -10000.0
    return m


@pytest.mark.parametrize("causal", [False, True])
def test_kv_skip_bit_identical_separate(dev, ext, monkeypatch, causal):
    q, k, v, do = _inputs(dev, nb=7, seed=1)
    mask = _masks_with_non_prefix(dev)
    derived = ext.attn_mask_kv_len(mask)
    assert derived.tolist() == LENS + [200]
    monkeypatch.setattr(attn_mod, "KV_SKIP", True)
    on = _run_sep(q, k, v, do, causal, mask=mask)
    monkeypatch.setattr(attn_mod, "KV_SKIP", False)
    off = _run_sep(q, k, v, do, causal, mask=mask)
    for name, a, b_ in zip(("o", "dq", "dk", "dv"), on, off):
        assert torch.equal(a, b_), f"{name} differs with KV_SKIP on"
    lse_on = ext.attn_fwd(q, k, v, mask, causal, SCALE, derived)[1]
    lse_off = ext.attn_fwd(q, k, v, mask, causal, SCALE)[1]
    assert torch.equal(lse_on, lse_off), "lse differs with a key horizon"


@pytest.mark.parametrize("causal,pdrop", [(False, 0.0), (True, 0.0),
                                          (False, 0.1)])
def test_kv_skip_bit_identical_packed(dev, ext, monkeypatch, causal, pdrop):
    q, k, v, do = _inputs(dev, nb=7, seed=2)
    qkv = _pack(q, k, v)
    do_tok = do.transpose(1, 2).flatten(2).contiguous()
    mask = _masks_with_non_prefix(dev)
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(attn_mod, "KV_SKIP", flag)
        torch.manual_seed(1234)  # the fused prob-dropout seed comes from it
        outs.append(_run_packed(qkv, do_tok, causal, mask=mask, pdrop=pdrop))
    (o_on, g_on), (o_off, g_off) = outs
    assert torch.isfinite(o_off).all() and torch.isfinite(g_off).all()
    assert torch.equal(o_on, o_off), "o differs with KV_SKIP on"
    assert torch.equal(g_on, g_off), "dqkv differs with KV_SKIP on"
    if pdrop == 0.0:
        derived = ext.attn_mask_kv_len(mask)
        lse_on = ext.attn_fwd_qkv(qkv, mask, causal, SCALE, 0.0, 0, None,
                                  derived)[1]
        lse_off = ext.attn_fwd_qkv(qkv, mask, causal, SCALE)[1]
        assert torch.equal(lse_on, lse_off)


# ---- 3. skipped key blocks are not read ---------------------------------
@pytest.mark.parametrize("layout", ["separate", "packed"])
def test_skipped_blocks_are_not_read(dev, layout):
    q, k, v, do = _inputs(dev, seed=3)
    kv_len = torch.tensor(LENS, device=dev)
    k, v = k.clone(), v.clone()
    first_poisoned = [(n + 127) // 128 * 128 for n in LENS]
    for b, p in enumerate(first_poisoned):
        k[b, :, p:] = float("nan")
        v[b, :, p:] = float("nan")
    assert torch.isnan(k).any()
    if layout == "separate":
        o, dq, dk, dv = _run_sep(q, k, v, do, False, kv_len=kv_len)
    else:
        do_tok = do.transpose(1, 2).flatten(2).contiguous()
        o, dqkv = _run_packed(_pack(q, k, v), do_tok, False, kv_len=kv_len)
        dq, dk, dv = _unpack_grad(dqkv)
    for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t).all(), f"{name} picked up a poisoned key"
    for b, p in enumerate(first_poisoned):
        assert (dk[b, :, p:] == 0).all() and (dv[b, :, p:] == 0).all()


# ---- 4. the derivation kernel -------------------------------------------
def _derivation_cases(n, dev):
    m = torch.full((8, n), -10000.0, device=dev)
    m[0, :] = 0.0                          # all live -> n
    m[1, :n // 3] = 0.0                    # right-padded -> n // 3
    m[2, :200] = 0.0
    m[2, 50:90] = -10000.0                 # hole in the prefix -> 200
    m[3, 150:161] = 0.0                    # live after a dead run -> 161
    # row 4: all dead -> n
    m[5, :] = 0.0
    m[5, 77:] = float("-inf")              # -inf counts as dead -> 77
    m[6, 0] = 0.0                          # single key -> 1
    m[7, n - 1] = 0.0                      # only the last key -> n
    return m


@pytest.mark.parametrize("n", [288, 512])
def test_mask_kv_len_kernel(dev, ext, n):
    m = _derivation_cases(n, dev)
    want = attn_mod.kv_len_from_mask(m.cpu())
    assert want.tolist() == [n, n // 3, 200, 161, n, 77, 1, n]
    for shaped in (m, m.view(8, 1, 1, n)):
        got = ext.attn_mask_kv_len(shaped)
        assert got.dtype == torch.int32 and got.shape == (8,)
        assert torch.equal(got.cpu(), want)
    assert torch.equal(attn_mod.kv_len_from_mask(m).cpu(), want)


# ---- 5. out-of-range lengths --------------------------------------------
def test_out_of_range_lengths_are_clamped(dev, ext):
    q, k, v, do = _inputs(dev, seed=5)
    wild = torch.tensor([0, S + 5, -7, 129, 2 ** 30, 288], device=dev)
    sane = torch.tensor([1, S, 1, 129, S, 288], device=dev)
    a = _run_sep(q, k, v, do, False, kv_len=wild)
    b_ = _run_sep(q, k, v, do, False, kv_len=sane)
    for name, x, y in zip(("o", "dq", "dk", "dv"), a, b_):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y), f"{name}: clamped length behaves differently"
    qkv = _pack(q, k, v)
    do_tok = do.transpose(1, 2).flatten(2).contiguous()
    a = _run_packed(qkv, do_tok, True, kv_len=wild)
    b_ = _run_packed(qkv, do_tok, True, kv_len=sane)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    with pytest.raises(RuntimeError):   # one entry per batch row
        ext.attn_fwd(q, k, v, EMPTY, False, SCALE,
                     sane[:3].to(torch.int32))
    with pytest.raises(RuntimeError):   # int32 only at the extension
        ext.attn_fwd(q, k, v, EMPTY, False, SCALE, sane)


# ---- 6. the bound is read at replay time --------------------------------
def test_graph_replay_follows_mask_contents(dev, monkeypatch):
    monkeypatch.setattr(attn_mod, "KV_SKIP", True)
    nb, n = 4, 256
    g = torch.Generator(device="cpu").manual_seed(6)
    qkv = torch.randn(nb, n, 3, H, D, generator=g).to(
        device=dev, dtype=torch.bfloat16).requires_grad_(True)
    dout = torch.randn(nb, n, H * D, generator=g).to(
        device=dev, dtype=torch.bfloat16)

    def mask_of(lens):
        cols = torch.arange(n, device=dev)
        dead = cols[None, :] >= torch.tensor(lens, device=dev)[:, None]
        return (dead.float() * -10000.0).view(nb, 1, 1, n)

    first, second = [64, 256, 5, 130], [256, 40, 200, 128]
    mask = mask_of(first)

    def step():
        o = attn_mod.attention_qkv(qkv, mask=mask)
        (dqkv,) = torch.autograd.grad(o, qkv, dout)
        return o, dqkv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, dqkv_g = step()

    for lens in (first, second, first):
        mask.copy_(mask_of(lens))
        graph.replay()
        torch.cuda.synchronize()
        o_e, dqkv_e = step()
        assert torch.equal(o_g, o_e), f"o stale after replay, lens {lens}"
        assert torch.equal(dqkv_g, dqkv_e), \
            f"dqkv stale after replay, lens {lens}"
        # and the bound really applies: no gradient past the last key
        dk = dqkv_g[:, :, 1]
        for b, ln in enumerate(lens):
            assert (dk[b, ln:] == 0).all()


# ---- 7. D = 128: v1 forward kernel, composed backward --------------------
def test_kv_len_head_dim_128(dev, ext):
    """The forward is the kernel under test; the backward is the composed
    torch path (library GEMMs with bf16 outputs, P and dS rounded to bf16).
    Gradients are held to 8e-2 * DO_SIGMA, the (B,H,S,D) tolerance scaled
    to this file's dO, on every sequence but kv_len = 1. There all 288
    queries put their whole weight on key 0, and two bf16 roundings that
    are spread over many keys elsewhere land on that one key's row:
      dv[key 0] is the sum of 288 dO rows, |value| up to ~16 at this
        sigma, so half a bf16 ulp is 3.1e-2 (module docstring);
      dk[key 0] is exactly 0 in the reference (P == 1 makes dP == delta),
        but the composed path takes dP = dO V^T from a GEMM with a bf16
        output and delta in fp32: each query leaves up to
        2^-9 * |dP| * scale (|dP| ~ sigma * sqrt(128) = 1.4, scale 0.088,
        so ~2.4e-4) times its q row, and 288 of those add up on key 0:
        ~sqrt(288) * 2.4e-4 = 4e-3 typical, three to four times that at
        the maximum over H*D elements.
    Both are relative roundings concentrated from 288 queries onto one
    key, proportional to dO, and would exceed the scaled bound at any
    sigma (scaled to sigma = 1 they read ~0.09 and ~0.18). That one
    sequence is therefore held to the plain 8e-2 at this file's sigma,
    which the estimates above sit under by a factor of 3 to 5.
    Measured: dk 1.2e-2 and dv 2.3e-2 on kv_len = 1, at most 2.1e-3 and
    2.8e-3 on the other sequences; dq 2.6e-3."""
    q, k, v, do = _inputs(dev, d=128, seed=7)
    kv_len = torch.tensor(LENS, device=dev)
    o_ref, lse_ref, dq_ref, dk_ref, dv_ref = _reference(
        q, k, v, do, _len_mask(LENS, dev, float("-inf")), False)
    o, dq, dk, dv = _run_sep(q, k, v, do, False, kv_len=kv_len)
    lse = ext.attn_fwd(q, k, v, EMPTY, False, 1.0 / math.sqrt(128),
                       kv_len.to(torch.int32))[1]
    gtol = 8e-2
    _assert_all([_check("o", o, o_ref, 3e-2),
                 _check("lse", lse, lse_ref, 2e-2),
                 _check("dq", dq, dq_ref, gtol * DO_SIGMA)]
                + _check_per_seq("dk", dk, dk_ref, gtol * DO_SIGMA, gtol)
                + _check_per_seq("dv", dv, dv_ref, gtol * DO_SIGMA, gtol))
    for b, n in enumerate(LENS):
        assert (dk[b, :, n:] == 0).all() and (dv[b, :, n:] == 0).all()


# ---- 8. model level ------------------------------------------------------
def test_bert_step_unchanged_by_kv_skip(dev, monkeypatch):
    """Logits and every parameter gradient of a training step are
    bit-identical with KV_SKIP on and off; the loss agrees to the order of
    its own summation.

    ops.CrossEntropyLoss adds the per-row terms with float atomicAdd
    (csrc/ce_loss.hip), so its scalar moves in the last bits between two
    IDENTICAL calls: this model with the switch off both times gave
    0x40de8881 then 0x40de8884. torch.equal on it would test the order of
    atomics, not attention. With bit-equal logits the two losses are the
    same n non-negative fp32 terms added in two orders, which differ by at
    most (n - 1) * 2^-24 * loss each way; that is the bound used. The
    gradient does not depend on that sum."""
    from ravnest_amd import set_seed
    from ravnest_amd.models import BertConfig, BertForMLM
    from ravnest_amd.ops import CrossEntropyLoss
    nb, n = 4, 256
    lens = [256, 130, 128, 5]
    set_seed(0)
    model = BertForMLM(BertConfig.tiny(max_seq=n)).to(dev).to(torch.bfloat16)
    crit = CrossEntropyLoss(-100)
    ids = torch.randint(0, model.cfg.vocab_size, (nb, n), device=dev)
    am = torch.zeros(nb, n, dtype=torch.int64, device=dev)
    for b, ln in enumerate(lens):
        am[b, :ln] = 1
    labels = torch.where(am.bool(), ids, torch.full_like(ids, -100))

    def run(flag):
        monkeypatch.setattr(attn_mod, "KV_SKIP", flag)
        model.zero_grad(set_to_none=True)
        set_seed(11)                    # same dropout masks both times
        logits = model(ids, am)
        loss = crit(logits, labels)
        loss.backward()
        return logits.detach().clone(), loss.detach().float(), {
            name: p.grad.detach().clone()
            for name, p in model.named_parameters() if p.grad is not None}

    logits_on, loss_on, g_on = run(True)
    logits_off, loss_off, g_off = run(False)
    assert torch.isfinite(loss_off)
    assert torch.equal(logits_on, logits_off)
    n_terms = int((labels != -100).sum())
    order_tol = 2 * (n_terms - 1) * 2.0 ** -24 * float(loss_off)
    print(f"loss on {float(loss_on)!r} off {float(loss_off)!r} "
          f"tol {order_tol:.3g}")
    assert abs(float(loss_on) - float(loss_off)) <= order_tol
    assert g_on.keys() == g_off.keys() and len(g_on) > 0
    for name in g_off:
        assert torch.equal(g_on[name], g_off[name]), name
