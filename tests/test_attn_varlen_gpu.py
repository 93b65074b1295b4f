"""Varlen attention kernels (csrc/attention_varlen64.hip) against a
per-sequence float64 reference, and the packed BERT path against the
padded one.

Bounds: 3 x the worst figure of the CPU rounding models on exactly these
cases (python tools/attn_fwd_round_model.py --varlen, and the same of
attn_bwd_round_model.py):

    case    causal  o        lse       dq      dk      dv
    edges   0       0.00368  4.55e-07  0.0044  0.0066  0.0035
    edges   1       0.00262  5.05e-07  0.0063  0.0099  0.0032
    long    0       0.00297  8.31e-07  0.0037  0.0036  0.0033
    long    1       0.00240  7.89e-07  0.0057  0.0054  0.0024
    gaps    0       0.00249  4.23e-07  0.0066  0.0042  0.0037
    gaps    1       0.00199  4.06e-07  0.0039  0.0032  0.0030
"""
import copy
import functools

import pytest
import torch

from attn_varlen_cases import CASES, SCALE, make_inputs, reference, rel_err

pytestmark = pytest.mark.gpu

BOUND_O = 3 * 0.00368
BOUND_LSE = 3 * 8.31e-07
BOUND_GRAD = 3 * 0.0099


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ravnest_amd.ops import get_ext
    get_ext(True)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _reference(name, causal):
    qkv, do, cu = make_inputs(name, 0)
    return reference(qkv, do, cu, causal)


@pytest.mark.parametrize("tail", [0, 37])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_varlen_vs_float64(dev, name, causal, tail):
    from ravnest_amd import ops
    qkv, do, cu = make_inputs(name, tail)
    live = cu[-1]
    qkv = qkv.to(dev).requires_grad_()
    do = do.to(dev)
    cu_d = torch.tensor(cu, dtype=torch.int32, device=dev)
    tiles = ops.varlen_tiles(cu_d, qkv.shape[0])

    def run():
        o = ops.attention_varlen_qkv(qkv, cu_d, causal=causal, tiles=tiles)
        return o.detach(), torch.autograd.grad(o, qkv, do)[0]

    (o, dqkv), (o2, dqkv2) = run(), run()
    o3, lse = ops.get_ext(True).attn_varlen_fwd_qkv(
        qkv.detach(), cu_d, tiles, causal, SCALE)
    assert torch.equal(o, o2) and torch.equal(o, o3)
    assert torch.equal(dqkv, dqkv2)
    assert (o[live:] == 0).all() and (dqkv[live:] == 0).all()
    assert (lse[:, live:] == float("-inf")).all()
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all()
    assert torch.isfinite(lse[:, :live]).all()

    o, lse, dqkv = o.cpu(), lse.cpu(), dqkv.cpu()
    worst = dict(o=0.0, lse=0.0, grad=0.0)
    nonempty = [(lo, hi) for lo, hi in zip(cu[:-1], cu[1:]) if hi > lo]
    for (lo, hi), ref in zip(nonempty, _reference(name, causal)):
        worst["o"] = max(worst["o"], rel_err(o[lo:hi].transpose(0, 1), ref[0]))
        worst["lse"] = max(worst["lse"], float(
            (lse[:, lo:hi].double() - ref[1]).abs().max()))
        for i in range(3):  # dq, dk, dv (every length here is >= 2)
            worst["grad"] = max(worst["grad"], rel_err(
                dqkv[lo:hi, i].transpose(0, 1), ref[2 + i]))
    print(f"{name} causal={causal} tail={tail}: " + ", ".join(
        f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst["o"] <= BOUND_O
    assert worst["lse"] <= BOUND_LSE
    assert worst["grad"] <= BOUND_GRAD


def _errors(model, ref_loss, ref_grads, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    errs = {"loss": abs(float(loss.detach()) - ref_loss)}
    for n, p in model.named_parameters():
        errs[n] = rel_err(p.grad.cpu(), ref_grads[n].double())
    return errs


def test_packed_bert_matches_padded(dev):
    """Loss and every parameter gradient of forward_loss_packed and of the
    padded forward_loss, each against the fp32 CPU padded model: the packed
    error stays within 2 x the padded one (bf16 ordering differences)."""
    from ravnest_amd import ops
    from ravnest_amd.models import BertConfig, BertForMLM
    torch.manual_seed(0)
    ref_model = BertForMLM(BertConfig.tiny(dropout=0.0)).to(torch.bfloat16)
    model = copy.deepcopy(ref_model).to(dev).train()
    ref_model = ref_model.float().train()
    lens = torch.tensor([64, 17, 40])
    mask = (torch.arange(64)[None, :] < lens[:, None]).long()
    ids = torch.randint(1, 1024, (3, 64)) * mask
    tgt = torch.where((torch.rand(3, 64) < 0.3) & (mask == 1), ids, -100)
    crit = ops.CrossEntropyLoss(-100)

    ref_loss = crit(ref_model(ids, mask), tgt)
    ref_loss.backward()
    ref_grads = {n: p.grad for n, p in ref_model.named_parameters()}

    padded = model.forward_loss(ids.to(dev), mask.to(dev), tgt.to(dev), crit)
    assert padded is not None
    e_pad = _errors(model, float(ref_loss.detach()), ref_grads, padded)
    pids, pos, cu, ptgt, _ = ops.unpad_batch(ids, mask, tgt)
    packed = model.forward_loss_packed(pids.to(dev), pos.to(dev), cu.to(dev),
                                       ptgt.to(dev), crit)
    assert packed is not None
    e_pack = _errors(model, float(ref_loss.detach()), ref_grads, packed)
    for k in e_pad:
        print(f"{k}: padded {e_pad[k]:.3g} packed {e_pack[k]:.3g}")
    bad = [k for k in e_pad if not e_pack[k] <= 2 * e_pad[k]]
    assert not bad, bad
