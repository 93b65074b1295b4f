"""CPU side of the fused MX quantisation: the tag helpers that carry
(q, s) from a producer to mx_linear, and the promise that emit_mx changes
neither state-dict keys, nor the fx graph, nor the CPU forward."""
import torch

from ravnest_amd.models import GPT, GPTConfig
from ravnest_amd.models.gpt import GPTBlock
from ravnest_amd.ops import (FusedLayerNorm, LinearGelu, attach_mx, mx,
                             take_mx)
from ravnest_amd.planner.splitter import trace_model


def _tagged(shape=(4, 64)):
    y = torch.randn(*shape)
    q = torch.zeros(*shape, dtype=torch.uint8)
    s = torch.zeros(shape[0], shape[1] // 32, dtype=torch.uint8)
    assert attach_mx(y, q, s) is y
    return y, q, s


def test_take_hits_same_object_once():
    y, q, s = _tagged()
    got = take_mx(y)
    assert got is not None and got[0] is q and got[1] is s
    assert not hasattr(y, mx._TAG)      # removed: q, s die with the GEMM
    assert take_mx(y) is None           # a second consumer gets nothing


def test_take_misses_other_objects():
    y, _, _ = _tagged()
    assert take_mx(y.view(4, 64)) is None
    assert take_mx(y[:]) is None
    assert take_mx(y.clone()) is None
    assert take_mx(y.detach()) is None
    assert take_mx(torch.randn(4, 64)) is None
    assert take_mx(y) is not None       # the misses left the tag alone


def test_take_misses_after_inplace_edit():
    y, _, _ = _tagged()
    y.add_(1)
    assert take_mx(y) is None
    assert not hasattr(y, mx._TAG)      # a stale tag is dropped as well
    y, _, _ = _tagged()
    y[0, 0] = 3.0
    assert take_mx(y) is None


def test_take_misses_after_shape_change():
    y, _, _ = _tagged()
    y.unsqueeze_(0)
    assert take_mx(y) is None
    y, _, _ = _tagged()
    y.resize_(2, 128)
    assert take_mx(y) is None


def test_switch_reads_environment_default_on():
    assert mx.FUSED_QUANT is True or mx.FUSED_QUANT is False
    import os
    assert mx.FUSED_QUANT == (
        os.environ.get("RAVNEST_FUSED_MX_QUANT", "1") != "0")


def _cfg(fp8):
    cfg = GPTConfig.nano64(vocab_size=16, block_size=16)
    cfg.dropout = 0.0
    cfg.fp8 = fp8
    return cfg


def test_emit_mx_set_by_fp8_only():
    blk = GPTBlock(_cfg(True))
    assert blk.ln1.emit_mx and blk.mlp_in.emit_mx
    assert not blk.ln2.emit_mx          # feeds mlp_in's bf16 GEMM
    blk = GPTBlock(_cfg(False))
    assert not blk.ln1.emit_mx and not blk.mlp_in.emit_mx
    assert not FusedLayerNorm(64).emit_mx
    assert not LinearGelu(64, 64).emit_mx


def test_state_dict_keys_unchanged():
    assert FusedLayerNorm(64, emit_mx=True).state_dict().keys() == \
        FusedLayerNorm(64).state_dict().keys()
    assert LinearGelu(64, 128, emit_mx=True).state_dict().keys() == \
        LinearGelu(64, 128).state_dict().keys()
    with_mx = GPT(_cfg(True))
    without = GPT(_cfg(True))
    for m in without.modules():
        if hasattr(m, "emit_mx"):
            m.emit_mx = False
    assert list(with_mx.state_dict().keys()) == \
        list(without.state_dict().keys())
    assert list(with_mx.state_dict().keys()) == \
        list(GPT(_cfg(False)).state_dict().keys())


def test_fx_nodes_unchanged(monkeypatch):
    def nodes(flag):
        monkeypatch.setattr(mx, "FUSED_QUANT", flag)
        torch.manual_seed(0)
        gm = trace_model(GPTBlock(_cfg(True)))
        return [(n.op, str(n.target), str(n.args)) for n in gm.graph.nodes]

    on, off = nodes(True), nodes(False)
    assert on == off
    assert ("call_module", "ln1", "(x,)") in on


def test_cpu_forward_attaches_nothing(monkeypatch):
    torch.manual_seed(0)
    model = GPT(_cfg(True)).eval()
    ids = torch.randint(0, 16, (2, 8))
    seen = []
    hook = model.blocks[0].ln1.register_forward_hook(
        lambda m, i, o: seen.append(hasattr(o, mx._TAG)))
    outs = []
    with torch.no_grad():
        for flag in (True, False):
            monkeypatch.setattr(mx, "FUSED_QUANT", flag)
            outs.append(model(ids))
    hook.remove()
    assert seen == [False, False]
    assert torch.equal(outs[0], outs[1])
