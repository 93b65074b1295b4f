"""The paired output of DropoutAddLayerNorm (ops/dropout_ln.py, pair) and its
threading through BertLayer / BertForMLM, where no fused kernel runs: on
the composed path the pair is one tensor twice, so a model that hands the
pair from layer to layer computes exactly what the single-output model
(RAVNEST_LN_BWD_DY2=0) computes, parameter names included, and an fx trace
still sees the module call with its single output.
"""
import pytest
import torch


def _model(monkeypatch, dy2):
    from ravnest_amd.models import BertConfig, BertForMLM
    monkeypatch.setenv("RAVNEST_LN_BWD_DY2", dy2)
    torch.manual_seed(11)
    model = BertForMLM(BertConfig.tiny(layers=2, max_seq=16))
    assert all(layer.ln1.pair_grads == (dy2 != "0")
               for layer in model.layers)
    return model.train()


def _step(model):
    torch.manual_seed(23)
    ids = torch.randint(0, model.cfg.vocab_size, (2, 16))
    mask = torch.ones(2, 16, dtype=torch.int64)
    mask[1, 11:] = 0
    emb = {}

    def keep(module, args, out):
        out.retain_grad()
        emb["x"] = out

    hook = model.embeddings.register_forward_hook(keep)
    logits = model(ids, mask)
    hook.remove()
    loss = torch.nn.functional.cross_entropy(
        logits.flatten(0, 1), ids.flatten())
    loss.backward()
    return logits.detach(), emb["x"].grad, \
        {n: p.grad for n, p in model.named_parameters()}


def test_paired_model_equals_single_output_model(monkeypatch):
    paired, single = _model(monkeypatch, "1"), _model(monkeypatch, "0")
    assert list(paired.state_dict()) == list(single.state_dict())
    for (n, p), (_, q) in zip(paired.named_parameters(),
                              single.named_parameters()):
        assert torch.equal(p, q), n
    lp, dxp, gp = _step(paired)
    ls, dxs, gs = _step(single)
    assert int((lp != 0).sum()) > 0
    assert torch.equal(lp, ls)
    assert torch.equal(dxp, dxs)            # the input gradient
    assert gp.keys() == gs.keys()
    for n in gp:
        assert gp[n] is not None and torch.equal(gp[n], gs[n]), n


def test_state_dict_keys_unchanged(monkeypatch):
    model = _model(monkeypatch, "1")
    ln_keys = sorted(k for k in model.state_dict() if ".ln1." in k
                     or ".ln2." in k)
    want = sorted(f"layers.{i}.{ln}.{p}" for i in range(2)
                  for ln in ("ln1", "ln2") for p in ("weight", "bias"))
    assert ln_keys == want


def test_module_pair_composed_path():
    from ravnest_amd.ops import DropoutAddLayerNorm
    m = DropoutAddLayerNorm(32, 1e-5, 0.1).train()
    a = torch.randn(3, 32, requires_grad=True)
    z = torch.randn(3, 32, requires_grad=True)
    st = torch.get_rng_state()
    y1, y2 = m(a, z, pair=True)
    assert y1 is y2
    (y1.sum() + (2 * y2).sum()).backward()
    got = a.grad.clone(), z.grad.clone(), m.weight.grad.clone()
    a.grad = z.grad = None
    m.zero_grad()
    torch.set_rng_state(st)
    y = m(a, z)
    assert torch.is_tensor(y) and torch.equal(y, y1)
    (3 * y).sum().backward()
    for g, w in zip(got, (a.grad, z.grad, m.weight.grad)):
        assert torch.allclose(g, w, rtol=1e-6, atol=1e-6)


def test_pair_backward_without_gradients():
    """Neither output reached the loss: no kernel call, no gradients."""
    from ravnest_amd.ops.dropout_ln import _DropoutAddLayerNormPairFn
    assert _DropoutAddLayerNormPairFn.backward(None, None, None) == \
        (None,) * 7


def test_fx_trace_keeps_the_module_calls(monkeypatch):
    from ravnest_amd.planner.splitter import trace_model
    model = _model(monkeypatch, "1")
    gm = trace_model(model)
    calls = [n for n in gm.graph.nodes if n.op == "call_module"
             and str(n.target).endswith((".ln1", ".ln2"))]
    assert len(calls) == 4
    for n in calls:
        assert "pair" not in n.kwargs and len(n.args) == 2
    model.eval(), gm.eval()
    ids = torch.randint(0, model.cfg.vocab_size, (2, 16))
    mask = torch.ones(2, 16, dtype=torch.int64)
    with torch.no_grad():
        assert torch.equal(gm(ids, mask), model(ids, mask))
