"""BERT-base encoder for MLM pretraining, built on the MI355X op library.

Workload parity: the reference's BERT pretraining example (HuggingFace
BertForPreTraining on tokenized WikiText, examples/bert/provider.py) —
re-implemented natively so the hot ops (fused LayerNorm, bias-GELU,
flash-style attention, replayable dropout) run on the hand-written CDNA4
kernels while projections use hipBLASLt. fx-traceable for the pipeline
splitter (custom-op modules are fx leaves).

BERT-base config: L=12, H=768, A=12, I=3072, vocab=30522, seq<=512.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import embedding_ln
from ..ops import (AttentionCoreQKV, Dropout, DropoutAddLayerNorm,
                   FusedLayerNorm, GELU, LinearGelu)
from ..ops.linear import make_linear


def _plain_biased_linear(lin) -> bool:
    return type(lin) is nn.Linear and lin.bias is not None


def _linear_bias_downstream(lin, x):
    """lin(x) with the bias detached: the same addmm runs forward, but
    autograd's addmm backward no longer reduces the output gradient over
    its rows for the bias. The caller hands lin.bias to the fused op that
    consumes the result, whose backward produces that gradient from
    registers (ops/dropout_ln.py zbias)."""
    return F.linear(x, lin.weight, lin.bias.detach())


class BertConfig:
    def __init__(self, vocab_size=30522, hidden=768, layers=12, heads=12,
                 intermediate=3072, max_seq=512, type_vocab=2,
                 dropout=0.1, layer_norm_eps=1e-12):
        self.vocab_size = vocab_size
        self.hidden = hidden
        self.layers = layers
        self.heads = heads
        self.intermediate = intermediate
        self.max_seq = max_seq
        self.type_vocab = type_vocab
        self.dropout = dropout
        self.layer_norm_eps = layer_norm_eps

    @classmethod
    def base(cls, **kw):
        return cls(**kw)

    @classmethod
    def tiny(cls, **kw):
        # head_dim 64 (the attention kernel's native size)
        d = dict(vocab_size=1024, hidden=128, layers=2, heads=2,
                 intermediate=256, max_seq=64)
        d.update(kw)
        return cls(**d)


class BertEmbeddings(nn.Module):
    _is_leaf_module = True  # fx: data-dependent position slice

    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.word = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.position = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.ln = FusedLayerNorm(cfg.hidden, cfg.layer_norm_eps)
        self.drop = Dropout(cfg.dropout)
        self.register_buffer(
            "pos_ids", torch.arange(cfg.max_seq).unsqueeze(0),
            persistent=False)

    def forward(self, input_ids):
        if input_ids.is_cuda and self.word.weight.dtype == torch.bfloat16:
            # single-pass gather+gather+LN kernel (ops/embedding.py)
            y = embedding_ln(input_ids, self.word.weight,
                             self.position.weight, self.ln.weight,
                             self.ln.bias, self.ln.eps)
            return self.drop(y)
        S = input_ids.size(1)
        x = self.word(input_ids) + self.position(self.pos_ids[:, :S])
        return self.drop(self.ln(x))


class BertSelfAttention(nn.Module):
    """DOCUMENTED SEMANTICS DIFFERENCE vs HuggingFace BERT: by default
    dropout is applied AFTER the output projection (inside BertLayer.ln1,
    fused with the residual add and the LayerNorm; this module returns the
    un-dropped projection) instead of on the attention probabilities — the fused flash kernel
    never materializes the S x S probs. Set RAVNEST_EXACT_ATTN_DROPOUT=1
    (before model construction) for exact HF prob-dropout semantics via
    the composed P-materializing path (replayable philox mask; lower
    throughput — ops/attention.py attention_qkv_prob_dropout)."""

    def __init__(self, cfg: BertConfig):
        super().__init__()
        import os
        self.heads = cfg.heads
        self.head_dim = cfg.hidden // cfg.heads
        self.qkv = make_linear(cfg.hidden, 3 * cfg.hidden)
        exact = os.environ.get("RAVNEST_EXACT_ATTN_DROPOUT", "0") == "1"
        self.core = AttentionCoreQKV(
            causal=False, prob_dropout=cfg.dropout if exact else 0.0)
        self.out = make_linear(cfg.hidden, cfg.hidden)

    def forward(self, x, mask, out_bias_downstream: bool = False):
        """out_bias_downstream: the caller takes the bias gradient of
        self.out from the op that consumes the result (BertLayer.ln1); the
        projection then runs with its bias detached."""
        # packed (B,S,3,H,D) qkv: the attention kernel reads the
        # projection's natural layout and returns token-major O — no
        # permute/contiguous copies (unflatten also keeps the fx graph
        # free of .size() scalar nodes)
        qkv = self.qkv(x).unflatten(-1, (3, self.heads, self.head_dim))
        o = self.core(qkv, mask)
        if out_bias_downstream:
            return _linear_bias_downstream(self.out, o)
        return self.out(o)


class BertLayer(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.attn = BertSelfAttention(cfg)
        # ln1/ln2 = LN(x + dropout(sublayer)): dropout, residual add and
        # LayerNorm in one kernel each way (ops/dropout_ln.py)
        self.ln1 = DropoutAddLayerNorm(cfg.hidden, cfg.layer_norm_eps,
                                       cfg.dropout)
        self.mlp_in = LinearGelu(cfg.hidden, cfg.intermediate)
        self.mlp_out = make_linear(cfg.intermediate, cfg.hidden)
        self.ln2 = DropoutAddLayerNorm(cfg.hidden, cfg.layer_norm_eps,
                                       cfg.dropout)
        # RAVNEST_FUSED_BIAS_GRAD=0: the attn.out and mlp_out bias gradients
        # come from autograd's own reduction again (A/B inside one build).
        # The qkv bias keeps autograd's reduction either way: summing dqkv in
        # the attention backward kernels measured slower than that reduction
        # (profiles/bias_grad_gelu.txt, section 2).
        self.fused_bias_grad = \
            os.environ.get("RAVNEST_FUSED_BIAS_GRAD", "1") != "0"

    def _bias_downstream(self, ln, a, lin) -> bool:
        # a plain nn.Linear whose consumer takes the fused kernel path.
        # Not while fx-tracing (a is a Proxy; torch.is_tensor comes first
        # because even reading a parameter there adds a node to the graph):
        # the pipeline splitter may cut between a projection and its
        # consumer, which would part the bias from its gradient; traced
        # graphs keep the module calls.
        return (self.fused_bias_grad and torch.is_tensor(a)
                and _plain_biased_linear(lin) and ln.takes_zbias(a, lin))

    def forward(self, x, mask):
        # attn.out -> ln1 and mlp_out -> ln2: the LayerNorm backward sums
        # dz for the projection's bias (ops/dropout_ln.py zbias)
        if self._bias_downstream(self.ln1, x, self.attn.out):
            x = self.ln1(x, self.attn(x, mask, out_bias_downstream=True),
                         zbias=self.attn.out.bias)
        else:
            x = self.ln1(x, self.attn(x, mask))
        if self._bias_downstream(self.ln2, x, self.mlp_out):
            x = self.ln2(x, _linear_bias_downstream(self.mlp_out,
                                                    self.mlp_in(x)),
                         zbias=self.mlp_out.bias)
        else:
            x = self.ln2(x, self.mlp_out(self.mlp_in(x)))
        return x


class BertMLMHead(nn.Module):
    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.dense = make_linear(cfg.hidden, cfg.hidden)
        self.act = GELU()
        self.ln = FusedLayerNorm(cfg.hidden, cfg.layer_norm_eps)
        self.decoder = make_linear(cfg.hidden, cfg.vocab_size)

    def transform(self, x):
        """dense -> GELU -> LayerNorm: the decoder's input."""
        return self.ln(self.act(self.dense(x)))

    def forward(self, x):
        return self.decoder(self.transform(x))


class BertForMLM(nn.Module):
    """input_ids (B,S) int64, attention_mask (B,S) {0,1} -> logits (B,S,V)."""

    def __init__(self, cfg: BertConfig | None = None):
        super().__init__()
        self.cfg = cfg or BertConfig.base()
        self.embeddings = BertEmbeddings(self.cfg)
        self.layers = nn.ModuleList(
            [BertLayer(self.cfg) for _ in range(self.cfg.layers)])
        self.head = BertMLMHead(self.cfg)
        self.apply(self._init)

    @staticmethod
    def _init(m):
        from ..ops import Linear as _OpsLinear
        if isinstance(m, (nn.Linear, _OpsLinear)):
            nn.init.normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=0.02)

    def _encode(self, input_ids, attention_mask):
        # additive mask: (B,S) {0,1} -> (B,1,1,S) {0,-inf-ish}
        m = (1.0 - attention_mask.to(torch.float32)) * -10000.0
        m = m.unsqueeze(1).unsqueeze(2)
        x = self.embeddings(input_ids)
        for layer in self.layers:
            x = layer(x, m)
        return x

    def forward(self, input_ids, attention_mask):
        return self.head(self._encode(input_ids, attention_mask))

    def forward_loss(self, input_ids, attention_mask, targets, criterion):
        """Opt-in fused model+criterion step: encoder and head transform
        as in forward(), then decoder + cross-entropy on the rows whose
        label is not ignored only (ops/mlm_head.py). Returns the loss, or
        None when the fused op does not apply — the caller then computes
        criterion(self(input_ids, attention_mask), targets)."""
        from ..ops.losses import CrossEntropyLoss
        from ..ops.mlm_head import (sparse_mlm_head_enabled,
                                    sparse_mlm_head_loss,
                                    sparse_mlm_head_supported)
        dec = self.head.decoder
        if not (self.training and sparse_mlm_head_enabled()
                and type(criterion) is CrossEntropyLoss
                and torch.is_tensor(targets) and input_ids.is_cuda
                and dec.weight.is_cuda
                and dec.weight.dtype == torch.bfloat16
                and not torch.is_autocast_enabled()
                and targets.numel() == input_ids.numel()):
            return None
        if not sparse_mlm_head_supported(dec.weight, dec.bias, targets):
            return None
        x = self._encode(input_ids, attention_mask)
        h = self.head.transform(x)
        return sparse_mlm_head_loss(h, dec.weight, dec.bias, targets,
                                    criterion.ignore_index)
