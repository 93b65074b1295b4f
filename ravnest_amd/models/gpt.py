"""GPT decoder family (gpt-nano ... gpt2-small) on the MI355X op library.

Workload parity: the reference's minGPT sorter example
(examples/sorter/mingpt/model_without_padding_mask.py) including the
fx-friendly structure (custom-op modules are fx leaves — the reference
patched arange/masked_fill into leaf modules for the same reason,
model_without_padding_mask.py:34-48). Causal attention runs on the fused
CDNA4 attention kernel.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import (AttentionCoreQKV, Dropout, FusedLayerNorm,
                   LinearGelu, MXLinear)
from ..ops import attention_decode, embedding_add


class GPTConfig:
    def __init__(self, vocab_size, block_size, n_layer, n_head, n_embd,
                 dropout=0.1, fp8=False):
        self.vocab_size = vocab_size
        self.block_size = block_size
        self.n_layer = n_layer
        self.n_head = n_head
        self.n_embd = n_embd
        self.dropout = dropout
        # fp8=True runs the block projections on the MX-scaled fp8 MFMA
        # path (ops.MXLinear, state-dict compatible with nn.Linear) —
        # BASELINE.json "GPT-Sorter fp8 CDNA4 MFMA path". Requires
        # n_embd % 64 == 0.
        self.fp8 = fp8

    @classmethod
    def nano(cls, vocab_size=16, block_size=16):
        return cls(vocab_size, block_size, n_layer=3, n_head=3, n_embd=48)

    @classmethod
    def nano64(cls, vocab_size=16, block_size=16):
        """gpt-nano scale with head_dim 64 (the GPU attention kernel's
        native size)."""
        return cls(vocab_size, block_size, n_layer=3, n_head=3, n_embd=192)

    @classmethod
    def nano128(cls, vocab_size=16, block_size=16):
        """gpt-nano scale with head_dim 128, the head size of most current
        decoder models (packed flash forward and backward kernels)."""
        return cls(vocab_size, block_size, n_layer=3, n_head=2, n_embd=256)

    @classmethod
    def gpt2_small(cls, vocab_size=50257, block_size=1024):
        return cls(vocab_size, block_size, n_layer=12, n_head=12, n_embd=768)


class GPTEmbeddings(nn.Module):
    _is_leaf_module = True  # fx: data-dependent position slice

    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.tok_emb = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.pos_emb = nn.Embedding(cfg.block_size, cfg.n_embd)
        self.drop = Dropout(cfg.dropout)
        self.register_buffer("pos_ids",
                             torch.arange(cfg.block_size).unsqueeze(0),
                             persistent=False)

    def forward(self, idx):
        # sequence-parallel shards carry a position offset in pos_ids
        # (parallel/sp.py); the fused stem indexes positions from 0, so
        # SP routes through the eager gather
        if idx.is_cuda and self.tok_emb.weight.dtype == torch.bfloat16 \
                and not getattr(self, "_sp_offset", 0):
            x = embedding_add(idx, self.tok_emb.weight, self.pos_emb.weight)
            return self.drop(x)
        S = idx.size(1)
        x = self.tok_emb(idx) + self.pos_emb(self.pos_ids[:, :S])
        return self.drop(x)


class GPTBlock(nn.Module):
    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.n_head = cfg.n_head
        self.head_dim = cfg.n_embd // cfg.n_head
        fp8 = getattr(cfg, "fp8", False)
        if fp8 and cfg.n_embd % 64 != 0:
            raise ValueError("fp8 GPT needs n_embd % 64 == 0")
        from ..ops.linear import make_linear
        lin = MXLinear if fp8 else make_linear
        # fp8: ln1 and mlp_in feed an MXLinear and hand it their output
        # already quantised (ops/mx.py FUSED_QUANT)
        self.ln1 = FusedLayerNorm(cfg.n_embd, emit_mx=fp8)
        self.qkv = lin(cfg.n_embd, 3 * cfg.n_embd)
        self.core = AttentionCoreQKV(causal=True)
        self.proj = lin(cfg.n_embd, cfg.n_embd)
        self.attn_drop = Dropout(cfg.dropout)
        self.ln2 = FusedLayerNorm(cfg.n_embd)
        self.mlp_in = LinearGelu(cfg.n_embd, 4 * cfg.n_embd, emit_mx=fp8)
        self.mlp_out = lin(4 * cfg.n_embd, cfg.n_embd)
        self.mlp_drop = Dropout(cfg.dropout)

    def forward(self, x):
        h = self.ln1(x)
        qkv = self.qkv(h).unflatten(-1, (3, self.n_head, self.head_dim))
        o = self.core(qkv)
        x = x + self.attn_drop(self.proj(o))
        x = x + self.mlp_drop(self.mlp_out(self.mlp_in(self.ln2(x))))
        return x

    def prefill(self, x, cache):
        """forward() over the prompt (B,S,C) that also copies the prompt's
        keys and values into rows [0, S) of cache = (k_cache, v_cache),
        each (B, H, block_size, D)."""
        h = self.ln1(x)
        qkv = self.qkv(h).unflatten(-1, (3, self.n_head, self.head_dim))
        S = x.size(1)
        cache[0][:, :, :S].copy_(qkv[:, :, 1].transpose(1, 2))
        cache[1][:, :, :S].copy_(qkv[:, :, 2].transpose(1, 2))
        o = self.core(qkv)
        x = x + self.attn_drop(self.proj(o))
        x = x + self.mlp_drop(self.mlp_out(self.mlp_in(self.ln2(x))))
        return x

    def decode(self, x, cache, cache_len, max_len=None):
        """One cached step: x (B,1,C) is the new token, cache_len (B,)
        int32 the keys already cached. Appends the token's k and v to the
        caches in place; the caller advances cache_len."""
        B = x.size(0)
        qkv = self.qkv(self.ln1(x)).view(B, 3, self.n_head, self.head_dim)
        o = attention_decode(qkv, cache[0], cache[1], cache_len,
                             max_len=max_len)
        x = x + self.attn_drop(self.proj(o.unsqueeze(1)))
        x = x + self.mlp_drop(self.mlp_out(self.mlp_in(self.ln2(x))))
        return x


class GPT(nn.Module):
    """idx (B,S) int64 -> logits (B,S,V)."""

    def __init__(self, cfg: GPTConfig):
        super().__init__()
        self.cfg = cfg
        self.embeddings = GPTEmbeddings(cfg)
        self.blocks = nn.ModuleList(
            [GPTBlock(cfg) for _ in range(cfg.n_layer)])
        self.ln_f = FusedLayerNorm(cfg.n_embd)
        from ..ops.linear import make_linear
        self.lm_head = make_linear(cfg.n_embd, cfg.vocab_size, bias=False)
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

    def forward(self, idx):
        x = self.embeddings(idx)
        for b in self.blocks:
            x = b(x)
        return self.lm_head(self.ln_f(x))

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, use_cache=False):
        """Greedy decode (parity: sorter inference,
        examples/sorter/mingpt/utils.py).

        use_cache=True keeps a key/value cache per block: one causal
        forward over the prompt, then one-token steps on the decode
        attention kernel instead of a full forward per token. Absolute
        position embeddings cannot slide a cached window, so the prompt
        plus max_new_tokens must fit block_size; fp8 models are not
        supported."""
        self.eval()
        if use_cache:
            return self._generate_cached(idx, max_new_tokens)
        for _ in range(max_new_tokens):
            idx_cond = idx[:, -self.cfg.block_size:]
            logits = self(idx_cond)
            nxt = logits[:, -1, :].argmax(dim=-1, keepdim=True)
            idx = torch.cat([idx, nxt], dim=1)
        return idx

    def _generate_cached(self, idx, max_new_tokens):
        cfg = self.cfg
        B, S0 = idx.shape
        if S0 + max_new_tokens > cfg.block_size:
            raise ValueError(
                f"use_cache=True needs prompt ({S0}) + max_new_tokens "
                f"({max_new_tokens}) <= block_size ({cfg.block_size})")
        if getattr(cfg, "fp8", False):
            raise ValueError("use_cache=True does not support fp8 models")
        if max_new_tokens <= 0:
            return idx
        emb = self.embeddings
        w = emb.tok_emb.weight
        shape = (B, cfg.n_head, cfg.block_size, cfg.n_embd // cfg.n_head)
        caches = [(torch.zeros(shape, dtype=w.dtype, device=w.device),
                   torch.zeros(shape, dtype=w.dtype, device=w.device))
                  for _ in self.blocks]
        # one counter for all layers, read by the kernels on the device
        cache_len = torch.full((B,), S0, dtype=torch.int32, device=w.device)
        x = emb(idx)
        for blk, cache in zip(self.blocks, caches):
            x = blk.prefill(x, cache)
        logits = self.lm_head(self.ln_f(x[:, -1:]))
        nxt = logits[:, -1, :].argmax(dim=-1, keepdim=True)
        idx = torch.cat([idx, nxt], dim=1)
        for step in range(1, max_new_tokens):
            x = emb.tok_emb(nxt) + emb.pos_emb(cache_len.long())[:, None]
            x = emb.drop(x)
            for blk, cache in zip(self.blocks, caches):
                # this step's token sits at row S0 + step - 1
                x = blk.decode(x, cache, cache_len, max_len=S0 + step)
            logits = self.lm_head(self.ln_f(x))
            nxt = logits[:, -1, :].argmax(dim=-1, keepdim=True)
            idx = torch.cat([idx, nxt], dim=1)
            cache_len += 1
        return idx
