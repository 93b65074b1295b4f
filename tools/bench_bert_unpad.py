#!/usr/bin/env python3
"""Eager BERT training step (forward_loss + backward + FusedAdam) on
variable-length batches: the padded (B,S) batch with KV_SKIP on against
the packed (T,) stream of ops.unpad_batch through forward_loss_packed, on
the same seeded batches.

    python tools/bench_bert_unpad.py [--batch 32] [--seq 512]
        [--model base] [--rounds 5] [--steps 4]

Lengths are the seeded uniform [16, seq] draw of examples/bert/provider.py
--var-len, one draw per step, so every packed step has its own T (eager
only: a captured step needs a static T). Arms alternate round after round
in one process on copies of one model; device events time `steps`
consecutive steps, host-side unpadding and copies to the device excluded
(both arms start from device tensors). The two arms' first-step losses
are printed; they differ by their dropout masks.
"""
import argparse
import copy
import importlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ravnest_amd import ops  # noqa: E402
from ravnest_amd.models import BertConfig, BertForMLM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--model", choices=("base", "tiny"), default="base")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    importlib.import_module("ravnest_amd.ops.attention").KV_SKIP = True
    torch.manual_seed(0)
    B, S = args.batch, args.seq
    cfg = BertConfig.base() if args.model == "base" \
        else BertConfig.tiny(max_seq=S)
    crit = ops.CrossEntropyLoss(-100)
    models = {"padded": BertForMLM(cfg).to(dev).to(torch.bfloat16).train()}
    models["packed"] = copy.deepcopy(models["padded"])
    opts = {k: ops.FusedAdam(m.parameters(), lr=1e-4)
            for k, m in models.items()}

    g = torch.Generator().manual_seed(42)
    batches = {"padded": [], "packed": []}
    live = 0
    for _ in range(args.steps):
        ids = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
        labels = ids.clone()
        labels[torch.rand(ids.shape, generator=g) > 0.15] = -100
        lens = torch.randint(16, S + 1, (B,), generator=g)
        mask = (torch.arange(S)[None, :] < lens[:, None]).to(ids.dtype)
        labels[mask == 0] = -100
        live += int(lens.sum())
        batches["padded"].append([t.to(dev) for t in (ids, mask, labels)])
        pids, pos, cu, ptgt, _ = ops.unpad_batch(ids, mask, labels)
        batches["packed"].append([t.to(dev) for t in (pids, pos, cu, ptgt)])

    def step(arm, batch):
        model = models[arm]
        fn = model.forward_loss if arm == "padded" \
            else model.forward_loss_packed
        loss = fn(*batch, crit)
        assert loss is not None, "the sparse MLM head did not apply"
        loss.backward()
        opts[arm].step()
        opts[arm].zero_grad(set_to_none=True)
        return loss

    def timed(arm):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for batch in batches[arm]:
            step(arm, batch)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / args.steps

    first = {arm: float(step(arm, batches[arm][0]).detach())
             for arm in models}
    for arm in models:  # warm-up on every shape the timed window uses
        timed(arm)
    res = {arm: [] for arm in models}
    for _ in range(args.rounds):
        for arm in models:
            res[arm].append(timed(arm))
    print(f"bench_bert_unpad: bert-{args.model} B={B} S={S}, live tokens "
          f"{live / (args.steps * B * S):.3f} of the padded batch, "
          f"{args.rounds} rounds x {args.steps} steps, eager "
          "fwd+bwd+FusedAdam, ms per step")
    for arm, v in res.items():
        print(f"  {arm:6s}: median {statistics.median(v):8.3f}  "
              f"min {min(v):8.3f}  max {max(v):8.3f}  "
              f"first-step loss {first[arm]:.4f}")
    print("  packed / padded = "
          f"{statistics.median(res['packed']) / statistics.median(res['padded']):.3f}")


if __name__ == "__main__":
    main()
