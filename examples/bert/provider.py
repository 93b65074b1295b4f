"""BERT-base MLM pretraining, 4-stage pipeline, LAMB + grad accumulation
(parity: reference examples/bert/provider.py — WikiText replaced by
synthetic token batches: no network in this environment)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import argparse  # noqa: E402

from examples.common import node_name  # noqa: E402

import torch  # noqa: E402

from ravnest_amd import Node, set_seed  # noqa: E402
from ravnest_amd.models import BertConfig, BertForMLM  # noqa: E402
from ravnest_amd.ops import CrossEntropyLoss, FusedLAMB  # noqa: E402
from examples.bert.bert_trainer import BertTrainer  # noqa: E402

SEQ, BATCH, NBATCH = 512, 8, 64


def synthetic_batches(vocab, var_len=False):
    """var_len: sequences of seeded random length (uniform on [16, SEQ]),
    right-padded to SEQ with attention_mask 0 and label -100 on the
    padding -- the shape of batch a pad_to_multiple_of=512 collator over
    text lines produces. The attention kernels skip the padded keys only
    with ops.attention.KV_SKIP on, which is off by default; --var-len
    below turns it on."""
    g = torch.Generator().manual_seed(42)
    out = []
    for _ in range(NBATCH):
        ids = torch.randint(0, vocab, (BATCH, SEQ), generator=g)
        labels = ids.clone()
        labels[torch.rand(ids.shape, generator=g) > 0.15] = -100
        mask = torch.ones_like(ids)
        if var_len:
            lens = torch.randint(16, SEQ + 1, (BATCH,), generator=g)
            mask = (torch.arange(SEQ)[None, :] < lens[:, None]).to(ids.dtype)
            labels[mask == 0] = -100
        out.append({"input_ids": ids,
                    "attention_mask": mask,
                    "labels": labels})
    return out


if __name__ == "__main__":
    set_seed(42)
    name, base_dir = node_name()
    ap = argparse.ArgumentParser()
    # clip gradients by their global L2 norm before each optimizer step
    # (per pipeline stage: each stage clips its own parameter shard)
    ap.add_argument("--max-grad-norm", type=float, default=None)
    # variable-length, right-padded batches instead of full 512-token ones;
    # also has attention derive its key horizon from the padding mask
    ap.add_argument("--var-len", action="store_true")
    args = ap.parse_known_args()[0]
    max_grad_norm = args.max_grad_norm
    if args.var_len:
        # (ops.attention the attribute is the function, not the module)
        import importlib
        importlib.import_module("ravnest_amd.ops.attention").KV_SKIP = True
    cfg = BertConfig.base()
    batches = synthetic_batches(cfg.vocab_size, var_len=args.var_len)
    crit = CrossEntropyLoss(-100)
    node = Node(name=name, base_dir=base_dir,
                optimizer=FusedLAMB,
                optimizer_params={"lr": 1.76e-3},
                criterion=lambda preds, b: crit(preds, b["labels"]),
                labels=batches,
                update_frequency=16,
                max_grad_norm=max_grad_norm)
    node.start()
    trainer = BertTrainer(node=node, train_loader=batches, epochs=45,
                          batch_size=BATCH)
    trainer.train()

    # clean shutdown: root drains + cascades STOP; every rank closes its
    # channels (prevents the gloo teardown abort on live recv threads)
    if node.node_type.value == "root":
        node.stop_cluster()
    node.stop()
