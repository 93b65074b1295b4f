"""Loss of the fused root+leaf stage: model forward + criterion.

A model may offer ``forward_loss(*args, targets, criterion)`` — a fused
model+criterion path that returns the loss directly, or None when it does
not apply (BertForMLM: decoder + cross-entropy on the non-ignored rows
only, ops/mlm_head.py). Models without it (GPT, ResNet, fx-split pipeline
stages) take the plain ``criterion(model(*args), targets)``.
"""
from __future__ import annotations

import torch


def model_loss(model, criterion, args, targets):
    fused = getattr(model, "forward_loss", None)
    if fused is not None and torch.is_tensor(targets) and \
            all(torch.is_tensor(a) for a in args):
        loss = fused(*args, targets, criterion)
        if loss is not None and loss is not NotImplemented:
            return loss
    return criterion(model(*args), targets)
