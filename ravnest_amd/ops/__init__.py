from ._ext import get_ext, has_ext
from .layernorm import (FusedLayerNorm, AddLayerNorm, layer_norm, add_layer_norm)
from .activation import (GELU, LinearGelu, Softmax, gelu, bias_gelu,
                         softmax)
from .dropout import Dropout, dropout
from .dropout_ln import DropoutAddLayerNorm, dropout_add_layer_norm
from .attention import (AttentionCore, AttentionCoreQKV, attention,
                        attention_qkv, kv_len_from_mask)
from .losses import CrossEntropyLoss, cross_entropy
from .mlm_head import sparse_mlm_head_loss
from .optim import FusedAdam, FusedSGD, FusedLAMB, clip_grad_norm_
from .batchnorm import (FusedBatchNorm2d, FusedBatchNormReLU2d,
                        FusedBatchNormAddReLU2d)
from .linear import Linear
from .conv import Conv1x1, conv2d_mfma
from .embedding import embedding_ln, embedding_add
from .pool import MaxPool2d, AvgPool2d, AdaptiveAvgPool2d
from .mx import MXLinear, mx_linear, attach_mx, take_mx

__all__ = [
    "get_ext", "has_ext",
    "FusedLayerNorm", "AddLayerNorm", "layer_norm", "add_layer_norm",
    "GELU", "LinearGelu", "Softmax", "gelu", "bias_gelu", "softmax",
    "Dropout", "dropout",
    "DropoutAddLayerNorm", "dropout_add_layer_norm",
    "AttentionCore", "AttentionCoreQKV", "attention", "attention_qkv",
    "kv_len_from_mask",
    "CrossEntropyLoss", "cross_entropy", "sparse_mlm_head_loss",
    "FusedAdam", "FusedSGD", "FusedLAMB", "clip_grad_norm_",
    "FusedBatchNorm2d", "FusedBatchNormReLU2d", "FusedBatchNormAddReLU2d",
    "Linear", "Conv1x1", "conv2d_mfma",
    "embedding_ln", "embedding_add",
    "MaxPool2d", "AvgPool2d", "AdaptiveAvgPool2d",
    "MXLinear", "mx_linear", "attach_mx", "take_mx",
]
