// Host side of the attention key horizon (device side: kv_horizon in
// common.h), shared by attention.hip and attention_bwd.hip.
#pragma once

#include <ATen/ATen.h>
#include <c10/util/Optional.h>

// Optional per-sequence key counts -> device pointer (nullptr = none).
// Checks int32, contiguous, CUDA, numel() == B. Defined in attention.hip.
const int* attn_kv_len_ptr(const c10::optional<at::Tensor>& kv_len, long B);
