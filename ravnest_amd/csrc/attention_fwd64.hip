// Flash-style fused attention FORWARD for CDNA4 (gfx950), bf16, D=64, on
// 64-key stages (the default D=64 path without probability dropout;
// attention.hip keeps the 32-key kernel for dropout and as the
// RAVNEST_ATTN_FWD64=0 arm).
//
// Geometry (that of attention_bwd64.hip's dQ kernel). A block is 4 waves =
// 128 query rows; a wave owns 32 rows and keeps its 4 Q fragments in
// registers. K and V stream through LDS in stages of 64 keys = two 32-key
// [K | V] sub-tiles (attention_stage64.h), both operands in the XOR image,
// both filled by global_load_lds one stage ahead into the other of two
// slots. K is read as the A operand (afrag), V as a [key][d] B operand by
// tr16 gathers on the same image, so V needs no padded image, no register
// round trip and no LDS write after the compute.
//
// Between two block barriers a wave runs both sub-tiles: 8 QK MFMAs issued
// together, then ONE running-max decision (defer-max, DEFER_THR = 8), one
// O-rescale check and one l update for the 64 keys, then exp/pack and the
// 4 PV MFMAs per sub-tile: 16 MFMAs per barrier against 8, and the chain
// max -> decision -> rescale is paid once per 64 keys.
//
// Scores live in the log2 domain: x = s * (scale * log2 e) + mask * log2 e
// is one fma ahead of exp2, m_run is a log2-domain maximum and
// lse = (m_run + log2 l) * ln 2 converts back. The additive mask of a
// stage's 64 keys is staged next to the slot by a 4-byte LDS-DMA and read
// in the accumulator's own key layout (key = (r&3) + 8(r>>2) + 4 hi: four
// b128 reads per sub-tile, every lane of a half reads the same address).
// Key >= L and causal compares run only in a stage that the horizon or
// the wave's diagonal crosses.
//
// Registers and occupancy (chosen, not inherited): Q 16 + O 32 + both
// score tiles 32 + P fragments and operands in flight; resource figures
// and the tier held by launch_bounds are in csrc/README.md.
#include <torch/extension.h>

#include "attention_fwd64_block.h"

namespace {

// one block per 128 q rows of a (batch, head); the body is fwd64_block
template <bool MASK>
FWD64_TARGET __global__ __launch_bounds__(256, 3) void attn_fwd64_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const float* __restrict__ mask,
    bf16_t* __restrict__ o, float* __restrict__ lse, int S, int causal,
    float scale, long H, StridesB sq, StridesB sk, StridesB sv, StridesB so,
    const int* __restrict__ kv_len) {
  const long bh = blockIdx.y;
  const long b = bh / H, h = bh % H;
  fwd64_block<MASK>(q + b * sq.bs + h * sq.hs, k + b * sk.bs + h * sk.hs,
                    v + b * sv.bs + h * sv.hs, mask + b * (long)S,
                    o + b * so.bs + h * so.hs, lse + bh * (long)S, S,
                    kv_horizon(kv_len, b, S), blockIdx.x, causal, scale,
                    sq.rs, sk.rs, sv.rs, so.rs);
}

}  // namespace

void attn_fwd64_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                       const float* mask, bf16_t* o, float* lse, bool causal,
                       float scale, long B, long H, int S, StridesB sq,
                       StridesB sk, StridesB sv, StridesB so, const int* kvl,
                       hipStream_t stream) {
  const dim3 block(256), grid((S + 127) / 128, B * H);
  const int c = causal ? 1 : 0;
  if (mask)
    hipLaunchKernelGGL((attn_fwd64_kernel<true>), grid, block, 0, stream, q,
                       k, v, mask, o, lse, S, c, scale, H, sq, sk, sv, so,
                       kvl);
  else
    hipLaunchKernelGGL((attn_fwd64_kernel<false>), grid, block, 0, stream, q,
                       k, v, mask, o, lse, S, c, scale, H, sq, sk, sv, so,
                       kvl);
}
