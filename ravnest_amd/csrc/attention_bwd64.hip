// Flash-style fused attention BACKWARD for CDNA4 (gfx950), bf16, D=64,
// on 64-row stages (the default D=64 path without probability dropout;
// attention_bwd.hip keeps the 32-row kernels for dropout and as the
// RAVNEST_ATTN_BWD64=0 arm).
//
//   attn_bwd64_kv_kernel  dK and dV: wave owns 32 keys, loops Q/dO stages
//   attn_bwd64_dq_kernel  dQ:        wave owns 32 q rows, loops K/V stages
//
// Geometry. A block is 4 waves = 128 keys (or q rows). The wave-owned
// operands (K+V, or Q+dO: 4 bf16x8 fragments each) stay in registers for
// the whole loop. The streamed operands go through LDS in stages of 64
// rows = two 32-row sub-tiles. Between two block barriers a wave runs both
// sub-tiles back to back with the fragment algebra of attention_bwd.hip:
//   kv: S, dP (8 MFMAs) -> P, dS in registers -> dV += P^T dO,
//       dK += dS^T Q (8 MFMAs), twice = 32 MFMAs per barrier;
//   dq: S^T, dP^T (8) -> dS^T -> dQ += dS K (4), twice = 24 per barrier,
// against 12 in the 32-row kernels. One S matmul and one staging of Q/dO
// feed both dK and dV, so the backward executes 7 matmul passes, not 8,
// in 3 launches (Delta, kv, dq), not 4. RAVNEST_ATTN_DELTA_FUSED=1 (read at
// every call) makes it 2 (dq, kv), with Delta computed by the dq kernel from
// its dO fragments: the Delta kernel's pass over dO and O (200 MB at
// BERT-base's shape for 4 bytes per row) becomes one O read by the waves
// that hold dO already. Off by default: the BERT step gained 0.3 %, inside
// the run-to-run spread (profiles/residual_delta.txt). When both sub-tiles of a stage are
// live their S/dP matmuls are issued together ahead of the first exp
// phase, so one sub-tile's MFMAs cover the other's LDS-read -> exp -> pack
// chain inside one wave as well as across waves.
//
// LDS image (attention_stage64.h). A sub-tile is two 4 KiB operand tiles,
// [Q | dO] or [K | V], each 32 rows of 128 B in the ((row & 15) << 4) XOR
// image of attention_bwd.hip (conflict-free b128 A-fragment reads and tr16
// B-fragment gathers). A stage slot is two sub-tiles = 16 KiB; two slots
// = 32 KiB, filled by global_load_lds one stage ahead of the compute (the
// XOR is applied on the source side, four 16-B DMA loads per thread and
// stage; rows past S-1 are clamped, a sub-tile wholly past the end is not
// staged). The kv kernel adds lse and Delta rows (16 KiB) while
// S <= 2048 and reads them from global memory above that: 48 KiB.
//
// Registers and occupancy (chosen, not inherited). kv: K and V fragments
// 32 + dK and dV accumulators 64 + S and dP of both sub-tiles 64 + P/dS
// fragments and B operands: 2 waves/SIMD (<= 256 registers) on purpose.
// The 32-row merged kernel this replaces kept one barrier per 32 rows and
// lost the occupancy tier that structure depends on; here a barrier
// interval carries 32 MFMAs and the second sub-tile's matmuls are the
// latency cover. dq: Q and dO fragments 32 + accumulators 32 + S and dP 64,
// also bound to 2 waves/SIMD. launch_bounds hold the compiler to that
// tier; resource figures are in csrc/README.md.
#include <torch/extension.h>

#include "attention_bwd64_block.h"

namespace {

// one block per 128 keys (kv) or q rows (dq) of a (batch, head); the
// bodies are bwd64_kv_block and bwd64_dq_block
BWD64_TARGET __global__ __launch_bounds__(256, 2) void attn_bwd64_kv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ mask, bf16_t* __restrict__ dk,
    bf16_t* __restrict__ dv, int S, int causal, float scale, int has_mask,
    long H, StridesB sio, StridesB sdo, StridesB sg,
    const int* __restrict__ kv_len) {
  const long bh = blockIdx.y;
  const long b = bh / H, h = bh % H;
  const long io = b * sio.bs + h * sio.hs, g = b * sg.bs + h * sg.hs;
  bwd64_kv_block(q + io, k + io, v + io, dout + b * sdo.bs + h * sdo.hs,
                 lse + bh * (long)S, delta + bh * (long)S, mask + b * (long)S,
                 dk + g, dv + g, S, kv_horizon(kv_len, b, S), blockIdx.x,
                 causal, scale, has_mask, sio.rs, sdo.rs, sg.rs);
}

// DELTA: o is read and delta written (bwd64_dq_block); else o is unused
template <bool DELTA>
BWD64_TARGET __global__ __launch_bounds__(256, 2) void attn_bwd64_dq_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ o,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, const float* __restrict__ mask,
    bf16_t* __restrict__ dq, int S,
    int causal, float scale, int has_mask, long H, StridesB sio,
    StridesB sdo, StridesB sg, const int* __restrict__ kv_len) {
  const long bh = blockIdx.y;
  const long b = bh / H, h = bh % H;
  const long io = b * sio.bs + h * sio.hs;
  const long od = b * sdo.bs + h * sdo.hs;
  bwd64_dq_block<DELTA>(
      q + io, k + io, v + io, dout + od, lse + bh * (long)S,
      delta + bh * (long)S, mask + b * (long)S, dq + b * sg.bs + h * sg.hs,
      S, kv_horizon(kv_len, b, S), blockIdx.x, causal, scale, has_mask,
      sio.rs, sdo.rs, sg.rs, o + od, delta + bh * (long)S);
}

}  // namespace

void attn_bwd64_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                       const bf16_t* o, const bf16_t* dout, const float* lse,
                       float* delta, const float* mask, bool causal,
                       float scale, long B, long H, int S, StridesB sio,
                       StridesB sdo, StridesB sg, bf16_t* dq, bf16_t* dk,
                       bf16_t* dv, const int* kvl, hipStream_t stream) {
  const dim3 block(256), grid((S + 127) / 128, B * H);
  const int c = causal ? 1 : 0, hm = mask ? 1 : 0;
  // read at every call, so that one process can run both arms
  const char* e = getenv("RAVNEST_ATTN_DELTA_FUSED");
  const bool fused = e && e[0] == '1';
  if (fused) {  // dq writes the Delta that kv reads
    hipLaunchKernelGGL(attn_bwd64_dq_kernel<true>, grid, block, 0, stream, q,
                       k, v, o, dout, lse, delta, mask, dq, S, c, scale, hm,
                       H, sio, sdo, sg, kvl);
  } else {
    const long NR = B * H * (long)S;
    hipLaunchKernelGGL((attn_bwd_delta_kernel<64>),
                       dim3((NR * 8 + 255) / 256), dim3(256), 0, stream, dout,
                       o, delta, S, H, NR, sdo);
  }
  hipLaunchKernelGGL(attn_bwd64_kv_kernel, grid, block, 0, stream, q, k, v,
                     dout, lse, (const float*)delta, mask, dk, dv, S, c,
                     scale, hm, H, sio, sdo, sg, kvl);
  if (!fused)
    hipLaunchKernelGGL(attn_bwd64_dq_kernel<false>, grid, block, 0, stream, q,
                       k, v, o, dout, lse, delta, mask, dq, S, c, scale, hm,
                       H, sio, sdo, sg, kvl);
}
