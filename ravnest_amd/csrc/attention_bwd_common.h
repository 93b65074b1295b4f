// Pieces shared by the flash-attention backward kernels (attention_bwd.hip
// and attention_bwd64.hip: D=64, attention_bwd128.hip: D=128) and the
// 64-key-stage forward (attention_fwd64.hip): the stride triple, the tr16 read and its offsets in the D=64 LDS image, the MFMA
// C-layout -> A-fragment repack and the Delta kernel.
#pragma once

#include "common.h"

typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// hardware transpose read (guide T10; semantics verified by tr16_probe in
// attention.hip): each lane loads 4 contiguous bf16 at its OWN 8-B
// address; per 16-lane group the loads form a [4][16] block M (lane
// order) and lane q receives column q.
#define DS_TR16(p) __builtin_amdgcn_ds_read_tr16_b64_v4bf16( \
    (__attribute__((address_space(3))) bf16x4v*)( \
        (__attribute__((address_space(3))) void*)(p)))

// element offset of (b, h, row) = b*bs + h*hs + row*rs (see attention.hip)
struct StridesB { long bs, hs, rs; };

DEVINL unsigned int pack_bf2b(float lo, float hi) {
  return (unsigned int)f2us(lo) | ((unsigned int)f2us(hi) << 16);
}

// the same pair through the hardware conversion (v_cvt_pk_bf16_f32):
// round-to-nearest-even as above, one instruction instead of nine
DEVINL unsigned int pack_bf2_cvt(float lo, float hi) {
  typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
  typedef float f32x2v __attribute__((ext_vector_type(2)));
  const f32x2v f = {lo, hi};
  return __builtin_bit_cast(unsigned int,
                            __builtin_convertvector(f, bf16x2v));
}

// transform a [row-pattern][col=lane] f32 acc (16 regs) into the A-operand
// fragments covering k=rows: pa[step] holds rows 16*step + (lane>>5)*8+e.
// CVT: pack with pack_bf2_cvt (the forward; NaN-free inputs give the same
// bits either way).
template <bool CVT>
DEVINL unsigned int pack_bf2_sel(float lo, float hi) {
  if constexpr (CVT) return pack_bf2_cvt(lo, hi);
  else return pack_bf2b(lo, hi);
}

template <bool CVT = false>
DEVINL void acc_to_afrag(const f32x16& acc, unsigned int pa[2][4]) {
#pragma unroll
  for (int step = 0; step < 2; ++step) {
    const int b0 = step * 8;
    unsigned int c01 = pack_bf2_sel<CVT>(acc[b0 + 0], acc[b0 + 1]);
    unsigned int c23 = pack_bf2_sel<CVT>(acc[b0 + 2], acc[b0 + 3]);
    unsigned int c45 = pack_bf2_sel<CVT>(acc[b0 + 4], acc[b0 + 5]);
    unsigned int c67 = pack_bf2_sel<CVT>(acc[b0 + 6], acc[b0 + 7]);
    {
      auto r2 = __builtin_amdgcn_permlane32_swap(c01, c45, false, false);
      pa[step][0] = r2[0];
      pa[step][2] = r2[1];
    }
    {
      auto r2 = __builtin_amdgcn_permlane32_swap(c23, c67, false, false);
      pa[step][1] = r2[0];
      pa[step][3] = r2[1];
    }
  }
}

// per-lane byte offset for a tr16 B-fragment read of
// B[k = kbase + 0..3][j = hh*32 + (lane&31)] from a 128-B-row LDS image,
// optionally XOR-swizzled ((row&15)<<4, 16-B granularity — an 8-B-aligned
// read never crosses the flipped boundary). The row-dependent XOR also
// de-conflicts the 4-lanes-per-row gather (rows r and r+2 land 32 B
// apart), so the swizzled images need no extra padding.
template <bool SWZ>
DEVINL int tr16_b_off(int lane, int kbase, int hh) {
  const int q4 = lane & 15;
  const int row = kbase + (q4 >> 2);
  int off = row * 128 + hh * 64 + ((lane >> 4) & 1) * 32 + 8 * (q4 & 3);
  if (SWZ) off ^= (row & 15) << 4;
  return off;
}

// Delta[row] = sum_d dO[row][d] * O[row][d]. D/8 lanes per row, bf16x8
// loads (the one-wave-per-row 2-B-scalar version measured 7x off the
// bandwidth bound at 2.5% of the BERT step — rocprofv3 r01 final).
template <int D>
__global__ void attn_bwd_delta_kernel(const bf16_t* __restrict__ dout,
                                      const bf16_t* __restrict__ o,
                                      float* __restrict__ delta, int S,
                                      long H, long NR, StridesB sdo) {
  constexpr int LPR = D / 8;  // lanes per row
  const int lane = threadIdx.x & (WAVE - 1);
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long id = t / LPR;
  if (id >= NR) return;
  const long bh = id / S;
  const long row = id % S;
  const long off = (bh / H) * sdo.bs + (bh % H) * sdo.hs + row * sdo.rs +
                   (t % LPR) * 8;
  bf16x8v a = *reinterpret_cast<const bf16x8v*>(dout + off);
  bf16x8v b = *reinterpret_cast<const bf16x8v*>(o + off);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (float)a[j] * (float)b[j];
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) s += __shfl_xor(s, m, WAVE);
  if ((lane & (LPR - 1)) == 0) delta[id] = s;
}

// D=128 backward (attention_bwd128.hip): Delta, dV, dK, dQ on `stream`.
// delta is fp32 scratch of B*H*S elements; kvl may be null.
void attn_bwd_d128_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                          const bf16_t* o, const bf16_t* dout,
                          const float* lse, float* delta, const float* mask,
                          bool causal, float scale, long B, long H, int S,
                          StridesB sio, StridesB sdo, StridesB sg,
                          bf16_t* dq, bf16_t* dk, bf16_t* dv, const int* kvl,
                          hipStream_t stream);

// D=64 backward on 64-row stages (attention_bwd64.hip): Delta, dK+dV, dQ
// on `stream`; same contract as attn_bwd_d128_launch.
void attn_bwd64_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                       const bf16_t* o, const bf16_t* dout, const float* lse,
                       float* delta, const float* mask, bool causal,
                       float scale, long B, long H, int S, StridesB sio,
                       StridesB sdo, StridesB sg, bf16_t* dq, bf16_t* dk,
                       bf16_t* dv, const int* kvl, hipStream_t stream);

// D=64 forward on 64-key stages (attention_fwd64.hip), no probability
// dropout: o (bf16) and lse = m + ln l (fp32, B*H*S) on `stream`; mask
// (fp32, B*S) and kvl may be null.
void attn_fwd64_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                       const float* mask, bf16_t* o, float* lse, bool causal,
                       float scale, long B, long H, int S, StridesB sq,
                       StridesB sk, StridesB sv, StridesB so, const int* kvl,
                       hipStream_t stream);
