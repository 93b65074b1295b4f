// The block body of the D=64 forward on 64-key stages, shared by the dense
// grid (attention_fwd64.hip: one block per 128 rows of a (B, S) batch) and
// the packed one (attention_varlen64.hip: one block per tile-table entry of
// a token stream). A caller hands it one sequence: base pointers of its
// first row, its length S, its key horizon L and the block's 128-row tile.
// The design notes are in attention_fwd64.hip.
#pragma once

#include "attention_stage64.h"

#if defined(__HIP_DEVICE_COMPILE__)
// no packed fp32 VALU ops in this kernel
#define FWD64_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define FWD64_TARGET
#endif

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
// defer-max threshold of attention.hip (8 in the natural-log domain)
constexpr float DEFER_THR2 = 8.f * LOG2E;
constexpr int MASKB = 256;  // one stage's 64 mask values

// wave-uniform "some lane has p"
DEVINL bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// one stage's 64 additive mask values by 4-byte LDS-DMA: lane j of wave 0
// sends key k0 + j (clamped at S-1; a key past the horizon is scored -inf
// whatever its slot holds)
DEVINL void stage_mask(const float* mp, int k0, int S, int lane, char* dst) {
  if (threadIdx.x < WAVE)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(
            mp + min(k0 + lane, S - 1)),
        (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
}

struct FwdRows {
  int key_lim;  // last live key of the lane's q row: horizon and diagonal
  int lane, hi, j32;
  float c2;     // scale * log2 e
};

// N live 32-key sub-tiles [K | V] at `sub` (SUBB apart), first key k0.
// acc = [key-pattern][qrow = lane&31]. MASK: mk holds the stage's additive
// mask. EDGE: the horizon or the wave's diagonal crosses the stage.
template <int N, bool MASK, bool EDGE>
DEVINL void fwd_tiles(const FwdRows& c, const char* sub, const float* mk,
                      int k0, const bf16x8v (&qf)[4], f32x16 (&oacc)[2],
                      float& m_run, float& l_run) {
  // S^T[key][qrow] = K Q^T
  f32x16 s_acc[N];
#pragma unroll
  for (int t = 0; t < N; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s_acc[t][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      s_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          afrag(sub + t * SUBB, c.j32, c.hi, s), qf[s], s_acc[t], 0, 0, 0);
  }
  // log2-domain scores and the stage's row maximum
  float tile_max = -INFINITY;
#pragma unroll
  for (int t = 0; t < N; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float madd[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MASK) {
        const float4 m4 = *reinterpret_cast<const float4*>(
            mk + t * 32 + 8 * i + 4 * c.hi);
        madd[0] = m4.x * LOG2E; madd[1] = m4.y * LOG2E;
        madd[2] = m4.z * LOG2E; madd[3] = m4.w * LOG2E;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * i + e;
        float x = __builtin_fmaf(s_acc[t][r], c.c2, madd[e]);
        if constexpr (EDGE) {
          const int key = k0 + t * 32 + 8 * i + 4 * c.hi + e;
          x = (key > c.key_lim) ? -INFINITY : x;
        }
        s_acc[t][r] = x;
        tile_max = __builtin_fmaxf(tile_max, x);
      }
    }
  }
  // the two lane halves hold the same q row, different keys
  tile_max = __builtin_fmaxf(tile_max, lane_read(tile_max, c.lane ^ 32));
  // defer-max: keep the running max while the stage's max is within the
  // threshold of it (P is then bounded by e^8, which the fp32 accumulator
  // carries); decided before any exponentiation
  float alpha = 1.f;
  if (wave_any(!(tile_max - m_run <= DEFER_THR2))) {
    const float m_new = __builtin_fmaxf(m_run, tile_max);
    if (m_new != m_run) {
      alpha = (m_run == -INFINITY) ? 0.f
                                   : __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
    }
  }
  l_run *= alpha;
  if (wave_any(alpha != 1.f)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a_r = lane_read(alpha, (r & 3) + 8 * (r >> 2) + 4 * c.hi);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) oacc[hh][r] *= a_r;
    }
  }
  // a row whose keys are all dead so far keeps m_run = -inf: exp2(-inf - 0)
  const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
  float psum = 0.f;
#pragma unroll
  for (int t = 0; t < N; ++t) {
    const char* v_lds = sub + t * SUBB + TILEB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __builtin_amdgcn_exp2f(s_acc[t][r] - m_use);
      s_acc[t][r] = p;
      psum += p;
    }
    // O += P V: A = repacked P over k = keys, B[k = key][j = d]
    unsigned int pa[2][4];
    acc_to_afrag<true>(s_acc[t], pa);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
      for (int step = 0; step < 2; ++step) {
        oacc[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_afrag(pa[step]),
            tr16_bfrag(v_lds, c.lane, step * 16 + 8 * c.hi, hh), oacc[hh],
            0, 0, 0);
      }
    }
  }
  l_run += psum + lane_read(psum, c.lane ^ 32);
}

// -------------------------------------------------------------------
// One block = q rows tile*128 .. +127 of one (sequence, head); a wave owns
// 32 of them and loops the sequence's K/V stages up to the horizon.
// qp/kp/vp/op: the sequence's first row of this head (row strides *rs in
// elements); mp: its S mask values (MASK); lsep: its S lse values.
// -------------------------------------------------------------------
template <bool MASK>
DEVINL void fwd64_block(const bf16_t* __restrict__ qp,
                        const bf16_t* __restrict__ kp,
                        const bf16_t* __restrict__ vp,
                        const float* __restrict__ mp,
                        bf16_t* __restrict__ op, float* __restrict__ lsep,
                        int S, int L, int tile, int causal, float scale,
                        long qrs, long krs, long vrs, long ors) {
  // two slots of [K | V][K | V], then the two slots' mask values
  __shared__ __attribute__((aligned(16))) char smem[2 * SLOTB + 2 * MASKB];
  const int lane = threadIdx.x & (WAVE - 1);
  const int hi = lane >> 5;
  const int j32 = lane & 31;
  const int q0 = (tile * 4 + (int)(threadIdx.x / WAVE)) * 32;
  const bool live_wave = q0 < S;

  const int qrow = q0 + j32;
  const bf16_t* qrp = qp + (long)min(qrow, S - 1) * qrs;
  bf16x8v qf[4];
  if (live_wave) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
      qf[s] = *reinterpret_cast<const bf16x8v*>(qrp + s * 16 + hi * 8);
  }
  // block-wide kv range (barriers are block-wide), lowered to the
  // sequence's key horizon; waves guard their own compute
  const int kv_end = min(causal ? min(S, tile * 128 + 128) : S, L);
  FwdRows c;
  c.key_lim = causal ? min(L - 1, qrow) : L - 1;
  c.lane = lane; c.hi = hi; c.j32 = j32;
  c.c2 = scale * LOG2E;

  f32x16 oacc[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[hh][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const StageSrc ss = stage_src();
  if (MASK) stage_mask(mp, 0, S, lane, smem + 2 * SLOTB);
  stage_slot(kp, krs, vp, vrs, 0, kv_end, S, smem, ss);
  for (int k0 = 0; k0 < kv_end; k0 += 64) {
    const int slot = (k0 >> 6) & 1;
    const char* sub = smem + slot * SLOTB;
    const float* mk =
        reinterpret_cast<const float*>(smem + 2 * SLOTB + slot * MASKB);
    // drains this slot's DMA; every wave is past its reads of the other
    block_sync();
    if (k0 + 64 < kv_end) {  // next stage's LDS-DMA under this compute
      if (MASK)
        stage_mask(mp, k0 + 64, S, lane,
                   smem + 2 * SLOTB + (slot ^ 1) * MASKB);
      stage_slot(kp, krs, vp, vrs, k0 + 64, kv_end, S,
                 smem + (slot ^ 1) * SLOTB, ss);
    }
    // causal: keys above the wave's last q row have P == 0; the second
    // sub-tile may lie past the block's kv range (then it is not staged)
    const bool c0 = live_wave && (!causal || k0 <= q0 + 31);
    const bool c1 = c0 && k0 + 32 < kv_end && (!causal || k0 + 32 <= q0 + 31);
    const bool edge = k0 + 64 > L || (causal && k0 + 63 > q0);
    if (c1) {
      if (edge)
        fwd_tiles<2, MASK, true>(c, sub, mk, k0, qf, oacc, m_run, l_run);
      else
        fwd_tiles<2, MASK, false>(c, sub, mk, k0, qf, oacc, m_run, l_run);
    } else if (c0) {
      fwd_tiles<1, MASK, true>(c, sub, mk, k0, qf, oacc, m_run, l_run);
    }
  }
  if (!live_wave) return;

  // O /= l (a row without a live key: l = 0, O = 0, lse = -inf)
  const float l_inv = (l_run > 0.f) ? 1.f / l_run : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row_local = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float li = lane_read(l_inv, row_local);
    const int row = q0 + row_local;
    if (row < S) {
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        op[(long)row * ors + hh * 32 + j32] = f2bf(oacc[hh][r] * li);
    }
  }
  if (qrow < S && hi == 0)
    lsep[qrow] = (l_run > 0.f) ? (m_run + __builtin_amdgcn_logf(l_run)) * LN2
                               : -INFINITY;
}

}  // namespace
