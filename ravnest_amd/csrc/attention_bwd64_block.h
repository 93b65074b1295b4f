// The block bodies of the D=64 backward on 64-row stages, shared by the
// dense grid (attention_bwd64.hip: one block per 128 rows of a (B, S)
// batch) and the packed one (attention_varlen64.hip: one block per
// tile-table entry of a token stream). A caller hands them one sequence:
// base pointers of its first row, its length S, its key horizon L and the
// block's 128-row tile. The design notes are in attention_bwd64.hip.
#pragma once

#include "attention_stage64.h"

#if defined(__HIP_DEVICE_COMPILE__)
// no packed fp32 VALU ops in these kernels
#define BWD64_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define BWD64_TARGET
#endif

namespace {

// wave's 32 x 64 accumulator tile -> rows row0.. of gp (ZERO: exact zeros
// for a key block wholly past the horizon, where P == 0)
template <bool ZERO>
DEVINL void store_rows(bf16_t* __restrict__ gp, const f32x16* acc, int row0,
                       int S, long rs, int hi, int j32) {
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (row < S)
        gp[(long)row * rs + hh * 32 + j32] = f2bf(ZERO ? 0.f : acc[hh][r]);
    }
  }
}

// what the softmax phase of a key-owning wave needs
struct KvRows {
  const float *lse_lds, *dlt_lds;   // read while S <= 2048 (IN_LDS),
  const float *lsep, *dltp;         // else the global rows
  int S, L, causal, key, lane, hi, j32;
  float scale, mask_val;
};

// N live 32-row sub-tiles [Q | dO] at `sub` (SUBB apart), first q row q0
template <int N, bool IN_LDS>
DEVINL void kv_tiles(const KvRows& c, const char* sub, int q0,
                     const bf16x8v (&kf)[4], const bf16x8v (&vf)[4],
                     f32x16 (&dv_acc)[2], f32x16 (&dk_acc)[2]) {
  // S[qrow][key] = Q K^T, dP[qrow][key] = dO V^T
  f32x16 s_acc[N], dp_acc[N];
#pragma unroll
  for (int t = 0; t < N; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s_acc[t][r] = 0.f;
      dp_acc[t][r] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      s_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          afrag(sub + t * SUBB, c.j32, c.hi, s), kf[s], s_acc[t], 0, 0, 0);
      dp_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          afrag(sub + t * SUBB + TILEB, c.j32, c.hi, s), vf[s], dp_acc[t],
          0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < N; ++t) {
    const char* q_lds = sub + t * SUBB;
    const char* do_lds = q_lds + TILEB;
    // An accumulator's rows come in runs of four: lse and Delta of a run
    // are one b128 read each from the LDS copy, issued ahead of the run's
    // exps (a run that starts past S holds only dead rows; min keeps its
    // read inside the 2048 staged floats).
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r0 = q0 + t * 32 + 8 * i + 4 * c.hi;
      float lrow[4], drow[4];
      if constexpr (IN_LDS) {
        const int g = min(r0, 2044);
        const float4 l4 = *reinterpret_cast<const float4*>(c.lse_lds + g);
        const float4 d4 = *reinterpret_cast<const float4*>(c.dlt_lds + g);
        lrow[0] = l4.x; lrow[1] = l4.y; lrow[2] = l4.z; lrow[3] = l4.w;
        drow[0] = d4.x; drow[1] = d4.y; drow[2] = d4.z; drow[3] = d4.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lrow[e] = c.lsep[min(r0 + e, c.S - 1)];
          drow[e] = c.dltp[min(r0 + e, c.S - 1)];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * i + e;
        const int qrow = r0 + e;
        const float l = lrow[e];
        const float sv = s_acc[t][r] * c.scale + c.mask_val;
        const bool dead = (qrow >= c.S) || (c.key >= c.L) ||
                          (c.causal && c.key > qrow) || !isfinite(l);
        // computed for every element and then selected: straight-line
        // code, which the scheduler can lay under the MFMAs
        const float ex = __expf(sv - l);
        const float ds = ex * (dp_acc[t][r] - drow[e]) * c.scale;
        s_acc[t][r] = dead ? 0.f : ex;    // P
        dp_acc[t][r] = dead ? 0.f : ds;   // dS
      }
    }
    // dV += P^T dO, dK += dS^T Q: A = repacked P / dS over k = qrows,
    // B[k = qrow][j = d] gathered from the dO / Q tile
    unsigned int pa_p[2][4], pa_ds[2][4];
    acc_to_afrag(s_acc[t], pa_p);
    acc_to_afrag(dp_acc[t], pa_ds);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
      for (int step = 0; step < 2; ++step) {
        const int kb = step * 16 + 8 * c.hi;
        dv_acc[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_afrag(pa_p[step]), tr16_bfrag(do_lds, c.lane, kb, hh),
            dv_acc[hh], 0, 0, 0);
        dk_acc[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_afrag(pa_ds[step]), tr16_bfrag(q_lds, c.lane, kb, hh),
            dk_acc[hh], 0, 0, 0);
      }
    }
  }
}

// one stage at `sub`, q rows q0..q0+63, for the wave's keys k0..k0+31.
// causal: a sub-tile whose last q row is above the wave's first key has
// P == 0; the second sub-tile may lie past S (then it is not staged).
template <bool IN_LDS>
DEVINL void kv_stage(const KvRows& c, const char* sub, int q0, int k0,
                     const bf16x8v (&kf)[4], const bf16x8v (&vf)[4],
                     f32x16 (&dv_acc)[2], f32x16 (&dk_acc)[2]) {
  const bool c0 = !c.causal || q0 + 31 >= k0;
  const bool c1 = q0 + 32 < c.S && (!c.causal || q0 + 63 >= k0);
  // the pair is issued together only on the LDS-row path: above S = 2048
  // the rows' global loads would add their registers to the pair's
  if (IN_LDS && c0 && c1) {
    kv_tiles<2, IN_LDS>(c, sub, q0, kf, vf, dv_acc, dk_acc);
  } else {
    if (c0) kv_tiles<1, IN_LDS>(c, sub, q0, kf, vf, dv_acc, dk_acc);
    if (c1)
      kv_tiles<1, IN_LDS>(c, sub + SUBB, q0 + 32, kf, vf, dv_acc, dk_acc);
  }
}

// -------------------------------------------------------------------
// dK and dV of keys tile*128 .. +127 of one (sequence, head); a wave owns
// 32 of them. qp/kp/vp (row stride rs_io), dop (rs_do), dkp/dvp (rs_g):
// the sequence's first row of this head; lsep, dltp: its S lse and Delta
// values; mp: its S mask values (has_mask).
// -------------------------------------------------------------------
DEVINL void bwd64_kv_block(const bf16_t* __restrict__ qp,
                           const bf16_t* __restrict__ kp,
                           const bf16_t* __restrict__ vp,
                           const bf16_t* __restrict__ dop,
                           const float* __restrict__ lsep,
                           const float* __restrict__ dltp,
                           const float* __restrict__ mp,
                           bf16_t* __restrict__ dkp,
                           bf16_t* __restrict__ dvp, int S, int L, int tile,
                           int causal, float scale, int has_mask, long rs_io,
                           long rs_do, long rs_g) {
  // two slots of [Q | dO][Q | dO], then lse and Delta rows
  __shared__ __attribute__((aligned(16))) char smem[2 * SLOTB + 16384];
  float* lse_lds = reinterpret_cast<float*>(smem + 2 * SLOTB);
  float* dlt_lds = lse_lds + 2048;
  const int lane = threadIdx.x & (WAVE - 1);
  const int hi = lane >> 5;
  const int j32 = lane & 31;
  const int k0 = (tile * 4 + (int)(threadIdx.x / WAVE)) * 32;
  const bool live_wave = k0 < S;
  // key horizon: block-uniform exit before the first barrier. In the
  // block that straddles L, a wave whose keys all lie past it skips its
  // compute (k0 < L below) and stores its zero accumulators.
  if (tile * 128 >= L) {
    if (live_wave) {
      store_rows<true>(dkp, nullptr, k0, S, rs_g, hi, j32);
      store_rows<true>(dvp, nullptr, k0, S, rs_g, hi, j32);
    }
    return;
  }
  const bool lse_in_lds = S <= 2048;
  if (lse_in_lds) {
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
      lse_lds[i] = lsep[i];
      dlt_lds[i] = dltp[i];
    }
  }

  const int key = k0 + j32;
  const long krow = (long)min(key, S - 1) * rs_io;
  bf16x8v kf[4], vf[4];
  if (live_wave) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kf[s] = *reinterpret_cast<const bf16x8v*>(kp + krow + s * 16 + hi * 8);
      vf[s] = *reinterpret_cast<const bf16x8v*>(vp + krow + s * 16 + hi * 8);
    }
  }
  KvRows c;
  c.lse_lds = lse_lds; c.dlt_lds = dlt_lds;
  c.lsep = lsep; c.dltp = dltp;
  c.S = S; c.L = L; c.causal = causal; c.key = key;
  c.lane = lane; c.hi = hi; c.j32 = j32;
  c.scale = scale;
  c.mask_val = (has_mask && key < S) ? mp[min(key, S - 1)] : 0.f;

  f32x16 dv_acc[2], dk_acc[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dv_acc[hh][r] = 0.f;
      dk_acc[hh][r] = 0.f;
    }

  const int q_start = causal ? tile * 128 : 0;
  const StageSrc ss = stage_src();
  stage_slot(qp, rs_io, dop, rs_do, q_start, S, S, smem, ss);
  for (int q0 = q_start; q0 < S; q0 += 64) {
    const int slot = ((q0 - q_start) >> 6) & 1;
    const char* sub = smem + slot * SLOTB;
    // drains this slot's DMA; every wave is past its reads of the other
    block_sync();
    if (q0 + 64 < S)  // next stage's LDS-DMA under this compute
      stage_slot(qp, rs_io, dop, rs_do, q0 + 64, S, S,
                 smem + (slot ^ 1) * SLOTB, ss);
    if (live_wave && k0 < L) {
      if (lse_in_lds)
        kv_stage<true>(c, sub, q0, k0, kf, vf, dv_acc, dk_acc);
      else
        kv_stage<false>(c, sub, q0, k0, kf, vf, dv_acc, dk_acc);
    }
  }
  if (!live_wave) return;
  store_rows<false>(dkp, dk_acc, k0, S, rs_g, hi, j32);
  store_rows<false>(dvp, dv_acc, k0, S, rs_g, hi, j32);
}

// what the softmax phase of a row-owning wave needs
struct DqRows {
  int S, L, causal, qrow, lane, hi, j32;
  float scale, l_row, dlt_row;
};

// N live 32-key sub-tiles [K | V] at `sub` (SUBB apart), first key k0
// (forward orientation: acc = [key-pattern][qrow = lane&31]). MASK: lane j
// holds in mk[t] the additive mask of key k0 + 32 t + j.
template <int N, bool MASK>
DEVINL void dq_tiles(const DqRows& c, const char* sub, int k0,
                     const float* mk, const bf16x8v (&qf)[4], const bf16x8v (&dof)[4],
                     f32x16 (&dq_acc)[2]) {
  // S^T[key][qrow] = K Q^T, dP^T[key][qrow] = V dO^T
  f32x16 s_acc[N], dp_acc[N];
#pragma unroll
  for (int t = 0; t < N; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s_acc[t][r] = 0.f;
      dp_acc[t][r] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      s_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          afrag(sub + t * SUBB, c.j32, c.hi, s), qf[s], s_acc[t], 0, 0, 0);
      dp_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          afrag(sub + t * SUBB + TILEB, c.j32, c.hi, s), dof[s], dp_acc[t],
          0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < N; ++t) {
    const char* k_lds = sub + t * SUBB;
    const int kt = k0 + t * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = kt + (r & 3) + 8 * (r >> 2) + 4 * c.hi;
      float sv = s_acc[t][r] * c.scale;
      if constexpr (MASK) sv += lane_read(mk[t], kk - kt);
      const bool dead = (c.qrow >= c.S) || (kk >= c.L) ||
                        (c.causal && kk > c.qrow) || !isfinite(c.l_row);
      // computed for every element, then selected (straight-line code)
      const float ds =
          __expf(sv - c.l_row) * (dp_acc[t][r] - c.dlt_row) * c.scale;
      dp_acc[t][r] = dead ? 0.f : ds;   // dS^T
    }
    // dQ += dS K: A = repacked dS^T over k = keys, B[k = key][j = d]
    unsigned int pa[2][4];
    acc_to_afrag(dp_acc[t], pa);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
      for (int step = 0; step < 2; ++step) {
        dq_acc[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_afrag(pa[step]),
            tr16_bfrag(k_lds, c.lane, step * 16 + 8 * c.hi, hh), dq_acc[hh],
            0, 0, 0);
      }
    }
  }
}

// one stage at `sub`, keys k0..k0+63, for the wave's q rows q0..q0+31.
// causal: keys above the wave's last q row have P == 0; the second
// sub-tile may lie past the block's kv range (then it is not staged).
template <bool MASK>
DEVINL void dq_stage(const DqRows& c, const char* sub, int k0, int q0,
                     int kv_end, const float (&mk)[2],
                     const bf16x8v (&qf)[4], const bf16x8v (&dof)[4],
                     f32x16 (&dq_acc)[2]) {
  const bool c0 = !c.causal || k0 <= q0 + 31;
  const bool c1 = k0 + 32 < kv_end && (!c.causal || k0 + 32 <= q0 + 31);
  if (c0 && c1)
    dq_tiles<2, MASK>(c, sub, k0, mk, qf, dof, dq_acc);
  else if (c0)
    dq_tiles<1, MASK>(c, sub, k0, mk, qf, dof, dq_acc);
  else if (c1)
    dq_tiles<1, MASK>(c, sub + SUBB, k0 + 32, mk + 1, qf, dof, dq_acc);
}

// -------------------------------------------------------------------
// dQ of q rows tile*128 .. +127 of one (sequence, head); a wave owns 32 of
// them and loops the sequence's K/V stages up to the horizon. Pointers as
// in bwd64_kv_block; dqp: the sequence's first dQ row of this head.
// DELTA: the rows' Delta = rowsum(dO * O) is not read from dltp but
// computed here, from the dO fragments the wave holds anyway and one read
// of its O rows (op, row stride rs_do, in the fragment layout), and stored
// to dlt_out for the kv kernel, which then has to run after this one.
// -------------------------------------------------------------------
template <bool DELTA = false>
DEVINL void bwd64_dq_block(const bf16_t* __restrict__ qp,
                           const bf16_t* __restrict__ kp,
                           const bf16_t* __restrict__ vp,
                           const bf16_t* __restrict__ dop,
                           const float* __restrict__ lsep,
                           const float* __restrict__ dltp,
                           const float* __restrict__ mp,
                           bf16_t* __restrict__ dqp, int S, int L, int tile,
                           int causal, float scale, int has_mask, long rs_io,
                           long rs_do, long rs_g,
                           const bf16_t* __restrict__ op = nullptr,
                           float* __restrict__ dlt_out = nullptr) {
  __shared__ __attribute__((aligned(16))) char smem[2 * SLOTB];  // [K | V] x2
  const int lane = threadIdx.x & (WAVE - 1);
  const int hi = lane >> 5;
  const int j32 = lane & 31;
  const int q0 = (tile * 4 + (int)(threadIdx.x / WAVE)) * 32;
  const bool live_wave = q0 < S;

  const int qrow = q0 + j32;
  const bf16_t* qrp = qp + (long)min(qrow, S - 1) * rs_io;
  const bf16_t* dorp = dop + (long)min(qrow, S - 1) * rs_do;
  bf16x8v qf[4], dof[4];
  if (live_wave) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[s] = *reinterpret_cast<const bf16x8v*>(qrp + s * 16 + hi * 8);
      dof[s] = *reinterpret_cast<const bf16x8v*>(dorp + s * 16 + hi * 8);
    }
  }
  // block-wide kv range (barriers are block-wide), lowered to the
  // sequence's key horizon; waves guard their own compute
  const int kv_end = min(causal ? min(S, tile * 128 + 128) : S, L);
  DqRows c;
  c.S = S; c.L = L; c.causal = causal; c.qrow = qrow;
  c.lane = lane; c.hi = hi; c.j32 = j32;
  c.scale = scale;
  c.l_row = (qrow < S) ? lsep[qrow] : -INFINITY;
  if constexpr (DELTA) {
    // the lane's 32 columns of its row in fp32, then the other half's lane
    float dlt = 0.f;
    if (qrow < S) {
      const bf16_t* orp = op + (long)qrow * rs_do;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8v of =
            *reinterpret_cast<const bf16x8v*>(orp + s * 16 + hi * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dlt += (float)dof[s][j] * (float)of[j];
      }
    }
    dlt += __shfl_xor(dlt, 32, WAVE);
    if (hi == 0 && qrow < S) dlt_out[qrow] = dlt;
    c.dlt_row = dlt;
  } else {
    c.dlt_row = (qrow < S) ? dltp[qrow] : 0.f;
  }

  f32x16 dq_acc[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[hh][r] = 0.f;

  // the stage's mask values are loaded one stage ahead and ahead of the
  // DMA, so that waiting for them never waits for the DMA behind them
  float mk[2] = {0.f, 0.f}, mk_next[2] = {0.f, 0.f};
  if (has_mask) {
    mk[0] = mp[min(j32, S - 1)];
    mk[1] = mp[min(32 + j32, S - 1)];
  }
  const StageSrc ss = stage_src();
  stage_slot(kp, rs_io, vp, rs_io, 0, kv_end, S, smem, ss);
  for (int k0 = 0; k0 < kv_end; k0 += 64) {
    const int slot = (k0 >> 6) & 1;
    const char* sub = smem + slot * SLOTB;
    block_sync();
    if (k0 + 64 < kv_end) {  // next stage's LDS-DMA under this compute
      if (has_mask) {
        mk_next[0] = mp[min(k0 + 64 + j32, S - 1)];
        mk_next[1] = mp[min(k0 + 96 + j32, S - 1)];
      }
      stage_slot(kp, rs_io, vp, rs_io, k0 + 64, kv_end, S,
                 smem + (slot ^ 1) * SLOTB, ss);
    }
    if (live_wave) {
      if (has_mask)
        dq_stage<true>(c, sub, k0, q0, kv_end, mk, qf, dof, dq_acc);
      else
        dq_stage<false>(c, sub, k0, q0, kv_end, mk, qf, dof, dq_acc);
    }
    mk[0] = mk_next[0];
    mk[1] = mk_next[1];
  }
  if (live_wave) store_rows<false>(dqp, dq_acc, q0, S, rs_g, hi, j32);
}

}  // namespace
