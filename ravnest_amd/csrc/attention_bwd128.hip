// Flash-style fused attention BACKWARD for CDNA4 (gfx950), bf16, D=128.
//
// Same split as attention_bwd.hip (Delta, then dV, dK, dQ as separate
// kernels, no atomics, P recomputed on chip from (Q,K,lse)), rebuilt for
// 256-byte rows:
//
//   attn_bwd128_kv_kernel<false>  dV: wave owns 32 keys, loops Q tiles
//   attn_bwd128_kv_kernel<true>   dK: same loop, S and dP -> dS -> dK
//   attn_bwd128_dq_kernel         dQ: wave owns 32 q rows, loops KV tiles
//
// Work split. A block is 4 waves = 128 keys (or q rows); the wave-owned
// operand (K, K+V, or Q+dO: 8 bf16x8 fragments each) stays in registers
// for the whole loop, the streamed 32-row tiles (Q+dO, or K+V) go through
// LDS, 16 KiB per slot, two slots, filled by global_load_lds (two 16-B
// DMA loads per thread and operand) one tile ahead of the compute (T14).
// dV/dK also keep lse (and Delta) in LDS while S <= 2048, as at D=64.
//
// LDS image. A row is 256 B = 16 chunks of 16 B and every row starts on
// the same bank, so a plain image would put the 32 rows of an A-fragment
// ds_read_b128 on one 16-B bank group. Chunk c of row r is stored at
// chunk c ^ f(r & 15), f(r) = ((r & 3) << 2) | (r >> 2) (the two 2-bit
// halves of r swapped). The XOR stays inside the row (unlike the 128-B
// rows of D=64, where it reaches the row's low bit), so it is its own
// inverse and the DMA applies it on the SOURCE side by a plain column
// XOR: the thread that fills chunk position p of row r reads global
// chunk p ^ f(r & 15).
//  - A fragments: lane (j32, hi) reads chunk 2s+hi of row j32. f is a
//    bijection of 0..15, so any 16 consecutive rows hit 16 different
//    chunk positions = all 64 banks once per 16 lanes: conflict-free.
//  - tr16 B fragments: 32 lanes read rows kb..kb+3 (kb % 4 == 0), 8 lanes
//    each, inside one 64-B column window. With r = 4a + i, f(r) =
//    (i << 2) | a moves row i to 64-B window hh ^ i and permutes the four
//    chunks inside it by a: the 32 8-B reads cover 16 distinct chunks,
//    two halves each = 256 distinct bytes: conflict-free. The D=64
//    swizzle (r & 15) itself would leave all four rows in one 64-B window
//    at this pitch (4-way conflict), hence the swapped halves.
//
// Occupancy (chosen, not inherited). dV: K fragments 32 + accumulators 64
// + S/P 16 fit the 3 waves/SIMD tier (<= 168 VGPRs, 40 KiB LDS). dK and
// dQ hold two resident operands (64) + accumulators (64) + S and dP (32)
// and land near 200 registers: they run at 2 waves/SIMD on purpose. The
// alternatives cost more than the tier: re-reading the resident operand
// from LDS doubles the A-fragment LDS traffic of every tile, and
// splitting the accumulator's D columns over a wave pair doubles the
// S/dP matmuls. A tile at D=128 carries 24 MFMAs between barriers (12 at
// D=64), so two waves per SIMD already overlap one wave's exp/convert
// phase with the other's MFMA phase. launch_bounds hold the compiler to
// those tiers; resource figures are in csrc/README.md.
//
// Fused attention-probability dropout is D=64 only.
#include <torch/extension.h>

#include "attention_bwd_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
// no packed fp32 VALU ops in the new kernels
#define D128_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define D128_TARGET
#endif

namespace {

constexpr int ROWB = 256;          // bytes of one 128 x bf16 row
constexpr int TILEB = 32 * ROWB;   // one 32-row tile, 8 KiB
constexpr int SLOTB = 2 * TILEB;   // two operands per slot

// byte XOR of the LDS image (file header)
DEVINL int swz(int row) {
  const int r = row & 15;
  return (((r & 3) << 2) | (r >> 2)) << 4;
}

// A fragment of k-step s: row j32, elements s*16 + hi*8 .. +7
DEVINL bf16x8v afrag(const char* tile, int j32, int hi, int s) {
  return *reinterpret_cast<const bf16x8v*>(
      tile + j32 * ROWB + (((2 * s + hi) << 4) ^ swz(j32)));
}

// B fragment B[k = kb + 0..7][j = hh*32 + (lane&31)] by two tr16 gathers
// of 4 rows each (8-B reads never cross a 16-B chunk)
DEVINL bf16x8v tr16_bfrag(const char* tile, int lane, int kb, int hh) {
  const int q4 = lane & 15;
  const int col = hh * 64 + ((lane >> 4) & 1) * 32 + 8 * (q4 & 3);
  const int r0 = kb + (q4 >> 2), r1 = r0 + 4;
  bf16x4v lo = DS_TR16(tile + r0 * ROWB + (col ^ swz(r0)));
  bf16x4v h4 = DS_TR16(tile + r1 * ROWB + (col ^ swz(r1)));
  bf16x8v f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[e] = lo[e]; f[e + 4] = h4[e]; }
  return f;
}

// LDS-DMA of one 32-row tile: thread t fills bytes t*16 and 4096 + t*16
// of the image (rows t>>4 and 16 + (t>>4), chunk position t&15) from the
// source chunk the swizzle maps there. Rows past S-1 are clamped.
struct StageSrc { int row, col, wdst; };

DEVINL StageSrc stage_src() {
  const int t = threadIdx.x;
  return {t >> 4, ((t & 15) << 4) ^ swz(t >> 4), (t >> 6) * 1024};
}

DEVINL void stage_tile(const bf16_t* gp, long rs, int t0, int S, char* dst,
                       const StageSrc& ss) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(
            reinterpret_cast<const char*>(gp) +
            (long)min(t0 + i * 16 + ss.row, S - 1) * rs * 2 + ss.col),
        (__attribute__((address_space(3))) void*)(dst + i * 4096 + ss.wdst),
        16, 0, 0);
  }
}

// one slot = two tiles side by side ([Q | dO] or [K | V])
DEVINL void stage_slot(const bf16_t* g0, long rs0, const bf16_t* g1,
                       long rs1, int t0, int S, char* slot,
                       const StageSrc& ss) {
  stage_tile(g0, rs0, t0, S, slot, ss);
  stage_tile(g1, rs1, t0, S, slot + TILEB, ss);
}

// The kernels carry a target attribute, and the HIP headers' plain
// inline functions (which carry none) are then not inlined into them but
// called, with a stack frame. These two are __syncthreads and __shfl
// spelled with the builtins, forced inline.
//
// block_sync also drains the wave's LDS-DMA: a global_load_lds counts in
// vmcnt until its bytes are in LDS, and the fences alone do not make the
// compiler wait for it (the dQ loop compiled to a barrier behind
// lgkmcnt(0) only). The loads were issued a whole tile of compute
// earlier, so the wait is normally already satisfied.
DEVINL void block_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

DEVINL float lane_read(float v, int src_lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src_lane << 2,
                                          __builtin_bit_cast(int, v)));
}

// wave's 32 x 128 accumulator tile -> rows row0.. of gp (ZERO: exact
// zeros for a key block wholly past the horizon, where P == 0)
template <bool ZERO>
DEVINL void store_rows(bf16_t* __restrict__ gp, const f32x16* acc, int row0,
                       int S, long rs, int hi, int j32) {
#pragma unroll
  for (int hh = 0; hh < 4; ++hh) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (row < S)
        gp[(long)row * rs + hh * 32 + j32] = f2bf(ZERO ? 0.f : acc[hh][r]);
    }
  }
}

// -------------------------------------------------------------------
// dV (DK = false) and dK (DK = true): wave owns keys k0..k0+31
// -------------------------------------------------------------------
template <bool DK>
D128_TARGET __global__ __launch_bounds__(256, DK ? 2 : 3)
void attn_bwd128_kv_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ mask, bf16_t* __restrict__ out, int S,
    int causal, float scale, int has_mask, long H, StridesB sio,
    StridesB sdo, StridesB sg, const int* __restrict__ kv_len) {
  // two slots of [Q | dO], then lse (and Delta for dK) rows
  __shared__ __attribute__((aligned(16))) char
      smem[2 * SLOTB + (DK ? 16384 : 8192)];
  float* lse_lds = reinterpret_cast<float*>(smem + 2 * SLOTB);
  float* dlt_lds = lse_lds + 2048;
  const int lane = threadIdx.x & (WAVE - 1);
  const int hi = lane >> 5;
  const int j32 = lane & 31;
  const int k0 = (blockIdx.x * 4 + (int)(threadIdx.x / WAVE)) * 32;
  const bool live_wave = k0 < S;
  const long bh = blockIdx.y;
  const long b = bh / H, h = bh % H;
  const bf16_t* qp = q + b * sio.bs + h * sio.hs;
  const bf16_t* kp = k + b * sio.bs + h * sio.hs;
  const bf16_t* dop = dout + b * sdo.bs + h * sdo.hs;
  bf16_t* outp = out + b * sg.bs + h * sg.hs;
  const float* lsep = lse + bh * (long)S;
  const float* dltp = DK ? delta + bh * (long)S : nullptr;
  const float* mp = has_mask ? (mask + b * (long)S) : nullptr;
  // key horizon: block-uniform exit before the first barrier. In the
  // block that straddles L, a wave whose keys all lie past it skips its
  // compute (k0 < L below) and stores its zero accumulators.
  const int L = kv_horizon(kv_len, b, S);
  if ((int)blockIdx.x * 128 >= L) {
    if (live_wave) store_rows<true>(outp, nullptr, k0, S, sg.rs, hi, j32);
    return;
  }
  const bool lse_in_lds = S <= 2048;
  if (lse_in_lds) {
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
      lse_lds[i] = lsep[i];
      if constexpr (DK) dlt_lds[i] = dltp[i];
    }
  }

  const int key = k0 + j32;
  const long krow = (long)min(key, S - 1) * sio.rs;
  bf16x8v kf[8], vf[DK ? 8 : 1];
  if (live_wave) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      kf[s] = *reinterpret_cast<const bf16x8v*>(kp + krow + s * 16 + hi * 8);
      if constexpr (DK)
        vf[s] = *reinterpret_cast<const bf16x8v*>(
            v + b * sio.bs + h * sio.hs + krow + s * 16 + hi * 8);
    }
  }
  const float mask_val = (has_mask && key < S) ? mp[min(key, S - 1)] : 0.f;

  f32x16 acc[4];
#pragma unroll
  for (int hh = 0; hh < 4; ++hh)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[hh][r] = 0.f;

  const int q_start = causal ? blockIdx.x * 128 : 0;
  const StageSrc ss = stage_src();
  stage_slot(qp, sio.rs, dop, sdo.rs, q_start, S, smem, ss);
  for (int q0 = q_start; q0 < S; q0 += 32) {
    const int slot = ((q0 - q_start) >> 5) & 1;
    const char* q_lds = smem + slot * SLOTB;
    const char* do_lds = q_lds + TILEB;
    // drains this slot's DMA; every wave is past its reads of the other
    block_sync();
    if (q0 + 32 < S)  // T14: next tile's LDS-DMA under this compute
      stage_slot(qp, sio.rs, dop, sdo.rs, q0 + 32, S,
                 smem + (slot ^ 1) * SLOTB, ss);
    const bool compute = live_wave && k0 < L && (!causal || q0 + 31 >= k0);
    if (compute) {
      // S[qrow][key] = Q K^T, dP[qrow][key] = dO V^T
      f32x16 s_acc, dp_acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s_acc[r] = 0.f;
        dp_acc[r] = 0.f;
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            afrag(q_lds, j32, hi, s), kf[s], s_acc, 0, 0, 0);
        if constexpr (DK)
          dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              afrag(do_lds, j32, hi, s), vf[s], dp_acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = q0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const int qclmp = min(qrow, S - 1);
        const float l = lse_in_lds ? lse_lds[qclmp] : lsep[qclmp];
        const float sv = s_acc[r] * scale + mask_val;
        const bool dead = (qrow >= S) || (key >= L) ||
                          (causal && key > qrow) || !isfinite(l);
        const float p = dead ? 0.f : __expf(sv - l);
        if constexpr (DK) {
          const float dlt = lse_in_lds ? dlt_lds[qclmp] : dltp[qclmp];
          s_acc[r] = dead ? 0.f : p * (dp_acc[r] - dlt) * scale;  // dS
        } else {
          s_acc[r] = p;
        }
      }
      // dV += P^T dO, dK += dS^T Q: A = repacked P / dS over k = qrows,
      // B[k = qrow][j = d] gathered from the dO / Q tile
      unsigned int pa[2][4];
      acc_to_afrag(s_acc, pa);
      const char* b_lds = DK ? q_lds : do_lds;
#pragma unroll
      for (int hh = 0; hh < 4; ++hh) {
#pragma unroll
        for (int step = 0; step < 2; ++step) {
          acc[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              *reinterpret_cast<const bf16x8v*>(&pa[step][0]),
              tr16_bfrag(b_lds, lane, step * 16 + 8 * hi, hh), acc[hh],
              0, 0, 0);
        }
      }
    }
  }
  if (live_wave) store_rows<false>(outp, acc, k0, S, sg.rs, hi, j32);
}

// -------------------------------------------------------------------
// dQ: wave owns q rows q0..q0+31, loops KV tiles up to the horizon
// (forward orientation: acc = [key-pattern][qrow = lane&31])
// -------------------------------------------------------------------
D128_TARGET __global__ __launch_bounds__(256, 2)
void attn_bwd128_dq_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ mask, bf16_t* __restrict__ dq, int S,
    int causal, float scale, int has_mask, long H, StridesB sio,
    StridesB sdo, StridesB sg, const int* __restrict__ kv_len) {
  __shared__ __attribute__((aligned(16))) char smem[2 * SLOTB];  // [K | V]
  const int lane = threadIdx.x & (WAVE - 1);
  const int hi = lane >> 5;
  const int j32 = lane & 31;
  const int q0 = (blockIdx.x * 4 + (int)(threadIdx.x / WAVE)) * 32;
  const bool live_wave = q0 < S;
  const long bh = blockIdx.y;
  const long b = bh / H, h = bh % H;
  const bf16_t* kp = k + b * sio.bs + h * sio.hs;
  const bf16_t* vp = v + b * sio.bs + h * sio.hs;
  bf16_t* dqp = dq + b * sg.bs + h * sg.hs;
  const float* mp = has_mask ? (mask + b * (long)S) : nullptr;

  const int qrow = q0 + j32;
  const bf16_t* qrp =
      q + b * sio.bs + h * sio.hs + (long)min(qrow, S - 1) * sio.rs;
  const bf16_t* dorp =
      dout + b * sdo.bs + h * sdo.hs + (long)min(qrow, S - 1) * sdo.rs;
  bf16x8v qf[8], dof[8];
  if (live_wave) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      qf[s] = *reinterpret_cast<const bf16x8v*>(qrp + s * 16 + hi * 8);
      dof[s] = *reinterpret_cast<const bf16x8v*>(dorp + s * 16 + hi * 8);
    }
  }
  const float l_row = (qrow < S) ? lse[bh * (long)S + qrow] : -INFINITY;
  const float dlt_row = (qrow < S) ? delta[bh * (long)S + qrow] : 0.f;

  f32x16 acc[4];
#pragma unroll
  for (int hh = 0; hh < 4; ++hh)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[hh][r] = 0.f;

  // block-wide kv range (barriers are block-wide), lowered to the
  // sequence's key horizon; waves guard their own compute
  const int L = kv_horizon(kv_len, b, S);
  const int kv_end = min(causal ? min(S, (int)blockIdx.x * 128 + 128) : S, L);
  const StageSrc ss = stage_src();
  stage_slot(kp, sio.rs, vp, sio.rs, 0, S, smem, ss);
  for (int k0 = 0; k0 < kv_end; k0 += 32) {
    const int slot = (k0 >> 5) & 1;
    const char* k_lds = smem + slot * SLOTB;
    const char* v_lds = k_lds + TILEB;
    block_sync();
    if (k0 + 32 < kv_end)  // T14: next tile's LDS-DMA under this compute
      stage_slot(kp, sio.rs, vp, sio.rs, k0 + 32, S,
                 smem + (slot ^ 1) * SLOTB, ss);
    const bool compute = live_wave && (!causal || k0 <= q0 + 31);
    if (compute) {
      // S^T[key][qrow] = K Q^T, dP^T[key][qrow] = V dO^T
      f32x16 s_acc, dp_acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s_acc[r] = 0.f;
        dp_acc[r] = 0.f;
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            afrag(k_lds, j32, hi, s), qf[s], s_acc, 0, 0, 0);
        dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            afrag(v_lds, j32, hi, s), dof[s], dp_acc, 0, 0, 0);
      }
      float mload = 0.f;
      if (has_mask) mload = mp[min(k0 + j32, S - 1)];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float sv = s_acc[r] * scale;
        if (has_mask && kk < S) sv += lane_read(mload, kk - k0);
        const bool dead = (qrow >= S) || (kk >= L) ||
                          (causal && kk > qrow) || !isfinite(l_row);
        const float p = dead ? 0.f : __expf(sv - l_row);
        s_acc[r] = dead ? 0.f : p * (dp_acc[r] - dlt_row) * scale;  // dS^T
      }
      // dQ += dS K: A = repacked dS^T over k = keys, B[k = key][j = d]
      unsigned int pa[2][4];
      acc_to_afrag(s_acc, pa);
#pragma unroll
      for (int hh = 0; hh < 4; ++hh) {
#pragma unroll
        for (int step = 0; step < 2; ++step) {
          acc[hh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              *reinterpret_cast<const bf16x8v*>(&pa[step][0]),
              tr16_bfrag(k_lds, lane, step * 16 + 8 * hi, hh), acc[hh],
              0, 0, 0);
        }
      }
    }
  }
  if (live_wave) store_rows<false>(dqp, acc, q0, S, sg.rs, hi, j32);
}

}  // namespace

void attn_bwd_d128_launch(const bf16_t* q, const bf16_t* k, const bf16_t* v,
                          const bf16_t* o, const bf16_t* dout,
                          const float* lse, float* delta, const float* mask,
                          bool causal, float scale, long B, long H, int S,
                          StridesB sio, StridesB sdo, StridesB sg,
                          bf16_t* dq, bf16_t* dk, bf16_t* dv, const int* kvl,
                          hipStream_t stream) {
  const long NR = B * H * (long)S;
  hipLaunchKernelGGL((attn_bwd_delta_kernel<128>),
                     dim3((NR * 16 + 255) / 256), dim3(256), 0, stream, dout,
                     o, delta, S, H, NR, sdo);
  const dim3 block(256), grid((S + 127) / 128, B * H);
  const int c = causal ? 1 : 0, hm = mask ? 1 : 0;
  hipLaunchKernelGGL((attn_bwd128_kv_kernel<false>), grid, block, 0, stream,
                     q, k, (const bf16_t*)nullptr, dout, lse,
                     (const float*)nullptr, mask, dv, S, c, scale, hm, H,
                     sio, sdo, sg, kvl);
  hipLaunchKernelGGL((attn_bwd128_kv_kernel<true>), grid, block, 0, stream,
                     q, k, v, dout, lse, (const float*)delta, mask, dk, S, c,
                     scale, hm, H, sio, sdo, sg, kvl);
  hipLaunchKernelGGL(attn_bwd128_dq_kernel, grid, block, 0, stream, q, k, v,
                     dout, lse, (const float*)delta, mask, dq, S, c, scale,
                     hm, H, sio, sdo, sg, kvl);
}
