// 64-row LDS stages for the D=64 flash attention kernels (backward:
// attention_bwd64.hip, forward: attention_fwd64.hip): the [g0 | g1]
// sub-tile image, its global_load_lds staging, the barrier that drains it
// and the fragment reads.
//
// A sub-tile is two 4 KiB operand tiles side by side, [Q | dO] or [K | V],
// each 32 rows of 128 B in the ((row & 15) << 4) XOR image (conflict-free
// b128 A-fragment reads and tr16 B-fragment gathers). A stage slot is two
// sub-tiles = 16 KiB. The XOR is applied on the source side of the DMA:
// four 16-B loads per thread and stage; rows past S-1 are clamped, a
// sub-tile wholly past the end is not staged.
#pragma once

#include "attention_bwd_common.h"

constexpr int TILEB = 4096;       // 32 rows x 128 B of one operand
constexpr int SUBB = 2 * TILEB;   // sub-tile: two operands side by side
constexpr int SLOTB = 2 * SUBB;   // 64-row stage

// LDS-DMA of one 4 KiB tile: thread t fills bytes t*16 .. +15 of the
// swizzled image, so it reads the source position that the swizzle maps
// there: the closed-form inverse of p ^ (((p >> 7) & 15) << 4).
struct StageSrc { int row, col, wdst; };

DEVINL StageSrc stage_src() {
  const int p16 = (int)threadIdx.x * 16;
  const int inv_r7 = ((p16 >> 7) & 1) ^ ((p16 >> 10) & 1);
  const int p_src = (p16 & ~0xF0) | ((((p16 >> 4) & 1) ^ inv_r7) << 4) |
                    ((((p16 >> 5) & 1) ^ ((p16 >> 8) & 1)) << 5) |
                    ((((p16 >> 6) & 1) ^ ((p16 >> 9) & 1)) << 6) |
                    (inv_r7 << 7);
  return {p_src >> 7, p_src & 127, ((int)threadIdx.x >> 6) * 1024};
}

// one 32-row sub-tile [g0 | g1] starting at row t0, rows clamped at S-1
DEVINL void stage_sub(const bf16_t* g0, long rs0, const bf16_t* g1, long rs1,
                      int t0, int S, char* dst, const StageSrc& ss) {
  const long row = min(t0 + ss.row, S - 1);
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)(
          reinterpret_cast<const char*>(g0) + row * rs0 * 2 + ss.col),
      (__attribute__((address_space(3))) void*)(dst + ss.wdst), 16, 0, 0);
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)(
          reinterpret_cast<const char*>(g1) + row * rs1 * 2 + ss.col),
      (__attribute__((address_space(3))) void*)(dst + TILEB + ss.wdst), 16,
      0, 0);
}

// a 64-row stage; its second sub-tile only if it has a row below `end`
DEVINL void stage_slot(const bf16_t* g0, long rs0, const bf16_t* g1,
                       long rs1, int t0, int end, int S, char* slot,
                       const StageSrc& ss) {
  stage_sub(g0, rs0, g1, rs1, t0, S, slot, ss);
  if (t0 + 32 < end) stage_sub(g0, rs0, g1, rs1, t0 + 32, S, slot + SUBB, ss);
}

// __syncthreads and __shfl spelled with builtins and forced inline: the
// kernels carry a target attribute, which keeps the HIP headers' plain
// inline functions from being inlined into them (attention_bwd128.hip).
// block_sync also drains the wave's LDS-DMA, which counts in vmcnt.
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

// A fragment of k-step s: row j32, elements s*16 + hi*8 .. +7
DEVINL bf16x8v afrag(const char* tile, int j32, int hi, int s) {
  return *reinterpret_cast<const bf16x8v*>(
      tile + ((j32 * 128 + (s * 16 + hi * 8) * 2) ^ ((j32 & 15) << 4)));
}

// B fragment B[k = kb + 0..7][j = hh*32 + (lane&31)] by two tr16 gathers
DEVINL bf16x8v tr16_bfrag(const char* tile, int lane, int kb, int hh) {
  bf16x4v lo = DS_TR16(tile + tr16_b_off<true>(lane, kb, hh));
  bf16x4v h4 = DS_TR16(tile + tr16_b_off<true>(lane, kb + 4, hh));
  bf16x8v f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[e] = lo[e]; f[e + 4] = h4[e]; }
  return f;
}

DEVINL bf16x8v as_afrag(const unsigned int (&pa)[4]) {
  return *reinterpret_cast<const bf16x8v*>(&pa[0]);
}
