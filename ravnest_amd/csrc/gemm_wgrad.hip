// Split-K weight-gradient GEMM for CDNA4 (gfx950):
//   dW[N,K] = dy[M,N]^T @ x[M,K]   (reduction over the huge token dim)
//
// The wgrad is the "skinny TN" case: both operands are stored M-major,
// so the MFMA fragments need 8 consecutive REDUCTION (m) elements per
// lane at a fixed column — a transposed read. Rather than pre-transpose
// 400 MB operands, tiles are staged row-major into LDS and the
// fragments are gathered with ds_read_b64_tr_b16, gfx950's hardware
// transpose-read (semantics verified on-device by attention's
// tr16_probe: per 16-lane group, lane q loads row (q>>2), cols 4*(q&3)
// of a [4][16] window and RECEIVES column q).
//
// v2 staging: global_load_lds into a LINEAR [64][256 B] image whose
// bank conflicts are killed by a column XOR swizzle applied to the
// glds SOURCE address and the tr16 read address (guide rule 21):
//   cb' = cb ^ ((row & 7) << 5)
// A tr16 32-lane group covers 8 rows x 4 8-B col-quads; bank =
// (colwin/4 + 2*(q&3)) ^ (8*(row&7)) — all 32 combinations distinct,
// so the gather is conflict-free with no row padding (v1's padded rows
// + register staging was LDS-write-bound: 8 ds_write_b128 per thread
// per tile at 13 cycles each exceeded the MFMA time).
// Tail blocks (ragged N/K) keep a register-staged masked path writing
// the SAME swizzled image (glds cannot zero out-of-range columns).
//
// Geometry: 256 threads = 4 waves as 2(N) x 2(K); output tile 128x128;
// 16x16x32 bf16 MFMA; each block owns one output tile x one M-slice of
// 64-deep m-tiles, double-buffered (2 x 32 KiB LDS -> 2 blocks/CU, the
// cross-block overlap hides the simple vmcnt(0)-per-tile pipeline).
// SPLITK partial sums land as fp32 atomicAdd into a zeroed workspace.
// (gemm_wgrad_bf16 / _rows: the MLM head and RAVNEST_HAND_GEMM=1. The
// default weight-gradient path is the second kernel of this file,
// gemm_wgrad256_bf16, below.)
//
// Parity: SURVEY.md §2.3 Linear/GEMM row (wgrad).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

#define DS_TR16(p)                                   \
  __builtin_amdgcn_ds_read_tr16_b64_v4bf16(          \
      (__attribute__((address_space(3))) bf16x4v*)(  \
          (__attribute__((address_space(3))) void*)(p)))

namespace {

constexpr int BN = 128, BK = 128, BM = 64;   // tile: n x k x m-depth
constexpr int ROWB = 256;                    // image row bytes (linear)
constexpr int DY_BYTES = BM * ROWB;          // 16 KiB per operand image
constexpr int PAIR_BYTES = 2 * DY_BYTES;
// LDS: [buf 2][dy | x] images = 64 KiB -> 2 blocks/CU
// (a BK=64 / 3-blocks-per-CU variant measured SLOWER: halving BK
// doubles the dy re-reads per FLOP and the kernel goes HBM-bound)

DEVINL int swz(int row, int cb) { return cb ^ ((row & 7) << 5); }

template <bool TAIL>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(
    const bf16_t* __restrict__ DY, const bf16_t* __restrict__ X,
    float* __restrict__ WS, long M, long N, long K, int NT, int KT,
    int splitk, long mTilesPer, const int* __restrict__ mbound) {
  __shared__ char smem[2 * PAIR_BYTES];

  // block -> (output tile, m-slice); slices of one tile stay adjacent
  // so (after the XCD remap) a tile's partials land on one XCD's L2
  const int ntiles = NT * KT;
  const int nwg = ntiles * splitk;
  int bid = blockIdx.x, wg;
  if ((nwg & 7) == 0) {
    wg = (bid & 7) * (nwg >> 3) + (bid >> 3);
  } else {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7, lin = bid >> 3;
    wg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + lin;
  }
  const int tile = wg / splitk, slice = wg % splitk;
  const int bn = tile % NT, bk = tile / NT;
  const long n0 = (long)bn * BN, k0 = (long)bk * BK;
  const bool is_tail = (n0 + BN > N) || (k0 + BK > K);
  if (TAIL != is_tail) return;  // the two specializations split the grid
  // optional device-side bound on the reduction (live rows of a
  // compacted operand): the m-tiles below round_up(*mbound, 64) are
  // re-split evenly over the slices; slices left empty exit. The caller
  // keeps rows [*mbound, round_up) zero in dy and finite in x.
  long mTiles = M / BM;
  if (mbound != nullptr) {
    const long bt = ((long)max(*mbound, 0) + BM - 1) / BM;
    if (bt < mTiles) mTiles = bt;
    mTilesPer = (mTiles + splitk - 1) / splitk;
  }
  const long mt0 = slice * mTilesPer;
  const long mt1 = min(mt0 + mTilesPer, mTiles);
  if (mt0 >= mt1) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wn = wid >> 1, wk = wid & 1;  // 2 x 2 wave grid

  auto img = [&](int b, int op) {
    return smem + b * PAIR_BYTES + op * DY_BYTES;
  };

  // ---- staging ------------------------------------------------------
  // 8 pieces of 16 B per thread cover the 32 KiB image pair. Piece i of
  // wave w lands lane-linear at (i*4 KiB + w*1 KiB + lane*16) — row =
  // off/256, cb = off%256 — and its SOURCE column carries the inverse
  // swizzle. 64-bit source offsets (operands can approach 4 GiB).
  long srcOff[8];          // byte offset into DY/X at m-tile 0
  int dstOff[8];           // byte offset into the image pair
  int shiftv[8], validv[8];  // tail masking (register path only)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int o = i * 4096 + wid * 1024 + lane * 16;
    const int op = o >= DY_BYTES;       // 0 = dy, 1 = x
    const int lo = op ? o - DY_BYTES : o;
    const int row = lo >> 8;
    const int cb = swz(row, lo & 255);
    const long cols = op ? K : N;
    const long cbase = op ? k0 : n0;
    long c = cbase + cb / 2;
    int sh = 0, va = 8;
    if (TAIL && c + 8 > cols) {
      const long cl = max(0l, cols - 8);
      sh = (int)(c - cl);
      va = (int)max(0l, min(8l, cols - c));
      c = cl;
    }
    srcOff[i] = ((long)row * cols + c) * 2;
    dstOff[i] = o;
    shiftv[i] = sh;
    validv[i] = va;
  }
  const long dyStep = (long)BM * N * 2, xStep = (long)BM * K * 2;

  auto stage_glds = [&](long mt, int b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int op = dstOff[i] >= DY_BYTES;
      const char* src = reinterpret_cast<const char*>(op ? X : DY) +
                        srcOff[i] + mt * (op ? xStep : dyStep);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(
              smem + b * PAIR_BYTES + (dstOff[i] - lane * 16)),
          16, 0, 0);
    }
  };

  s16x8 stg[8];
  auto issue_loads = [&](long mt) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int op = dstOff[i] >= DY_BYTES;
      const char* s = reinterpret_cast<const char*>(op ? X : DY) +
                      srcOff[i] + mt * (op ? xStep : dyStep);
      stg[i] = *reinterpret_cast<const s16x8*>(s);
    }
  };
  auto write_stage = [&](int b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s16x8 v = stg[i];
      if (shiftv[i] | (validv[i] ^ 8)) {
        s16x8 w;
        for (int j = 0; j < 8; ++j)
          w[j] = (j < validv[i]) ? v[j + shiftv[i]] : short(0);
        v = w;
      }
      *reinterpret_cast<s16x8*>(smem + b * PAIR_BYTES + dstOff[i]) = v;
    }
  };

  // ---- tr16 fragment addressing (swizzled) -------------------------
  // lane l reads operand[m = mc*32+g*8+r*4+(q>>2)][colwin + 4*(q&3)..]
  const int q4 = lane & 15, g = lane >> 4;
  auto tr_off = [&](int mc, int r, int colwin) {
    const int row = mc * 32 + g * 8 + r * 4 + (q4 >> 2);
    const int cb = (colwin + 4 * (q4 & 3)) * 2;
    return row * ROWB + swz(row, cb);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: stage tile mt0 into buf 0
  if (TAIL) {
    issue_loads(mt0);
    write_stage(0);
    __syncthreads();
  } else {
    stage_glds(mt0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  for (long mt = mt0; mt < mt1; ++mt) {
    const int b = (int)((mt - mt0) & 1);
    if (mt + 1 < mt1) {
      if (TAIL)
        issue_loads(mt + 1);
      else
        stage_glds(mt + 1, b ^ 1);
    }

    // fragments: dyT[nf][mc] from the dy image, x[kf][mc] from x image
    bf16x8v aF[4][2], bF[4][2];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
      for (int mc = 0; mc < 2; ++mc) {
        bf16x4v lo = DS_TR16(img(b, 0) + tr_off(mc, 0, wn * 64 + nf * 16));
        bf16x4v hi = DS_TR16(img(b, 0) + tr_off(mc, 1, wn * 64 + nf * 16));
        bf16x8v f;
        f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
        f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
        aF[nf][mc] = f;
      }
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int mc = 0; mc < 2; ++mc) {
        bf16x4v lo = DS_TR16(img(b, 1) + tr_off(mc, 0, wk * 64 + kf * 16));
        bf16x4v hi = DS_TR16(img(b, 1) + tr_off(mc, 1, wk * 64 + kf * 16));
        bf16x8v f;
        f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
        f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
        bF[kf][mc] = f;
      }

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mc = 0; mc < 2; ++mc)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
          acc[nf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              aF[nf][mc], bF[kf][mc], acc[nf][kf], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);

    if (TAIL) {
      if (mt + 1 < mt1) write_stage(b ^ 1);
      __syncthreads();
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  // ---- epilogue: fp32 atomic accumulation into the workspace -------
  // D layout: row i = n = (lane>>4)*4 + v, col j = k = lane&15
#pragma unroll
  for (int nf = 0; nf < 4; ++nf)
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      const long k = k0 + wk * 64 + kf * 16 + (lane & 15);
      if (k >= K) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long n = n0 + wn * 64 + nf * 16 + ((lane >> 4) << 2) + v;
        if (n < N) atomicAdd(WS + n * K + k, acc[nf][kf][v]);
      }
    }
}

}  // namespace

static at::Tensor launch_wgrad(const at::Tensor& dy, const at::Tensor& x,
                               const int* mbound) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
              dy.is_contiguous() && dy.dim() == 2);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.is_contiguous() && x.dim() == 2);
  const long M = dy.size(0), N = dy.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M, "gemm_wgrad: M mismatch");
  TORCH_CHECK(M % BM == 0 && M >= 2 * BM,
              "gemm_wgrad: M % 64 == 0 and M >= 128 required");
  TORCH_CHECK(N >= 8 && K >= 8);
  // the 16 B staging loads (registers and LDS-DMA) need 4 B aligned rows
  TORCH_CHECK(N % 2 == 0 && K % 2 == 0,
              "gemm_wgrad: N and K must be even");
  auto ws = at::zeros({N, K}, dy.options().dtype(at::kFloat));
  const int NT = (int)((N + BN - 1) / BN), KT = (int)((K + BK - 1) / BK);
  const long mTiles = M / BM;
  const int ntiles = NT * KT;
  // split the reduction so the grid reaches ~3 block-waves (2/CU occ)
  int splitk = (int)std::min<long>(
      mTiles, std::max<long>(1, (1536 + ntiles - 1) / ntiles));
  const long mTilesPer = (mTiles + splitk - 1) / splitk;
  splitk = (int)((mTiles + mTilesPer - 1) / mTilesPer);
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  dim3 grid((unsigned)(ntiles * splitk)), block(256);
  const bool has_tail = (N % BN) || (K % BK);
  hipLaunchKernelGGL((wgrad_kernel<false>), grid, block, 0, stream,
                     reinterpret_cast<const bf16_t*>(dy.data_ptr()),
                     reinterpret_cast<const bf16_t*>(x.data_ptr()),
                     ws.data_ptr<float>(), M, N, K, NT, KT, splitk,
                     mTilesPer, mbound);
  if (has_tail)
    hipLaunchKernelGGL((wgrad_kernel<true>), grid, block, 0, stream,
                       reinterpret_cast<const bf16_t*>(dy.data_ptr()),
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       ws.data_ptr<float>(), M, N, K, NT, KT, splitk,
                       mTilesPer, mbound);
  HIP_CHECK_LAST();
  return ws;
}

at::Tensor gemm_wgrad_bf16(at::Tensor dy, at::Tensor x) {
  return launch_wgrad(dy, x, nullptr);
}

// dW = dy[0:R]^T @ x[0:R] with R = round_up(min(*row_bound, M), 64) read
// ON DEVICE (a captured graph cannot size the grid by it).
at::Tensor gemm_wgrad_bf16_rows(at::Tensor dy, at::Tensor x,
                                at::Tensor row_bound) {
  TORCH_CHECK(row_bound.is_cuda() && row_bound.scalar_type() == at::kInt &&
              row_bound.numel() == 1);
  return launch_wgrad(dy, x, row_bound.data_ptr<int>());
}

// =====================================================================
// 256x256 split-M wgrad (gemm_wgrad256_bf16): the staging, transpose
// reads and swizzle of the kernel above on the tile geometry and the
// counted-vmcnt pipeline of gemm.hip, with a deterministic reduction.
//
// Geometry: 512 threads = 8 waves as 2(N) x 4(K); output tile 256(N) x
// 256(K), each wave owns 128 x 64 = 8 x 4 fragments of 16x16x32 bf16
// MFMA (64 MFMAs per wave per 64-deep M-tile). Operand lanes are swapped
// (mfma(x-frag, dy-frag)), so a lane's 4 accumulator values are 4
// CONSECUTIVE k of one n: the epilogue stores 16 B per fragment.
//
// LDS: the unit of staging is a HALF-TILE, 32 rows of M: 4 pieces of
// [32 rows][256 B] = dy columns 0-127, dy 128-255, x 0-127, x 128-255
// of the output tile, 32 KiB. Four half-tile slots = 128 KiB, one block
// per CU. Rows stay 256 B wide (a 256-column operand is two pieces side
// by side, a wave reads exactly one piece per operand), and every piece
// starts at a multiple of 8 KiB, so the bank argument of the header
// carries over unchanged: bank = (byte offset / 4) % 64 depends on the
// offset within the 256 B row only, the swizzle depends on row & 7 only,
// and a tr16 32-lane group still covers 8 rows x 4 col-quads of one
// piece -> 32 distinct banks.
//
// Pipeline, per half-tile h (frags(h) are in registers when it starts):
//   s_waitcnt lgkmcnt(0)   every LDS read of slot h & 3 has returned
//   s_waitcnt vmcnt(8)     half-tile h+1 has landed; h+2, h+3 in flight
//   s_barrier              ... for every wave
//   stage(h + 4)           into slot h & 3, which nobody reads any more
//   read x frags(h+1); per dy fragment: its 4 MFMAs of h, then read the
//   same fragment of h+1 into the registers just consumed
// so three to four half-tiles (1.5 to 2 M-tiles) of LDS-DMA are in
// flight across the raw barriers, and the fragment reads of one half
// run under the MFMAs of the other. Near the end of the slice nothing
// is staged any more and the count drops to 4, then 0.
//
// Bounds: N % 256 == 0, K % 256 == 0 and M % 64 == 0 are host-checked,
// there is no tail path. A staged address is row mt0*64 + h*32 + r with
// h < 2*(mt1-mt0), r < 32, mt1 <= M/64, column n0 + c (k0 + c) with
// c < 256 and n0 + 256 <= N (k0 + 256 <= K): inside the operand by
// construction, nothing is clamped. Slices are never empty: the host
// takes split <= M/64 and the M-tiles are dealt out evenly (the first
// M/64 % split slices get one more).
//
// Reduction: no atomics. Block (tile, slice) stores its fp32 partial
// tile with plain 16 B stores into WS[slice][N][K]; wgrad256_finalize
// sums the slices in index order and rounds once (bf16, or fp32 as is),
// so the result is a pure function of the inputs.
//
// Bias gradient (DB): db[n] = sum_m dy[m][n] from the dy pieces already
// in LDS. The K-tile blocks of one (N-tile, slice) share the work: block
// bk sums the M-tiles with mt % KT == bk, so no block of the single-wave
// grid carries all of it. Thread t sums column pair t & 127 over rows
// (t >> 7)*8..+7 of each half-tile; partials go to
// DBWS[slice][bk][t >> 7][N] and the finalize kernel folds them in index
// order and rounds once.
// =====================================================================
#if defined(__HIP_DEVICE_COMPILE__)
// no packed fp32 VALU ops in the new kernels
#define W256_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define W256_TARGET
#endif

namespace w256 {

constexpr int TN = 256, TK = 256;          // output tile
constexpr int HM = 32;                     // half-tile depth (rows of M)
constexpr int PIECE = HM * ROWB;           // 8 KiB
constexpr int SLOT = 4 * PIECE;            // 32 KiB: dy0 | dy1 | x0 | x1
constexpr int NSLOT = 4;
constexpr int DBG = 4;                     // row groups of the column sums

#define W256_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// One 16 B-per-lane LDS-DMA load: lane l's 16 B from `gsrc` land at
// wave_base + l*16 (wave_base is wave-uniform and goes through M0).
// Issued as an asm statement, not through the builtin: the compiler
// puts s_waitcnt vmcnt(0) in front of the first tr16 read after a
// builtin LDS-DMA (the tr16 intrinsic carries no alias info, unlike the
// plain LDS loads of gemm.hip), which would drain the pipeline every
// half-tile. The waits below are counted by hand either way.
DEVINL void glds16(const char* gsrc, char* wave_base) {
  const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(
      __UINTPTR_TYPE__)(__attribute__((address_space(3))) char*)wave_base);
  asm volatile(
      "s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
      :
      : "v"(gsrc), "s"(m0v)
      : "memory", "m0");
}

template <bool DB>
W256_TARGET __global__ __launch_bounds__(512) void wgrad256_kernel(
    const bf16_t* __restrict__ DY, const bf16_t* __restrict__ X,
    float* __restrict__ WS, float* __restrict__ DBWS, long M, long N, long K,
    int NT, int KT, int split) {
  __shared__ char smem[NSLOT * SLOT];

  // block -> (output tile, m-slice); slices of one tile stay adjacent
  // under the XCD remap
  const int nwg = NT * KT * split;
  int bid = blockIdx.x, wg;
  if ((nwg & 7) == 0) {
    wg = (bid & 7) * (nwg >> 3) + (bid >> 3);
  } else {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7, lin = bid >> 3;
    wg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + lin;
  }
  const int tile = wg / split, slice = wg % split;
  const int bn = tile % NT, bk = tile / NT;
  const long n0 = (long)bn * TN, k0 = (long)bk * TK;
  // M-tiles dealt evenly: the first `rem` slices get one more
  const int mTiles = (int)(M / 64);
  const int per = mTiles / split, rem = mTiles % split;
  const int mt0 = slice * per + min(slice, rem);
  const int nh = 2 * (per + (slice < rem ? 1 : 0));  // half-tiles, >= 2

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wn = wid >> 2, wk = wid & 3;  // 2 x 4 wave grid

  // ---- staging: piece p of a half-tile is one 16 B glds per thread,
  // lane-linear at wid*1 KiB + lane*16 (row = wid*4 + lane/16), the
  // swizzle on the SOURCE column
  const int srow = wid * 4 + (lane >> 4);
  const int scb = swz(srow, (lane & 15) * 16);
  const char* src[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const long cols = p < 2 ? N : K;
    const long c = (p < 2 ? n0 : k0) + (p & 1) * 128 + scb / 2;
    src[p] = reinterpret_cast<const char*>(p < 2 ? DY : X) +
             (((long)mt0 * 64 + srow) * cols + c) * 2;
  }
  const long dyStep = (long)HM * N * 2, xStep = (long)HM * K * 2;
  auto stage = [&](int h) __attribute__((always_inline)) {
    char* const lb = smem + (h & 3) * SLOT + wid * 1024;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      glds16(src[p] + h * (p < 2 ? dyStep : xStep), lb + p * PIECE);
  };

  // ---- tr16 fragment addressing inside a piece (swizzled): lane reads
  // rows g*8 + r*4 + (q>>2), cols colwin + 4*(q&3).. and receives
  // m = g*8 + r*4 + 0..3 at column colwin + q
  const int q4 = lane & 15, g = lane >> 4;
  auto tr_off = [&](int r, int colwin) __attribute__((always_inline)) {
    const int row = g * 8 + r * 4 + (q4 >> 2);
    return row * ROWB + swz(row, (colwin + 4 * (q4 & 3)) * 2);
  };
  auto frag = [&](const char* piece, int colwin)
                  __attribute__((always_inline)) {
    const bf16x4v lo = DS_TR16(piece + tr_off(0, colwin));
    const bf16x4v hi = DS_TR16(piece + tr_off(1, colwin));
    bf16x8v f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
  };
  auto dy_frag = [&](int h, int nf) __attribute__((always_inline)) {
    return frag(smem + (h & 3) * SLOT + wn * PIECE, nf * 16);
  };
  auto x_frag = [&](int h, int kf) __attribute__((always_inline)) {
    return frag(smem + (h & 3) * SLOT + (2 + (wk >> 1)) * PIECE,
                (wk & 1) * 64 + kf * 16);
  };

  // ---- bias-gradient column sums of half-tile h (DB only)
  float db0 = 0.f, db1 = 0.f;
  const int dpair = tid & 127, drg = tid >> 7;
  auto colsum = [&](int h) __attribute__((always_inline)) {
    if ((mt0 + (h >> 1)) % KT != bk) return;  // block-uniform
    const char* const piece =
        smem + (h & 3) * SLOT + (dpair >> 6) * PIECE;
#pragma unroll
    for (int i = 0; i < HM / DBG; ++i) {
      const int row = drg * (HM / DBG) + i;
      const unsigned v = *reinterpret_cast<const unsigned*>(
          piece + row * ROWB + swz(row, (dpair & 63) * 4));
      db0 += __builtin_bit_cast(float, v << 16);
      db1 += __builtin_bit_cast(float, v & 0xffff0000u);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: up to four half-tiles in flight, half-tile 0 landed
  stage(0);
  stage(1);
  if (nh >= 4) {
    stage(2);
    stage(3);
    W256_VMCNT(12);
  } else {
    W256_VMCNT(4);
  }
  __builtin_amdgcn_s_barrier();
  bf16x8v dyF[8], xA[4], xB[4];
#pragma unroll
  for (int kf = 0; kf < 4; ++kf) xA[kf] = x_frag(0, kf);
#pragma unroll
  for (int nf = 0; nf < 8; ++nf) dyF[nf] = dy_frag(0, nf);
  if (DB) colsum(0);

  // one half-tile: MFMAs of h on (xc, dyF) while frags(h+1) are read
  // into (xn, dyF). Past the last half-tile the reads fetch stale LDS
  // that nothing uses.
  auto phase = [&](int h, bf16x8v (&xc)[4], bf16x8v (&xn)[4])
                   __attribute__((always_inline)) {
    const int left = nh - 1 - h;  // half-tiles after h
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (left >= 3) {
      W256_VMCNT(8);
    } else if (left == 2) {
      W256_VMCNT(4);
    } else {
      W256_VMCNT(0);
    }
    __builtin_amdgcn_s_barrier();
    if (h + 4 < nh) stage(h + 4);
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) xn[kf] = x_frag(h + 1, kf);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nf = 0; nf < 8; ++nf) {
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
        acc[nf][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            xc[kf], dyF[nf], acc[nf][kf], 0, 0, 0);
      dyF[nf] = dy_frag(h + 1, nf);
    }
    __builtin_amdgcn_s_setprio(0);
    if (DB && left >= 1) colsum(h + 1);
  };
  for (int h = 0; h < nh; h += 2) {
    phase(h, xA, xB);
    phase(h + 1, xB, xA);
  }

  // ---- epilogue: plain fp32 stores of the partial tile. D layout with
  // swapped operands: k = (lane>>4)*4 + v, n = lane & 15.
  float* const ws = WS + (long)slice * N * K;
#pragma unroll
  for (int nf = 0; nf < 8; ++nf) {
    const long n = n0 + wn * 128 + nf * 16 + (lane & 15);
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      const long k = k0 + wk * 64 + kf * 16 + ((lane >> 4) << 2);
      *reinterpret_cast<f32x4*>(ws + n * K + k) = acc[nf][kf];
    }
  }
  if (DB) {
    float* const d =
        DBWS + (((long)slice * KT + bk) * DBG + drg) * N + n0 + 2 * dpair;
    d[0] = db0;
    d[1] = db1;
  }
}

// dW[i..i+3] = sum over slices (index order) of WS[s][i..i+3], rounded
// once; the blocks past nblkW fold the bias-gradient partials.
template <bool OUT_BF16>
W256_TARGET __global__ __launch_bounds__(256) void wgrad256_finalize(
    const float* __restrict__ WS, void* __restrict__ DW, long NK, int split,
    const float* __restrict__ DBWS, bf16_t* __restrict__ DBO, long N,
    int nparts, int nblkW) {
  if ((int)blockIdx.x < nblkW) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= NK) return;
    f32x4 s = *reinterpret_cast<const f32x4*>(WS + i);
    for (int p = 1; p < split; ++p) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(WS + p * NK + i);
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    if (OUT_BF16) {
      typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<u16x4*>(reinterpret_cast<bf16_t*>(DW) + i) =
          u16x4{f2us(s[0]), f2us(s[1]), f2us(s[2]), f2us(s[3])};
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(DW) + i) = s;
    }
  } else {
    const long n = ((long)blockIdx.x - nblkW) * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += DBWS[p * N + n];
    DBO[n] = f2bf(s);
  }
}

}  // namespace w256

// dW[N,K] = dy[M,N]^T @ x[M,K] on the 256x256 template, bf16 (or fp32)
// out, plus db[N] = dy.sum(0) in bf16 when want_db. Deterministic.
std::vector<at::Tensor> gemm_wgrad256_bf16(at::Tensor dy, at::Tensor x,
                                           bool want_db, bool out_fp32) {
  using namespace w256;
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
              dy.is_contiguous() && dy.dim() == 2);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
              x.is_contiguous() && x.dim() == 2);
  const long M = dy.size(0), N = dy.size(1), K = x.size(1);
  TORCH_CHECK(x.size(0) == M, "gemm_wgrad256: M mismatch");
  TORCH_CHECK(M % 64 == 0 && M >= 128,
              "gemm_wgrad256: M % 64 == 0 and M >= 128 required");
  TORCH_CHECK(N > 0 && K > 0 && N % TN == 0 && K % TK == 0,
              "gemm_wgrad256: N % 256 == 0 and K % 256 == 0 required");
  const int NT = (int)(N / TN), KT = (int)(K / TK);
  const long mTiles = M / 64;
  const long ntiles = (long)NT * KT;
  TORCH_CHECK(ntiles < (1 << 20), "gemm_wgrad256: output too large");
  // one block per CU in a single wave of blocks; never an empty slice
  const int split =
      (int)std::min<long>(mTiles, std::max<long>(1, 256 / ntiles));
  const int nparts = split * KT * DBG;
  const long NK = N * K;
  auto ws = at::empty({split * NK + (want_db ? nparts * N : 0)},
                      dy.options().dtype(at::kFloat));
  auto dw = at::empty({N, K},
                      dy.options().dtype(out_fp32 ? at::kFloat
                                                  : at::kBFloat16));
  at::Tensor db;
  if (want_db) db = at::empty({N}, dy.options());
  float* const wsp = ws.data_ptr<float>();
  float* const dbws = want_db ? wsp + split * NK : nullptr;
  auto* dyp = reinterpret_cast<const bf16_t*>(dy.data_ptr());
  auto* xp = reinterpret_cast<const bf16_t*>(x.data_ptr());
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  dim3 grid((unsigned)(ntiles * split)), block(512);
  if (want_db)
    hipLaunchKernelGGL((wgrad256_kernel<true>), grid, block, 0, stream, dyp,
                       xp, wsp, dbws, M, N, K, NT, KT, split);
  else
    hipLaunchKernelGGL((wgrad256_kernel<false>), grid, block, 0, stream,
                       dyp, xp, wsp, dbws, M, N, K, NT, KT, split);
  HIP_CHECK_LAST();
  const int nblkW = (int)((NK / 4 + 255) / 256);
  const int nblkB = want_db ? (int)((N + 255) / 256) : 0;
  dim3 fgrid((unsigned)(nblkW + nblkB)), fblock(256);
  auto* dbo = want_db ? reinterpret_cast<bf16_t*>(db.data_ptr()) : nullptr;
  if (out_fp32)
    hipLaunchKernelGGL((wgrad256_finalize<false>), fgrid, fblock, 0, stream,
                       wsp, dw.data_ptr(), NK, split, dbws, dbo, N, nparts,
                       nblkW);
  else
    hipLaunchKernelGGL((wgrad256_finalize<true>), fgrid, fblock, 0, stream,
                       wsp, dw.data_ptr(), NK, split, dbws, dbo, N, nparts,
                       nblkW);
  HIP_CHECK_LAST();
  if (want_db) return {dw, db};
  return {dw};
}
