// Decode attention for CDNA4 (gfx950): ONE new query per head against a
// key/value cache, bf16, D = 64 or 128. Split-KV ("flash-decoding").
//
//   attn_decode_kernel<D>          grid (n_split, B*H), 256 threads
//   attn_decode_combine_kernel<D>  grid (B*H), D threads (n_split > 1 only)
//
// Bound. Per cached key the step moves 4*D bytes (K and V rows) for 4*D
// flops, so it is limited by streaming the cache from HBM; one query row
// would fill 1/32 of a 32x32 MFMA tile. No matrix instructions: fp32
// vector FMA, and the design is about keeping loads in flight.
//
// Work split. Split s of head (b,h) owns keys [s*chunk, (s+1)*chunk),
// chunk a multiple of 64 chosen on the host from B*H and max_len alone;
// the host never reads cache_len. With L = cache_len[b] the live keys are
// rows [0, L]: L cached rows plus the new token. A block whose chunk starts
// past L writes a neutral partial (m = -inf, l = 0, o = 0) and leaves
// without touching the cache. Deviation from "max_len is a hard bound":
// the LAST split runs on to row L instead of stopping at its chunk end, so
// a max_len below L+1 costs load balance, not correctness, and the new
// row always finds an owner.
//
// Data movement. A D-wide row is 16 B per lane on LPR = D/8 lanes (8 or
// 16), so a wave load instruction fetches RPW = 64/LPR consecutive rows =
// 1 KiB of consecutive cache. A block walks its chunk in 64-key tiles;
// wave w takes keys 16w..16w+15 of the tile in NI = 16/RPW loads of K and
// NI of V per lane. The next tile's 2*NI loads are issued before the
// current tile's scores, so 4*NI KiB per wave stay in flight. q (times
// scale, fp32) and each lane's 8 output dims live in registers. The dot
// product is finished by __shfl_xor inside the lane group.
//
// Softmax. Deviation from "online softmax per wave": every lane GROUP
// keeps its own running (m, l, o[8]) in fp32 over the keys it owns, which
// needs no cross-group max per tile; p is never rounded. At the end of the
// chunk the groups of a wave merge by __shfl_xor, then the four waves
// merge through LDS (4 x (D + 2) floats, the only LDS use).
//
// New token. Its K and V come from qkv_new (B,3,H,D) in registers. The one
// lane group whose key index equals L scores them from registers and
// stores them to row L of the caches with ordinary 16-byte vector stores;
// no block reads row L from the cache, so blocks need no ordering. The
// store is guarded: L outside [0, S_max) stores nothing, and the compute
// clamps L into range so every load stays inside the cache (the output
// row of such a sequence is unspecified). Rows past L are never loaded.
//
// Partials. fp32 (B*H, n_split, D + 2) = o[D], m, l, plain stores; the
// combine kernel folds the splits of a head in index order (log-sum-exp
// algebra, no atomics: bitwise reproducible). n_split == 1 writes bf16 o
// directly and skips the combine launch.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   attn_decode_kernel<64>   74 VGPR, 0 scratch, 1056 B LDS, 6 waves/SIMD
//   attn_decode_kernel<128> 106 VGPR, 0 scratch, 2080 B LDS, 4 waves/SIMD
//   attn_decode_combine_*     8 VGPR, 0 scratch,    0 B LDS, 8 waves/SIMD
// Measured (profiles/attn_decode.txt): 4.28 TB/s over the live cache at
// B=32 H=12 D=64 L=1023, 3.81 TB/s at B=32 H=16 D=128; calls under
// ~15 us measure the host enqueue, not the kernel.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

#if defined(__HIP_DEVICE_COMPILE__)
// no packed fp32 VALU ops in these kernels
#define DECODE_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define DECODE_TARGET
#endif

namespace {

constexpr int DEC_TILE = 64;     // keys per block and loop step
constexpr int DEC_WKEYS = 16;    // keys per wave and loop step
constexpr int DEC_THREADS = 256;

// 16 bytes of row kidx: from the cache below L, the new token at L, and
// zeros (never a load) for a key this block does not own.
template <int D>
DEVINL bf16x8 dec_row(const bf16_t* __restrict__ base, int kidx, int L,
                      int kend, int c, bf16x8 fresh) {
  bf16x8 r = {};
  if (kidx < kend) {
    if (kidx < L)
      r = *reinterpret_cast<const bf16x8*>(base + (long)kidx * D + c * 8);
    else
      r = fresh;  // kend <= L + 1, so kidx == L
  }
  return r;
}

// (m, l, o) <- merge of (m, l, o) and (m2, l2, o2); m = -inf means empty
DEVINL void lse_weights(float m, float m2, float& mn, float& a, float& b) {
  mn = fmaxf(m, m2);
  const float ms = (mn == -INFINITY) ? 0.f : mn;
  a = __expf(m - ms);
  b = __expf(m2 - ms);
}

template <int D>
DECODE_TARGET __global__ __launch_bounds__(DEC_THREADS) void
attn_decode_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                   bf16_t* __restrict__ vc, const int* __restrict__ cache_len,
                   float* __restrict__ ws, bf16_t* __restrict__ out, int H,
                   int S_max, int chunk, int n_split, float scale) {
  constexpr int LPR = D / 8;           // lanes per row
  constexpr int RPW = WAVE / LPR;      // rows per wave load
  constexpr int NI = DEC_WKEYS / RPW;  // loads of K (and of V) per tile
  __shared__ float sm_o[4][D];
  __shared__ float sm_m[4], sm_l[4];

  const int split = blockIdx.x;
  const long bh = blockIdx.y;
  const int b = (int)(bh / H), h = (int)(bh % H);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int g = lane / LPR, c = lane % LPR;

  const int Lraw = cache_len[b];
  const bool can_store = Lraw >= 0 && Lraw < S_max;
  const int L = min(max(Lraw, 0), S_max - 1);
  const long kstart_l = (long)split * chunk;
  float* wsp = ws + (bh * n_split + split) * (D + 2);

  if (kstart_l > L) {  // whole chunk past the live keys: neutral partial
    if (tid < D) wsp[tid] = 0.f;
    if (tid == 0) { wsp[D] = -INFINITY; wsp[D + 1] = 0.f; }
    return;
  }
  const int kstart = (int)kstart_l;
  const bool last = split == n_split - 1;
  const int kend = last ? L + 1 : min(kstart + chunk, L + 1);

  // q * scale, and the new token's k and v: this lane's 8 dims
  const bf16_t* qn = qkv + (((long)b * 3 + 0) * H + h) * D + c * 8;
  const long plane = (long)H * D;
  float q[8];
  {
    const bf16x8 qr = *reinterpret_cast<const bf16x8*>(qn);
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = us2f((unsigned short)qr[j]) * scale;
  }
  const bf16x8 knew = *reinterpret_cast<const bf16x8*>(qn + plane);
  const bf16x8 vnew = *reinterpret_cast<const bf16x8*>(qn + 2 * plane);

  bf16_t* kb = kc + bh * (long)S_max * D;
  bf16_t* vb = vc + bh * (long)S_max * D;

  // the owner of row L appends the new token (kstart <= L < kend here
  // exactly when this block owns it)
  if (can_store && L < kend) {
    const int r = (L - kstart) % DEC_TILE;
    if (w == r / DEC_WKEYS && g == r % RPW) {
      *reinterpret_cast<bf16x8*>(kb + (long)L * D + c * 8) = knew;
      *reinterpret_cast<bf16x8*>(vb + (long)L * D + c * 8) = vnew;
    }
  }

  float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;

  const int koff = w * DEC_WKEYS + g;  // + i * RPW: this lane's keys
  bf16x8 kn[NI], vn[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int kidx = kstart + koff + i * RPW;
    kn[i] = dec_row<D>(kb, kidx, L, kend, c, knew);
    vn[i] = dec_row<D>(vb, kidx, L, kend, c, vnew);
  }

  for (int t = kstart; t < kend; t += DEC_TILE) {
    bf16x8 kr[NI], vr[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) { kr[i] = kn[i]; vr[i] = vn[i]; }
    if (t + DEC_TILE < kend) {  // next tile's loads before this tile's math
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int kidx = t + DEC_TILE + koff + i * RPW;
        kn[i] = dec_row<D>(kb, kidx, L, kend, c, knew);
        vn[i] = dec_row<D>(vb, kidx, L, kend, c, vnew);
      }
    }
    float s[NI];
    float mt = -INFINITY;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc = fmaf(q[j], us2f((unsigned short)kr[i][j]), acc);
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1)
        acc += __shfl_xor(acc, off, WAVE);
      s[i] = (t + koff + i * RPW < kend) ? acc : -INFINITY;
      mt = fmaxf(mt, s[i]);
    }
    const float mn = fmaxf(m, mt);
    if (mn > -INFINITY) {  // this group has seen a live key
      const float alpha = __expf(m - mn);
      l *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] *= alpha;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const float p = __expf(s[i] - mn);  // dead key: exp(-inf) = 0
        l += p;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = fmaf(p, us2f((unsigned short)vr[i][j]), o[j]);
      }
      m = mn;
    }
  }

  // lane groups of the wave
#pragma unroll
  for (int off = LPR; off < WAVE; off <<= 1) {
    const float m2 = __shfl_xor(m, off, WAVE);
    const float l2 = __shfl_xor(l, off, WAVE);
    float mn, a, bb;
    lse_weights(m, m2, mn, a, bb);
    l = l * a + l2 * bb;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = o[j] * a + __shfl_xor(o[j], off, WAVE) * bb;
    m = mn;
  }
  // waves of the block
  if (g == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sm_o[w][c * 8 + j] = o[j];
    if (c == 0) { sm_m[w] = m; sm_l[w] = l; }
  }
  __syncthreads();
  if (tid < D) {
    float M = sm_m[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) M = fmaxf(M, sm_m[i]);
    // M is finite: the block owns at least key kstart <= L
    float acc = 0.f, lsum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float wt = __expf(sm_m[i] - M);
      acc += sm_o[i][tid] * wt;
      lsum += sm_l[i] * wt;
    }
    if (n_split == 1) {
      out[bh * D + tid] = f2bf(acc / lsum);
    } else {
      wsp[tid] = acc;
      if (tid == 0) { wsp[D] = M; wsp[D + 1] = lsum; }
    }
  }
}

// one block per head, thread d owns output dim d; splits in index order
template <int D>
DECODE_TARGET __global__ __launch_bounds__(D) void
attn_decode_combine_kernel(const float* __restrict__ ws,
                           bf16_t* __restrict__ out, int n_split) {
  const long bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* p = ws + bh * n_split * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < n_split; ++s) M = fmaxf(M, p[s * (D + 2) + D]);
  // split 0 always owns key 0 <= L, so M is finite
  float acc = 0.f, lsum = 0.f;
  for (int s = 0; s < n_split; ++s) {
    const float wt = __expf(p[s * (D + 2) + D] - M);
    acc += p[s * (D + 2) + d] * wt;
    lsum += p[s * (D + 2) + D + 1] * wt;
  }
  out[bh * D + d] = f2bf(acc / lsum);
}

// keys per split: a multiple of 64 that covers max_len in n_split pieces
int dec_chunk(long max_len, long n_split) {
  const long per = (max_len + n_split - 1) / n_split;
  return (int)((per + DEC_TILE - 1) / DEC_TILE * DEC_TILE);
}

}  // namespace

// Split count from B*H and max_len alone: about two blocks per CU on 256
// CUs, never less than one 64-key tile per split.
int64_t attn_decode_splits(int64_t bh, int64_t max_len) {
  const long target = 2 * 256;
  const long tiles = (max_len + DEC_TILE - 1) / DEC_TILE;
  long n = (target + bh - 1) / bh;
  n = std::max(1L, std::min(n, tiles));
  // drop splits that the rounded-up chunk leaves empty
  const long chunk = dec_chunk(max_len, n);
  return (max_len + chunk - 1) / chunk;
}

at::Tensor attn_decode(at::Tensor qkv_new, at::Tensor k_cache,
                       at::Tensor v_cache, at::Tensor cache_len, double scale,
                       c10::optional<int64_t> max_len,
                       c10::optional<int64_t> n_split) {
  TORCH_CHECK(qkv_new.is_cuda() && k_cache.is_cuda() && v_cache.is_cuda() &&
              cache_len.is_cuda(), "attn_decode: device tensors expected");
  TORCH_CHECK(qkv_new.scalar_type() == at::kBFloat16 &&
              k_cache.scalar_type() == at::kBFloat16 &&
              v_cache.scalar_type() == at::kBFloat16,
              "attn_decode: bf16 qkv_new and caches expected");
  TORCH_CHECK(qkv_new.is_contiguous() && k_cache.is_contiguous() &&
              v_cache.is_contiguous() && cache_len.is_contiguous(),
              "attn_decode: contiguous tensors expected");
  TORCH_CHECK(qkv_new.dim() == 4 && qkv_new.size(1) == 3,
              "attn_decode: qkv_new must be (B, 3, H, D)");
  const long B = qkv_new.size(0), H = qkv_new.size(2), D = qkv_new.size(3);
  TORCH_CHECK(D == 64 || D == 128, "attn_decode: D must be 64 or 128");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(0) == B &&
              k_cache.size(1) == H && k_cache.size(3) == D &&
              k_cache.size(2) >= 1,
              "attn_decode: k_cache must be (B, H, S_max, D)");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(),
              "attn_decode: v_cache must have k_cache's shape");
  TORCH_CHECK(cache_len.scalar_type() == at::kInt && cache_len.dim() == 1 &&
              cache_len.size(0) == B,
              "attn_decode: cache_len must be int32 of shape (B,)");
  const long S_max = k_cache.size(2);
  TORCH_CHECK(S_max < (1L << 30), "attn_decode: S_max too large");
  TORCH_CHECK(B >= 1 && H >= 1 && B * H <= 65535,
              "attn_decode: B*H must be in [1, 65535]");
  const long ml = max_len.has_value() ? *max_len : S_max;
  TORCH_CHECK(ml >= 1 && ml <= S_max,
              "attn_decode: max_len must be in [1, S_max]");
  const long ns = n_split.has_value() ? *n_split
                                      : attn_decode_splits(B * H, ml);
  TORCH_CHECK(ns >= 1 && ns <= 1024,
              "attn_decode: n_split must be in [1, 1024]");
  const int chunk = dec_chunk(ml, ns);

  auto out = at::empty({B, H * D}, qkv_new.options());
  at::Tensor ws;
  if (ns > 1)
    ws = at::empty({B * H, ns, D + 2}, qkv_new.options().dtype(at::kFloat));
  float* wsp = ns > 1 ? ws.data_ptr<float>() : nullptr;
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const bf16_t* qp = reinterpret_cast<const bf16_t*>(qkv_new.data_ptr());
  bf16_t* kp = reinterpret_cast<bf16_t*>(k_cache.data_ptr());
  bf16_t* vp = reinterpret_cast<bf16_t*>(v_cache.data_ptr());
  bf16_t* op = reinterpret_cast<bf16_t*>(out.data_ptr());
  const int* lp = cache_len.data_ptr<int>();
  dim3 grid((unsigned)ns, (unsigned)(B * H));
  if (D == 64) {
    hipLaunchKernelGGL((attn_decode_kernel<64>), grid, dim3(DEC_THREADS), 0,
                       stream, qp, kp, vp, lp, wsp, op, (int)H, (int)S_max,
                       chunk, (int)ns, (float)scale);
  } else {
    hipLaunchKernelGGL((attn_decode_kernel<128>), grid, dim3(DEC_THREADS), 0,
                       stream, qp, kp, vp, lp, wsp, op, (int)H, (int)S_max,
                       chunk, (int)ns, (float)scale);
  }
  HIP_CHECK_LAST();
  if (ns > 1) {
    if (D == 64) {
      hipLaunchKernelGGL((attn_decode_combine_kernel<64>),
                         dim3((unsigned)(B * H)), dim3(64), 0, stream, wsp, op,
                         (int)ns);
    } else {
      hipLaunchKernelGGL((attn_decode_combine_kernel<128>),
                         dim3((unsigned)(B * H)), dim3(128), 0, stream, wsp,
                         op, (int)ns);
    }
    HIP_CHECK_LAST();
  }
  return out;
}
