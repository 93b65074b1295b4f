// Sparse MLM head: vocabulary decoder + cross-entropy on the LIVE rows
// only (rows whose label is not ignore_index — about 15 % under MLM
// masking). The dense path runs three 65536 x 768 x 30522 GEMMs and two
// 4 GB cross-entropy passes of which ~85 % feed nothing.
//
//   loss = f(h[N,Hd], W[V,Hd], b[V], targets[N], ignore_index)
//
// The live count changes every step and the step is replayed from one
// captured graph, so the host never sees it: every shape, workspace and
// grid is sized for the worst case (count == N), the count lives in a
// device int written by the scan kernel, and every kernel downstream
// reads it and lets its surplus blocks return at once.
//
// forward : count + scan (idx/pos/count) -> gather live rows of h into hc ->
//           gemm_nt (+bias, device row limit) -> live-row CE forward
// backward: live-row CE backward IN PLACE on the logits -> W^T (padded)
//           -> gemm_nt dgrad (row limit) -> scatter into dense dh ->
//           wgrad (device reduction bound) -> bias-gradient column sum
//
// Padding contract (rounded count R = round_up(count, 64), padded vocab
// Vp = round_up(V, 128)): hc rows [count, R) are zero; after the CE
// backward, dlogits rows [count, R) and columns [V, Vp) are zero; W^T
// columns [V, Vp) are zero. So the 64-deep reduction tiles of the dgrad
// (over Vp) and the wgrad (over R) only ever read defined values, also
// when an earlier replay with a larger count left stale rows behind.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

void gemm_nt_bf16_rows(at::Tensor A2, at::Tensor B,
                       c10::optional<at::Tensor> bias, int64_t epi,
                       at::Tensor C, at::Tensor row_limit);
at::Tensor gemm_wgrad_bf16_rows(at::Tensor dy, at::Tensor x,
                                at::Tensor row_bound);
std::vector<at::Tensor> ce_rows_fwd(at::Tensor logits, at::Tensor tc,
                                    at::Tensor count, int64_t V);
void ce_rows_bwd_(at::Tensor logits, at::Tensor tc, at::Tensor count,
                  at::Tensor lse, at::Tensor dloss, int64_t V);

namespace {

constexpr int SCAN_THREADS = 256, SCAN_CHUNKS = 8;
constexpr int SCAN_ROWS = SCAN_THREADS * SCAN_CHUNKS;  // rows per block

DEVINL int block_sum_int(int v, int* lds) {  // blockDim.x == SCAN_THREADS
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / WAVE; ++w) r += lds[w];
  __syncthreads();
  return r;
}

// Stable compaction of targets != ignore_index in two small kernels
// (coalesced reads; one block over all N rows measured 128 us):
// 1. live rows per block of SCAN_ROWS consecutive rows
__global__ __launch_bounds__(SCAN_THREADS) void mlm_count_kernel(
    const long* __restrict__ targets, long N, long ignore_index,
    int* __restrict__ blockcnt) {
  __shared__ int lds[SCAN_THREADS / WAVE];
  const long r0 = (long)blockIdx.x * SCAN_ROWS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < SCAN_CHUNKS; ++k) {
    const long i = r0 + k * SCAN_THREADS + threadIdx.x;
    if (i < N) c += targets[i] != ignore_index;
  }
  c = block_sum_int(c, lds);
  if (threadIdx.x == 0) blockcnt[blockIdx.x] = c;
}

// 2. each block sums the counts of the blocks before it, then scans its
// own rows 256 at a time (wave ballots + wave totals through LDS) and
// writes
//   pos[i] = compact row of dense row i, or -1 when ignored   (N entries)
//   idx[c] = dense row of compact row c                    (count entries)
// the last block also writes the total into count[0].
__global__ __launch_bounds__(SCAN_THREADS) void mlm_scan_kernel(
    const long* __restrict__ targets, long N, long ignore_index,
    const int* __restrict__ blockcnt, int* __restrict__ pos,
    int* __restrict__ idx, int* __restrict__ count) {
  __shared__ int lds[SCAN_THREADS / WAVE];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  int part = 0;
  for (int j = tid; j < (int)blockIdx.x; j += SCAN_THREADS)
    part += blockcnt[j];
  int run = block_sum_int(part, lds);
  const long r0 = (long)blockIdx.x * SCAN_ROWS;
  for (int k = 0; k < SCAN_CHUNKS; ++k) {
    const long i = r0 + k * SCAN_THREADS + tid;
    const bool live = i < N && targets[i] != ignore_index;
    const unsigned long long mask = __ballot(live);
    const int wpre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) lds[wid] = __popcll(mask);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / WAVE; ++w) {
      const int t = lds[w];
      if (w < wid) off += t;
      tot += t;
    }
    __syncthreads();
    if (live) {
      const int p = run + off + wpre;
      pos[i] = p;
      idx[p] = (int)i;
    } else if (i < N) {
      pos[i] = -1;
    }
    run += tot;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) count[0] = run;
}

// one wave per compact row r: r < count copies h[idx[r]] and its label;
// r in [count, round_up(count, 64)) is zero-filled; later rows untouched.
__global__ void mlm_gather_kernel(const bf16_t* __restrict__ h,
                                  const long* __restrict__ targets,
                                  const int* __restrict__ idx,
                                  const int* __restrict__ count,
                                  bf16_t* __restrict__ hc,
                                  long* __restrict__ tc, long cap, int Hd) {
  const long r = (long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int cnt = *count;
  if (r >= cap || r >= (((long)cnt + 63) & ~63l)) return;
  bf16x8* dst = reinterpret_cast<bf16x8*>(hc + r * Hd);
  const int nv = Hd >> 3;
  if (r < cnt) {
    const long src_row = idx[r];
    const bf16x8* src = reinterpret_cast<const bf16x8*>(h + src_row * Hd);
    for (int g = lane; g < nv; g += WAVE) dst[g] = src[g];
    if (lane == 0) tc[r] = targets[src_row];
  } else {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = lane; g < nv; g += WAVE) dst[g] = z;
    if (lane == 0) tc[r] = 0;
  }
}

// dense dh[N,Hd]: row i takes compact row pos[i], ignored rows get exact
// zeros — every row is written, so dh needs no memset
__global__ void mlm_scatter_kernel(const bf16_t* __restrict__ dhc,
                                   const int* __restrict__ pos,
                                   bf16_t* __restrict__ dh, long N, int Hd) {
  const long i = (long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (i >= N) return;
  bf16x8* dst = reinterpret_cast<bf16x8*>(dh + i * Hd);
  const int nv = Hd >> 3;
  const int p = pos[i];
  if (p >= 0) {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(dhc + (long)p * Hd);
    for (int g = lane; g < nv; g += WAVE) dst[g] = src[g];
  } else {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = lane; g < nv; g += WAVE) dst[g] = z;
  }
}

// Wt[Hd][Vp] = W[V][Hd]^T, columns [V, Vp) zero. 64 x 64 tiles through
// LDS (row pitch 65 keeps the transposed read conflict-free).
__global__ __launch_bounds__(256) void mlm_transpose_pad_kernel(
    const bf16_t* __restrict__ W, bf16_t* __restrict__ Wt, long V, long Vp,
    int Hd) {
  __shared__ unsigned short tile[64][65];
  const long v0 = (long)blockIdx.x * 64;
  const int h0 = blockIdx.y * 64;
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  const unsigned short* w = reinterpret_cast<const unsigned short*>(W);
  unsigned short* wt = reinterpret_cast<unsigned short*>(Wt);
  for (int r = r0; r < 64; r += 4) {
    const long v = v0 + r;
    tile[r][c] = v < V ? w[v * Hd + h0 + c] : (unsigned short)0;
  }
  __syncthreads();
  for (int r = r0; r < 64; r += 4)
    wt[(long)(h0 + r) * Vp + v0 + c] = tile[c][r];
}

// column sum of rows [0, count) of x[cap][ld] bf16 -> fp32 out[ld]
// (out zeroed by the caller). The rows are split over gridDim.y chunks
// ON DEVICE, so the 15 % case is not walked by a single chunk.
__global__ void mlm_colsum_kernel(const bf16_t* __restrict__ x,
                                  const int* __restrict__ count,
                                  float* __restrict__ out, long ld) {
  const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ld) return;
  const long cnt = *count;
  const long per = (cnt + gridDim.y - 1) / gridDim.y;
  const long r0 = blockIdx.y * per, r1 = min(cnt, r0 + per);
  if (r0 >= r1) return;
  float s = 0.f;
  long r = r0;
  for (; r + 8 <= r1; r += 8) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bf2f(x[(r + j) * ld + col]);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += acc[j];
  }
  for (; r < r1; ++r) s += bf2f(x[r * ld + col]);
  atomicAdd(&out[col], s);
}

inline long round_up64(long v) { return (v + 63) / 64 * 64; }
// padded vocab: a multiple of the wgrad kernel's 128-wide tile, so the
// wgrad runs without its (slow, register-staged) ragged-tile launch
inline long pad_vocab(long v) { return (v + 127) / 128 * 128; }

}  // namespace

// -> {loss_sum f32[], count i32[1], logits_c bf16[cap,Vp], lse f32[cap],
//     hc bf16[cap,Hd], tc i64[cap], pos i32[N]}
// loss = loss_sum / max(count, 1) is left to the caller.
std::vector<at::Tensor> mlm_head_fwd(at::Tensor h, at::Tensor W,
                                     at::Tensor b, at::Tensor targets,
                                     int64_t ignore_index) {
  TORCH_CHECK(h.is_cuda() && h.scalar_type() == at::kBFloat16 &&
              h.is_contiguous() && h.dim() == 2);
  TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kBFloat16 &&
              W.is_contiguous() && W.dim() == 2 && W.size(1) == h.size(1));
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == at::kBFloat16 &&
              b.is_contiguous() && b.numel() == W.size(0));
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == at::kLong &&
              targets.is_contiguous() && targets.numel() == h.size(0));
  const long N = h.size(0), Hd = h.size(1), V = W.size(0);
  TORCH_CHECK(Hd % 64 == 0 && Hd >= 128,
              "mlm_head: hidden % 64 == 0 and >= 128 required");
  TORCH_CHECK(N >= 1 && N < (1l << 31));
  const long cap = std::max(round_up64(N), 128l), Vp = pad_vocab(V);
  TORCH_CHECK(cap * Vp * 2 < (1ll << 32),
              "mlm_head: compact logits must stay < 4 GiB");
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto iopt = h.options().dtype(at::kInt);
  auto count = at::empty({1}, iopt);
  auto pos = at::empty({N}, iopt);
  auto idx = at::empty({cap}, iopt);
  auto hc = at::empty({cap, Hd}, h.options());
  auto tc = at::empty({cap}, targets.options());
  auto logits = at::empty({cap, Vp}, h.options());

  const unsigned sblocks = (unsigned)((N + SCAN_ROWS - 1) / SCAN_ROWS);
  auto blockcnt = at::empty({(long)sblocks}, iopt);
  hipLaunchKernelGGL(mlm_count_kernel, dim3(sblocks), dim3(SCAN_THREADS), 0,
                     stream, targets.data_ptr<long>(), N, (long)ignore_index,
                     blockcnt.data_ptr<int>());
  hipLaunchKernelGGL(mlm_scan_kernel, dim3(sblocks), dim3(SCAN_THREADS), 0,
                     stream, targets.data_ptr<long>(), N, (long)ignore_index,
                     blockcnt.data_ptr<int>(), pos.data_ptr<int>(),
                     idx.data_ptr<int>(), count.data_ptr<int>());
  hipLaunchKernelGGL(mlm_gather_kernel, dim3((unsigned)((cap + 3) / 4)),
                     dim3(256), 0, stream,
                     reinterpret_cast<const bf16_t*>(h.data_ptr()),
                     targets.data_ptr<long>(), idx.data_ptr<int>(),
                     count.data_ptr<int>(),
                     reinterpret_cast<bf16_t*>(hc.data_ptr()),
                     tc.data_ptr<long>(), cap, (int)Hd);
  HIP_CHECK_LAST();
  gemm_nt_bf16_rows(hc, W, b, 1, logits, count);
  auto ce = ce_rows_fwd(logits, tc, count, V);
  return {ce[0], count, logits, ce[1], hc, tc, pos};
}

// -> {dh bf16[N,Hd], dW bf16[V,Hd], db bf16[V]}. OVERWRITES logits_c with
// dlogits (the saved forward state is consumed: one backward per forward).
std::vector<at::Tensor> mlm_head_bwd(at::Tensor dloss, at::Tensor logits_c,
                                     at::Tensor lse, at::Tensor hc,
                                     at::Tensor tc, at::Tensor pos,
                                     at::Tensor count, at::Tensor W) {
  TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kBFloat16 &&
              W.is_contiguous() && W.dim() == 2);
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.is_contiguous());
  const long N = pos.numel(), Hd = W.size(1), V = W.size(0);
  const long cap = logits_c.size(0), Vp = logits_c.size(1);
  TORCH_CHECK(Vp == pad_vocab(V) && cap >= N && cap % 64 == 0);
  TORCH_CHECK(hc.dim() == 2 && hc.size(0) == cap && hc.size(1) == Hd &&
              Hd % 64 == 0);
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  auto gs = dloss.to(at::kFloat).reshape({1}).contiguous();
  ce_rows_bwd_(logits_c, tc, count, lse, gs, V);  // logits_c is dlogits now

  // dgrad: dhc = dlogits_c[:, :Vp] @ W^T[Hd, Vp]^T, live rows only
  auto Wt = at::empty({Hd, Vp}, W.options());
  hipLaunchKernelGGL(mlm_transpose_pad_kernel,
                     dim3((unsigned)(Vp / 64), (unsigned)(Hd / 64)),
                     dim3(256), 0, stream,
                     reinterpret_cast<const bf16_t*>(W.data_ptr()),
                     reinterpret_cast<bf16_t*>(Wt.data_ptr()), V, Vp,
                     (int)Hd);
  HIP_CHECK_LAST();
  auto dhc = at::empty({cap, Hd}, W.options());
  gemm_nt_bf16_rows(logits_c, Wt, c10::nullopt, 0, dhc, count);
  auto dh = at::empty({N, Hd}, W.options());
  hipLaunchKernelGGL(mlm_scatter_kernel, dim3((unsigned)((N + 3) / 4)),
                     dim3(256), 0, stream,
                     reinterpret_cast<const bf16_t*>(dhc.data_ptr()),
                     pos.data_ptr<int>(),
                     reinterpret_cast<bf16_t*>(dh.data_ptr()), N, (int)Hd);
  HIP_CHECK_LAST();

  // wgrad over the padded vocab (pad columns of dlogits are zero -> zero
  // rows, sliced away), reduction bounded by the device count
  auto dWp = gemm_wgrad_bf16_rows(logits_c, hc, count);
  auto dW = dWp.narrow(0, 0, V).to(W.scalar_type());

  auto dbp = at::zeros({Vp}, W.options().dtype(at::kFloat));
  const int col_blocks = (int)((Vp + 255) / 256);
  const int nchunks = (int)std::min<long>(
      cap / 64, std::max<long>(1, 8192 / col_blocks));
  hipLaunchKernelGGL(mlm_colsum_kernel, dim3(col_blocks, nchunks), dim3(256),
                     0, stream,
                     reinterpret_cast<const bf16_t*>(logits_c.data_ptr()),
                     count.data_ptr<int>(), dbp.data_ptr<float>(), Vp);
  HIP_CHECK_LAST();
  auto db = dbp.narrow(0, 0, V).to(W.scalar_type());
  return {dh, dW, db};
}
