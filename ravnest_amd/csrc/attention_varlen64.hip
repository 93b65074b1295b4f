// Variable-length ("unpadded") flash attention for CDNA4 (gfx950), bf16,
// D=64, forward and backward, on a packed token stream:
//
//   qkv  (T, 3, H, 64) bf16   token-major, the qkv projection's layout
//   cu   int32 (B+1,)         sequence b is rows [cu[b], cu[b+1]); rows
//                             [cu[B], T) are a tail
//   O    (T, H, 64) bf16, lse (H, T) fp32, dqkv (T, 3, H, 64) bf16
//
// Work split. Nothing on the host knows a length, so the grid cannot be
// (tiles of S, B*H). attn_varlen_tiles, one block, turns cu into a TILE
// TABLE: entry i = {sequence, first row inside it} of the i-th 128-row
// tile, sequences in order, from an exclusive scan of ceil(len_b / 128);
// an empty sequence gets no entry. Tail tiles follow as {-1, first row of
// the stream}, and the entry at the table's last index holds the count.
// The worst-case count, NT = T / 128 + B + 1, depends on shapes only, so
// the compute kernels launch grid (NT, H): a block reads its entry, a block
// at or past the count returns before its first barrier, a tail tile
// stores its exact zeros (lse: -inf) and returns, and a live tile runs the
// block body of the dense kernels (attention_fwd64_block.h,
// attention_bwd64_block.h) on a view of its own sequence: base pointers
// moved by cu[b] rows, S = len_b. Every row clamp of those bodies is
// min(row, S - 1), so no staged row, score or store leaves the sequence;
// the dK/dV body picks the LDS or the global lse/Delta rows from its own
// S, which is block-uniform. One table per batch serves every layer in
// both directions. No atomics: results are bit-equal from call to call.
//
// Delta = rowsum(dO * O) is row-wise, so it is attn_bwd_delta_kernel<64>
// run on the stream as one sequence of T rows; tail rows get a value that
// nothing reads.
//
// Lengths are read through seq_view, which clamps them into [0, T]: a
// malformed cu can give wrong results, never an access outside the
// tensors.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include "attention_bwd64_block.h"
#include "attention_fwd64_block.h"

namespace {

constexpr int TILE_ROWS = 128;

struct SeqView { int start, len; };

// rows of sequence b, clamped into the stream
DEVINL SeqView seq_view(const int* __restrict__ cu, int b, int T) {
  const int lo = min(max(cu[b], 0), T);
  const int hi = min(max(cu[b + 1], lo), T);
  return {lo, hi - lo};
}

DEVINL int tiles_of(int rows) { return (rows + TILE_ROWS - 1) / TILE_ROWS; }

// cu -> tile table of NT + 1 int pairs (file comment). One block: the
// exclusive scan runs over chunks of blockDim.x sequences through LDS.
__global__ void attn_varlen_tiles_kernel(const int* __restrict__ cu,
                                         int* __restrict__ tiles, int B,
                                         int T, int NT) {
  __shared__ int scan[256];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < B; base += blockDim.x) {
    const int b = base + tid;
    const int n = (b < B) ? tiles_of(seq_view(cu, b, T).len) : 0;
    scan[tid] = n;
    __syncthreads();
    for (int off = 1; off < (int)blockDim.x; off <<= 1) {
      const int add = (tid >= off) ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    const int first = carry + scan[tid] - n;  // exclusive prefix
    for (int j = 0; j < n && first + j < NT; ++j) {
      tiles[2 * (first + j)] = b;
      tiles[2 * (first + j) + 1] = j * TILE_ROWS;
    }
    __syncthreads();
    if (tid == (int)blockDim.x - 1) carry += scan[tid];
    __syncthreads();
  }
  const int live = min(carry, NT);
  const int tail0 = seq_view(cu, B - 1, T).start + seq_view(cu, B - 1, T).len;
  const int n_tail = min(tiles_of(T - tail0), NT - live);
  for (int j = tid; j < n_tail; j += blockDim.x) {
    tiles[2 * (live + j)] = -1;
    tiles[2 * (live + j) + 1] = tail0 + j * TILE_ROWS;
  }
  if (tid == 0) {
    tiles[2 * NT] = live + n_tail;
    tiles[2 * NT + 1] = 0;
  }
}

// exact zeros on rows row0 .. row_end-1 of one head's 128-byte rows: 16
// bytes per thread and step, a 128-row tile in four steps
DEVINL void zero_rows(bf16_t* __restrict__ gp, long rs, int row0,
                      int row_end) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = (int)threadIdx.x + 256 * i;
    const int row = row0 + (idx >> 3);
    if (row < row_end)
      *reinterpret_cast<uint4*>(gp + (long)row * rs + (idx & 7) * 8) =
          make_uint4(0u, 0u, 0u, 0u);
  }
}

// a block's table entry; false = past the count (no work)
struct TileRef { int seq, row; };

DEVINL bool tile_ref(const int* __restrict__ tiles, TileRef& t) {
  if ((int)blockIdx.x >= tiles[2 * gridDim.x]) return false;
  t.seq = tiles[2 * blockIdx.x];
  t.row = tiles[2 * blockIdx.x + 1];
  return true;
}

// packed strides in elements: qkv / dqkv rows 3*H*64, O / dO rows H*64
FWD64_TARGET __global__ __launch_bounds__(256, 3) void attn_varlen_fwd64_kernel(
    const bf16_t* __restrict__ qkv, const int* __restrict__ cu,
    const int* __restrict__ tiles, bf16_t* __restrict__ o,
    float* __restrict__ lse, int T, int causal, float scale) {
  TileRef t;
  if (!tile_ref(tiles, t)) return;
  const long H = gridDim.y, h = blockIdx.y;
  const long HD = H * 64, rs = 3 * HD;
  if (t.seq < 0) {  // tail tile
    const int end = min(t.row + TILE_ROWS, T);
    zero_rows(o + h * 64, HD, t.row, end);
    const int row = t.row + (int)threadIdx.x;
    if (threadIdx.x < TILE_ROWS && row < end) lse[h * T + row] = -INFINITY;
    return;
  }
  const SeqView s = seq_view(cu, t.seq, T);
  const bf16_t* qp = qkv + s.start * rs + h * 64;
  fwd64_block<false>(qp, qp + HD, qp + 2 * HD, nullptr,
                     o + s.start * HD + h * 64, lse + h * T + s.start, s.len,
                     s.len, t.row / TILE_ROWS, causal, scale, rs, rs, rs, HD);
}

BWD64_TARGET __global__ __launch_bounds__(256, 2) void attn_varlen_bwd64_kv_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const int* __restrict__ cu, const int* __restrict__ tiles,
    bf16_t* __restrict__ dqkv, int T, int causal, float scale) {
  TileRef t;
  if (!tile_ref(tiles, t)) return;
  const long H = gridDim.y, h = blockIdx.y;
  const long HD = H * 64, rs = 3 * HD;
  if (t.seq < 0) {  // tail tile
    const int end = min(t.row + TILE_ROWS, T);
    zero_rows(dqkv + HD + h * 64, rs, t.row, end);
    zero_rows(dqkv + 2 * HD + h * 64, rs, t.row, end);
    return;
  }
  const SeqView s = seq_view(cu, t.seq, T);
  const bf16_t* qp = qkv + s.start * rs + h * 64;
  bf16_t* gp = dqkv + s.start * rs + h * 64;
  bwd64_kv_block(qp, qp + HD, qp + 2 * HD, dout + s.start * HD + h * 64,
                 lse + h * T + s.start, delta + h * T + s.start, nullptr,
                 gp + HD, gp + 2 * HD, s.len, s.len, t.row / TILE_ROWS,
                 causal, scale, 0, rs, HD, rs);
}

BWD64_TARGET __global__ __launch_bounds__(256, 2) void attn_varlen_bwd64_dq_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const int* __restrict__ cu, const int* __restrict__ tiles,
    bf16_t* __restrict__ dqkv, int T, int causal, float scale) {
  TileRef t;
  if (!tile_ref(tiles, t)) return;
  const long H = gridDim.y, h = blockIdx.y;
  const long HD = H * 64, rs = 3 * HD;
  if (t.seq < 0) {  // tail tile
    zero_rows(dqkv + h * 64, rs, t.row, min(t.row + TILE_ROWS, T));
    return;
  }
  const SeqView s = seq_view(cu, t.seq, T);
  const bf16_t* qp = qkv + s.start * rs + h * 64;
  bwd64_dq_block(qp, qp + HD, qp + 2 * HD, dout + s.start * HD + h * 64,
                 lse + h * T + s.start, delta + h * T + s.start, nullptr,
                 dqkv + s.start * rs + h * 64, s.len, s.len,
                 t.row / TILE_ROWS, causal, scale, 0, rs, HD, rs);
}

long table_tiles(long T, long B) { return T / TILE_ROWS + B + 1; }

// shapes and dtypes of one call; returns B
long check_varlen(const at::Tensor& qkv, const at::Tensor& cu,
                  const at::Tensor& tiles, const char* who) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() &&
                  qkv.scalar_type() == at::kBFloat16,
              who, ": qkv must be a contiguous bf16 device tensor");
  TORCH_CHECK(qkv.dim() == 4 && qkv.size(1) == 3 && qkv.size(3) == 64,
              who, ": qkv must be (T, 3, H, 64)");
  TORCH_CHECK(qkv.size(0) >= 1 && qkv.size(0) < (1L << 31) / (3 * 64) &&
                  qkv.size(2) >= 1 && qkv.size(2) <= 65535,
              who, ": T or H out of range");
  TORCH_CHECK(cu.scalar_type() == at::kInt && cu.dim() == 1 &&
                  cu.numel() >= 2 && cu.is_contiguous() &&
                  cu.device() == qkv.device(),
              who, ": cu_seqlens must be contiguous int32 (B+1,) on the "
                   "device of qkv");
  const long B = cu.numel() - 1;
  TORCH_CHECK(tiles.scalar_type() == at::kInt && tiles.is_contiguous() &&
                  tiles.device() == qkv.device() &&
                  tiles.numel() == 2 * (table_tiles(qkv.size(0), B) + 1),
              who, ": tiles must be the int32 table of attn_varlen_tiles "
                   "for this T and B");
  return B;
}

}  // namespace

at::Tensor attn_varlen_tiles(at::Tensor cu_seqlens, int64_t T) {
  TORCH_CHECK(cu_seqlens.is_cuda() && cu_seqlens.scalar_type() == at::kInt &&
                  cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 &&
                  cu_seqlens.is_contiguous(),
              "attn_varlen_tiles: cu_seqlens must be contiguous int32 "
              "(B+1,) on the device");
  TORCH_CHECK(T >= 1 && T < (1L << 31) / (3 * 64),
              "attn_varlen_tiles: T out of range");
  const long B = cu_seqlens.numel() - 1;
  const long NT = table_tiles(T, B);
  auto tiles = at::empty({NT + 1, 2}, cu_seqlens.options());
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  hipLaunchKernelGGL(attn_varlen_tiles_kernel, dim3(1), dim3(256), 0, stream,
                     cu_seqlens.data_ptr<int>(), tiles.data_ptr<int>(),
                     (int)B, (int)T, (int)NT);
  HIP_CHECK_LAST();
  return tiles;
}

std::vector<at::Tensor> attn_varlen_fwd_qkv(at::Tensor qkv,
                                            at::Tensor cu_seqlens,
                                            at::Tensor tiles, bool causal,
                                            double scale) {
  const long B = check_varlen(qkv, cu_seqlens, tiles, "attn_varlen_fwd_qkv");
  const long T = qkv.size(0), H = qkv.size(2);
  auto o = at::empty({T, H, 64L}, qkv.options());
  auto lse = at::empty({H, T}, qkv.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  hipLaunchKernelGGL(attn_varlen_fwd64_kernel,
                     dim3(table_tiles(T, B), H), dim3(256), 0, stream,
                     reinterpret_cast<const bf16_t*>(qkv.data_ptr()),
                     cu_seqlens.data_ptr<int>(), tiles.data_ptr<int>(),
                     reinterpret_cast<bf16_t*>(o.data_ptr()),
                     lse.data_ptr<float>(), (int)T, causal ? 1 : 0,
                     (float)scale);
  HIP_CHECK_LAST();
  return {o, lse};
}

at::Tensor attn_varlen_bwd_qkv(at::Tensor qkv, at::Tensor o, at::Tensor dout,
                               at::Tensor lse, at::Tensor cu_seqlens,
                               at::Tensor tiles, bool causal, double scale) {
  const long B = check_varlen(qkv, cu_seqlens, tiles, "attn_varlen_bwd_qkv");
  const long T = qkv.size(0), H = qkv.size(2);
  for (const at::Tensor* t : {&o, &dout})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == at::kBFloat16 && t->dim() == 3 &&
                    t->size(0) == T && t->size(1) == H && t->size(2) == 64,
                "attn_varlen_bwd_qkv: o and dout must be contiguous bf16 "
                "(T, H, 64)");
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == H && lse.size(1) == T,
              "attn_varlen_bwd_qkv: lse must be contiguous fp32 (H, T)");
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty_like(lse);
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const bf16_t* qp = reinterpret_cast<const bf16_t*>(qkv.data_ptr());
  const bf16_t* dop = reinterpret_cast<const bf16_t*>(dout.data_ptr());
  // Delta on the stream as one sequence of T rows: delta[h * T + row]
  const long NR = H * T;
  hipLaunchKernelGGL((attn_bwd_delta_kernel<64>), dim3((NR * 8 + 255) / 256),
                     dim3(256), 0, stream, dop,
                     reinterpret_cast<const bf16_t*>(o.data_ptr()),
                     delta.data_ptr<float>(), (int)T, H, NR,
                     StridesB{0, 64, H * 64});
  const dim3 grid(table_tiles(T, B), H), block(256);
  const int c = causal ? 1 : 0;
  hipLaunchKernelGGL(attn_varlen_bwd64_kv_kernel, grid, block, 0, stream, qp,
                     dop, (const float*)lse.data_ptr<float>(),
                     (const float*)delta.data_ptr<float>(),
                     cu_seqlens.data_ptr<int>(), tiles.data_ptr<int>(),
                     reinterpret_cast<bf16_t*>(dqkv.data_ptr()), (int)T, c,
                     (float)scale);
  hipLaunchKernelGGL(attn_varlen_bwd64_dq_kernel, grid, block, 0, stream, qp,
                     dop, (const float*)lse.data_ptr<float>(),
                     (const float*)delta.data_ptr<float>(),
                     cu_seqlens.data_ptr<int>(), tiles.data_ptr<int>(),
                     reinterpret_cast<bf16_t*>(dqkv.data_ptr()), (int)T, c,
                     (float)scale);
  HIP_CHECK_LAST();
  return dqkv;
}
