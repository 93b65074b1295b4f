// Fused bias + GELU (tanh approximation) forward/backward for CDNA4.
// Elementwise, HBM-bound: vectorized 16-byte bf16x8 accesses, grid-stride
// with the grid capped (guide Guideline 11/13).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "mx_quant.h"

namespace {

template <typename PT>
DEVINL float load_pt(const PT* p);
template <>
DEVINL float load_pt<float>(const float* p) { return *p; }
template <>
DEVINL float load_pt<bf16_t>(const bf16_t* p) { return bf2f(*p); }

// tanh via the fast hardware exp (libm tanhf is a long VALU chain;
// these kernels are otherwise HBM-bound). Written as 1 - 2/(t+1), not
// (t-1)/(t+1): exp(2x) overflows to inf from x = 44.4 (a pre-activation
// of 10.06), where the quotient is inf/inf = NaN and this form is
// 1 - 2/inf = 1; t underflowing to 0 gives -1 in both. The reciprocal is
// the hardware v_rcp_f32 (1 ulp; rcp(inf) = 0, rcp(1) = 1): an IEEE
// division expands to ~10 VALU ops per element.
DEVINL float fast_tanh(float x) {
  const float t = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(t + 1.f);
}

DEVINL float gelu_f(float x) {
  const float k = 0.7978845608028654f;  // sqrt(2/pi)
  float t = fast_tanh(k * (x + 0.044715f * x * x * x));
  return 0.5f * x * (1.f + t);
}

DEVINL float gelu_grad_f(float x) {
  const float k = 0.7978845608028654f;
  float x2 = x * x;
  float th = fast_tanh(k * (x + 0.044715f * x * x2));
  float sech2 = 1.f - th * th;
  return 0.5f * (1.f + th) + 0.5f * x * sech2 * k * (1.f + 3.f * 0.044715f * x2);
}

// MX: also emit the MX fp8 quantisation of the bf16-ROUNDED y (e4m3 bytes
// q + one e8m0 scale per 32 elements in qs, what mx_quant(y) would return).
// bf16 x and H % 32 == 0 only (host checked): nv is then a multiple of 4
// and so are i0 and the stride, so the 4 lanes that share a 32-block take
// the same trips of the vector loop.
template <typename T, typename PT, bool MX = false>
__global__ void bias_gelu_fwd_kernel(const T* __restrict__ x,
                                     const PT* __restrict__ bias,
                                     T* __restrict__ y, long n, int H,
                                     unsigned char* __restrict__ q = nullptr,
                                     unsigned char* __restrict__ qs = nullptr) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (sizeof(T) == 2) {
    // vectors of 8 only when H % 8 == 0 (then they never straddle a row
    // end and n % 8 == 0); any other H takes the scalar loop below
    const long nv = (H & 7) ? 0 : n >> 3;
    for (long i = i0; i < nv; i += stride) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i * 8);
      const int hb = (int)((i * 8) % H);  // H%8==0: the 8 never wrap
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float b = load_pt(bias + hb + j);
        o[j] = (short)f2us(gelu_f(us2f((unsigned short)v[j]) + b));
      }
      *reinterpret_cast<bf16x8*>(y + i * 8) = o;
      if constexpr (MX) {
        float yq[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) yq[j] = us2f((unsigned short)o[j]);
        mx_quant8(yq, q + i * 8, qs + (i >> 2), threadIdx.x);
      }
    }
    // H % 8 != 0: everything
    for (long i = nv * 8 + i0; i < n; i += stride)
      y[i] = f2bf(gelu_f(bf2f(x[i]) + load_pt(bias + i % H)));
  } else {
    for (long i = i0; i < n; i += stride) {
      float b = load_pt(bias + i % H);
      y[i] = gelu_f(x[i] + b);
    }
  }
}

template <typename T, typename PT>
__global__ void bias_gelu_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const PT* __restrict__ bias,
                                     T* __restrict__ dx, long n, int H) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (sizeof(T) == 2) {
    const long nv = (H & 7) ? 0 : n >> 3;  // as in the forward
    for (long i = i0; i < nv; i += stride) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i * 8);
      bf16x8 g = *reinterpret_cast<const bf16x8*>(dy + i * 8);
      const int hb = (int)((i * 8) % H);  // H%8==0: the 8 never wrap
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float b = load_pt(bias + hb + j);
        float xf = us2f((unsigned short)v[j]) + b;
        o[j] = (short)f2us(us2f((unsigned short)g[j]) * gelu_grad_f(xf));
      }
      *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
    }
    for (long i = nv * 8 + i0; i < n; i += stride)
      dx[i] = f2bf(bf2f(dy[i]) * gelu_grad_f(bf2f(x[i]) + load_pt(bias + i % H)));
  } else {
    for (long i = i0; i < n; i += stride)
      dx[i] = dy[i] * gelu_grad_f(x[i] + load_pt(bias + i % H));
  }
}

// column sum of a bf16 (N,H) tensor -> fp32 (H), chunked rows +
// atomics (the LN dwdb recipe). Used for the fused bias grad.
__global__ void colsum_kernel(const bf16_t* __restrict__ x,
                              float* __restrict__ out, int H, long N,
                              long rows_per_chunk) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int chunk = blockIdx.y;
  if (col >= H) return;
  const long r0 = (long)chunk * rows_per_chunk;
  const long r1 = min(N, r0 + rows_per_chunk);
  float s = 0.f;
  long r = r0;
  // 8 independent loads in flight per thread (a 1-deep column walk is
  // pure latency: measured 0.9 TB/s; unrolled ~4-6x faster)
  for (; r + 8 <= r1; r += 8) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bf2f(x[(r + j) * H + col]);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += acc[j];
  }
  for (; r < r1; ++r) s += bf2f(x[r * H + col]);
  atomicAdd(&out[col], s);
}

// fused bias_gelu backward + bias-grad column reduction for bf16:
// dx = dy * gelu'(x+b) written AND column-summed in the same pass (the
// separate colsum re-read of dx measured 1.5% of the BERT step).
// Column-walk layout (colsum recipe): thread owns a column, 8 rows of
// both streams in flight, one atomicAdd per (column, chunk).
template <typename PT>
__global__ void bias_gelu_bwd_db_kernel(const bf16_t* __restrict__ dy,
                                        const bf16_t* __restrict__ x,
                                        const PT* __restrict__ bias,
                                        bf16_t* __restrict__ dx,
                                        float* __restrict__ db, int H,
                                        long N, long rows_per_chunk) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int chunk = blockIdx.y;
  if (col >= H) return;
  const float b = load_pt(bias + col);
  const long r0 = (long)chunk * rows_per_chunk;
  const long r1 = min(N, r0 + rows_per_chunk);
  float s = 0.f;
  long r = r0;
  for (; r + 8 <= r1; r += 8) {
    float xv[8], gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xv[j] = bf2f(x[(r + j) * H + col]);
      gv[j] = bf2f(dy[(r + j) * H + col]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = gv[j] * gelu_grad_f(xv[j] + b);
      dx[(r + j) * H + col] = f2bf(d);
      s += d;
    }
  }
  for (; r < r1; ++r) {
    const float d = bf2f(dy[r * H + col]) * gelu_grad_f(bf2f(x[r * H + col]) + b);
    dx[r * H + col] = f2bf(d);
    s += d;
  }
  atomicAdd(&db[col], s);
}

// ---- bf16, H % 8 == 0: column-group forward --------------------------
// bias_gelu_fwd_kernel pays per 8 elements for what depends on the column
// alone: a 64-bit i % H and eight bias loads with their conversions. With
// exp and rcp per element the kernel sits close to the vector-ALU limit as
// well as the HBM one, so that overhead is run time. Here a thread keeps
// one group of 8 columns, holds its bias in registers and walks rows with
// VEC_UNROLL 16-byte loads in flight. The per-element arithmetic and its
// rounding points are unchanged: y, q and s are bit-identical.
// (bias_gelu_bwd_db_kernel was rebuilt the same way and measured no faster,
// 237 against 233 us at 65536 x 3072: its 30-odd vector-ALU operations per
// element bound it, not its 2-byte accesses. It stays as it is.)
constexpr int VEC_UNROLL = 4;

template <typename PT>
DEVINL void load_bias8(const PT* p, float b[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = load_pt(p + j);
}

// Flat mapping: thread t of the first rows_per_sweep * G (G = H / 8) owns
// column group t % G and the rows t / G + m * rows_per_sweep, so one sweep
// of the grid is rows_per_sweep whole consecutive rows. MX needs G % 4 == 0
// (host checked): the 4 lanes of a 32-block then share a row and take the
// same trips.
template <typename PT, bool MX>
__global__ __launch_bounds__(256) void bias_gelu_fwd_vec_kernel(
    const bf16_t* __restrict__ x, const PT* __restrict__ bias,
    bf16_t* __restrict__ y, long N, int G, long rows_per_sweep,
    unsigned char* __restrict__ q, unsigned char* __restrict__ qs) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows_per_sweep * G) return;
  const int cg = (int)(t % G);
  float b[8];
  load_bias8(bias + 8 * cg, b);

  auto one = [&](long r, bf16x8 v) {
    const long i = r * G + cg;  // index of the 8-element group
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = (short)f2us(gelu_f(us2f((unsigned short)v[j]) + b[j]));
    *reinterpret_cast<bf16x8*>(y + i * 8) = o;
    if constexpr (MX) {
      float yq[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) yq[j] = us2f((unsigned short)o[j]);
      mx_quant8(yq, q + i * 8, qs + (i >> 2), threadIdx.x);
    }
  };

  long r = t / G;
  for (; r + (VEC_UNROLL - 1) * rows_per_sweep < N;
       r += VEC_UNROLL * rows_per_sweep) {
    bf16x8 v[VEC_UNROLL];
#pragma unroll
    for (int u = 0; u < VEC_UNROLL; ++u)
      v[u] = *reinterpret_cast<const bf16x8*>(
          x + ((r + u * rows_per_sweep) * G + cg) * 8);
#pragma unroll
    for (int u = 0; u < VEC_UNROLL; ++u) one(r + u * rows_per_sweep, v[u]);
  }
  for (; r < N; r += rows_per_sweep)
    one(r, *reinterpret_cast<const bf16x8*>(x + (r * G + cg) * 8));
}

}  // namespace

static int grid_for(long work, int block) {
  long g = (work + block - 1) / block;
  return (int)std::min<long>(g, 2048);
}

// RAVNEST_GELU_V1=1 keeps the element-stride forward for bf16 with
// H % 8 == 0 too (A/B timing, and the bit-equality test of the column-group
// kernel against it).
static bool gelu_v1() {
  const char* e = std::getenv("RAVNEST_GELU_V1");
  return e && e[0] == '1';
}

static bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// forward through the column-group kernel; false: not applicable
template <bool MX>
static bool bias_gelu_fwd_vec(const at::Tensor& x, const at::Tensor& bias,
                              at::Tensor& y, unsigned char* q,
                              unsigned char* qs) {
  const int H = (int)bias.numel();
  if (gelu_v1() || x.scalar_type() != at::kBFloat16 || (H & 7) ||
      x.numel() == 0 || !aligned16(x) || !aligned16(y))
    return false;
  const int G = H >> 3;
  const long N = x.numel() / H;
  const int blocks = grid_for(N * G, 256);
  const long rows_per_sweep = std::min<long>(N, (long)blocks * 256 / G);
  if (rows_per_sweep == 0) return false;  // a row wider than the grid
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (bias.scalar_type() == at::kFloat)
    hipLaunchKernelGGL((bias_gelu_fwd_vec_kernel<float, MX>), dim3(blocks),
                       dim3(256), 0, stream,
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       bias.data_ptr<float>(),
                       reinterpret_cast<bf16_t*>(y.data_ptr()), N, G,
                       rows_per_sweep, q, qs);
  else
    hipLaunchKernelGGL((bias_gelu_fwd_vec_kernel<bf16_t, MX>), dim3(blocks),
                       dim3(256), 0, stream,
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       reinterpret_cast<const bf16_t*>(bias.data_ptr()),
                       reinterpret_cast<bf16_t*>(y.data_ptr()), N, G,
                       rows_per_sweep, q, qs);
  HIP_CHECK_LAST();
  return true;
}

// x: bf16 or fp32, contiguous; bias: fp32, or bf16 next to a bf16 x, of
// length x.size(-1). The launches below pick a kernel by these two dtypes
// alone, so anything else has to stop here.
static void check_bias_gelu(const at::Tensor& x, const at::Tensor& bias,
                            const char* who) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 1, who,
              ": x must be a contiguous GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 ||
                  x.scalar_type() == at::kFloat,
              who, ": x must be bf16 or fp32");
  TORCH_CHECK(bias.is_cuda() && bias.is_contiguous(), who,
              ": bias must be a contiguous GPU tensor");
  TORCH_CHECK(bias.scalar_type() == at::kFloat ||
                  (bias.scalar_type() == at::kBFloat16 &&
                   x.scalar_type() == at::kBFloat16),
              who, ": bias must be fp32, or bf16 with a bf16 x");
  TORCH_CHECK(bias.numel() >= 1 && x.size(-1) == bias.numel(), who,
              ": bias size mismatch");
}

at::Tensor bias_gelu_fwd(at::Tensor x, at::Tensor bias) {
  check_bias_gelu(x, bias, "bias_gelu_fwd");
  const int H = bias.numel();
  const long n = x.numel();
  auto y = at::empty_like(x);
  if (bias_gelu_fwd_vec<false>(x, bias, y, nullptr, nullptr)) return y;
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  dim3 block(256);
  dim3 grid(grid_for(n / 8 + 1, 256));
  if (x.scalar_type() == at::kBFloat16 && bias.scalar_type() == at::kFloat) {
    hipLaunchKernelGGL((bias_gelu_fwd_kernel<bf16_t, float>), grid, block, 0,
                       stream, reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       bias.data_ptr<float>(),
                       reinterpret_cast<bf16_t*>(y.data_ptr()), n, H);
  } else if (x.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL((bias_gelu_fwd_kernel<bf16_t, bf16_t>), grid, block, 0,
                       stream, reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       reinterpret_cast<const bf16_t*>(bias.data_ptr()),
                       reinterpret_cast<bf16_t*>(y.data_ptr()), n, H);
  } else {
    hipLaunchKernelGGL((bias_gelu_fwd_kernel<float, float>), grid, block, 0,
                       stream, x.data_ptr<float>(), bias.data_ptr<float>(),
                       y.data_ptr<float>(), n, H);
  }
  HIP_CHECK_LAST();
  return y;
}

// bias_gelu_fwd + the MX fp8 quantisation of y: (y, q, s) with y
// bit-identical to bias_gelu_fwd and (q, s) to mx_quant(y).
std::vector<at::Tensor> bias_gelu_mx_fwd(at::Tensor x, at::Tensor bias) {
  check_bias_gelu(x, bias, "bias_gelu_mx_fwd");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16,
              "bias_gelu_mx_fwd: x must be bf16");
  const int H = bias.numel();
  TORCH_CHECK(H % 32 == 0,
              "bias_gelu_mx_fwd: last dim % 32 == 0 required, got ", H);
  const long n = x.numel();
  auto y = at::empty_like(x);
  auto q = at::empty_like(x, x.options().dtype(at::kByte));
  auto s = at::empty({n / H, (long)(H / 32)}, x.options().dtype(at::kByte));
  if (n == 0) return {y, q, s};
  if (bias_gelu_fwd_vec<true>(x, bias, y, q.data_ptr<unsigned char>(),
                              s.data_ptr<unsigned char>()))
    return {y, q, s};
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  dim3 block(256);
  dim3 grid(grid_for(n / 8 + 1, 256));
  if (bias.scalar_type() == at::kFloat) {
    hipLaunchKernelGGL((bias_gelu_fwd_kernel<bf16_t, float, true>), grid,
                       block, 0, stream,
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       bias.data_ptr<float>(),
                       reinterpret_cast<bf16_t*>(y.data_ptr()), n, H,
                       q.data_ptr<unsigned char>(),
                       s.data_ptr<unsigned char>());
  } else {
    hipLaunchKernelGGL((bias_gelu_fwd_kernel<bf16_t, bf16_t, true>), grid,
                       block, 0, stream,
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       reinterpret_cast<const bf16_t*>(bias.data_ptr()),
                       reinterpret_cast<bf16_t*>(y.data_ptr()), n, H,
                       q.data_ptr<unsigned char>(),
                       s.data_ptr<unsigned char>());
  }
  HIP_CHECK_LAST();
  return {y, q, s};
}

at::Tensor bias_gelu_bwd(at::Tensor dy, at::Tensor x, at::Tensor bias) {
  check_bias_gelu(x, bias, "bias_gelu_bwd");
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() &&
                  dy.scalar_type() == x.scalar_type() &&
                  dy.sizes() == x.sizes(),
              "bias_gelu_bwd: dy must match x in dtype and shape");
  const int H = bias.numel();
  const long n = x.numel();
  auto dx = at::empty_like(x);
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  dim3 block(256);
  dim3 grid(grid_for(n / 8 + 1, 256));
  if (x.scalar_type() == at::kBFloat16 && bias.scalar_type() == at::kFloat) {
    hipLaunchKernelGGL((bias_gelu_bwd_kernel<bf16_t, float>), grid, block, 0,
                       stream, reinterpret_cast<const bf16_t*>(dy.data_ptr()),
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       bias.data_ptr<float>(),
                       reinterpret_cast<bf16_t*>(dx.data_ptr()), n, H);
  } else if (x.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL((bias_gelu_bwd_kernel<bf16_t, bf16_t>), grid, block, 0,
                       stream, reinterpret_cast<const bf16_t*>(dy.data_ptr()),
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       reinterpret_cast<const bf16_t*>(bias.data_ptr()),
                       reinterpret_cast<bf16_t*>(dx.data_ptr()), n, H);
  } else {
    hipLaunchKernelGGL((bias_gelu_bwd_kernel<float, float>), grid, block, 0,
                       stream, dy.data_ptr<float>(), x.data_ptr<float>(),
                       bias.data_ptr<float>(), dx.data_ptr<float>(), n, H);
  }
  HIP_CHECK_LAST();
  return dx;
}


std::vector<at::Tensor> bias_gelu_bwd_db(at::Tensor dy, at::Tensor x,
                                         at::Tensor bias) {
  check_bias_gelu(x, bias, "bias_gelu_bwd_db");
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() &&
                  dy.sizes() == x.sizes(),
              "bias_gelu_bwd_db: dy must match x in shape");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 &&
              x.scalar_type() == at::kBFloat16);
  const int H = (int)bias.numel();
  const long N = x.numel() / H;
  auto dx = at::empty_like(dy);
  auto db = at::zeros({H}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int col_blocks = (H + 255) / 256;
  int nchunks = (int)std::min<long>((N + 63) / 64,
                                    std::max(1L, (long)(768 / col_blocks)));
  const long rows_per_chunk = (N + nchunks - 1) / nchunks;
  dim3 grid(col_blocks, nchunks);
  if (bias.scalar_type() == at::kFloat)
    hipLaunchKernelGGL((bias_gelu_bwd_db_kernel<float>), grid, dim3(256), 0,
                       stream,
                       reinterpret_cast<const bf16_t*>(dy.data_ptr()),
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       bias.data_ptr<float>(),
                       reinterpret_cast<bf16_t*>(dx.data_ptr()),
                       db.data_ptr<float>(), H, N, rows_per_chunk);
  else
    hipLaunchKernelGGL((bias_gelu_bwd_db_kernel<bf16_t>), grid, dim3(256), 0,
                       stream,
                       reinterpret_cast<const bf16_t*>(dy.data_ptr()),
                       reinterpret_cast<const bf16_t*>(x.data_ptr()),
                       reinterpret_cast<const bf16_t*>(bias.data_ptr()),
                       reinterpret_cast<bf16_t*>(dx.data_ptr()),
                       db.data_ptr<float>(), H, N, rows_per_chunk);
  HIP_CHECK_LAST();
  return {dx, db};
}

at::Tensor colsum_bf16(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16);
  const int H = x.size(-1);
  const long N = x.numel() / H;
  auto out = at::zeros({H}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int col_blocks = (H + 255) / 256;
  int nchunks = (int)std::min<long>((N + 63) / 64,
                                    std::max(1L, (long)(768 / col_blocks)));
  const long rows_per_chunk = (N + nchunks - 1) / nchunks;
  hipLaunchKernelGGL(colsum_kernel, dim3(col_blocks, nchunks), dim3(256), 0,
                     stream, reinterpret_cast<const bf16_t*>(x.data_ptr()),
                     out.data_ptr<float>(), H, N, rows_per_chunk);
  HIP_CHECK_LAST();
  return out;
}
