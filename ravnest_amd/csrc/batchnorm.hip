// Fused BatchNorm2d (NCHW) forward/backward for CDNA4.
//
// SURVEY.md section 2.3 standalone BN fwd/bwd row (ResNet / Inception /
// CNN workloads). Layout: one block per channel for the reductions
// (contiguous HW runs per (n,c) keep accesses coalesced), elementwise
// grid-stride kernels for the apply passes. fp32 statistics; x in fp32 or
// bf16.
//
// Statistics: ONE read of x, sums of (x - K) and (x - K)^2 with K the
// channel's first element (shifted sums, not Welford). K lies within a few
// sigma of the mean, so var = E[d^2] - E[d]^2 cancels at most a few bits,
// where the unshifted E[x^2] - E[x]^2 loses every bit once |mean| / sigma
// reaches ~2^12 in fp32 (post-ReLU and input-layer channels get there).
// The subtraction itself is exact or within half an ulp of x. (A first
// element k sigma off the mean costs about log2(k^2) bits of the variance.)
//
// Eval mode normalizes with the running statistics, which do not depend
// on x: its backward is dx = dy * w * rstd, without the two batch terms.
//
// The second half of the file fuses the ReLU, and the residual add of a
// ResNet block's tail, into the apply kernels of both directions
// (batchnorm_relu_fwd / batchnorm_relu_bwd).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"

namespace {

template <typename T>
DEVINL float ldb(const T* p);
template <>
DEVINL float ldb<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <>
DEVINL float ldb<float>(const float* p) { return *p; }

template <typename T>
DEVINL void stb(T* p, float v);
template <>
DEVINL void stb<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }
template <>
DEVINL void stb<float>(float* p, float v) { *p = v; }

// per-channel shifted sum + sumsq (one block per channel)
template <typename T>
__global__ void bn_stats_kernel(const T* __restrict__ x,
                                float* __restrict__ mean,
                                float* __restrict__ rstd,
                                float* __restrict__ running_mean,
                                float* __restrict__ running_var,
                                int C, long N, long HW, float eps,
                                float momentum, int update_running) {
  __shared__ float scratch[16];
  const int c = blockIdx.x;
  if (c >= C) return;
  const long cnt = N * HW;
  const float K = ldb(x + (long)c * HW);  // shift: element (n=0, hw=0)
  float s = 0.f, s2 = 0.f;
  for (long i = threadIdx.x; i < cnt; i += blockDim.x) {
    const long n = i / HW, hw = i % HW;
    const float d = ldb(x + (n * C + c) * HW + hw) - K;
    s += d;
    s2 += d * d;
  }
  s = block_sum(s, scratch);
  s2 = block_sum(s2, scratch);
  if (threadIdx.x == 0) {
    const float md = s / cnt;  // mean of the shifted values
    const float mu = K + md;
    const float var = fmaxf(s2 / cnt - md * md, 0.f);
    mean[c] = mu;
    rstd[c] = rsqrtf(var + eps);
    if (update_running) {
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
      // running_var uses the unbiased estimate (torch semantics)
      const float ub = (cnt > 1) ? var * cnt / (cnt - 1) : var;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * ub;
    }
  }
}

template <typename T>
__global__ void bn_apply_kernel(const T* __restrict__ x,
                                const float* __restrict__ mean,
                                const float* __restrict__ rstd,
                                const float* __restrict__ w,
                                const float* __restrict__ b,
                                T* __restrict__ y, int C, long total,
                                long HW) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < total; i += stride) {
    const int c = (int)((i / HW) % C);
    const float v = (ldb(x + i) - mean[c]) * rstd[c] * w[c] + b[c];
    stb(const_cast<T*>(y) + i, v);
  }
}

// per-channel sum(dy) and sum(dy * xhat)
template <typename T>
__global__ void bn_bwd_stats_kernel(const T* __restrict__ dy,
                                    const T* __restrict__ x,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    float* __restrict__ sum_dy,
                                    float* __restrict__ sum_dyxh, int C,
                                    long N, long HW) {
  __shared__ float scratch[16];
  const int c = blockIdx.x;
  if (c >= C) return;
  const long cnt = N * HW;
  const float mu = mean[c], rs = rstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (long i = threadIdx.x; i < cnt; i += blockDim.x) {
    const long n = i / HW, hw = i % HW;
    const long off = (n * C + c) * HW + hw;
    const float g = ldb(dy + off);
    s1 += g;
    s2 += g * (ldb(x + off) - mu) * rs;
  }
  s1 = block_sum(s1, scratch);
  s2 = block_sum(s2, scratch);
  if (threadIdx.x == 0) {
    sum_dy[c] = s1;
    sum_dyxh[c] = s2;
  }
}

template <typename T>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ dy,
                                    const T* __restrict__ x,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    const float* __restrict__ w,
                                    const float* __restrict__ sum_dy,
                                    const float* __restrict__ sum_dyxh,
                                    T* __restrict__ dx, int C, long total,
                                    long HW, long cnt, int training) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < total; i += stride) {
    const int c = (int)((i / HW) % C);
    const float xh = (ldb(x + i) - mean[c]) * rstd[c];
    const float g = ldb(dy + i);
    // eval: mean/rstd are constants of x, the batch terms vanish
    const float d = w[c] * rstd[c] *
        (training ? g - sum_dy[c] / cnt - xh * sum_dyxh[c] / cnt : g);
    stb(const_cast<T*>(dx) + i, d);
  }
}

int bn_grid(long total) {
  return (int)std::min<long>((total + 255) / 256, 2048);
}

// ---- BatchNorm + [residual add] + ReLU -------------------------------
//
// y = relu(bn(x)) or y = relu(bn(x) + r), results identical to the composed
// bn_apply_kernel -> torch add -> torch relu. The statistics come from
// bn_stats_kernel above; the backward reads the ReLU mask from the saved
// output y (g = y <= 0 ? 0 : dy, as threshold_backward does) and reduces
// with the thread mapping and accumulation order of bn_bwd_stats_kernel,
// so dgamma, dbeta and dx are the composed path's bit for bit.
//
// The two elementwise kernels move 16 bytes per lane (4 fp32 / 8 bf16) when
// HW is a multiple of that width: a vector then lies inside one (n, c)
// plane and the per-channel constants are read once per vector.

constexpr int BNR_BLOCK = 256;
constexpr int BNR_GRID_CAP = 2048;

int bnr_grid(long work) {
  return (int)std::min<long>((work + BNR_BLOCK - 1) / BNR_BLOCK,
                             BNR_GRID_CAP);
}

// the expression of bn_apply_kernel: same operations, same order
DEVINL float bn_norm(float x, float mu, float rs, float w, float b) {
  return (x - mu) * rs * w + b;
}

// the value a float takes once it is stored as T
template <typename T>
DEVINL float rnd(float v);
template <>
DEVINL float rnd<bf16_t>(float v) { return bf2f(f2bf(v)); }
template <>
DEVINL float rnd<float>(float v) { return v; }

// NaN compares false and passes through, as in torch
DEVINL float relu(float v) { return v <= 0.f ? 0.f : v; }
// threshold_backward: a select, so an infinite dy under a dead y gives 0
DEVINL float relu_grad(float y, float dy) { return y <= 0.f ? 0.f : dy; }

// V contiguous elements of T as floats; V * sizeof(T) == 16 moves one
// 16-byte access, V == 1 one element
template <typename T, int V>
struct Pack {
  float v[V];
};

template <typename T, int V>
DEVINL Pack<T, V> ld_pack(const T* p) {
  Pack<T, V> r;
  if constexpr (V == 1) {
    r.v[0] = ldb(p);
  } else if constexpr (sizeof(T) == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = q[j];
  } else {
    const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) r.v[j] = us2f((unsigned short)q[j]);
  }
  return r;
}

// values must already be representable in T (rnd<T> applied)
template <typename T, int V>
DEVINL void st_pack(T* p, const Pack<T, V>& r) {
  if constexpr (V == 1) {
    stb(p, r.v[0]);
  } else if constexpr (sizeof(T) == 4) {
    f32x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = r.v[j];
    *reinterpret_cast<f32x4*>(p) = q;
  } else {
    bf16x8 q;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      q[j] = (short)(__builtin_bit_cast(unsigned int, r.v[j]) >> 16);
    *reinterpret_cast<bf16x8*>(p) = q;
  }
}

// nwork = total / V packs; total % V == 0 and HW % V == 0 (host-checked)
template <typename T, int V, bool RES>
__global__ void bn_relu_apply_kernel(const T* __restrict__ x,
                                     const T* __restrict__ r,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     const float* __restrict__ w,
                                     const float* __restrict__ b,
                                     T* __restrict__ y, int C, long nwork,
                                     long HW) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long k = i0; k < nwork; k += stride) {
    const long i = k * V;
    const int c = (int)((i / HW) % C);
    const float mu = mean[c], rs = rstd[c], wc = w[c], bc = b[c];
    const Pack<T, V> px = ld_pack<T, V>(x + i);
    Pack<T, V> pr, py;
    if constexpr (RES) pr = ld_pack<T, V>(r + i);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      // the composed path stores bn(x) as T, then stores the sum as T
      float v = rnd<T>(bn_norm(px.v[j], mu, rs, wc, bc));
      if constexpr (RES) v = rnd<T>(v + pr.v[j]);
      py.v[j] = relu(v);
    }
    st_pack<T, V>(y + i, py);
  }
}

// per-channel sum(g) and sum(g * xhat), g = relu_grad(y, dy): the loop of
// bn_bwd_stats_kernel with g formed in registers
template <typename T>
__global__ void bn_relu_bwd_stats_kernel(const T* __restrict__ dy,
                                         const T* __restrict__ y,
                                         const T* __restrict__ x,
                                         const float* __restrict__ mean,
                                         const float* __restrict__ rstd,
                                         float* __restrict__ sum_dy,
                                         float* __restrict__ sum_dyxh, int C,
                                         long N, long HW) {
  __shared__ float scratch[16];
  const int c = blockIdx.x;
  if (c >= C) return;
  const long cnt = N * HW;
  const float mu = mean[c], rs = rstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (long i = threadIdx.x; i < cnt; i += blockDim.x) {
    const long n = i / HW, hw = i % HW;
    const long off = (n * C + c) * HW + hw;
    const float g = relu_grad(ldb(y + off), ldb(dy + off));
    s1 += g;
    s2 += g * (ldb(x + off) - mu) * rs;
  }
  s1 = block_sum(s1, scratch);
  s2 = block_sum(s2, scratch);
  if (threadIdx.x == 0) {
    sum_dy[c] = s1;
    sum_dyxh[c] = s2;
  }
}

// dx as bn_bwd_apply_kernel computes it from g; DR also writes g itself,
// the gradient of the residual, to a tensor of its own
template <typename T, int V, bool DR>
__global__ void bn_relu_bwd_apply_kernel(const T* __restrict__ dy,
                                         const T* __restrict__ y,
                                         const T* __restrict__ x,
                                         const float* __restrict__ mean,
                                         const float* __restrict__ rstd,
                                         const float* __restrict__ w,
                                         const float* __restrict__ sum_dy,
                                         const float* __restrict__ sum_dyxh,
                                         T* __restrict__ dx,
                                         T* __restrict__ dr, int C,
                                         long nwork, long HW, long cnt,
                                         int training) {
  const long i0 = (long)(blockIdx.x * blockDim.x + threadIdx.x);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long k = i0; k < nwork; k += stride) {
    const long i = k * V;
    const int c = (int)((i / HW) % C);
    const float mu = mean[c], rs = rstd[c], wc = w[c];
    const float sdy = sum_dy[c], sdyxh = sum_dyxh[c];
    const Pack<T, V> pdy = ld_pack<T, V>(dy + i);
    const Pack<T, V> py = ld_pack<T, V>(y + i);
    const Pack<T, V> px = ld_pack<T, V>(x + i);
    Pack<T, V> pdx, pg;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xh = (px.v[j] - mu) * rs;
      const float g = relu_grad(py.v[j], pdy.v[j]);
      // eval: mean/rstd are constants of x, the batch terms vanish
      const float d = wc * rs *
          (training ? g - sdy / cnt - xh * sdyxh / cnt : g);
      pdx.v[j] = rnd<T>(d);
      pg.v[j] = g;  // 0 or dy: already a T
    }
    st_pack<T, V>(dx + i, pdx);
    if constexpr (DR) st_pack<T, V>(dr + i, pg);
  }
}

bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

std::vector<at::Tensor> batchnorm_fwd(at::Tensor x, at::Tensor w,
                                      at::Tensor b, at::Tensor running_mean,
                                      at::Tensor running_var, bool training,
                                      double momentum, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4);
  TORCH_CHECK(x.scalar_type() == at::kFloat ||
                  x.scalar_type() == at::kBFloat16,
              "batchnorm_fwd: x must be float32 or bfloat16, got ",
              x.scalar_type());
  TORCH_CHECK(w.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat);
  TORCH_CHECK(running_mean.scalar_type() == at::kFloat &&
                  running_var.scalar_type() == at::kFloat,
              "batchnorm_fwd: running statistics must be float32");
  const long N = x.size(0), HW = x.size(2) * x.size(3);
  const int C = x.size(1);
  auto y = at::empty_like(x);
  auto mean = at::empty({C}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({C}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const long total = x.numel();

#define BN_FWD(T)                                                           \
  do {                                                                      \
    if (training) {                                                         \
      hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(C), dim3(256), 0,       \
                         stream, reinterpret_cast<const T*>(x.data_ptr()),  \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),    \
                         running_mean.data_ptr<float>(),                    \
                         running_var.data_ptr<float>(), C, N, HW,           \
                         (float)eps, (float)momentum, 1);                   \
    } else {                                                                \
      mean.copy_(running_mean);                                             \
      rstd.copy_((running_var + eps).rsqrt());                              \
    }                                                                       \
    hipLaunchKernelGGL((bn_apply_kernel<T>), dim3(bn_grid(total)),          \
                       dim3(256), 0, stream,                                \
                       reinterpret_cast<const T*>(x.data_ptr()),            \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),      \
                       w.data_ptr<float>(), b.data_ptr<float>(),            \
                       reinterpret_cast<T*>(y.data_ptr()), C, total, HW);   \
  } while (0)

  if (x.scalar_type() == at::kBFloat16) {
    BN_FWD(bf16_t);
  } else {
    BN_FWD(float);
  }
  HIP_CHECK_LAST();
  return {y, mean, rstd};
}

std::vector<at::Tensor> batchnorm_bwd(at::Tensor dy, at::Tensor x,
                                      at::Tensor w, at::Tensor mean,
                                      at::Tensor rstd, bool training) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kFloat ||
                  x.scalar_type() == at::kBFloat16,
              "batchnorm_bwd: x must be float32 or bfloat16, got ",
              x.scalar_type());
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && dy.sizes() == x.sizes(),
              "batchnorm_bwd: dy must match x");
  TORCH_CHECK(w.scalar_type() == at::kFloat &&
              mean.scalar_type() == at::kFloat &&
              rstd.scalar_type() == at::kFloat);
  const long N = x.size(0), HW = x.size(2) * x.size(3);
  const int C = x.size(1);
  const long total = x.numel();
  const long cnt = N * HW;
  auto dx = at::empty_like(x);
  auto sum_dy = at::empty({C}, x.options().dtype(at::kFloat));
  auto sum_dyxh = at::empty({C}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();

#define BN_BWD(T)                                                           \
  do {                                                                      \
    hipLaunchKernelGGL((bn_bwd_stats_kernel<T>), dim3(C), dim3(256), 0,     \
                       stream, reinterpret_cast<const T*>(dy.data_ptr()),   \
                       reinterpret_cast<const T*>(x.data_ptr()),            \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),      \
                       sum_dy.data_ptr<float>(),                            \
                       sum_dyxh.data_ptr<float>(), C, N, HW);               \
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(bn_grid(total)),      \
                       dim3(256), 0, stream,                                \
                       reinterpret_cast<const T*>(dy.data_ptr()),           \
                       reinterpret_cast<const T*>(x.data_ptr()),            \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),      \
                       w.data_ptr<float>(), sum_dy.data_ptr<float>(),       \
                       sum_dyxh.data_ptr<float>(),                          \
                       reinterpret_cast<T*>(dx.data_ptr()), C, total, HW,   \
                       cnt, training ? 1 : 0);                              \
  } while (0)

  if (x.scalar_type() == at::kBFloat16) {
    BN_BWD(bf16_t);
  } else {
    BN_BWD(float);
  }
  HIP_CHECK_LAST();
  // dw = sum_dyxh, db = sum_dy (already per-channel)
  return {dx, sum_dyxh, sum_dy};
}

// launch constants of the two BN+ReLU elementwise kernels: one grid-stride
// trip covers grid_cap * block * (16 / element size) elements
std::vector<int64_t> batchnorm_relu_launch_constants() {
  return {BNR_GRID_CAP, BNR_BLOCK, 16};
}

// y = relu(bn(x)) or, with a residual, y = relu(bn(x) + residual)
std::vector<at::Tensor> batchnorm_relu_fwd(
    at::Tensor x, c10::optional<at::Tensor> residual, at::Tensor w,
    at::Tensor b, at::Tensor running_mean, at::Tensor running_var,
    bool training, double momentum, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4);
  TORCH_CHECK(x.scalar_type() == at::kFloat ||
                  x.scalar_type() == at::kBFloat16,
              "batchnorm_relu_fwd: x must be float32 or bfloat16, got ",
              x.scalar_type());
  TORCH_CHECK(w.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat);
  TORCH_CHECK(running_mean.scalar_type() == at::kFloat &&
                  running_var.scalar_type() == at::kFloat,
              "batchnorm_relu_fwd: running statistics must be float32");
  const bool has_res = residual.has_value();
  if (has_res) {
    TORCH_CHECK(residual->is_cuda() && residual->is_contiguous() &&
                    residual->scalar_type() == x.scalar_type() &&
                    residual->sizes() == x.sizes(),
                "batchnorm_relu_fwd: residual must match x in shape and "
                "dtype");
  }
  const long N = x.size(0), HW = x.size(2) * x.size(3);
  const int C = x.size(1);
  TORCH_CHECK(w.numel() == C && b.numel() == C &&
              running_mean.numel() == C && running_var.numel() == C);
  auto y = at::empty_like(x);
  auto mean = at::empty({C}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({C}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const long total = x.numel();
  const long vec = 16 / (long)x.element_size();
  const bool wide = HW % vec == 0 && aligned16(x) && aligned16(y) &&
                    (!has_res || aligned16(*residual));
  const void* rp = has_res ? residual->data_ptr() : nullptr;

#define BNR_APPLY(T, V, RES)                                                \
  hipLaunchKernelGGL((bn_relu_apply_kernel<T, V, RES>),                     \
                     dim3(bnr_grid(total / V)), dim3(BNR_BLOCK), 0, stream, \
                     reinterpret_cast<const T*>(x.data_ptr()),              \
                     reinterpret_cast<const T*>(rp),                        \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),        \
                     w.data_ptr<float>(), b.data_ptr<float>(),              \
                     reinterpret_cast<T*>(y.data_ptr()), C, total / V, HW)

#define BNR_FWD(T, VW)                                                      \
  do {                                                                      \
    if (training) {                                                         \
      hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(C), dim3(256), 0,       \
                         stream, reinterpret_cast<const T*>(x.data_ptr()),  \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),    \
                         running_mean.data_ptr<float>(),                    \
                         running_var.data_ptr<float>(), C, N, HW,           \
                         (float)eps, (float)momentum, 1);                   \
    } else {                                                                \
      mean.copy_(running_mean);                                             \
      rstd.copy_((running_var + eps).rsqrt());                              \
    }                                                                       \
    if (wide) {                                                             \
      if (has_res) BNR_APPLY(T, VW, true);                                  \
      else BNR_APPLY(T, VW, false);                                         \
    } else {                                                                \
      if (has_res) BNR_APPLY(T, 1, true);                                   \
      else BNR_APPLY(T, 1, false);                                          \
    }                                                                       \
  } while (0)

  if (total > 0) {
    if (x.scalar_type() == at::kBFloat16) {
      BNR_FWD(bf16_t, 8);
    } else {
      BNR_FWD(float, 4);
    }
  }
  HIP_CHECK_LAST();
  return {y, mean, rstd};
}

// returns {dx, dw, db} and, with want_dr, the residual's gradient as a
// fourth tensor of its own storage
std::vector<at::Tensor> batchnorm_relu_bwd(at::Tensor dy, at::Tensor x,
                                           at::Tensor y, at::Tensor w,
                                           at::Tensor mean, at::Tensor rstd,
                                           bool training, bool want_dr) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && x.is_contiguous() &&
              y.is_contiguous() && x.dim() == 4);
  TORCH_CHECK(x.scalar_type() == at::kFloat ||
                  x.scalar_type() == at::kBFloat16,
              "batchnorm_relu_bwd: x must be float32 or bfloat16, got ",
              x.scalar_type());
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() &&
                  dy.sizes() == x.sizes() &&
                  y.scalar_type() == x.scalar_type() &&
                  y.sizes() == x.sizes(),
              "batchnorm_relu_bwd: dy and y must match x");
  TORCH_CHECK(w.scalar_type() == at::kFloat &&
              mean.scalar_type() == at::kFloat &&
              rstd.scalar_type() == at::kFloat);
  const long N = x.size(0), HW = x.size(2) * x.size(3);
  const int C = x.size(1);
  TORCH_CHECK(w.numel() == C && mean.numel() == C && rstd.numel() == C);
  const long total = x.numel();
  const long cnt = N * HW;
  auto dx = at::empty_like(x);
  at::Tensor dr;
  if (want_dr) dr = at::empty_like(x);
  auto sum_dy = at::empty({C}, x.options().dtype(at::kFloat));
  auto sum_dyxh = at::empty({C}, x.options().dtype(at::kFloat));
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const long vec = 16 / (long)x.element_size();
  const bool wide = HW % vec == 0 && aligned16(dy) && aligned16(x) &&
                    aligned16(y) && aligned16(dx) &&
                    (!want_dr || aligned16(dr));
  void* drp = want_dr ? dr.data_ptr() : nullptr;

#define BNR_BWD_APPLY(T, V, DR)                                             \
  hipLaunchKernelGGL((bn_relu_bwd_apply_kernel<T, V, DR>),                  \
                     dim3(bnr_grid(total / V)), dim3(BNR_BLOCK), 0, stream, \
                     reinterpret_cast<const T*>(dy.data_ptr()),             \
                     reinterpret_cast<const T*>(y.data_ptr()),              \
                     reinterpret_cast<const T*>(x.data_ptr()),              \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),        \
                     w.data_ptr<float>(), sum_dy.data_ptr<float>(),         \
                     sum_dyxh.data_ptr<float>(),                            \
                     reinterpret_cast<T*>(dx.data_ptr()),                   \
                     reinterpret_cast<T*>(drp), C, total / V, HW, cnt,      \
                     training ? 1 : 0)

#define BNR_BWD(T, VW)                                                      \
  do {                                                                      \
    hipLaunchKernelGGL((bn_relu_bwd_stats_kernel<T>), dim3(C), dim3(256),   \
                       0, stream,                                           \
                       reinterpret_cast<const T*>(dy.data_ptr()),           \
                       reinterpret_cast<const T*>(y.data_ptr()),            \
                       reinterpret_cast<const T*>(x.data_ptr()),            \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),      \
                       sum_dy.data_ptr<float>(),                            \
                       sum_dyxh.data_ptr<float>(), C, N, HW);               \
    if (wide) {                                                             \
      if (want_dr) BNR_BWD_APPLY(T, VW, true);                              \
      else BNR_BWD_APPLY(T, VW, false);                                     \
    } else {                                                                \
      if (want_dr) BNR_BWD_APPLY(T, 1, true);                               \
      else BNR_BWD_APPLY(T, 1, false);                                      \
    }                                                                       \
  } while (0)

  if (total > 0) {
    if (x.scalar_type() == at::kBFloat16) {
      BNR_BWD(bf16_t, 8);
    } else {
      BNR_BWD(float, 4);
    }
  } else {
    sum_dy.zero_();
    sum_dyxh.zero_();
  }
  HIP_CHECK_LAST();
  // dw = sum_dyxh, db = sum_dy (already per-channel)
  std::vector<at::Tensor> out = {dx, sum_dyxh, sum_dy};
  if (want_dr) out.push_back(dr);
  return out;
}
