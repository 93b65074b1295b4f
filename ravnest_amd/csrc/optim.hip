// Fused multi-tensor optimizers (Adam / SGD+momentum / LAMB) for CDNA4.
//
// ONE kernel launch applies the update across every parameter tensor
// (apex-style chunking: host builds a chunk table, each 256-thread block
// owns one chunk) — SURVEY.md section 2.3 "fused multi-tensor apply
// kernels (one launch per bucket), incl. LAMB trust-ratio".
//
// Two parameter modes:
//  * fp32 params + fp32 grads (CPU-parity training)
//  * bf16 params + bf16 grads with an fp32 MASTER copy in optimizer
//    state (the MI355X-native mode: bf16 weights halve HBM traffic for
//    every GEMM; the master preserves convergence).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <vector>

#include "common.h"

namespace {

constexpr int CHUNK = 1 << 16;

struct Chunk {
  void* p;        // param (fp32 or bf16)
  void* g;        // grad  (same dtype as p)
  float* m;
  float* v;
  float* master;  // fp32 master (bf16 mode) or nullptr
  int n;
  int tensor_idx;
};

template <typename T>
DEVINL float ldv(const void* p, int i) {
  if constexpr (sizeof(T) == 2)
    return bf2f(reinterpret_cast<const bf16_t*>(p)[i]);
  else
    return reinterpret_cast<const float*>(p)[i];
}

template <typename T>
DEVINL void stv(void* p, int i, float v) {
  if constexpr (sizeof(T) == 2)
    reinterpret_cast<bf16_t*>(p)[i] = f2bf(v);
  else
    reinterpret_cast<float*>(p)[i] = v;
}

// global-norm clip coefficient applied to a gradient as it is loaded.
// The product is made opaque to the optimizer (an empty asm, no
// instruction): the compiler then contracts the arithmetic that follows
// (g + wd*p -> fma) exactly as it does for an unscaled gradient, instead
// of fusing or packing the scale into it. A coefficient of exactly 1 thus
// reproduces the unclipped update bit for bit.
DEVINL float gscaled(float g, float s) {
  float r = g * s;
  asm("" : "+v"(r));
  return r;
}

template <typename T>
DEVINL void adam_one(float& p, float g, float& m, float& v, float lr,
                     float b1, float b2, float eps, float wd, float bc1,
                     float bc2) {
  if (wd != 0.f) g += wd * p;
  m = b1 * m + (1.f - b1) * g;
  v = b2 * v + (1.f - b2) * g * g;
  p -= lr * (m / bc1) / (sqrtf(v / bc2) + eps);
}

// vectorized: 4 elements/thread/iter with 16-byte fp32 state accesses
// (m/v/master are the traffic; chunks are 64Ki elements so the body is
// always aligned and the tail only exists in the last chunk)
template <typename T, bool CLIP>
__global__ void adam_mt_kernel(const Chunk* __restrict__ chunks, float lr,
                               float b1, float b2, float eps, float wd,
                               float bc1, float bc2,
                               const float* __restrict__ lr_buf,
                               const long long* __restrict__ step_buf,
                               const float* __restrict__ gscale) {
  // hipGraph-capturable mode: lr and the bias-correction step come from
  // DEVICE buffers so replays see live values (host scalars would
  // freeze at capture — engine/graphstep.py)
  if (lr_buf) {
    lr = *lr_buf;
    const float st = (float)*step_buf;
    bc1 = 1.f - __powf(b1, st);
    bc2 = 1.f - __powf(b2, st);
  }
  // clip-by-global-norm coefficient (grad_norm_finalize_kernel). CLIP is
  // a template flag, not a runtime branch, so that the no-clip
  // instantiation (null gscale) carries no instruction of the option
  float gs = 1.f;
  if constexpr (CLIP) gs = *gscale;
  const Chunk c = chunks[blockIdx.x];
  const int n4 = c.n >> 2;
  float4* m4 = reinterpret_cast<float4*>(c.m);
  float4* v4 = reinterpret_cast<float4*>(c.v);
  float4* w4 = reinterpret_cast<float4*>(c.master);
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 m = m4[i], v = v4[i];
    float4 p;
    float g[4];
    if constexpr (sizeof(T) == 2) {
      unsigned long long graw =
          reinterpret_cast<const unsigned long long*>(c.g)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        g[j] = us2f((unsigned short)(graw >> (16 * j)));
      p = w4[i];
    } else {
      const float4 gv = reinterpret_cast<const float4*>(c.g)[i];
      g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
      p = reinterpret_cast<const float4*>(c.p)[i];
    }
    if constexpr (CLIP) {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = gscaled(g[j], gs);
    }
    adam_one<T>(p.x, g[0], m.x, v.x, lr, b1, b2, eps, wd, bc1, bc2);
    adam_one<T>(p.y, g[1], m.y, v.y, lr, b1, b2, eps, wd, bc1, bc2);
    adam_one<T>(p.z, g[2], m.z, v.z, lr, b1, b2, eps, wd, bc1, bc2);
    adam_one<T>(p.w, g[3], m.w, v.w, lr, b1, b2, eps, wd, bc1, bc2);
    m4[i] = m;
    v4[i] = v;
    if constexpr (sizeof(T) == 2) {
      w4[i] = p;
      unsigned long long praw =
          ((unsigned long long)f2us(p.x)) |
          ((unsigned long long)f2us(p.y) << 16) |
          ((unsigned long long)f2us(p.z) << 32) |
          ((unsigned long long)f2us(p.w) << 48);
      reinterpret_cast<unsigned long long*>(c.p)[i] = praw;
    } else {
      reinterpret_cast<float4*>(c.p)[i] = p;
    }
  }
  // scalar tail
  for (int i = (n4 << 2) + threadIdx.x; i < c.n; i += blockDim.x) {
    float g = ldv<T>(c.g, i);
    if constexpr (CLIP) g = gscaled(g, gs);
    float p = c.master ? c.master[i] : ldv<T>(c.p, i);
    float m = c.m[i], v = c.v[i];
    adam_one<T>(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2);
    c.m[i] = m;
    c.v[i] = v;
    if (c.master) c.master[i] = p;
    stv<T>(c.p, i, p);
  }
}

template <typename T, bool CLIP>
__global__ void sgd_mt_kernel(const Chunk* __restrict__ chunks, float lr,
                              float momentum, float wd, int nesterov,
                              const float* __restrict__ gscale) {
  float gs = 1.f;
  if constexpr (CLIP) gs = *gscale;
  const Chunk c = chunks[blockIdx.x];
  for (int i = threadIdx.x; i < c.n; i += blockDim.x) {
    float g = ldv<T>(c.g, i);
    if constexpr (CLIP) g = gscaled(g, gs);
    float p = c.master ? c.master[i] : ldv<T>(c.p, i);
    if (wd != 0.f) g += wd * p;
    if (momentum != 0.f) {
      float b = c.m[i] = momentum * c.m[i] + g;
      g = nesterov ? g + momentum * b : b;
    }
    p -= lr * g;
    if (c.master) c.master[i] = p;
    stv<T>(c.p, i, p);
  }
}

// LAMB phase 1: update m/v, accumulate ||w||^2 and ||update||^2 per tensor
template <typename T, bool CLIP>
__global__ void lamb_phase1_kernel(const Chunk* __restrict__ chunks,
                                   float* __restrict__ norms,  // [T][2]
                                   float b1, float b2, float eps, float wd,
                                   float bc1, float bc2,
                                   const float* __restrict__ gscale) {
  __shared__ float scratch[16];
  float gs = 1.f;
  if constexpr (CLIP) gs = *gscale;
  const Chunk c = chunks[blockIdx.x];
  float wsq = 0.f, usq = 0.f;
  for (int i = threadIdx.x; i < c.n; i += blockDim.x) {
    float g = ldv<T>(c.g, i);
    if constexpr (CLIP) g = gscaled(g, gs);
    float p = c.master ? c.master[i] : ldv<T>(c.p, i);
    float m = c.m[i] = b1 * c.m[i] + (1.f - b1) * g;
    float v = c.v[i] = b2 * c.v[i] + (1.f - b2) * g * g;
    float upd = (m / bc1) / (sqrtf(v / bc2) + eps);
    if (wd != 0.f) upd += wd * p;
    wsq += p * p;
    usq += upd * upd;
  }
  wsq = block_sum(wsq, scratch);
  usq = block_sum(usq, scratch);
  if (threadIdx.x == 0) {
    atomicAdd(&norms[c.tensor_idx * 2 + 0], wsq);
    atomicAdd(&norms[c.tensor_idx * 2 + 1], usq);
  }
}

template <typename T>
__global__ void lamb_phase2_kernel(const Chunk* __restrict__ chunks,
                                   const float* __restrict__ norms, float lr,
                                   float b1, float b2, float eps, float wd,
                                   float bc1, float bc2, float clamp_trust) {
  const Chunk c = chunks[blockIdx.x];
  const float wn = sqrtf(norms[c.tensor_idx * 2 + 0]);
  const float un = sqrtf(norms[c.tensor_idx * 2 + 1]);
  float trust = 1.f;
  if (wn > 0.f && un > 0.f) trust = fminf(wn / un, clamp_trust);
  const float step = lr * trust;
  for (int i = threadIdx.x; i < c.n; i += blockDim.x) {
    float m = c.m[i], v = c.v[i];
    float p = c.master ? c.master[i] : ldv<T>(c.p, i);
    float upd = (m / bc1) / (sqrtf(v / bc2) + eps);
    if (wd != 0.f) upd += wd * p;
    p -= step * upd;
    if (c.master) c.master[i] = p;
    stv<T>(c.p, i, p);
  }
}

// ---- global-norm gradient clipping ---------------------------------
// sum of squares of one chunk's gradients -> partials[blockIdx.x]. One
// plain store per block and a fixed summation order (no float atomics):
// the norm is bit-reproducible run to run. 16-byte loads (8 bf16 / 4 fp32
// per lane per iteration) with one fp32 accumulator per vector slot, so a
// lane adds at most 64 terms serially per accumulator on a full chunk.
// A chunk whose base is not 16-byte aligned (a grad that is a view into
// a larger buffer) takes the scalar path.
template <typename T>
__global__ void grad_sqnorm_mt_kernel(const Chunk* __restrict__ chunks,
                                      float* __restrict__ partials) {
  __shared__ float scratch[16];
  constexpr int VEC = 16 / (int)sizeof(T);
  const Chunk c = chunks[blockIdx.x];
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  int done = 0;
  if ((reinterpret_cast<unsigned long long>(c.g) & 15ull) == 0) {
    const int nv = c.n / VEC;
#pragma unroll 4
    for (int i = threadIdx.x; i < nv; i += blockDim.x) {
      if constexpr (sizeof(T) == 2) {
        const bf16x8 raw = reinterpret_cast<const bf16x8*>(c.g)[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float g = us2f((unsigned short)raw[j]);
          acc[j] += g * g;
        }
      } else {
        const f32x4 raw = reinterpret_cast<const f32x4*>(c.g)[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += raw[j] * raw[j];
      }
    }
    done = nv * VEC;
  }
  // scalar tail (n % VEC) or the whole misaligned chunk
  for (int i = done + threadIdx.x; i < c.n; i += blockDim.x) {
    const float g = ldv<T>(c.g, i);
    acc[0] += g * g;
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) s += acc[j];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one block: fixed-order sum of the per-chunk partials, then
//   stats[0] = ||g||_2 (before clipping)
//   stats[1] = min(1, max_norm / (norm + 1e-6))   (torch clip_grad_norm_)
//   stats[2] += 1 when the norm is not finite
// max_norm comes from a device scalar when one is given, so a hipGraph
// replay sees the live value. A NaN coefficient stays NaN, as torch's
// clamp leaves it (error_if_nonfinite=False behaviour).
__global__ void grad_norm_finalize_kernel(const float* __restrict__ partials,
                                          int n,
                                          const float* __restrict__ max_norm_buf,
                                          float max_norm,
                                          float* __restrict__ stats) {
  __shared__ float scratch[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) {
    if (max_norm_buf) max_norm = *max_norm_buf;
    const float norm = sqrtf(acc);
    float coef = max_norm / (norm + 1e-6f);
    if (coef > 1.f) coef = 1.f;
    stats[0] = norm;
    stats[1] = coef;
    if (!isfinite(norm)) stats[2] += 1.f;
  }
}

// in-place multi-tensor g *= *gscale (standalone clip_grad_norm_). A
// coefficient of exactly 1 leaves memory untouched.
template <typename T>
__global__ void scale_mt_kernel(const Chunk* __restrict__ chunks,
                                const float* __restrict__ gscale) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const float gs = *gscale;
  if (gs == 1.f) return;
  const Chunk c = chunks[blockIdx.x];
  int done = 0;
  if ((reinterpret_cast<unsigned long long>(c.g) & 15ull) == 0) {
    const int nv = c.n / VEC;
    for (int i = threadIdx.x; i < nv; i += blockDim.x) {
      if constexpr (sizeof(T) == 2) {
        bf16x8 raw = reinterpret_cast<const bf16x8*>(c.g)[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          raw[j] = (short)f2us(us2f((unsigned short)raw[j]) * gs);
        reinterpret_cast<bf16x8*>(c.g)[i] = raw;
      } else {
        f32x4 raw = reinterpret_cast<const f32x4*>(c.g)[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j) raw[j] *= gs;
        reinterpret_cast<f32x4*>(c.g)[i] = raw;
      }
    }
    done = nv * VEC;
  }
  for (int i = done + threadIdx.x; i < c.n; i += blockDim.x)
    stv<T>(c.g, i, ldv<T>(c.g, i) * gs);
}

// one record per chunk of fused_copy: tensors of 2- and 4-byte elements
// may share a launch, so the element size travels with the chunk
struct CopyRec {
  const void* src;
  void* dst;
  int n;      // elements in this chunk
  int esize;  // 2 or 4
};

// multi-tensor device copy: ONE launch clones every parameter into its
// snapshot slot (the versioning engine's per-step param snapshot was ~200
// separate hipMemcpy calls — SURVEY.md section 2.3 "multi-tensor
// clone/copy kernels ... versioned weight arena"). Per chunk a 16-byte
// vector body, which assumes 16-byte aligned tensor bases, then a scalar
// tail.
__global__ void copy_mt_kernel(const CopyRec* __restrict__ recs) {
  const CopyRec c = recs[blockIdx.x];
  if (c.esize == 2) {
    const int n4 = c.n >> 3;  // 16B groups of 8 bf16
    const ulong2* src = reinterpret_cast<const ulong2*>(c.src);
    ulong2* dst = reinterpret_cast<ulong2*>(c.dst);
    for (int i = threadIdx.x; i < n4; i += blockDim.x) dst[i] = src[i];
    for (int i = (n4 << 3) + threadIdx.x; i < c.n; i += blockDim.x)
      reinterpret_cast<bf16_t*>(c.dst)[i] =
          reinterpret_cast<const bf16_t*>(c.src)[i];
  } else {
    const int n4 = c.n >> 2;
    const float4* src = reinterpret_cast<const float4*>(c.src);
    float4* dst = reinterpret_cast<float4*>(c.dst);
    for (int i = threadIdx.x; i < n4; i += blockDim.x) dst[i] = src[i];
    for (int i = (n4 << 2) + threadIdx.x; i < c.n; i += blockDim.x)
      reinterpret_cast<float*>(c.dst)[i] =
          reinterpret_cast<const float*>(c.src)[i];
  }
}

// ---- host side ---------------------------------------------------------
// emit(offset, count) for every CHUNK-sized piece of an n-element tensor
template <typename F>
void for_each_chunk(long n, F&& emit) {
  for (long off = 0; off < n; off += CHUNK)
    emit(off, (int)std::min<long>(CHUNK, n - off));
}

// chunk records -> device byte tensor. The copy blocks, so the host vector
// may die when this returns; no records give an empty tensor.
template <typename Rec>
at::Tensor upload(const std::vector<Rec>& recs, const at::Device& device) {
  const auto bytes = at::TensorOptions().dtype(at::kByte);
  if (recs.empty()) return at::empty({0}, bytes.device(device));
  return at::from_blob(const_cast<Rec*>(recs.data()),
                       {(long)(recs.size() * sizeof(Rec))}, bytes)
      .to(device);
}

// one 256-thread block per chunk record, on the current stream
template <typename... Params, typename... Args>
void launch_mt(void (*kernel)(Params...), long nblocks, Args... args) {
  hipLaunchKernelGGL(
      kernel, dim3((int)nblocks), dim3(256), 0,
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(), args...);
  HIP_CHECK_LAST();
}

inline const Chunk* table_ptr(const at::Tensor& table) {
  return reinterpret_cast<const Chunk*>(table.data_ptr());
}

// &stats[1]: the clip coefficient written by grad_norm_finalize_kernel
inline const float* gscale_ptr(const c10::optional<at::Tensor>& gstats) {
  if (!gstats.has_value()) return nullptr;
  const at::Tensor& s = *gstats;
  TORCH_CHECK(s.is_cuda() && s.scalar_type() == at::kFloat &&
                  s.is_contiguous() && s.numel() >= 3,
              "grad-norm stats must be a device fp32 tensor of 3");
  return s.data_ptr<float>() + 1;
}

inline void check_table(const at::Tensor& table, long nchunks, long esize) {
  TORCH_CHECK(table.is_cuda() && nchunks > 0 &&
                  table.numel() == nchunks * (long)sizeof(Chunk),
              "chunk table / nchunks mismatch");
  TORCH_CHECK(esize == 2 || esize == 4, "esize must be 2 or 4");
}

// the one dtype x clip dispatch: calls f(Elem<T>{}, bool_constant<CLIP>{})
// with T picked by esize (2 = bf16, 4 = fp32). Kernel families without a
// CLIP parameter pass clip = false and ignore the second argument.
template <typename T>
struct Elem {
  using type = T;
};

template <typename F>
void dispatch(long esize, bool clip, F&& f) {
  if (esize == 2 && clip)
    f(Elem<bf16_t>{}, std::true_type{});
  else if (esize == 2)
    f(Elem<bf16_t>{}, std::false_type{});
  else if (clip)
    f(Elem<float>{}, std::true_type{});
  else
    f(Elem<float>{}, std::false_type{});
}

// the Adam launch behind fused_adam_table (host lr / bias corrections,
// null lr_buf and step_buf) and fused_adam_graph (device lr and step)
void launch_adam(const at::Tensor& table, long nchunks, long esize, float lr,
                 float b1, float b2, float eps, float wd, float bc1,
                 float bc2, const float* lr_buf, const long long* step_buf,
                 const c10::optional<at::Tensor>& gstats) {
  check_table(table, nchunks, esize);
  const float* gscale = gscale_ptr(gstats);
  dispatch(esize, gscale != nullptr, [&](auto elem, auto clip) {
    using T = typename decltype(elem)::type;
    launch_mt(adam_mt_kernel<T, decltype(clip)::value>, nchunks,
              table_ptr(table), lr, b1, b2, eps, wd, bc1, bc2, lr_buf,
              step_buf, gscale);
  });
}

}  // namespace

// prebuilt chunk table: ONE blocking upload that several launches of the
// same step share (norm reduction + update), or that a captured step
// reuses across replays (pointers are stable inside a captured step:
// params/state outside the graph pool, grads at fixed pool addresses).
// Returns (table, nchunks, element size 2|4).
std::tuple<at::Tensor, long, long> mt_build_table(
    std::vector<at::Tensor> ps, std::vector<at::Tensor> gs,
    std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
    std::vector<at::Tensor> masters) {
  TORCH_CHECK(!ps.empty());
  std::vector<Chunk> chunks;
  const int esize = ps[0].scalar_type() == at::kBFloat16 ? 2 : 4;
  for (size_t t = 0; t < ps.size(); ++t) {
    // any DENSE layout is fine (channels_last conv weights included):
    // the update is elementwise over raw storage, so p/g/state only need
    // to share one layout
    const bool dense =
        ps[t].is_contiguous() ||
        ps[t].is_contiguous(at::MemoryFormat::ChannelsLast) ||
        ps[t].is_contiguous(at::MemoryFormat::ChannelsLast3d);
    TORCH_CHECK(dense, "fused optimizer: param must be dense");
    TORCH_CHECK(gs[t].strides() == ps[t].strides(),
                "grad layout must match param layout");
    TORCH_CHECK(gs[t].scalar_type() == ps[t].scalar_type(),
                "grad dtype must match param dtype");
    char* p = (char*)ps[t].data_ptr();
    char* g = (char*)gs[t].data_ptr();
    float* m = (ms.empty() || ms[t].numel() == 0)
                   ? nullptr : ms[t].data_ptr<float>();
    float* v = (vs.empty() || vs[t].numel() == 0)
                   ? nullptr : vs[t].data_ptr<float>();
    float* master = masters.empty() ? nullptr
                                    : masters[t].data_ptr<float>();
    const int es = ps[t].scalar_type() == at::kBFloat16 ? 2 : 4;
    TORCH_CHECK(es == esize, "mixed param dtypes in one group");
    TORCH_CHECK(es == 4 || master != nullptr,
                "bf16 params require fp32 masters");
    for_each_chunk(ps[t].numel(), [&](long off, int n) {
      chunks.push_back({p + off * es, g + off * es, m ? m + off : nullptr,
                        v ? v + off : nullptr,
                        master ? master + off : nullptr, n, (int)t});
    });
  }
  // release the tensor handles before the blocking upload, not after it:
  // their refcount decrements then overlap the wait for the stream instead
  // of standing between the upload and the launch that follows it
  const at::Device device = ps[0].device();
  for (auto* list : {&ps, &gs, &ms, &vs, &masters}) list->clear();
  return {upload(chunks, device), (long)chunks.size(), (long)esize};
}

// grads-only chunk table (standalone clip_grad_norm_): any dense grads of
// ONE dtype, including views at unaligned offsets. Only zero-element grads
// give an empty table with nchunks == 0.
std::tuple<at::Tensor, long, long> grad_build_table(
    std::vector<at::Tensor> gs) {
  TORCH_CHECK(!gs.empty());
  std::vector<Chunk> chunks;
  const auto dt = gs[0].scalar_type();
  TORCH_CHECK(dt == at::kBFloat16 || dt == at::kFloat,
              "clip_grad_norm_: grads must be bf16 or fp32");
  const int es = dt == at::kBFloat16 ? 2 : 4;
  for (size_t t = 0; t < gs.size(); ++t) {
    TORCH_CHECK(gs[t].is_cuda() && gs[t].device() == gs[0].device(),
                "clip_grad_norm_: grads must live on one GPU");
    TORCH_CHECK(gs[t].scalar_type() == dt, "mixed dtypes in one table");
    TORCH_CHECK(gs[t].is_non_overlapping_and_dense(),
                "clip_grad_norm_: grad must be dense");
    char* g = (char*)gs[t].data_ptr();
    for_each_chunk(gs[t].numel(), [&](long off, int n) {
      chunks.push_back({g + off * es, g + off * es, nullptr, nullptr,
                        nullptr, n, (int)t});
    });
  }
  return {upload(chunks, gs[0].device()), (long)chunks.size(), (long)es};
}

// partials[offset + i] = sum of squares of chunk i's grads
void grad_sqnorm(at::Tensor table, long nchunks, long esize,
                 at::Tensor partials, long offset) {
  check_table(table, nchunks, esize);
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
              partials.is_contiguous());
  TORCH_CHECK(offset >= 0 && offset + nchunks <= partials.numel(),
              "partials buffer too small");
  float* out = partials.data_ptr<float>() + offset;
  dispatch(esize, false, [&](auto elem, auto) {
    using T = typename decltype(elem)::type;
    launch_mt(grad_sqnorm_mt_kernel<T>, nchunks, table_ptr(table), out);
  });
}

// stats = [norm, clip coefficient, running non-finite count]; max_norm is
// read from max_norm_buf (device) when given, else from the host value
void grad_norm_finalize(at::Tensor partials, long n, at::Tensor stats,
                        double max_norm,
                        c10::optional<at::Tensor> max_norm_buf) {
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
              partials.is_contiguous());
  TORCH_CHECK(n >= 0 && n <= partials.numel(), "partials buffer too small");
  gscale_ptr(stats);  // validates the stats tensor
  const float* mn = nullptr;
  if (max_norm_buf.has_value()) {
    TORCH_CHECK(max_norm_buf->is_cuda() &&
                max_norm_buf->scalar_type() == at::kFloat &&
                max_norm_buf->numel() >= 1);
    mn = max_norm_buf->data_ptr<float>();
  }
  launch_mt(grad_norm_finalize_kernel, 1, partials.data_ptr<float>(), (int)n,
            mn, (float)max_norm, stats.data_ptr<float>());
}

// in-place g *= stats[1] over a grads-only (or full) chunk table
void scale_mt(at::Tensor table, long nchunks, long esize, at::Tensor gstats) {
  check_table(table, nchunks, esize);
  const float* gscale = gscale_ptr(gstats);
  dispatch(esize, false, [&](auto elem, auto) {
    using T = typename decltype(elem)::type;
    launch_mt(scale_mt_kernel<T>, nchunks, table_ptr(table), gscale);
  });
}

// the *_table entry points run the update from a prebuilt table; gstats
// (optional) is the grad-norm stats tensor whose [1] scales every grad
void fused_adam_table(at::Tensor table, long nchunks, long esize, double lr,
                      double b1, double b2, double eps, double wd, double bc1,
                      double bc2, c10::optional<at::Tensor> gstats) {
  launch_adam(table, nchunks, esize, (float)lr, (float)b1, (float)b2,
              (float)eps, (float)wd, (float)bc1, (float)bc2, nullptr, nullptr,
              gstats);
}

// graph-capturable Adam: lr and step in device buffers, so that replays
// see live values; the kernel derives the bias corrections from step
void fused_adam_graph(at::Tensor table, long nchunks, long esize,
                      at::Tensor lr_buf, double b1, double b2, double eps,
                      double wd, at::Tensor step_buf,
                      c10::optional<at::Tensor> gstats) {
  TORCH_CHECK(table.is_cuda() && lr_buf.is_cuda() && step_buf.is_cuda());
  TORCH_CHECK(lr_buf.scalar_type() == at::kFloat &&
              step_buf.scalar_type() == at::kLong);
  launch_adam(table, nchunks, esize, 0.f, (float)b1, (float)b2, (float)eps,
              (float)wd, 1.f, 1.f, lr_buf.data_ptr<float>(),
              reinterpret_cast<const long long*>(step_buf.data_ptr<int64_t>()),
              gstats);
}

void fused_sgd_table(at::Tensor table, long nchunks, long esize, double lr,
                     double momentum, double wd, bool nesterov,
                     c10::optional<at::Tensor> gstats) {
  check_table(table, nchunks, esize);
  const float* gscale = gscale_ptr(gstats);
  dispatch(esize, gscale != nullptr, [&](auto elem, auto clip) {
    using T = typename decltype(elem)::type;
    launch_mt(sgd_mt_kernel<T, decltype(clip)::value>, nchunks,
              table_ptr(table), (float)lr, (float)momentum, (float)wd,
              (int)nesterov, gscale);
  });
}

void fused_lamb_table(at::Tensor table, long nchunks, long esize,
                      long ntensors, double lr, double b1, double b2,
                      double eps, double wd, double bc1, double bc2,
                      double clamp_trust, c10::optional<at::Tensor> gstats) {
  check_table(table, nchunks, esize);
  TORCH_CHECK(ntensors > 0);
  const float* gscale = gscale_ptr(gstats);
  auto norms = at::zeros({ntensors, 2}, table.options().dtype(at::kFloat));
  dispatch(esize, gscale != nullptr, [&](auto elem, auto clip) {
    using T = typename decltype(elem)::type;
    launch_mt(lamb_phase1_kernel<T, decltype(clip)::value>, nchunks,
              table_ptr(table), norms.data_ptr<float>(), (float)b1, (float)b2,
              (float)eps, (float)wd, (float)bc1, (float)bc2, gscale);
    launch_mt(lamb_phase2_kernel<T>, nchunks, table_ptr(table),
              norms.data_ptr<float>(), (float)lr, (float)b1, (float)b2,
              (float)eps, (float)wd, (float)bc1, (float)bc2,
              (float)clamp_trust);
  });
}

// one launch for all tensors; 2- and 4-byte element types may be mixed
void fused_copy(std::vector<at::Tensor> srcs, std::vector<at::Tensor> dsts) {
  TORCH_CHECK(srcs.size() == dsts.size(), "fused_copy: list lengths differ");
  std::vector<CopyRec> recs;
  for (size_t t = 0; t < srcs.size(); ++t) {
    TORCH_CHECK(srcs[t].strides() == dsts[t].strides(),
                "fused_copy: layouts must match");
    TORCH_CHECK(srcs[t].scalar_type() == dsts[t].scalar_type());
    const int es = srcs[t].element_size();
    TORCH_CHECK(es == 2 || es == 4, "fused_copy: 2- or 4-byte elems");
    const char* sp = (const char*)srcs[t].data_ptr();
    char* dp = (char*)dsts[t].data_ptr();
    for_each_chunk(srcs[t].numel(), [&](long off, int n) {
      recs.push_back({sp + off * es, dp + off * es, n, es});
    });
  }
  if (recs.empty()) return;
  auto table = upload(recs, srcs[0].device());
  launch_mt(copy_mt_kernel, (long)recs.size(),
            reinterpret_cast<const CopyRec*>(table.data_ptr()));
}
