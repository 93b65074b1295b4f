// Transposing MX fp8 quantiser for the backward GEMMs of MXLinear.
//
//   mx_quant_t(x)    x (R, C) bf16 -> qt (C, Rp) e4m3, st (C, Rp/32) e8m0
//   mx_quant_dual(x) the same plus q (R, C), s (R, C/32) from ONE read of x
//
// qt/st are the MX quantisation of x^T: a block is 32 consecutive ROWS of
// one column, which is what a GEMM contracting over the rows of x (wgrad)
// or over out_features of a weight (dgrad) needs along its K axis.
// Rp = max(256, round_up(R, 128)) so mx_gemm2 takes it as a contraction;
// rows [R, Rp) read as +0 and so encode as byte 0 under scale byte 0.
// Bit for bit mx_quant(pad_rows(x, Rp).t().contiguous()): same
// mx_finite_abs / mx_scale_exp / f32_to_e4m3, and a max has no order.
//
// One 256-thread block per 128-row x 64-column tile (128 rows = one K-tile
// of mx_gemm2 = 128 contiguous bytes of each of 64 qt rows):
//   1. thread (row = pass*32 + tid/8, group = tid%8) loads 8 consecutive
//      bf16 with one 16 B load, 4 passes; 8 lanes cover a row's 128 B.
//      DUAL: lanes 4k..4k+3 hold one 32-column block of a row, exactly the
//      quad mx_quant8 wants, so q/s come straight from these registers.
//   2. the bf16 tile goes to LDS as loaded, 128 B per row (16 KiB). The
//      wave's writes are one contiguous 1 KiB run per 8 rows.
//   3. thread (col = tid%64, rb = tid/64) owns column col of rows
//      rb*32..+31: a wave reads 64 consecutive u16 of one LDS row per step
//      (128 B = every bank once, two lanes per dword), so no padding is
//      needed. amax, scale, 32 encodes -> 32 bytes in 8 registers.
//   4. the bytes are restaged through an 8 KiB LDS image [64 cols][128 B]
//      whose 16 B chunks are XOR-swizzled with col&7 (8 lanes of different
//      columns hit 8 different chunks), and the 4 scale bytes per column
//      through [64][4]; then 8 consecutive lanes store one qt row's whole
//      128 B run and 64 lanes one u32 of scales each.
// No atomics, no host read, no memset: tiles past R write the zeros.
//
// HBM traffic per element: 2 B in, 1 B out (+1 B for DUAL's q) + 1/32 B
// per scale; profiles/mx_bwd.txt has the measured bandwidth.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "mx_quant.h"

#if defined(__HIP_DEVICE_COMPILE__)
// no packed fp32 VALU ops in the new kernels
#define MXQT_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define MXQT_TARGET
#endif

namespace {

typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));

constexpr int TR = 128, TC = 64;  // tile rows x columns
constexpr int NTHR = 256;

// VEC: C % 8 == 0 and a 16-byte-aligned base, so a lane's 8 elements are
// one load; else element by element with a column bound.
template <bool DUAL, bool VEC>
MXQT_TARGET __global__ __launch_bounds__(NTHR) void mx_quant_t_kernel(
    const bf16_t* __restrict__ X, unsigned char* __restrict__ Q,
    unsigned char* __restrict__ S, unsigned char* __restrict__ QT,
    unsigned char* __restrict__ ST, long R, long C, long Rp, int CT) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[TR * TC];
  __shared__ __attribute__((aligned(16))) unsigned char outq[TC * TR];
  __shared__ unsigned int outs[TC];

  const int tid = threadIdx.x;
  const long r0 = (long)(blockIdx.x / CT) * TR;
  const long c0 = (long)(blockIdx.x % CT) * TC;
  const unsigned short* const xu =
      reinterpret_cast<const unsigned short*>(X);

  // ---- 1 + 2: load, (row-blocked quantise,) stage
  const int lr = tid >> 3, lg = tid & 7;
  const long c = c0 + lg * 8;
#pragma unroll
  for (int p = 0; p < TR / 32; ++p) {
    const long r = r0 + p * 32 + lr;
    bf16x8 in = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < R) {
      if constexpr (VEC) {
        if (c < C) in = *reinterpret_cast<const bf16x8*>(xu + r * C + c);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c + j < C) in[j] = (short)xu[r * C + c + j];
      }
    }
    *reinterpret_cast<bf16x8*>(&tile[(p * 32 + lr) * TC + lg * 8]) = in;
    if constexpr (DUAL) {
      // C % 32 == 0: a quad (one row, 32 columns) is in or out as a whole
      if (r < R && c < C) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = us2f((unsigned short)in[j]);
        mx_quant8(v, Q + r * C + c, S + r * (C >> 5) + (c >> 5), tid);
      }
    }
  }
  __syncthreads();

  // ---- 3: one column x one 32-row block per thread
  const int col = tid & 63, rb = tid >> 6;
  {
    float v[32];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      v[i] = us2f(tile[(rb * 32 + i) * TC + col]);
      amax = fmaxf(amax, mx_finite_abs(v[i]));
    }
    const int s = mx_scale_exp(amax);
    unsigned int o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = 0u;
#pragma unroll
    for (int i = 0; i < 32; ++i)
      o[i >> 2] |= (unsigned int)f32_to_e4m3(ldexpf(v[i], -s))
                   << (8 * (i & 3));
    // ---- 4: restage, 16 B chunk j of column col at chunk j ^ (col & 7)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      *reinterpret_cast<u32x4v*>(
          &outq[col * TR + (((rb * 2 + h) ^ (col & 7)) << 4)]) =
          u32x4v{o[4 * h], o[4 * h + 1], o[4 * h + 2], o[4 * h + 3]};
    reinterpret_cast<unsigned char*>(outs)[col * 4 + rb] =
        (unsigned char)(s + 127);
  }
  __syncthreads();

  // Rp % 128 == 0: a run starts on a 128 B boundary of its qt row and the
  // tile's 4 scale bytes on a 4 B boundary of its st row
#pragma unroll
  for (int p = 0; p < (TC * TR / 16) / NTHR; ++p) {
    const int idx = p * NTHR + tid;
    const int oc = idx >> 3, j = idx & 7;
    if (c0 + oc < C)
      *reinterpret_cast<u32x4v*>(QT + (c0 + oc) * Rp + r0 + j * 16) =
          *reinterpret_cast<const u32x4v*>(
              &outq[oc * TR + ((j ^ (oc & 7)) << 4)]);
  }
  if (tid < TC && c0 + tid < C)
    *reinterpret_cast<unsigned int*>(ST + (c0 + tid) * (Rp >> 5) +
                                     (r0 >> 5)) = outs[tid];
}

std::vector<at::Tensor> run(const at::Tensor& x, bool dual,
                            const char* name) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                  x.is_contiguous() && x.dim() == 2,
              name, ": x must be a contiguous 2-d bf16 GPU tensor");
  const long R = x.size(0), C = x.size(1);
  TORCH_CHECK(R >= 1 && C >= 1, name, ": empty input");
  if (dual) TORCH_CHECK(C % 32 == 0, name, ": C % 32 == 0 required");
  const long Rp = std::max<long>(256, (R + 127) / 128 * 128);
  const long CT = (C + TC - 1) / TC;
  TORCH_CHECK(CT * (Rp / TR) <= 0x7FFFFFFFl && CT <= 0x7FFFFFFFl, name,
              ": too large");
  auto bopt = x.options().dtype(at::kByte);
  auto qt = at::empty({C, Rp}, bopt);
  auto st = at::empty({C, Rp / 32}, bopt);
  at::Tensor q, s;
  if (dual) {
    q = at::empty({R, C}, bopt);
    s = at::empty({R, C / 32}, bopt);
  }
  auto* xp = reinterpret_cast<const bf16_t*>(x.data_ptr());
  const bool vec = C % 8 == 0 && reinterpret_cast<uintptr_t>(xp) % 16 == 0;
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  dim3 grid((unsigned)(CT * (Rp / TR))), block(NTHR);
#define LAUNCH_QT(DUAL, VEC)                                                \
  hipLaunchKernelGGL((mx_quant_t_kernel<DUAL, VEC>), grid, block, 0,        \
                     stream, xp,                                            \
                     DUAL ? q.data_ptr<unsigned char>() : nullptr,          \
                     DUAL ? s.data_ptr<unsigned char>() : nullptr,          \
                     qt.data_ptr<unsigned char>(),                          \
                     st.data_ptr<unsigned char>(), R, C, Rp, (int)CT)
  if (dual) {
    if (vec) LAUNCH_QT(true, true); else LAUNCH_QT(true, false);
  } else {
    if (vec) LAUNCH_QT(false, true); else LAUNCH_QT(false, false);
  }
#undef LAUNCH_QT
  HIP_CHECK_LAST();
  if (dual) return {q, s, qt, st};
  return {qt, st};
}

}  // namespace

std::vector<at::Tensor> mx_quant_t(at::Tensor x) {
  return run(x, false, "mx_quant_t");
}

std::vector<at::Tensor> mx_quant_dual(at::Tensor x) {
  return run(x, true, "mx_quant_dual");
}
