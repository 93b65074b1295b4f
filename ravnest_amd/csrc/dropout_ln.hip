// Fused dropout + residual add + LayerNorm, forward and backward (gfx950).
//
//   forward :  d = bf16(dropout(z));  s = bf16(a + d);  y = LN(s)
//   backward:  dx = dLN(dy, s);  dz = keep ? bf16(bf16(dx) * scale) : 0;
//              dw = sum_rows dy * xhat;  db = sum_rows dy
//
// Both roundings of the composed path (dropout_fwd, then layernorm_add_fwd)
// are reproduced, and the mask is the one dropout_fwd_kernel draws for the
// same (seed ^ *seed_buf): element i uses Philox counter i >> 2, word i & 3.
// The mask is stored as one bit per element: bit (i & 7) of byte (i >> 3).
//
// Mapping: bf16 activations only, H % 8 == 0, H <= 2048. One 64-lane wave
// per row; a lane owns the 8-byte groups g = lane + 64 * k, k < VPL, so a
// group is exactly one Philox call and H = 768 is three full trips (the
// 16-byte mapping of layernorm.hip leaves half the lanes idle in its second
// trip). The row stays in registers between the statistics pass and the
// output pass: z, a, dy and s are read from HBM exactly once. The grids are
// persistent (as many blocks as are resident at once, waves stride over
// rows), so a lane's columns are fixed: gamma/beta are loaded once per wave
// (VPL <= 4), and in backward each lane sums dy * xhat and dy for its
// columns in fp32 registers over all its rows. mean/rstd come from a
// two-pass variance over the registers (layernorm.hip uses E[x^2] - mean^2).
//
// dgamma/dbeta across blocks: every block reduces its waves through LDS and
// writes one fp32 partial row of 2 * H floats with plain stores; a second
// small kernel sums the partials and writes dw/db in the weight dtype (no
// zero fill, no conversion launch). Atomics into the one 2 * H-float row
// were not used: in a persistent kernel all blocks arrive at the end
// together, the case measured at ~0.09 TB/s. Measured at N = 65536,
// H = 768 (profiles/dropout_add_ln.txt): forward 77 us (5.3 TB/s of the
// bytes it must move), backward 84 us (4.9 TB/s) including 5 us for the sum
// kernel over 512 partial rows; 88 and 125 VGPRs, 5 and 4 waves per SIMD.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

#include "common.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));  // 4 x bf16
typedef __bf16 hwbf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Both kernels are bound by vector ALU work as much as by memory (Philox is
// 40 quarter-rate 32-bit multiplies per 4 elements), so conversions use the
// packed hardware instruction: round-to-nearest-even like f2us (the two
// differ only for NaN payloads), two values per instruction.
DEVINL unsigned int pack2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned int,
                            __builtin_convertvector(v, hwbf16x2));
}
DEVINL u32x2 pack4(const float f[4]) {
  u32x2 r;
  r[0] = pack2(f[0], f[1]);
  r[1] = pack2(f[2], f[3]);
  return r;
}
DEVINL void unpack4(u32x2 v, float f[4]) {
  f[0] = __builtin_bit_cast(float, v[0] << 16);
  f[1] = __builtin_bit_cast(float, v[0] & 0xffff0000u);
  f[2] = __builtin_bit_cast(float, v[1] << 16);
  f[3] = __builtin_bit_cast(float, v[1] & 0xffff0000u);
}

// philox4x32-10 on the counter (ctr, 0): the stream of Philox4::gen in
// common.h, with each round's high and low product halves taken from one
// 64-bit multiply (one instruction instead of two quarter-rate ones)
DEVINL void philox4_gen(unsigned int key0, unsigned int key1,
                        unsigned long long ctr, unsigned int out[4]) {
  const unsigned int M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const unsigned int B0 = 0x9E3779B9u, B1 = 0xBB67AE85u;
  unsigned int c0 = (unsigned int)ctr, c1 = (unsigned int)(ctr >> 32);
  unsigned int c2 = 0, c3 = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)M0 * c0;
    const unsigned long long p1 = (unsigned long long)M1 * c2;
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ key0;
    const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ key1;
    c0 = n0; c1 = (unsigned int)p1; c2 = n2; c3 = (unsigned int)p0;
    key0 += B0; key1 += B1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

constexpr int FWD_THREADS = 256;   // 4 waves
constexpr int BWD_THREADS = 512;   // 8 waves: fewer partial rows
constexpr int MAX_H = 2048;        // VPL <= 8: the row fits in registers

template <typename PT>
DEVINL void load_p4(const PT* p, float out[4]);
template <>
DEVINL void load_p4<float>(const float* p, float out[4]) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = v[j];
}
template <>
DEVINL void load_p4<bf16_t>(const bf16_t* p, float out[4]) {
  unpack4(*reinterpret_cast<const u32x2*>(p), out);
}

template <typename PT>
DEVINL void store_p1(PT* p, float v);
template <>
DEVINL void store_p1<float>(float* p, float v) { *p = v; }
template <>
DEVINL void store_p1<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }

// ---------------- forward ----------------
// FULL: H is a multiple of 256, so every lane owns VPL groups and the range
// checks (and the branches and waits they put between the loads) drop out
template <typename PT, int VPL, bool FULL>
__global__ __launch_bounds__(FWD_THREADS) void dropout_add_ln_fwd_kernel(
    const bf16_t* __restrict__ z, const bf16_t* __restrict__ a,
    const PT* __restrict__ w, const PT* __restrict__ bias,
    bf16_t* __restrict__ y, bf16_t* __restrict__ s_out,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    unsigned char* __restrict__ maskbits, int H, long N, float eps, float p,
    float scale, unsigned long long seed,
    const long long* __restrict__ seed_buf) {
  constexpr bool HOIST = VPL <= 4;  // gamma/beta live in registers
  constexpr int PV = HOIST ? VPL : 1;
  const unsigned long long key =
      seed_buf ? seed ^ (unsigned long long)*seed_buf : seed;
  const unsigned int key0 = (unsigned int)key;
  const unsigned int key1 = (unsigned int)(key >> 32);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int wpb = blockDim.x / WAVE;
  const long nwaves = (long)gridDim.x * wpb;
  const int G = H >> 2;  // 8-byte groups per row (even: H % 8 == 0)

  float wv[PV][4], bv[PV][4];
  if constexpr (HOIST) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) {
        load_p4(w + 4 * g, wv[k]);
        load_p4(bias + 4 * g, bv[k]);
      }
    }
  }

  for (long row = (long)blockIdx.x * wpb + wid; row < N; row += nwaves) {
    const long base = row * H;
    u32x2 vz[VPL], va[VPL];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) {
        vz[k] = *reinterpret_cast<const u32x2*>(z + base + 4 * g);
        va[k] = *reinterpret_cast<const u32x2*>(a + base + 4 * g);
      }
    }

    float sv[VPL][4];
    float s1 = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      unsigned int nib = 0;
      if (FULL || g < G) {
        unsigned int r[4];
        philox4_gen(key0, key1, (unsigned long long)((base >> 2) + g), r);
        float zf[4], af[4];
        unpack4(vz[k], zf);
        unpack4(va[k], af);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float u = (r[j] >> 8) * (1.0f / 16777216.0f);
          const bool keep = u >= p;
          nib |= (keep ? 1u : 0u) << j;
          zf[j] = keep ? zf[j] * scale : 0.f;
        }
        // the composed path's two roundings: d to bf16, then a + d
        unpack4(pack4(zf), zf);
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] += zf[j];
        const u32x2 vs = pack4(af);
        unpack4(vs, sv[k]);
#pragma unroll
        for (int j = 0; j < 4; ++j) s1 += sv[k][j];
        *reinterpret_cast<u32x2*>(s_out + base + 4 * g) = vs;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[k][j] = 0.f;
      }
      // lanes 2m and 2m+1 hold the two nibbles of one mask byte; G is
      // even, so both lanes of a pair are in range or neither is
      const unsigned int hi = __shfl_xor(nib, 1, WAVE);
      if ((FULL || g < G) && !(lane & 1))
        maskbits[(base >> 3) + (g >> 1)] = (unsigned char)(nib | (hi << 4));
    }

    const float mean = wave_sum(s1) / H;
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      if (FULL || lane + WAVE * k < G) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float c = sv[k][j] - mean;
          s2 += c * c;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(s2) / H + eps);
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }

#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) {
        float wk[4], bk[4];
        if constexpr (HOIST) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            wk[j] = wv[k][j];
            bk[j] = bv[k][j];
          }
        } else {
          load_p4(w + 4 * g, wk);
          load_p4(bias + 4 * g, bk);
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = (sv[k][j] - mean) * rstd * wk[j] + bk[j];
        *reinterpret_cast<u32x2*>(y + base + 4 * g) = pack4(o);
      }
    }
  }
}

// ---------------- backward ----------------
// part: [gridDim.x][2 * H] fp32, row b = block b's (dgamma | dbeta) sums
// H = 768 needs two registers more than four waves per SIMD allow; the
// occupancy hint makes the compiler fit them (no scratch, checked with
// -Rpass-analysis=kernel-resource-usage)
// DZS: also sum the columns of dz, as stored (after the bf16 rounding), into
// a third slab of the partial row: part is [gridDim.x][3 * H]. That sum is
// the bias gradient of the Linear that produced z, which autograd would
// otherwise get from a pass of its own over dz. Twelve more accumulators
// do not fit at H = 768 (128 VGPRs and 16 bytes of scratch), so up to
// VPL = 4 every wave keeps its dz sums in an LDS row of its own, behind the
// 2 * H floats of the final reduction: a lane adds to its own columns with
// plain 16-byte reads and writes, in row order, so there is no race and
// the sum is deterministic. VPL = 8 (H > 1024) would need more than 64 KiB
// of LDS for that and sums in registers.
template <typename PT, int VPL, bool FULL, bool DZS = false>
__global__ __launch_bounds__(BWD_THREADS)
__attribute__((amdgpu_waves_per_eu(VPL <= 3 ? 4 : 1)))
void dropout_add_ln_bwd_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ s,
    const PT* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd,
    const unsigned char* __restrict__ maskbits, bf16_t* __restrict__ dx,
    bf16_t* __restrict__ dz, float* __restrict__ part, int H, long N,
    float scale) {
  extern __shared__ float red[];  // bwd_lds_floats<VPL, DZS>(H)
  constexpr int NS = DZS ? 3 : 2;
  constexpr bool ZLDS = DZS && VPL <= 4;  // dz sums in LDS wave rows
  constexpr bool ZREG = DZS && !ZLDS;     // ... in registers
  constexpr int ZV = ZREG ? VPL : 1;
  constexpr bool HOIST = VPL <= 4;
  constexpr int PV = HOIST ? VPL : 1;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int wpb = blockDim.x / WAVE;
  const long nwaves = (long)gridDim.x * wpb;
  const int G = H >> 2;

  float wv[PV][4];
  if constexpr (HOIST) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) load_p4(w + 4 * g, wv[k]);
    }
  }
  float accw[VPL][4], accb[VPL][4];
#pragma unroll
  for (int k = 0; k < VPL; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) accw[k][j] = accb[k][j] = 0.f;
  float accz[ZV][4];
  if constexpr (ZREG) {
#pragma unroll
    for (int k = 0; k < VPL; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) accz[k][j] = 0.f;
  }
  // column c of this wave's dz sums; a lane touches only its own groups
  float* zrow = red + 2 * H + wid * H;
  if constexpr (ZLDS) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G)
        *reinterpret_cast<f32x4*>(zrow + 4 * g) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  for (long row = (long)blockIdx.x * wpb + wid; row < N; row += nwaves) {
    const long base = row * H;
    u32x2 vd[VPL], vx[VPL];
    unsigned int mb[VPL];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) {
        vd[k] = *reinterpret_cast<const u32x2*>(dy + base + 4 * g);
        vx[k] = *reinterpret_cast<const u32x2*>(s + base + 4 * g);
        mb[k] = maskbits[(base >> 3) + (g >> 1)];
      }
    }
    const float mu = mean[row], rs = rstd[row];

    float gv[VPL][4], xh[VPL][4];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) {
        float wk[4];
        if constexpr (HOIST) {
#pragma unroll
          for (int j = 0; j < 4; ++j) wk[j] = wv[k][j];
        } else {
          load_p4(w + 4 * g, wk);
        }
        float df[4], xf[4];
        unpack4(vd[k], df);
        unpack4(vx[k], xf);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = df[j];
          const float xhat = (xf[j] - mu) * rs;
          const float gg = d * wk[j];
          c1 += gg * xhat;
          c2 += gg;
          accw[k][j] += d * xhat;
          accb[k][j] += d;
          gv[k][j] = gg;
          xh[k][j] = xhat;
        }
      }
    }
    c1 = wave_sum(c1) / H;
    c2 = wave_sum(c2) / H;

#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int g = lane + WAVE * k;
      if (FULL || g < G) {
        const unsigned int nib = mb[k] >> ((lane & 1) * 4);
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = rs * (gv[k][j] - xh[k][j] * c1 - c2);
        const u32x2 ox = pack4(o);
        // dz is rounded from the bf16 dx, as dropout_bwd sees it
        unpack4(ox, o);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = ((nib >> j) & 1) ? o[j] * scale : 0.f;
        *reinterpret_cast<u32x2*>(dx + base + 4 * g) = ox;
        const u32x2 oz = pack4(o);
        *reinterpret_cast<u32x2*>(dz + base + 4 * g) = oz;
        if constexpr (DZS) unpack4(oz, o);
        if constexpr (ZREG) {
#pragma unroll
          for (int j = 0; j < 4; ++j) accz[k][j] += o[j];
        }
        if constexpr (ZLDS) {
          f32x4 zs = *reinterpret_cast<f32x4*>(zrow + 4 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) zs[j] += o[j];
          *reinterpret_cast<f32x4*>(zrow + 4 * g) = zs;
        }
      }
    }
  }

  // the block's waves add their column sums into LDS one after another
  // (waves without rows add zeros), then the block stores its partial row
  for (int t = 0; t < wpb; ++t) {
    if (wid == t) {
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        const int g = lane + WAVE * k;
        if (FULL || g < G) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = 4 * g + j;
            if (t == 0) {
              red[c] = accw[k][j];
              red[H + c] = accb[k][j];
              if constexpr (ZREG) red[2 * H + c] = accz[k][j];
            } else {
              red[c] += accw[k][j];
              red[H + c] += accb[k][j];
              if constexpr (ZREG) red[2 * H + c] += accz[k][j];
            }
          }
        }
      }
    }
    __syncthreads();
  }
  float* prow = part + (long)blockIdx.x * NS * H;
  if constexpr (ZLDS) {
    // the barrier of the loop above has made every wave's row visible
    for (int i = threadIdx.x; i < 2 * H; i += blockDim.x) prow[i] = red[i];
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
      float t = 0.f;
      for (int w = 0; w < wpb; ++w) t += red[2 * H + w * H + i];
      prow[2 * H + i] = t;
    }
  } else {
    for (int i = threadIdx.x; i < NS * H; i += blockDim.x) prow[i] = red[i];
  }
}

// sums the per-block partial rows; 32 columns x 32 row slices per block.
// ns slabs per partial row: 2, or 3 with the dz column sums, which go to
// dzs in the dtype ZT of the Linear bias they are the gradient of
template <typename PT, typename ZT>
__global__ __launch_bounds__(1024) void dropout_add_ln_bwd_finalize_kernel(
    const float* __restrict__ part, PT* __restrict__ dw, PT* __restrict__ db,
    ZT* __restrict__ dzs, int H, int nparts, int ns) {
  __shared__ float tile[32][33];
  const int c = threadIdx.x & 31;
  const int sl = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + c;  // in [0, ns * H)
  float acc = 0.f;
  if (col < ns * H) {
#pragma unroll 4
    for (int q = sl; q < nparts; q += 32)
      acc += part[(long)q * ns * H + col];
  }
  tile[sl][c] = acc;
  __syncthreads();
  if (sl == 0 && col < ns * H) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) t += tile[i][c];
    if (col < H)
      store_p1(dw + col, t);
    else if (col < 2 * H)
      store_p1(db + (col - H), t);
    else
      store_p1(dzs + (col - 2 * H), t);
  }
}

// blocks of `kernel` that are resident at once on the current device
template <typename K>
int resident_blocks(K kernel, int threads, size_t lds) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, kernel, threads, lds);
  int dev = 0, cus = 0;
  if (e == hipSuccess) e = hipGetDevice(&dev);
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev);
  TORCH_CHECK(e == hipSuccess && per_cu > 0 && cus > 0,
              "dropout_add_ln: occupancy query failed");
  return per_cu * cus;
}

template <typename PT, int VPL, bool FULL>
int fwd_resident_blocks() {
  static const int n = resident_blocks(
      dropout_add_ln_fwd_kernel<PT, VPL, FULL>, FWD_THREADS, 0);
  return n;
}
// floats of dynamic LDS the backward kernel uses (see its DZS comment)
template <int VPL, bool DZS>
constexpr size_t bwd_lds_floats(int H) {
  return (size_t)(!DZS ? 2 : VPL <= 4 ? 2 + BWD_THREADS / WAVE : 3) * H;
}
template <typename PT, int VPL, bool FULL, bool DZS>
int bwd_resident_blocks() {
  static const int n = resident_blocks(
      dropout_add_ln_bwd_kernel<PT, VPL, FULL, DZS>, BWD_THREADS,
      bwd_lds_floats<VPL, DZS>(VPL * 256) * sizeof(float));
  return n;
}

bool aligned8(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 8 == 0;
}
bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

void check_common(const at::Tensor& x, const at::Tensor& w, const char* op) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == at::kBFloat16 && x.dim() >= 1,
              op, ": bf16 contiguous device activations only");
  const long H = x.size(-1);
  TORCH_CHECK(H % 8 == 0 && H <= MAX_H && H > 0, op,
              ": hidden size must be a multiple of 8, at most ", MAX_H);
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.numel() == H &&
                  (w.scalar_type() == at::kFloat ||
                   w.scalar_type() == at::kBFloat16) &&
                  aligned16(w),
              op, ": LN parameters must be fp32 or bf16 of size H");
}

}  // namespace

// VPL: 8-byte groups per lane, rounded up to an instantiated value
#define DAL_FULL(PT, VPL, LAUNCH)                                           \
  do {                                                                      \
    if (full_ && vpl_ == VPL) { LAUNCH(PT, VPL, true); }                    \
    else { LAUNCH(PT, VPL, false); }                                        \
  } while (0)
#define DAL_DISPATCH_VPL(PT, LAUNCH)                                        \
  do {                                                                      \
    const int vpl_ = (H / 4 + WAVE - 1) / WAVE;                             \
    const bool full_ = H % (4 * WAVE) == 0;                                 \
    if (vpl_ <= 1) { DAL_FULL(PT, 1, LAUNCH); }                             \
    else if (vpl_ == 2) { DAL_FULL(PT, 2, LAUNCH); }                        \
    else if (vpl_ == 3) { DAL_FULL(PT, 3, LAUNCH); }                        \
    else if (vpl_ == 4) { DAL_FULL(PT, 4, LAUNCH); }                        \
    else { DAL_FULL(PT, 8, LAUNCH); }                                       \
  } while (0)

std::vector<at::Tensor> dropout_add_ln_fwd(at::Tensor z, at::Tensor a,
                                           at::Tensor w, at::Tensor bias,
                                           double eps, double p, int64_t seed,
                                           c10::optional<at::Tensor> seed_buf) {
  check_common(a, w, "dropout_add_ln_fwd");
  check_common(z, bias, "dropout_add_ln_fwd");
  TORCH_CHECK(a.sizes() == z.sizes() && w.scalar_type() == bias.scalar_type());
  TORCH_CHECK(p > 0.0 && p < 1.0, "dropout_add_ln_fwd: p must be in (0, 1)");
  TORCH_CHECK(aligned8(z) && aligned8(a));
  const long long* sb = nullptr;
  if (seed_buf.has_value()) {
    TORCH_CHECK(seed_buf->is_cuda() && seed_buf->scalar_type() == at::kLong);
    sb = reinterpret_cast<const long long*>(seed_buf->data_ptr<int64_t>());
  }
  const int H = a.size(-1);
  const long N = a.numel() / H;
  auto y = at::empty_like(a);
  auto s_out = at::empty_like(a);
  auto mean = at::empty({N}, a.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, a.options().dtype(at::kFloat));
  auto maskbits = at::empty({N * H / 8}, a.options().dtype(at::kByte));
  if (N == 0) return {y, s_out, mean, rstd, maskbits};
  const float scale = 1.0f / (1.0f - (float)p);
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int wpb = FWD_THREADS / WAVE;

#define DAL_LAUNCH_FWD(PT, VPL, FULL)                                       \
  do {                                                                      \
    const long want = (N + wpb - 1) / wpb;                                  \
    const int cap = fwd_resident_blocks<PT, VPL, FULL>();                   \
    dim3 grid((unsigned)std::min<long>(want, cap));                         \
    hipLaunchKernelGGL((dropout_add_ln_fwd_kernel<PT, VPL, FULL>), grid,    \
                       dim3(FWD_THREADS), 0, stream,                        \
                       reinterpret_cast<const bf16_t*>(z.data_ptr()),       \
                       reinterpret_cast<const bf16_t*>(a.data_ptr()),       \
                       reinterpret_cast<const PT*>(w.data_ptr()),           \
                       reinterpret_cast<const PT*>(bias.data_ptr()),        \
                       reinterpret_cast<bf16_t*>(y.data_ptr()),             \
                       reinterpret_cast<bf16_t*>(s_out.data_ptr()),         \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),      \
                       maskbits.data_ptr<unsigned char>(), H, N,            \
                       (float)eps, (float)p, scale,                         \
                       (unsigned long long)seed, sb);                       \
  } while (0)

  if (w.scalar_type() == at::kFloat)
    DAL_DISPATCH_VPL(float, DAL_LAUNCH_FWD);
  else
    DAL_DISPATCH_VPL(bf16_t, DAL_LAUNCH_FWD);
  HIP_CHECK_LAST();
  return {y, s_out, mean, rstd, maskbits};
}

// zs: 0 = {dx, dz, dw, db}; 1 / 2 = those and the column sums of dz as
// fp32 / bf16
static std::vector<at::Tensor> dropout_add_ln_bwd_impl(
    at::Tensor dy, at::Tensor s, at::Tensor w, at::Tensor mean,
    at::Tensor rstd, at::Tensor maskbits, double p, int zs) {
  check_common(s, w, "dropout_add_ln_bwd");
  check_common(dy, w, "dropout_add_ln_bwd");
  TORCH_CHECK(dy.sizes() == s.sizes() && aligned8(dy) && aligned8(s));
  const int H = s.size(-1);
  const long N = s.numel() / H;
  TORCH_CHECK(mean.is_cuda() && mean.scalar_type() == at::kFloat &&
              mean.is_contiguous() && mean.numel() == N);
  TORCH_CHECK(rstd.is_cuda() && rstd.scalar_type() == at::kFloat &&
              rstd.is_contiguous() && rstd.numel() == N);
  TORCH_CHECK(maskbits.is_cuda() && maskbits.scalar_type() == at::kByte &&
              maskbits.is_contiguous() && maskbits.numel() == N * H / 8);
  TORCH_CHECK(p > 0.0 && p < 1.0, "dropout_add_ln_bwd: p must be in (0, 1)");
  auto dx = at::empty_like(s);
  auto dz = at::empty_like(s);
  auto dw = at::empty({H}, w.options());
  auto db = at::empty({H}, w.options());
  at::Tensor dzs;
  if (zs)
    dzs = at::empty({H}, w.options().dtype(zs == 1 ? at::kFloat
                                                   : at::kBFloat16));
  if (N == 0) {
    dw.zero_();
    db.zero_();
    if (zs) {
      dzs.zero_();
      return {dx, dz, dw, db, dzs};
    }
    return {dx, dz, dw, db};
  }
  const float scale = 1.0f / (1.0f - (float)p);
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int wpb = BWD_THREADS / WAVE;
  const int ns = zs ? 3 : 2;
  const long want = (N + wpb - 1) / wpb;
  at::Tensor part;
  int nparts = 0;

#define DAL_LAUNCH_BWD_MAIN(PT, VPL, FULL, DZS)                             \
  do {                                                                      \
    nparts = (int)std::min<long>(                                           \
        want, bwd_resident_blocks<PT, VPL, FULL, DZS>());                   \
    part = at::empty({nparts, ns * H}, s.options().dtype(at::kFloat));      \
    hipLaunchKernelGGL((dropout_add_ln_bwd_kernel<PT, VPL, FULL, DZS>),     \
                       dim3(nparts),                                        \
                       dim3(BWD_THREADS),                                   \
                       (bwd_lds_floats<VPL, DZS>(H)) * sizeof(float),       \
                       stream,                                              \
                       reinterpret_cast<const bf16_t*>(dy.data_ptr()),      \
                       reinterpret_cast<const bf16_t*>(s.data_ptr()),       \
                       reinterpret_cast<const PT*>(w.data_ptr()),           \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),      \
                       maskbits.data_ptr<unsigned char>(),                  \
                       reinterpret_cast<bf16_t*>(dx.data_ptr()),            \
                       reinterpret_cast<bf16_t*>(dz.data_ptr()),            \
                       part.data_ptr<float>(), H, N, scale);                \
  } while (0)
#define DAL_LAUNCH_BWD_FIN(PT, ZT)                                          \
  hipLaunchKernelGGL((dropout_add_ln_bwd_finalize_kernel<PT, ZT>),          \
                     dim3((ns * H + 31) / 32), dim3(1024), 0, stream,       \
                     part.data_ptr<float>(),                                \
                     reinterpret_cast<PT*>(dw.data_ptr()),                  \
                     reinterpret_cast<PT*>(db.data_ptr()),                  \
                     zs ? reinterpret_cast<ZT*>(dzs.data_ptr()) : nullptr,  \
                     H, nparts, ns)
#define DAL_LAUNCH_BWD(PT, VPL, FULL)                                       \
  do {                                                                      \
    if (zs) DAL_LAUNCH_BWD_MAIN(PT, VPL, FULL, true);                       \
    else DAL_LAUNCH_BWD_MAIN(PT, VPL, FULL, false);                         \
    if (zs == 2) DAL_LAUNCH_BWD_FIN(PT, bf16_t);                            \
    else DAL_LAUNCH_BWD_FIN(PT, float);                                     \
  } while (0)

  if (w.scalar_type() == at::kFloat)
    DAL_DISPATCH_VPL(float, DAL_LAUNCH_BWD);
  else
    DAL_DISPATCH_VPL(bf16_t, DAL_LAUNCH_BWD);
  HIP_CHECK_LAST();
  if (zs) return {dx, dz, dw, db, dzs};
  return {dx, dz, dw, db};
}

std::vector<at::Tensor> dropout_add_ln_bwd(at::Tensor dy, at::Tensor s,
                                           at::Tensor w, at::Tensor mean,
                                           at::Tensor rstd,
                                           at::Tensor maskbits, double p) {
  return dropout_add_ln_bwd_impl(dy, s, w, mean, rstd, maskbits, p, 0);
}

// dropout_add_ln_bwd and dzsum = dz.sum(0) (fp32 sums of the stored bf16
// values), returned as fp32 or bf16: {dx, dz, dw, db, dzsum}
std::vector<at::Tensor> dropout_add_ln_bwd_dzsum(
    at::Tensor dy, at::Tensor s, at::Tensor w, at::Tensor mean,
    at::Tensor rstd, at::Tensor maskbits, double p, bool dzsum_bf16) {
  return dropout_add_ln_bwd_impl(dy, s, w, mean, rstd, maskbits, p,
                                 dzsum_bf16 ? 2 : 1);
}
