// Shared MX fp8 block quantiser: bf16-valued floats -> OCP e4m3 bytes +
// one e8m0 scale per 32-element block (round-to-nearest-even).
//
// A 32-block is held by a QUAD of 4 consecutive lanes, 8 consecutive
// elements each (the bf16x8 group mapping of the LayerNorm / GELU
// kernels), so a producer that has a row in registers quantises it in
// place: two __shfl_xor steps for the block amax, 8 encodes, one 8-byte
// store per lane and one scale byte per quad.
//
// The shuffles read the quad's other lanes: every quad that calls
// mx_quant8 must be WHOLLY active. Callers loop over 8-element groups
// with a group count that is a multiple of 4 (last dim % 32 == 0) and a
// lane stride that is a multiple of 4, so a quad is in or out as a whole.
//
// Host-compilable (MXQ_FN) so the encoder can be checked on a CPU
// against every bf16 value.
#pragma once

#ifdef __HIPCC__
#include "common.h"
#define MXQ_FN DEVINL
#else
#define MXQ_FN static inline
#endif

MXQ_FN unsigned int mxq_f2u(float f) {
  return __builtin_bit_cast(unsigned int, f);
}
MXQ_FN float mxq_u2f(unsigned int u) { return __builtin_bit_cast(float, u); }

// float -> OCP e4m3fn byte, round-to-nearest-even, saturate to +-448;
// NaN and +-inf -> 0x7F (e4m3fn has no infinity, and saturating one to
// 448 would hand the GEMM a finite value). Integer rounding for the
// normals; the subnormals (|v| < 2^-6, units of 2^-9) round in the
// adder: |v| + 2^14 has exactly 2^-9 as its last mantissa bit.
MXQ_FN unsigned char f32_to_e4m3(float v) {
  const unsigned int bits = mxq_f2u(v);
  const unsigned int a = bits & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return 0x7F;
  const unsigned int sign = (bits >> 24) & 0x80u;
  unsigned int code;
  if (a >= 0x3C800000u) {  // >= 2^-6: normal in e4m3
    // RNE to 3 mantissa bits; a carry runs into the exponent, as it should
    const unsigned int r = (a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20;
    code = r - (120u << 3);  // rebias 127 -> 7
    if (code > 0x7Eu) code = 0x7Eu;  // max finite, 448
  } else {
    // 0..8; 8 is the encoding 0x08 of the smallest normal 2^-6
    code = mxq_f2u(mxq_u2f(a) + 16384.f) - 0x46800000u;
  }
  return (unsigned char)(sign | code);
}

// biased e8m0 byte of a block whose largest finite |element| is amax:
// 2^s with s = floor(log2(amax / 448)) + 1 clamped to [-127, 127], so
// the scaled amax lands in [224, 448). Read off the bits: amax =
// 1.m * 2^(E-127) and 448 = 1.75 * 2^8, so the floor is E - 135 when
// 1.m >= 1.75 and E - 136 below (subnormal amax: E = 0, clamped).
// amax = 0 gives s = -127, byte 0.
MXQ_FN int mx_scale_exp(float amax) {
  int s = -127;
  if (amax > 0.f) {
    const unsigned int ab = mxq_f2u(amax);
    s = (int)(ab >> 23) - 135 + ((ab & 0x7FFFFFu) >= 0x600000u ? 1 : 0);
    if (s < -127) s = -127;
    if (s > 127) s = 127;
  }
  return s;
}

// |v| for the block amax: NaN and +-inf count as 0 (they encode as 0x7F
// and leave the scale to the rest of the block)
MXQ_FN float mx_finite_abs(float v) {
  const float a = __builtin_fabsf(v);
  return a <= 3.3895314e38f ? a : 0.f;  // bf16 max; false for NaN
}

#ifdef __HIPCC__
typedef unsigned int mxq_u32x2 __attribute__((ext_vector_type(2)));

// One lane's 8 consecutive elements v[0..8) of a 32-block held by the
// quad (lane & ~3 .. +3). q8: where this lane's 8 bytes go (8-byte
// aligned); sc: the block's scale byte, written by the quad's first lane.
DEVINL void mx_quant8(const float (&v)[8], unsigned char* __restrict__ q8,
                      unsigned char* __restrict__ sc, int lane) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, mx_finite_abs(v[j]));
  amax = fmaxf(amax, __shfl_xor(amax, 1, WAVE));
  amax = fmaxf(amax, __shfl_xor(amax, 2, WAVE));
  const int s = mx_scale_exp(amax);
  mxq_u32x2 o = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j >> 2] |= (unsigned int)f32_to_e4m3(ldexpf(v[j], -s)) << (8 * (j & 3));
  *reinterpret_cast<mxq_u32x2*>(q8) = o;
  if ((lane & 3) == 0) *sc = (unsigned char)(s + 127);
}
#endif
