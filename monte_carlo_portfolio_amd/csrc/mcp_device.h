// mcp_device.h -- device-side building blocks of the Monte Carlo path kernel (gfx950 only).
//
// SPEC.md sections 2-4: Philox4x32-10 counter layout, the exact-arithmetic inverse-CDF normal transform and
// the key transform used by the radix select.  Every floating-point operation below is an explicit IEEE
// binary32 op (the translation unit is compiled with -ffp-contract=off), so the CPU oracle
// (oracle/mc_oracle.c) reproduces terminal values bit for bit.
//
// The reference has no counterpart for this file (app.py contains no normal draws, SURVEY.md
// section 0.2); the conventions it inherits from the reference are cited in mcp_paths.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcp_reduce.h"  // wave_sum, wave_min, ..., block_sum
#include "mcp_route.h"   // ICDF_ENTRIES, ICDF_PAD, ICDF_LDS_ENTRIES: the sizes of the table that the host's routing needs too

namespace mcp {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t PHILOX_M0 = 0xD2511F53u;
constexpr uint32_t PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u;
constexpr uint32_t PHILOX_W1 = 0xBB67AE85u;

#ifndef MCP_EXP_BITOP3
#define MCP_EXP_BITOP3 1
#endif
#ifndef MCP_EXP_VMUL
#define MCP_EXP_VMUL 0
#endif
#ifndef MCP_EXP_NORMALS4
#define MCP_EXP_NORMALS4 1
#endif
#ifndef MCP_EXP_ICDF_CENTRED  // 1: the lean kernel runs normal_icdf_centred on a binade-scaled LDS table; 0: normal_icdf (lab builds)
#define MCP_EXP_ICDF_CENTRED 1
#endif

// a ^ b ^ c in one VALU instruction (v_bitop3_b32, truth table 0x96).
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if MCP_EXP_BITOP3
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}

// Round keys of Philox4x32-10: key_r = key_0 + r*(W0, W1).  They depend on the seed only.
struct PhiloxKeys {
  uint32_t k0[10], k1[10];
  uint32_t m0, m1;      // the two multipliers (MCP_EXP_VMUL pins them in VGPRs)
};
__device__ __forceinline__ PhiloxKeys philox_keys(uint32_t k0, uint32_t k1) {
  PhiloxKeys ks;
#pragma unroll
  for (int r = 0; r < 10; r++) { ks.k0[r] = k0 + (uint32_t)r * PHILOX_W0; ks.k1[r] = k1 + (uint32_t)r * PHILOX_W1; }
  ks.m0 = PHILOX_M0; ks.m1 = PHILOX_M1;
#if MCP_EXP_VMUL
  asm volatile("" : "+v"(ks.m0), "+v"(ks.m1));
#endif
  return ks;
}

// One Philox4x32-10 block: per round two v_mad_u64_u32 and two three-input xors per lane.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              const PhiloxKeys& ks, uint32_t (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
#if MCP_EXP_VMUL
    const uint64_t p0 = (uint64_t)ks.m0 * c0;
    const uint64_t p1 = (uint64_t)ks.m1 * c2;
#else
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c0;
    const uint64_t p1 = (uint64_t)PHILOX_M1 * c2;
#endif
    const uint32_t n0 = xor3((uint32_t)(p1 >> 32), c1, ks.k0[r]);
    const uint32_t n2 = xor3((uint32_t)(p0 >> 32), c3, ks.k1[r]);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// Scalar copies of the round keys that meet a wave-uniform operand in philox4x32_10_uhi: from the seed alone, never pinned in
// VGPRs, so the compiler keeps them and everything folded with them on the SALU.
struct PhiloxUniformKeys {
  uint32_t k1_0, k0_1, k1_1, k0_2;
};
__device__ __forceinline__ PhiloxUniformKeys philox_uniform_keys(uint32_t k0, uint32_t k1) {
  PhiloxUniformKeys sk = {k1, k0 + PHILOX_W0, k1 + PHILOX_W1, k0 + 2u * PHILOX_W0};
  sk.k1_0 = __builtin_amdgcn_readfirstlane(sk.k1_0); sk.k0_1 = __builtin_amdgcn_readfirstlane(sk.k0_1);
  sk.k1_1 = __builtin_amdgcn_readfirstlane(sk.k1_1); sk.k0_2 = __builtin_amdgcn_readfirstlane(sk.k0_2);
  return sk;
}

// philox4x32_10 on the counter (blk, 0, p_lo, p_hi) with blk AND p_hi wave-uniform (SGPRs; every path of the launch shares
// p_hi).  Round 1's c2 = hi(M0 blk) ^ p_hi ^ k1[0] and c3 = lo(M0 blk) are then scalar, and so is round 2's M1 c2: written out on
// scalars, with scalar ^ key folded on the SALU so that every vector xor that remains reads one SGPR.  The words are those of
// philox4x32_10 bit for bit (xor is associative; the products are the same products).  What depends on p_lo and the keys
// alone -- M1 p_lo, round 1's c0 and round 2's M0 c0 -- is loop-invariant in the walk over t, as in philox4x32_10.
__device__ __forceinline__ void philox4x32_10_uhi(uint32_t blk, uint32_t p_lo, uint32_t p_hi, const PhiloxKeys& ks,
                                                  const PhiloxUniformKeys& sk, uint32_t (&x)[4]) {
  // round 1: c0 = blk, c1 = 0, c2 = p_lo, c3 = p_hi
  const uint64_t q0 = (uint64_t)PHILOX_M0 * blk;                 // scalar
  const uint64_t p1 = (uint64_t)PHILOX_M1 * p_lo;
  const uint32_t a0 = (uint32_t)(p1 >> 32) ^ ks.k0[0];
  const uint32_t s2 = (uint32_t)(q0 >> 32) ^ p_hi ^ sk.k1_0;     // scalar
  // round 2: c0 = a0, c1 = lo(p1), c2 = s2, c3 = lo(q0)
  const uint64_t p0 = (uint64_t)PHILOX_M0 * a0;
  const uint64_t q1 = (uint64_t)PHILOX_M1 * s2;                  // scalar: s_mul_hi_u32, s_mul_i32
  uint32_t f0 = (uint32_t)(q1 >> 32) ^ sk.k0_1, f2 = (uint32_t)q0 ^ sk.k1_1, f1 = (uint32_t)q1 ^ sk.k0_2;
  asm("" : "+s"(f0), "+s"(f2), "+s"(f1));                        // folded on the SALU, not re-associated into the vector xors
  uint32_t c0 = (uint32_t)p1 ^ f0;
  uint32_t c2 = (uint32_t)(p0 >> 32) ^ f2;
  uint32_t c3 = (uint32_t)p0;
  uint32_t c1 = 0u;
#pragma unroll
  for (int r = 2; r < 10; r++) {
    const uint64_t r0 = (uint64_t)PHILOX_M0 * c0;
    const uint64_t r1 = (uint64_t)PHILOX_M1 * c2;
    // round 3: c1 = lo(q1) is scalar and meets k0[2] in f1
    const uint32_t n0 = r == 2 ? (uint32_t)(r1 >> 32) ^ f1 : xor3((uint32_t)(r1 >> 32), c1, ks.k0[r]);
    const uint32_t n2 = xor3((uint32_t)(r0 >> 32), c3, ks.k1[r]);
    c1 = (uint32_t)r1;
    c3 = (uint32_t)r0;
    c0 = n0;
    c2 = n2;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

constexpr float NEG_2LN2 = -0x1.62e43p+0f;       // -2 ln 2 (native Box-Muller only)

constexpr uint32_t ICDF_E_LO = 94;   // u in [2^-33, 1/2]: binary32 exponents 94..126

__device__ __forceinline__ float fma32(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// Constants of the transform that must sit in VGPRs: an SGPR (or, in VOP3, any non-inline) operand halves the issue
// rate of a VALU instruction on gfx950 (profiles/r01_valu_rates.txt).
struct IcdfConsts {
  uint32_t m18, m31;
  float su, sh;         // the scaling of u: us = fma(v, su, sh)
};
// The constants of normal_icdf_centred: the scaling is y = fma(v, 4, 2), and the bin centre 2^17 of the low 18 mantissa bits sits
// in a VGPR next to m18.  A type of its own: as one more member of IcdfConsts it moved two instructions of two antithetic kernels.
struct IcdfCentredConsts : IcdfConsts {
  uint32_t ctr;
};
// PIN_SCALE: su and sh sit in VGPRs too (otherwise they are literals, and the compiler forms the pair with a v_mov_b64 per step).
// CENTRED: IcdfCentredConsts, everything pinned.
template <bool PIN_SCALE = false, bool CENTRED = false>
__device__ __forceinline__ auto icdf_consts() {
  if constexpr (CENTRED) {
    IcdfCentredConsts c = {{0x0003ffffu, 0x7fffffffu, 0x1p+2f, 0x1p+1f}, 0x00020000u};
    asm volatile("" : "+v"(c.m18), "+v"(c.m31));
    asm volatile("" : "+v"(c.su), "+v"(c.sh));
    asm volatile("" : "+v"(c.ctr));
    return c;
  } else {
    IcdfConsts c = {0x0003ffffu, 0x7fffffffu, 0x1p-125f, 0x1p-126f};
    asm volatile("" : "+v"(c.m18), "+v"(c.m31));
    if constexpr (PIN_SCALE) asm volatile("" : "+v"(c.su), "+v"(c.sh));
    return c;
  }
}

// (a & m) | (b & ~m) in one v_bfi_b32
__device__ __forceinline__ uint32_t bitselect(uint32_t m, uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}

// Exact-arithmetic normal transform (SPEC.md section 3): one 32-bit word -> one N(0,1) draw by table-driven inverse
// CDF.  bit 31 = sign; v = low 31 bits, u = (v + 1/2) 2^-32; u's exponent and top 5 mantissa bits pick a cubic in the
// remaining 18 mantissa bits: one ds_read_b128 from the LDS copy of the table, three fma, no transcendental.
// `tab` is the PADDED LDS table (entry ICDF_PAD holds T[0]).  10.5 VALU instructions per normal.
__device__ __forceinline__ float normal_icdf(uint32_t x, const float4* tab, const IcdfConsts& k) {
  const float us = fma32((float)(x & 0x7fffffffu), k.su, k.sh);          // u * 2^-93: exponent field 1..33
  const uint32_t b = __float_as_uint(us);
  const float4 c = *(const float4*)((const char*)tab + ((b >> 14) & 0x0003fff0u));   // tab[b >> 18]
  const float dc = __uint_as_float((b & k.m18) | 0x3f800000u) - 0x1.04p+0f;
  float a = fma32(c.w, dc, c.z);
  a = fma32(a, dc, c.y);
  a = fma32(a, dc, c.x);
  return __uint_as_float(bitselect(k.m31, __float_as_uint(a), x));                  // |a| with the sign of bit 31
}

// The same transform on ten VALU instructions, bit for bit.  y = fma(v, 4, 2) = u 2^34 has u's significand
// and the binary32 exponent field 128..160, so table entry i = 32 (E - 1) + (top 5 mantissa bits) has the unbiased exponent
// E = 1 + i / 32 in [1, 33].  yc is y with its low 18 mantissa bits replaced by the bin centre 2^17: d = y - yc is exact (one
// binade) and equals dc 2^E, dc the delta of normal_icdf.  `tab` holds entry i SCALED by its binade, {c0, c1 2^-E, c2 2^-2E,
// c3 2^-3E} (icdf_scaled_entry): a power-of-two scaling commutes with the rounding of an fma while nothing is subnormal or
// overflows, so the Horner chain on d walks through 2^-2E a, 2^-E a, a with a the chain of normal_icdf
// (tests/test_icdf_centred_cpu.py checks every entry and every delta).  The table's byte offset is one instruction: bits 14..29
// of yc are 16 i + 8 (the centre's set bit 17 lands on bit 3; the exponent's always-set top bit is masked off), and the
// constant part, ICDF_PAD entries less 8 bytes, folds into the ds_read_b128's immediate offset.
__device__ __forceinline__ uint32_t icdf_centred_offset(uint32_t yc) {
  return (yc >> 14) & 0xffffu;                           // v_bfe_u32; written on the high word in 16 bits it compiles to two
}
constexpr int ICDF_CENTRED_BIAS = ICDF_PAD * 16 - 8;   // byte offset of T[0] in the padded table, less the centre's 8
__device__ __forceinline__ float4 icdf_scaled_entry(float4 c, int i) {
  const int e = 1 + i / 32;
  return make_float4(c.x, __builtin_ldexpf(c.y, -e), __builtin_ldexpf(c.z, -2 * e), __builtin_ldexpf(c.w, -3 * e));
}
__device__ __forceinline__ float normal_icdf_centred(uint32_t x, const float4* tab, const IcdfCentredConsts& k) {
  const float y = fma32((float)(x & 0x7fffffffu), k.su, k.sh);           // u * 2^34: exponent field 128..160
  const uint32_t yc = bitselect(k.m18, k.ctr, __float_as_uint(y));
  const float4 c = *(const float4*)((const char*)tab + ICDF_CENTRED_BIAS + icdf_centred_offset(yc));
  const float d = y - __uint_as_float(yc);
  float a = fma32(c.w, d, c.z);
  a = fma32(a, d, c.y);
  a = fma32(a, d, c.x);
  return __uint_as_float(bitselect(k.m31, __float_as_uint(a), x));
}

// MCP_FLAG_NATIVE_MATH: Box-Muller on the hardware approximations (v_log_f32, v_sqrt_f32, v_sin_f32, v_cos_f32) of
// word pairs.  Statistically equivalent N(0,1) draws from the same Philox stream, but NOT the spec's normals: results
// are comparable to the oracle only in distribution.  Every draw is held to the float64 evaluation of this formula on the same
// words, |z - z_ref| <= 2^-20 max(1, R) (tests/native_ref.py, tests/test_gpu_native.py; SPEC.md section 3).
__device__ __forceinline__ void box_muller_native(uint32_t xa, uint32_t xb, float& z_sin, float& z_cos) {
  const float u = fma32((float)xa, 0x1p-32f, 0x1p-32f);
  const float t = __builtin_amdgcn_logf(u) * NEG_2LN2;
  const float s = __builtin_amdgcn_sqrtf(t);
  const float turns = (float)xb * 0x1p-32f;
  z_sin = s * __builtin_amdgcn_sinf(turns);
  z_cos = s * __builtin_amdgcn_cosf(turns);
}

// The four normals of one Philox block.  CENTRED: by normal_icdf_centred, `tab` the binade-scaled table and k IcdfCentredConsts.
template <bool NATIVE, bool CENTRED = false, class K = IcdfConsts>
__device__ __forceinline__ void block_normals(const uint32_t (&x)[4], const float4* tab, const K& k, float& z0, float& z1,
                                              float& z2, float& z3) {
  if constexpr (NATIVE) {
    box_muller_native(x[0], x[1], z0, z1);
    box_muller_native(x[2], x[3], z2, z3);
  } else if constexpr (CENTRED) {
    // as below: the four table reads issued together, ahead of everything that depends on them, the four chains interleaved
    uint32_t yc[4];
    float4 c[4];
    float y[4], d[4], a[4];
#pragma unroll
    for (int i = 0; i < 4; i += 2) {                       // the scaling as one v_pk_fma_f32 per pair, as the compiler forms it below
      const f32x2 v2 = {(float)(x[i] & 0x7fffffffu), (float)(x[i + 1] & 0x7fffffffu)};
      const f32x2 y2 = __builtin_elementwise_fma(v2, (f32x2){k.su, k.su}, (f32x2){k.sh, k.sh});
      y[i] = y2.x; y[i + 1] = y2.y;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) yc[i] = bitselect(k.m18, k.ctr, __float_as_uint(y[i]));
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = *(const float4*)((const char*)tab + ICDF_CENTRED_BIAS + icdf_centred_offset(yc[i]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; i++) d[i] = y[i] - __uint_as_float(yc[i]);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = fma32(c[i].w, d[i], c[i].z);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = fma32(a[i], d[i], c[i].y);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = fma32(a[i], d[i], c[i].x);
    z0 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[0]), x[0]));
    z1 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[1]), x[1]));
    z2 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[2]), x[2]));
    z3 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[3]), x[3]));
  } else {
#if MCP_EXP_NORMALS4
    // the same four transforms with the four table reads issued together, ahead of everything that depends on them
    // (one s_waitcnt per block instead of one per normal), and the four Horner chains interleaved
    uint32_t b[4];
    float4 c[4];
    float dc[4], a[4];
#pragma unroll
    for (int i = 0; i < 4; i++) b[i] = __float_as_uint(fma32((float)(x[i] & 0x7fffffffu), k.su, k.sh));
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = *(const float4*)((const char*)tab + ((b[i] >> 14) & 0x0003fff0u));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; i++) dc[i] = __uint_as_float((b[i] & k.m18) | 0x3f800000u) - 0x1.04p+0f;   // (as v_pk_add_f32 pairs: +4 %)
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = fma32(c[i].w, dc[i], c[i].z);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = fma32(a[i], dc[i], c[i].y);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = fma32(a[i], dc[i], c[i].x);
    z0 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[0]), x[0]));
    z1 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[1]), x[1]));
    z2 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[2]), x[2]));
    z3 = __uint_as_float(bitselect(k.m31, __float_as_uint(a[3]), x[3]));
#else
    z0 = normal_icdf(x[0], tab, k);
    z1 = normal_icdf(x[1], tab, k);
    z2 = normal_icdf(x[2], tab, k);
    z3 = normal_icdf(x[3], tab, k);
#endif
  }
}

// Order-preserving map float -> uint32 (ascending floats <-> ascending keys), used by the select.
__host__ __device__ __forceinline__ uint32_t float_to_key(float v) {
  uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = __float_as_uint(v);
#else
  __builtin_memcpy(&b, &v, 4);
#endif
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ __forceinline__ float key_to_float(uint32_t k) {
  const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float v;
  __builtin_memcpy(&v, &b, 4);
  return v;
#endif
}

}  // namespace mcp
