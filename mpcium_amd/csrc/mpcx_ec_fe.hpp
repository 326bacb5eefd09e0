// mpcx_ec_fe.hpp -- secp256k1 field and point arithmetic of the EC kernels
// (device code): k_ec_combine (mpcx_ec.hip) and the test probe k_ec_probe
// (mpcx_ec_probe.hip) include the same text, so what the probe checks is what
// the combination kernel runs.
//
// Field: p = 2^256 - 2^32 - 977, eight 32-bit limbs, values kept < p; a product
// is folded with 2^256 = 2^32 + 977 (mod p). Points: Jacobian (X, Y, Z) with
// a = 0 formulas (dbl-2009-l, add-2007-bl, madd-2007-bl).
#ifndef MPCX_EC_FE_HPP_
#define MPCX_EC_FE_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcx {
namespace {

struct Fe {
  uint32_t v[8];
};

__device__ __constant__ const uint32_t kP[8] = {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                                0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};

__device__ __forceinline__ bool fe_is_zero(const Fe& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a.v[i];
  return o == 0;
}
// a >= p (a < 2^256)
__device__ __forceinline__ bool fe_geq_p(const Fe& a) {
  // p's limbs 2..7 are all ones: a >= p iff those are all ones and (a1, a0) >= (p1, p0)
  uint32_t hi = 0xFFFFFFFFu;
#pragma unroll
  for (int i = 2; i < 8; ++i) hi &= a.v[i];
  if (hi != 0xFFFFFFFFu) return false;
  if (a.v[1] != kP[1]) return a.v[1] > kP[1];
  return a.v[0] >= kP[0];
}
// a + k (k < 2^40) * (2^32 + 977) folded into a 256-bit value, then < p
__device__ __forceinline__ void fe_fold(Fe& r, uint64_t k) {
  while (k) {
    // r += k * 977 + (k << 32)
    uint64_t lo = k * 977u;  // < 2^50
    uint64_t c = (uint64_t)r.v[0] + (uint32_t)lo;
    r.v[0] = (uint32_t)c;
    c = (c >> 32) + (uint64_t)r.v[1] + (uint32_t)(lo >> 32) + (uint32_t)k;
    r.v[1] = (uint32_t)c;
    c = (c >> 32) + (uint64_t)r.v[2] + (uint32_t)(k >> 32);
    r.v[2] = (uint32_t)c;
    c >>= 32;
#pragma unroll
    for (int i = 3; i < 8; ++i) {
      c += r.v[i];
      r.v[i] = (uint32_t)c;
      c >>= 32;
    }
    k = c;  // 2^256 wrapped: fold once more (at most twice in total)
  }
  if (fe_geq_p(r)) {  // r - p = r + (2^32 + 977) - 2^256
    uint64_t c = (uint64_t)r.v[0] + 977u;
    r.v[0] = (uint32_t)c;
    c = (c >> 32) + (uint64_t)r.v[1] + 1u;
    r.v[1] = (uint32_t)c;
    c >>= 32;
#pragma unroll
    for (int i = 2; i < 8; ++i) {
      c += r.v[i];
      r.v[i] = (uint32_t)c;
      c >>= 32;
    }
  }
}
__device__ __forceinline__ Fe fe_add(const Fe& a, const Fe& b) {
  Fe r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] + b.v[i];
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  fe_fold(r, c);
  return r;
}
__device__ __forceinline__ Fe fe_sub(const Fe& a, const Fe& b) {
  Fe r;
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t d = (int64_t)a.v[i] - (int64_t)b.v[i] + br;
    r.v[i] = (uint32_t)d;
    br = d >> 32;  // 0 or -1
  }
  if (br) {  // a < b: add p back (mod 2^256)
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      c += (uint64_t)r.v[i] + kP[i];
      r.v[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  return r;
}
__device__ __forceinline__ Fe fe_dbl(const Fe& a) { return fe_add(a, a); }
// t (512 bits, 16 limbs) mod p: two folds of the high half by
// 2^256 = 2^32 + 977
__device__ __forceinline__ Fe fe_reduce512(const uint32_t (&t)[16]) {
  // r = lo + hi * 977 + (hi << 32)
  Fe r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)t[i] + (uint64_t)t[8 + i] * 977u + (i ? t[7 + i] : 0u);
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  c += t[15];  // the last shifted limb
  fe_fold(r, c);
  return r;
}
// a * b mod p: 8 x 8 schoolbook rows into 16 limbs, then the fold
__device__ __forceinline__ Fe fe_mul(const Fe& a, const Fe& b) {
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c += (uint64_t)a.v[i] * b.v[j] + t[i + j];
      t[i + j] = (uint32_t)c;
      c >>= 32;
    }
    t[i + 8] = (uint32_t)c;
  }
  return fe_reduce512(t);
}
// a^2 mod p: the 28 products a_i a_j (i < j) once, doubled by a shift, plus
// the 8 squares on the diagonal (36 limb products against fe_mul's 64)
__device__ __forceinline__ Fe fe_sqr(const Fe& a) {
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    uint64_t c = 0;
#pragma unroll
    for (int j = i + 1; j < 8; ++j) {
      c += (uint64_t)a.v[i] * a.v[j] + t[i + j];
      t[i + j] = (uint32_t)c;
      c >>= 32;
    }
    t[i + 8] = (uint32_t)c;  // no earlier row reaches limb i + 8
  }
  uint32_t top = 0;  // off-diagonal sum < 2^511: doubling fits 16 limbs
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t v = t[k];
    t[k] = (v << 1) | top;
    top = v >> 31;
  }
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t sq = (uint64_t)a.v[i] * a.v[i];
    c += (uint64_t)t[2 * i] + (uint32_t)sq;
    t[2 * i] = (uint32_t)c;
    c >>= 32;
    c += (uint64_t)t[2 * i + 1] + (sq >> 32);
    t[2 * i + 1] = (uint32_t)c;
    c >>= 32;
  }
  return fe_reduce512(t);
}
__device__ Fe fe_sqr_n(Fe r, int n) {
  for (int i = 0; i < n; ++i) r = fe_sqr(r);
  return r;
}
// a^(p-2) by an addition chain: p - 2 = 2^256 - 2^32 - 979 is 223 ones, a
// zero, then 0xFFFFFC2D = 22 ones, 00001, 011, 01. x_k = a^(2^k - 1) built
// up to x223 (x_{i+j} = x_i^(2^j) x_j), then the low 33 bits appended:
// 255 squarings and 15 multiplications (square-and-multiply: 255 + 238)
__device__ Fe fe_inv(const Fe& a) {
  const Fe x2 = fe_mul(fe_sqr(a), a);
  const Fe x3 = fe_mul(fe_sqr(x2), a);
  const Fe x6 = fe_mul(fe_sqr_n(x3, 3), x3);
  const Fe x9 = fe_mul(fe_sqr_n(x6, 3), x3);
  const Fe x11 = fe_mul(fe_sqr_n(x9, 2), x2);
  const Fe x22 = fe_mul(fe_sqr_n(x11, 11), x11);
  const Fe x44 = fe_mul(fe_sqr_n(x22, 22), x22);
  const Fe x88 = fe_mul(fe_sqr_n(x44, 44), x44);
  const Fe x176 = fe_mul(fe_sqr_n(x88, 88), x88);
  const Fe x220 = fe_mul(fe_sqr_n(x176, 44), x44);
  const Fe x223 = fe_mul(fe_sqr_n(x220, 3), x3);
  Fe r = fe_mul(fe_sqr_n(x223, 23), x22);  // 223 ones, 0, 22 ones
  r = fe_mul(fe_sqr_n(r, 5), a);           // 00001
  r = fe_mul(fe_sqr_n(r, 3), x2);          // 011
  r = fe_mul(fe_sqr_n(r, 2), a);           // 01
  return r;
}

struct Jac {
  Fe X, Y, Z;  // Z == 0: infinity
};

__device__ __forceinline__ bool jac_inf(const Jac& p) { return fe_is_zero(p.Z); }

// dbl-2009-l (a = 0)
__device__ Jac jac_dbl(const Jac& p) {
  if (jac_inf(p) || fe_is_zero(p.Y)) return Jac{};
  const Fe A = fe_sqr(p.X), B = fe_sqr(p.Y), C = fe_sqr(B);
  const Fe D = fe_dbl(fe_sub(fe_sqr(fe_add(p.X, B)), fe_add(A, C)));
  const Fe E = fe_add(fe_dbl(A), A), F = fe_sqr(E);
  Jac r;
  r.X = fe_sub(F, fe_dbl(D));
  const Fe C8 = fe_dbl(fe_dbl(fe_dbl(C)));
  r.Y = fe_sub(fe_mul(E, fe_sub(D, r.X)), C8);
  r.Z = fe_dbl(fe_mul(p.Y, p.Z));
  return r;
}
// add-2007-bl
__device__ Jac jac_add(const Jac& p, const Jac& q) {
  if (jac_inf(p)) return q;
  if (jac_inf(q)) return p;
  const Fe Z1Z1 = fe_sqr(p.Z), Z2Z2 = fe_sqr(q.Z);
  const Fe U1 = fe_mul(p.X, Z2Z2), U2 = fe_mul(q.X, Z1Z1);
  const Fe S1 = fe_mul(fe_mul(p.Y, q.Z), Z2Z2), S2 = fe_mul(fe_mul(q.Y, p.Z), Z1Z1);
  const Fe H = fe_sub(U2, U1), R = fe_sub(S2, S1);
  if (fe_is_zero(H)) {
    if (fe_is_zero(R)) return jac_dbl(p);
    return Jac{};
  }
  const Fe HH = fe_sqr(H), HHH = fe_mul(H, HH), V = fe_mul(U1, HH);
  Jac r;
  r.X = fe_sub(fe_sub(fe_sqr(R), HHH), fe_dbl(V));
  r.Y = fe_sub(fe_mul(R, fe_sub(V, r.X)), fe_mul(S1, HHH));
  r.Z = fe_mul(fe_mul(p.Z, q.Z), H);
  return r;
}
// p + (x, y) affine (madd-2007-bl style, Z2 = 1)
__device__ Jac jac_madd(const Jac& p, const Fe& x, const Fe& y) {
  if (jac_inf(p)) {
    Jac r;
    r.X = x;
    r.Y = y;
    r.Z = Fe{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    return r;
  }
  const Fe Z1Z1 = fe_sqr(p.Z);
  const Fe U2 = fe_mul(x, Z1Z1), S2 = fe_mul(fe_mul(y, p.Z), Z1Z1);
  const Fe H = fe_sub(U2, p.X), R = fe_sub(S2, p.Y);
  if (fe_is_zero(H)) {
    if (fe_is_zero(R)) return jac_dbl(p);
    return Jac{};
  }
  const Fe HH = fe_sqr(H), HHH = fe_mul(H, HH), V = fe_mul(p.X, HH);
  Jac r;
  r.X = fe_sub(fe_sub(fe_sqr(R), HHH), fe_dbl(V));
  r.Y = fe_sub(fe_mul(R, fe_sub(V, r.X)), fe_mul(p.Y, HHH));
  r.Z = fe_mul(p.Z, H);
  return r;
}

__device__ __forceinline__ Fe load_fe(const uint32_t* w) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = w[i];
  return r;
}

}  // namespace
}  // namespace mpcx

#endif
