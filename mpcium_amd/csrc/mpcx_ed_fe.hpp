// mpcx_ed_fe.hpp -- Ed25519 field and point arithmetic of the Edwards kernels
// (device code): k_ed_msm (mpcx_ed_msm.hip), k_ed_admit (mpcx_ed_admit.hip)
// and the test probe k_ed_probe (mpcx_ed_probe.hip) include the same text, so
// what the probe checks is what the kernels run.
//
// Field: p = 2^255 - 19, eight 32-bit limbs, values kept < p (the contract of
// mpcx_ec_fe.hpp); a product is folded with 2^256 = 38 and bit 255 with
// 2^255 = 19 (mod p), then one conditional subtraction of p. Points: extended
// twisted Edwards coordinates (X, Y, Z, T), x = X/Z, y = Y/Z, T = XY/Z, on
// -x^2 + y^2 = 1 + d x^2 y^2 (a = -1). The addition is the unified
// add-2008-hwcd-3: a = -1 is a square and d is not, so it is complete -- equal
// points, opposite points, the identity (0, 1, 1, 0) and the eight small-order
// points all go through the same straight-line code.
#ifndef MPCX_ED_FE_HPP_
#define MPCX_ED_FE_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcx {
namespace {

struct Fe25 {
  uint32_t v[8];
};

// 2 d, d = -121665 / 121666 (mod p)
__device__ __constant__ const uint32_t kEd2D[8] = {0x26B2F159u, 0xEBD69B94u, 0x8283B156u, 0x00E0149Au,
                                                   0xEEF3D130u, 0x198E80F2u, 0x56DFFCE7u, 0x2406D9DCu};

// a >= p (a < 2^256): bit 255 set, or limbs 1..6 all ones, limb 7 = 2^31 - 1 and limb 0 >= 2^32 - 19
__device__ __forceinline__ bool fe25_geq_p(const Fe25& a) {
  if (a.v[7] >> 31) return true;
  uint32_t hi = a.v[7] | 0x80000000u;
#pragma unroll
  for (int i = 1; i < 7; ++i) hi &= a.v[i];
  return hi == 0xFFFFFFFFu && a.v[0] >= 0xFFFFFFEDu;
}
// r + s (s < 2^32) into r, the carry out of limb 7 returned
__device__ __forceinline__ uint32_t fe25_add_small(Fe25& r, uint32_t s) {
  uint64_t c = s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += r.v[i];
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}
// r + k 2^256 (k < 2^26) mod p, the result < p
__device__ __forceinline__ void fe25_fold(Fe25& r, uint32_t k) {
  while (k) k = fe25_add_small(r, k * 38u);  // 2^256 wrapped: once more (at most twice in total)
  if (r.v[7] >> 31) {                        // bit 255 = 19: r < 2^255 + 19 after it
    r.v[7] &= 0x7FFFFFFFu;
    fe25_add_small(r, 19u);
  }
  if (fe25_geq_p(r)) {  // r - p = r + 19 - 2^255, r < 2^255 + 19
    fe25_add_small(r, 19u);
    r.v[7] &= 0x7FFFFFFFu;
  }
}
__device__ __forceinline__ Fe25 fe25_add(const Fe25& a, const Fe25& b) {
  Fe25 r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] + b.v[i];
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  fe25_fold(r, (uint32_t)c);  // a + b < 2 p < 2^256: c is 0 here
  return r;
}
__device__ __forceinline__ Fe25 fe25_sub(const Fe25& a, const Fe25& b) {
  Fe25 r;
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t d = (int64_t)a.v[i] - (int64_t)b.v[i] + br;
    r.v[i] = (uint32_t)d;
    br = d >> 32;  // 0 or -1
  }
  if (br) {  // a < b: r = a - b + 2^256; + p - 2^256 = r - 19 - 2^255
    int64_t d = (int64_t)r.v[0] - 19;
    r.v[0] = (uint32_t)d;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
      d = (int64_t)r.v[i] + (d >> 32);
      r.v[i] = (uint32_t)d;
    }
    r.v[7] -= 0x80000000u;
  }
  return r;
}
// t (512 bits, 16 limbs) mod p: the high half times 38 onto the low half, then the folds
__device__ __forceinline__ Fe25 fe25_reduce512(const uint32_t (&t)[16]) {
  Fe25 r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)t[i] + (uint64_t)t[8 + i] * 38u;
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  fe25_fold(r, (uint32_t)c);  // c <= 38
  return r;
}
// a * b mod p: 8 x 8 schoolbook rows into 16 limbs, then the fold
__device__ __forceinline__ Fe25 fe25_mul(const Fe25& a, const Fe25& b) {
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
  return fe25_reduce512(t);
}
// a^2 mod p: the 28 products a_i a_j (i < j) once, doubled by a shift, plus
// the 8 squares on the diagonal (36 limb products against fe25_mul's 64)
__device__ __forceinline__ Fe25 fe25_sqr(const Fe25& a) {
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
  return fe25_reduce512(t);
}
__device__ Fe25 fe25_sqr_n(Fe25 r, int n) {
  for (int i = 0; i < n; ++i) r = fe25_sqr(r);
  return r;
}
// a^(p-2) by the usual addition chain: p - 2 = 2^255 - 21 is 250 ones then
// 01011. x_k = a^(2^k - 1): 254 squarings and 11 multiplications
__device__ Fe25 fe25_inv(const Fe25& a) {
  const Fe25 a2 = fe25_sqr(a);
  const Fe25 a9 = fe25_mul(fe25_sqr_n(a2, 2), a);
  const Fe25 a11 = fe25_mul(a9, a2);
  const Fe25 x5 = fe25_mul(fe25_sqr(a11), a9);
  const Fe25 x10 = fe25_mul(fe25_sqr_n(x5, 5), x5);
  const Fe25 x20 = fe25_mul(fe25_sqr_n(x10, 10), x10);
  const Fe25 x40 = fe25_mul(fe25_sqr_n(x20, 20), x20);
  const Fe25 x50 = fe25_mul(fe25_sqr_n(x40, 10), x10);
  const Fe25 x100 = fe25_mul(fe25_sqr_n(x50, 50), x50);
  const Fe25 x200 = fe25_mul(fe25_sqr_n(x100, 100), x100);
  const Fe25 x250 = fe25_mul(fe25_sqr_n(x200, 50), x50);
  return fe25_mul(fe25_sqr_n(x250, 5), a11);
}

__device__ __forceinline__ Fe25 load_fe25(const uint32_t* w) {
  Fe25 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = w[i];
  return r;
}
__device__ __forceinline__ Fe25 fe25_one() { return Fe25{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}; }

struct Ed {
  Fe25 X, Y, Z, T;  // the identity is (0, 1, 1, 0) up to scaling: no special value
};
// a second operand prepared for additions: Y + X, Y - X, 2 Z, 2 d T (a table entry)
struct EdCached {
  Fe25 YpX, YmX, Z2, T2d;
};
// an affine operand prepared for mixed additions: y + x, y - x, 2 d x y (a comb entry)
struct EdAffine {
  Fe25 ypx, ymx, xy2d;
};

__device__ __forceinline__ Ed ed_identity() {
  Ed r = {};
  r.Y.v[0] = 1u;
  r.Z.v[0] = 1u;
  return r;
}
// the affine point (x, y)
__device__ __forceinline__ Ed ed_from_affine(const Fe25& x, const Fe25& y) {
  Ed r;
  r.X = x;
  r.Y = y;
  r.Z = fe25_one();
  r.T = fe25_mul(x, y);
  return r;
}
__device__ EdCached ed_cache(const Ed& p) {
  EdCached c;
  c.YpX = fe25_add(p.Y, p.X);
  c.YmX = fe25_sub(p.Y, p.X);
  c.Z2 = fe25_add(p.Z, p.Z);
  c.T2d = fe25_mul(p.T, load_fe25(kEd2D));
  return c;
}
__device__ __forceinline__ EdAffine ed_affine_entry(const Fe25& x, const Fe25& y) {
  EdAffine e;
  e.ypx = fe25_add(y, x);
  e.ymx = fe25_sub(y, x);
  e.xy2d = fe25_mul(fe25_mul(x, y), load_fe25(kEd2D));
  return e;
}
// the common tail of the additions: E = B - A, F = D - C, G = D + C, H = B + A
__device__ __forceinline__ Ed ed_finish(const Fe25& A, const Fe25& B, const Fe25& C, const Fe25& D) {
  const Fe25 E = fe25_sub(B, A), F = fe25_sub(D, C), G = fe25_add(D, C), H = fe25_add(B, A);
  Ed r;
  r.X = fe25_mul(E, F);
  r.Y = fe25_mul(G, H);
  r.Z = fe25_mul(F, G);
  r.T = fe25_mul(E, H);
  return r;
}
// add-2008-hwcd-3 (a = -1), unified and complete: 8 products
__device__ Ed ed_add(const Ed& p, const EdCached& q) {
  const Fe25 A = fe25_mul(fe25_sub(p.Y, p.X), q.YmX), B = fe25_mul(fe25_add(p.Y, p.X), q.YpX);
  const Fe25 C = fe25_mul(p.T, q.T2d), D = fe25_mul(p.Z, q.Z2);
  return ed_finish(A, B, C, D);
}
// the same with Z2 = 1 (madd-2008-hwcd-3): 7 products
__device__ Ed ed_madd(const Ed& p, const EdAffine& q) {
  const Fe25 A = fe25_mul(fe25_sub(p.Y, p.X), q.ymx), B = fe25_mul(fe25_add(p.Y, p.X), q.ypx);
  const Fe25 C = fe25_mul(p.T, q.xy2d), D = fe25_add(p.Z, p.Z);
  return ed_finish(A, B, C, D);
}
// dbl-2008-hwcd (a = -1): 4 squarings and 4 products; it does not read T
__device__ Ed ed_dbl(const Ed& p) {
  const Fe25 A = fe25_sqr(p.X), B = fe25_sqr(p.Y), ZZ = fe25_sqr(p.Z), C = fe25_add(ZZ, ZZ);
  const Fe25 E = fe25_sub(fe25_sub(fe25_sqr(fe25_add(p.X, p.Y)), A), B);
  const Fe25 G = fe25_sub(B, A), F = fe25_sub(G, C), H = fe25_sub(fe25_sub(Fe25{}, A), B);
  Ed r;
  r.X = fe25_mul(E, F);
  r.Y = fe25_mul(G, H);
  r.Z = fe25_mul(F, G);
  r.T = fe25_mul(E, H);
  return r;
}

}  // namespace
}  // namespace mpcx

#endif
