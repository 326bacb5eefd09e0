// mpcx_ed_admit.hip -- admission of received Ed25519 points on gfx950, what
// tss-lib does to every commitment point of a keygen or resharing round
// (up:eddsa/keygen round 3): crypto.NewECPoint's check that the coordinates are
// field elements on the curve, then EightInvEight, P -> 8 (c P) with
// c = 8^-1 mod L, which keeps the order-L component of P and drops any
// small-order one. One thread per point, over the field and point code of
// k_ed_msm (mpcx_ed_fe.hpp).
//
// The scalar is a constant, so the chain is fixed: c in non-adjacent form has
// 252 digits, 44 of them nonzero, the top one +1. The accumulator starts as P,
// then 251 doublings with a mixed addition of +P or -P after 43 of them, then 3
// doublings and one inversion. No table, no workspace, no LDS; the loop counter
// and the digit are scalar, so every branch is wave-uniform. A rejected lane
// runs the chain on the identity and its result is dropped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcx_ed_fe.hpp"

namespace mpcx {
namespace {

// the non-adjacent form of c = 8^-1 mod L, digits 0..250 (digit 251 is +1):
// bit i of kAdmitPos is a digit +1, of kAdmitNeg a digit -1
constexpr int kAdmitTop = 251;
__device__ __constant__ const uint32_t kAdmitPos[8] = {0x04004001u, 0x8108052Au, 0x01210010u, 0x08142004u,
                                                       0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u};
__device__ __constant__ const uint32_t kAdmitNeg[8] = {0x21241088u, 0x20012000u, 0x84042540u, 0x00408250u,
                                                       0x00000000u, 0x00000000u, 0x00000000u, 0x02000000u};

// d = -121665 / 121666 (mod p)
__device__ __constant__ const uint32_t kEdD[8] = {0x135978A3u, 0x75EB4DCAu, 0x4141D8ABu, 0x00700A4Du,
                                                  0x7779E898u, 0x8CC74079u, 0x2B6FFE73u, 0x52036CEEu};

__device__ __forceinline__ bool fe25_eq(const Fe25& a, const Fe25& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.v[i] ^ b.v[i];
  return d == 0;
}

}  // namespace

// pts: count x 16 words (x, y, any 256-bit values), out: count x 16 words,
// status: count bytes (0 accepted, 1 a coordinate >= p, 2 not on the curve)
__global__ __launch_bounds__(64) void k_ed_admit(const uint32_t* __restrict__ pts, uint32_t* __restrict__ out,
                                                 uint8_t* __restrict__ status, uint32_t count, uint32_t clear) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  const bool active = item < count;
  Fe25 x = {}, y = fe25_one();  // the identity stands in for an inactive or rejected lane
  uint32_t st = 0;
  if (active) {
    x = load_fe25(pts + (size_t)item * 16u);
    y = load_fe25(pts + (size_t)item * 16u + 8u);
    if (fe25_geq_p(x) || fe25_geq_p(y)) st = 1;
  }
  if (st) {
    x = Fe25{};
    y = fe25_one();
  }
  // -x^2 + y^2 = 1 + d x^2 y^2, both sides < p
  const Fe25 xx = fe25_sqr(x), yy = fe25_sqr(y);
  const Fe25 lhs = fe25_sub(yy, xx);
  const Fe25 rhs = fe25_add(fe25_one(), fe25_mul(fe25_mul(xx, yy), load_fe25(kEdD)));
  if (!fe25_eq(lhs, rhs)) {  // never a substituted lane: the identity is on the curve
    st = 2;
    x = Fe25{};
    y = fe25_one();
  }
  if (clear) {  // a kernel argument: wave-uniform
    const EdAffine q = ed_affine_entry(x, y);
    const Fe25 nxy2d = fe25_sub(Fe25{}, q.xy2d);
    Ed acc = ed_from_affine(x, y);
    for (int i = kAdmitTop - 1; i >= 0; --i) {
      acc = ed_dbl(acc);
      const uint32_t w = (uint32_t)i >> 5, b = (uint32_t)i & 31u;
      const bool pos = (kAdmitPos[w] >> b) & 1u, neg = (kAdmitNeg[w] >> b) & 1u;
      if (pos || neg) {
        // one addition for both signs (one copy of its code in the loop); -P:
        // y + x and y - x change places, 2 d x y changes sign
        EdAffine s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s.ypx.v[j] = neg ? q.ymx.v[j] : q.ypx.v[j];
          s.ymx.v[j] = neg ? q.ypx.v[j] : q.ymx.v[j];
          s.xy2d.v[j] = neg ? nxy2d.v[j] : q.xy2d.v[j];
        }
        acc = ed_madd(acc, s);
      }
    }
    acc = ed_dbl(acc);
    acc = ed_dbl(acc);
    acc = ed_dbl(acc);
    const Fe25 zi = fe25_inv(acc.Z);  // Z is never zero: the addition is complete
    x = fe25_mul(acc.X, zi);
    y = fe25_mul(acc.Y, zi);
  }
  if (!active) return;
  uint32_t* o = out + (size_t)item * 16u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] = st ? 0u : x.v[i];
    o[8 + i] = st ? 0u : y.v[i];
  }
  status[item] = (uint8_t)st;
}

}  // namespace mpcx

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ed_admit(const uint32_t* pts, uint32_t* out,
                                                                      uint8_t* status, uint32_t count,
                                                                      uint32_t clear, hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ed_admit, dim3(blocks), dim3(64), 0, st, pts, out, status, count, clear);
  return hipGetLastError();
}
