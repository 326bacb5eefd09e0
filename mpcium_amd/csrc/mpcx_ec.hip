// mpcx_ec.hip -- batched secp256k1 point combinations on gfx950:
//   out_i = a_i G + b_i P_i + c_i Q_i
// Every point equation of tss-lib's GG18 signing outside the MtA is one of
// these (up:ecdsa/signing round_1.go .. finalize.go; btcec/v2 S256 arithmetic,
// /root/reference/go.mod:29): Gamma_i = gamma_i G, the Schnorr / ZKV proofs'
// alpha = a G (+ b R) and their checks t G - c X == alpha, R = theta^-1 sum
// Gamma, V_i = s_i R + l_i G, U_i = rho_i V, and ecdsa.Verify's u1 G + u2 X.
// One thread per item: the batch is thousands of independent small
// computations (wallets x signers), integer work with no shared operand.
//
// Field: p = 2^256 - 2^32 - 977, eight 32-bit limbs, values kept < p; a product
// is folded with 2^256 = 2^32 + 977 (mod p). Points: Jacobian (X, Y, Z) with
// a = 0 formulas (dbl-2009-l, add-2007-bl, madd-2007-bl). a G uses a fixed-base
// comb of 8-bit windows (32 x 255 affine points, 522 KB in HBM, built once per
// device by this kernel itself as plain multiples of G: 32 mixed additions, no
// doublings); b P + c Q share
// 256 doublings with 4-bit windows (Shamir's trick; 15-entry Jacobian tables per
// thread in a lane-coalesced global workspace). One field inversion per item
// returns the affine result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcx_ec_fe.hpp"  // Fe, Jac, fe_* and jac_*: shared with the test probe
#include "mpcx_internal.h"

namespace mpcx {
namespace {

// per-thread table workspace: entry e (0..29: P's 1..15, Q's 1..15), coordinate
// word k (24 per Jacobian point), lane-coalesced across the block
__device__ __forceinline__ void tbl_put(uint32_t* ws, int e, const Jac& p) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ws[((e * 24) + i) * 64 + lane] = p.X.v[i];
    ws[((e * 24) + 8 + i) * 64 + lane] = p.Y.v[i];
    ws[((e * 24) + 16 + i) * 64 + lane] = p.Z.v[i];
  }
}
__device__ __forceinline__ Jac tbl_get(const uint32_t* ws, int e) {
  const int lane = threadIdx.x;
  Jac p;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    p.X.v[i] = ws[((e * 24) + i) * 64 + lane];
    p.Y.v[i] = ws[((e * 24) + 8 + i) * 64 + lane];
    p.Z.v[i] = ws[((e * 24) + 16 + i) * 64 + lane];
  }
  return p;
}

__device__ __forceinline__ uint32_t nibble(const uint32_t* k, int w) { return (k[w >> 3] >> ((w & 7) * 4)) & 15u; }

}  // namespace

// a: count x 24 words (a, b, c), pts: count x 32 words (P.x, P.y, Q.x, Q.y;
// all-zero = infinity), out: count x 16 words (x, y; all-zero = infinity),
// gtab: 32 x 255 affine points (x, y as 8 words each) of d 256^w G, ws: the
// per-thread tables (blocks x 30 x 24 x 64 words)
__global__ __launch_bounds__(64) void k_ec_combine(const uint32_t* __restrict__ sc, const uint32_t* __restrict__ pts,
                                                   uint32_t* __restrict__ out, const uint32_t* __restrict__ gtab,
                                                   uint32_t* __restrict__ ws_all, uint32_t count) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  const bool active = item < count;
  uint32_t* ws = ws_all + (size_t)blockIdx.x * (30u * 24u * 64u);
  const uint32_t* s = sc + (size_t)(active ? item : 0u) * 24u;
  const uint32_t* pp = pts + (size_t)(active ? item : 0u) * 32u;
  uint32_t kb[8], kc[8];
  bool usep = false, useq = false;
  {
    uint32_t ob = 0, oc = 0, op = 0, oq = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      kb[i] = active ? s[8 + i] : 0u;
      kc[i] = active ? s[16 + i] : 0u;
      ob |= kb[i];
      oc |= kc[i];
      op |= pp[i] | pp[8 + i];
      oq |= pp[16 + i] | pp[24 + i];
    }
    usep = ob && op;
    useq = oc && oq;
  }
  // tables kP, kQ for k = 1..15
  for (int t = 0; t < 2; ++t) {
    if (!(t ? useq : usep)) continue;
    Jac base;
    base.X = load_fe(pp + 16 * t);
    base.Y = load_fe(pp + 16 * t + 8);
    base.Z = Fe{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    Jac acc = base;
    tbl_put(ws, 15 * t, acc);
    for (int k = 2; k <= 15; ++k) {
      acc = jac_madd(acc, base.X, base.Y);
      tbl_put(ws, 15 * t + k - 1, acc);
    }
  }
  Jac acc = {};
  if (usep || useq) {
    for (int w = 63; w >= 0; --w) {
      if (!jac_inf(acc)) {
        acc = jac_dbl(acc);
        acc = jac_dbl(acc);
        acc = jac_dbl(acc);
        acc = jac_dbl(acc);
      }
      if (usep) {
        const uint32_t d = nibble(kb, w);
        if (d) acc = jac_add(acc, tbl_get(ws, (int)d - 1));
      }
      if (useq) {
        const uint32_t d = nibble(kc, w);
        if (d) acc = jac_add(acc, tbl_get(ws, 15 + (int)d - 1));
      }
    }
  }
  // + a G: one mixed addition per nonzero byte of a
  for (int j = 0; j < 32; ++j) {
    const uint32_t d = active ? (s[j >> 2] >> ((j & 3) * 8)) & 0xFFu : 0u;
    if (!d) continue;
    const uint32_t* e = gtab + ((size_t)j * 255u + (d - 1u)) * 16u;
    acc = jac_madd(acc, load_fe(e), load_fe(e + 8));
  }
  if (!active) return;
  uint32_t* o = out + (size_t)item * 16u;
  if (jac_inf(acc)) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0u;
    return;
  }
  const Fe zi = fe_inv(acc.Z), zi2 = fe_sqr(zi), zi3 = fe_mul(zi2, zi);
  const Fe x = fe_mul(acc.X, zi2), y = fe_mul(acc.Y, zi3);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] = x.v[i];
    o[8 + i] = y.v[i];
  }
}

}  // namespace mpcx

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ec_combine(const uint32_t* sc, const uint32_t* pts,
                                                                        uint32_t* out, const uint32_t* gtab,
                                                                        uint32_t* ws, uint32_t count,
                                                                        hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ec_combine, dim3(blocks), dim3(64), 0, st, sc, pts, out, gtab, ws, count);
  return hipGetLastError();
}
