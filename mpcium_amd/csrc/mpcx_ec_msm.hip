// mpcx_ec_msm.hip -- batched secp256k1 multi-scalar sums on gfx950:
//   out_i = a_i G + sum_{k < n_points} b_ik P_ik,   1 <= n_points <= 16
// The point equations of Feldman VSS (up:crypto/vss feldman_vss.go): the share
// check s G == sum_k id^k V_k, the public shares X_j = sum_k id_j^k Vc_k and
// plain sums of points (every scalar 1). One thread per item, as k_ec_combine
// (mpcx_ec.hip), over the same field and point code (mpcx_ec_fe.hpp).
//
// Straus with 4-bit windows: a 15-entry Jacobian table per point (1..15 P_k by
// mixed additions) in a lane-coalesced global workspace, one chain of doublings
// shared by all points, one jac_add per point and window with a nonzero nibble.
// The window loop starts at the highest window in which any lane of the
// wavefront has a nonzero nibble (a wave-uniform bound), so small scalars cost
// a few windows and a wavefront of zero scalars none. The nibble words are read
// from memory when needed: 16 scalars do not fit in registers beside the point
// arithmetic. a G comes last from the device's 8-bit base-point comb.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcx_ec_fe.hpp"  // Fe, Jac, fe_* and jac_*: shared with k_ec_combine and the probe
#include "mpcx_internal.h"

namespace mpcx {
namespace {

constexpr uint32_t kMsmPointWords = 15u * 24u * 64u;  // one point's tables of one block

// per-thread table workspace of one block: [point][entry 0..14][word 0..23][lane]
__device__ __forceinline__ void msm_put(uint32_t* ws, uint32_t e, const Jac& p) {
  const uint32_t lane = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ws[((e * 24u) + i) * 64u + lane] = p.X.v[i];
    ws[((e * 24u) + 8u + i) * 64u + lane] = p.Y.v[i];
    ws[((e * 24u) + 16u + i) * 64u + lane] = p.Z.v[i];
  }
}
__device__ __forceinline__ Jac msm_get(const uint32_t* ws, uint32_t e) {
  const uint32_t lane = threadIdx.x;
  Jac p;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    p.X.v[i] = ws[((e * 24u) + i) * 64u + lane];
    p.Y.v[i] = ws[((e * 24u) + 8u + i) * 64u + lane];
    p.Z.v[i] = ws[((e * 24u) + 16u + i) * 64u + lane];
  }
  return p;
}

}  // namespace

// a: count x 8 words or null (no G term), sc: count x n_points x 8 words,
// pts: count x n_points x 16 words (x, y; all-zero = infinity), out: count x 16
// words (x, y; all-zero = infinity), gtab: 32 x 255 affine points of
// d 256^w G, ws: blocks x n_points x 15 x 24 x 64 words
__global__ __launch_bounds__(64) void k_ec_msm(const uint32_t* __restrict__ a, const uint32_t* __restrict__ sc,
                                               const uint32_t* __restrict__ pts, uint32_t* __restrict__ out,
                                               const uint32_t* __restrict__ gtab, uint32_t* __restrict__ ws_all,
                                               uint32_t count, uint32_t n_points) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  const bool active = item < count;
  uint32_t* ws = ws_all + (size_t)blockIdx.x * n_points * kMsmPointWords;
  // an inactive lane keeps use == 0 and top == -1: it reads no scalar, point or
  // table word and contributes nothing to the wave's window bound
  const uint32_t* s = sc + (size_t)(active ? item : 0u) * n_points * 8u;
  const uint32_t* pp = pts + (size_t)(active ? item : 0u) * n_points * 16u;
  uint32_t use = 0;  // bit k: term k has a nonzero scalar and a finite point
  int top = -1;      // highest window with a nonzero nibble among the used terms
  for (uint32_t k = 0; active && k < n_points; ++k) {
    uint32_t ob = 0, op = 0;
    int hi = -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t w = s[k * 8u + i];
      ob |= w;
      if (w) hi = i * 8 + (31 - __clz(w)) / 4;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) op |= pp[k * 16u + i];
    if (!ob || !op) continue;
    use |= 1u << k;
    top = hi > top ? hi : top;
    // table j P_k for j = 1..15
    Jac base;
    base.X = load_fe(pp + k * 16u);
    base.Y = load_fe(pp + k * 16u + 8u);
    base.Z = Fe{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
    Jac t = base;
    msm_put(ws, k * 15u, t);
    for (uint32_t j = 2; j <= 15; ++j) {
      t = jac_madd(t, base.X, base.Y);
      msm_put(ws, k * 15u + j - 1u, t);
    }
  }
  // the wave's highest window: all 64 lanes of the block are here
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const int v = __shfl_xor(top, o);
    top = v > top ? v : top;
  }
  top = __builtin_amdgcn_readfirstlane(top);
  Jac acc = {};
  for (int w = top; w >= 0; --w) {
    if (!jac_inf(acc)) {
      acc = jac_dbl(acc);
      acc = jac_dbl(acc);
      acc = jac_dbl(acc);
      acc = jac_dbl(acc);
    }
    for (uint32_t k = 0; k < n_points; ++k) {
      if (!((use >> k) & 1u)) continue;
      const uint32_t d = (s[k * 8u + ((uint32_t)w >> 3)] >> (((uint32_t)w & 7u) * 4u)) & 15u;
      if (d) acc = jac_add(acc, msm_get(ws, k * 15u + d - 1u));
    }
  }
  // + a G: one mixed addition per nonzero byte of a
  if (a && active) {
    const uint32_t* sa = a + (size_t)item * 8u;
    for (int j = 0; j < 32; ++j) {
      const uint32_t d = (sa[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
      if (!d) continue;
      const uint32_t* e = gtab + ((size_t)j * 255u + (d - 1u)) * 16u;
      acc = jac_madd(acc, load_fe(e), load_fe(e + 8));
    }
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

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ec_msm(const uint32_t* a, const uint32_t* sc,
                                                                    const uint32_t* pts, uint32_t* out,
                                                                    const uint32_t* gtab, uint32_t* ws, uint32_t count,
                                                                    uint32_t n_points, hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ec_msm, dim3(blocks), dim3(64), 0, st, a, sc, pts, out, gtab, ws, count, n_points);
  return hipGetLastError();
}
