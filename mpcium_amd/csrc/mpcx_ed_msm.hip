// mpcx_ed_msm.hip -- batched Ed25519 multi-scalar sums on gfx950:
//   out_i = a_i B + sum_{k < n_points} b_ik P_ik,   0 <= n_points <= 16
// The point equations of tss-lib's threshold EdDSA (up:eddsa/signing): R_i =
// r_i B (n_points = 0), the Schnorr check t B - c R_j, R = sum R_j (scalars 1)
// and edwards.Verify's s B - h A. One thread per item, the shape of k_ec_msm
// (mpcx_ec_msm.hip), over the Edwards field and point code (mpcx_ed_fe.hpp).
//
// Straus with 4-bit windows: a 15-entry table per point (1..15 P_k, each entry
// prepared for additions as Y + X, Y - X, 2 Z, 2 d T) in a lane-coalesced
// global workspace, one chain of doublings shared by all points, one ed_add per
// point and window with a nonzero nibble. The window loop starts at the highest
// window in which any lane of the wavefront has a nonzero nibble (a
// wave-uniform bound). The addition is complete, so the accumulator starts as
// the identity and no case is told apart. a B comes last from the device's
// 8-bit base-point comb. Scalars are used as 256-bit integers, not reduced mod
// the group order L: the same point for a point of order L, and defined for the
// small-order ones.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcx_ed_fe.hpp"  // Fe25, Ed, fe25_* and ed_*: shared with the probe
#include "mpcx_internal.h"

namespace mpcx {
namespace {

constexpr uint32_t kEdPointWords = 15u * 32u * 64u;  // one point's tables of one block

// per-thread table workspace of one block: [point][entry 0..14][word 0..31][lane]
__device__ __forceinline__ void ed_put(uint32_t* ws, uint32_t e, const EdCached& p) {
  const uint32_t lane = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ws[((e * 32u) + i) * 64u + lane] = p.YpX.v[i];
    ws[((e * 32u) + 8u + i) * 64u + lane] = p.YmX.v[i];
    ws[((e * 32u) + 16u + i) * 64u + lane] = p.Z2.v[i];
    ws[((e * 32u) + 24u + i) * 64u + lane] = p.T2d.v[i];
  }
}
__device__ __forceinline__ EdCached ed_get(const uint32_t* ws, uint32_t e) {
  const uint32_t lane = threadIdx.x;
  EdCached p;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    p.YpX.v[i] = ws[((e * 32u) + i) * 64u + lane];
    p.YmX.v[i] = ws[((e * 32u) + 8u + i) * 64u + lane];
    p.Z2.v[i] = ws[((e * 32u) + 16u + i) * 64u + lane];
    p.T2d.v[i] = ws[((e * 32u) + 24u + i) * 64u + lane];
  }
  return p;
}

}  // namespace

// a: count x 8 words or null (no B term), sc: count x n_points x 8 words,
// pts: count x n_points x 16 words (x, y; all-zero = no term), out: count x 16
// words (x, y; the identity is (0, 1)), btab: 32 x 255 comb entries of
// d 256^w B (y + x, y - x, 2 d x y: 24 words), ws: blocks x n_points x 15 x 32
// x 64 words
__global__ __launch_bounds__(64) void k_ed_msm(const uint32_t* __restrict__ a, const uint32_t* __restrict__ sc,
                                               const uint32_t* __restrict__ pts, uint32_t* __restrict__ out,
                                               const uint32_t* __restrict__ btab, uint32_t* __restrict__ ws_all,
                                               uint32_t count, uint32_t n_points) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  const bool active = item < count;
  uint32_t* ws = ws_all + (size_t)blockIdx.x * n_points * kEdPointWords;
  // an inactive lane keeps use == 0 and top == -1: it reads no scalar, point or
  // table word and contributes nothing to the wave's window bound
  const uint32_t* s = sc + (size_t)(active ? item : 0u) * n_points * 8u;
  const uint32_t* pp = pts + (size_t)(active ? item : 0u) * n_points * 16u;
  uint32_t use = 0;  // bit k: term k has a nonzero scalar and a point that is not all-zero
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
    Ed t = ed_from_affine(load_fe25(pp + k * 16u), load_fe25(pp + k * 16u + 8u));
    const EdCached base = ed_cache(t);
    ed_put(ws, k * 15u, base);
    for (uint32_t j = 2; j <= 15; ++j) {
      t = ed_add(t, base);
      ed_put(ws, k * 15u + j - 1u, ed_cache(t));
    }
  }
  // the wave's highest window: all 64 lanes of the block are here
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const int v = __shfl_xor(top, o);
    top = v > top ? v : top;
  }
  top = __builtin_amdgcn_readfirstlane(top);
  Ed acc = ed_identity();
  for (int w = top; w >= 0; --w) {
    if (w != top) {  // wave-uniform: the accumulator is the identity before the first window
      acc = ed_dbl(acc);
      acc = ed_dbl(acc);
      acc = ed_dbl(acc);
      acc = ed_dbl(acc);
    }
    for (uint32_t k = 0; k < n_points; ++k) {
      if (!((use >> k) & 1u)) continue;
      const uint32_t d = (s[k * 8u + ((uint32_t)w >> 3)] >> (((uint32_t)w & 7u) * 4u)) & 15u;
      if (d) acc = ed_add(acc, ed_get(ws, k * 15u + d - 1u));
    }
  }
  // + a B: one mixed addition per nonzero byte of a
  if (a && active) {
    const uint32_t* sa = a + (size_t)item * 8u;
    for (int j = 0; j < 32; ++j) {
      const uint32_t d = (sa[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
      if (!d) continue;
      const uint32_t* e = btab + ((size_t)j * 255u + (d - 1u)) * 24u;
      EdAffine q;
      q.ypx = load_fe25(e);
      q.ymx = load_fe25(e + 8);
      q.xy2d = load_fe25(e + 16);
      acc = ed_madd(acc, q);
    }
  }
  if (!active) return;
  const Fe25 zi = fe25_inv(acc.Z);  // Z is never zero: the addition is complete
  const Fe25 x = fe25_mul(acc.X, zi), y = fe25_mul(acc.Y, zi);
  uint32_t* o = out + (size_t)item * 16u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] = x.v[i];
    o[8 + i] = y.v[i];
  }
}

// The comb's entries from affine points: in: count x 16 words (x, y), out:
// count x 24 words (y + x, y - x, 2 d x y). Runs once per device.
__global__ __launch_bounds__(64) void k_ed_comb_entries(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                        uint32_t count) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  if (item >= count) return;
  const EdAffine e = ed_affine_entry(load_fe25(in + (size_t)item * 16u), load_fe25(in + (size_t)item * 16u + 8u));
  uint32_t* o = out + (size_t)item * 24u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] = e.ypx.v[i];
    o[8 + i] = e.ymx.v[i];
    o[16 + i] = e.xy2d.v[i];
  }
}

}  // namespace mpcx

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ed_msm(const uint32_t* a, const uint32_t* sc,
                                                                    const uint32_t* pts, uint32_t* out,
                                                                    const uint32_t* btab, uint32_t* ws, uint32_t count,
                                                                    uint32_t n_points, hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ed_msm, dim3(blocks), dim3(64), 0, st, a, sc, pts, out, btab, ws, count, n_points);
  return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ed_comb_entries(const uint32_t* in,
                                                                             uint32_t* out, uint32_t count,
                                                                             hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ed_comb_entries, dim3(blocks), dim3(64), 0, st, in, out, count);
  return hipGetLastError();
}
