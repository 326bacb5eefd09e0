// mpcx_ed_probe.hip -- one Ed25519 field or point operation per thread, for
// tests and tools (C-ABI mpcx_ed_probe): the device functions k_ed_msm is made
// of (mpcx_ed_fe.hpp), reachable one at a time so that their carry branches
// and the exceptional inputs of the point formulas can be driven with chosen
// operands and compared with integer arithmetic. Not on any hot path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcx.h"
#include "mpcx_ed_fe.hpp"

namespace mpcx {
namespace {

__device__ __forceinline__ Ed load_ed(const uint32_t* w) {
  Ed p;
  p.X = load_fe25(w);
  p.Y = load_fe25(w + 8);
  p.Z = load_fe25(w + 16);
  p.T = load_fe25(w + 24);
  return p;
}

}  // namespace

// a, b: count x 32 words (an extended point X, Y, Z, T, or a field element in
// the first 8 words; ed_madd reads b's first 24 words as the affine entry
// y + x, y - x, 2 d x y), out: count x 32 words (a field result in the first
// 8, the rest zero). Every input limb string is < p (checked by the host entry).
__global__ __launch_bounds__(64) void k_ed_probe(uint32_t op, const uint32_t* __restrict__ a,
                                                 const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                                 uint32_t count) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  if (item >= count) return;
  const uint32_t* pa = a + (size_t)item * 32u;
  const uint32_t* pb = b + (size_t)item * 32u;
  Ed r = {};
  switch (op) {
    case MPCX_ED_OP_ADD: r.X = fe25_add(load_fe25(pa), load_fe25(pb)); break;
    case MPCX_ED_OP_SUB: r.X = fe25_sub(load_fe25(pa), load_fe25(pb)); break;
    case MPCX_ED_OP_MUL: r.X = fe25_mul(load_fe25(pa), load_fe25(pb)); break;
    case MPCX_ED_OP_SQR: r.X = fe25_sqr(load_fe25(pa)); break;
    case MPCX_ED_OP_INV: r.X = fe25_inv(load_fe25(pa)); break;
    case MPCX_ED_OP_ED_DBL: r = ed_dbl(load_ed(pa)); break;
    case MPCX_ED_OP_ED_ADD: r = ed_add(load_ed(pa), ed_cache(load_ed(pb))); break;
    case MPCX_ED_OP_ED_MADD: {
      EdAffine q;
      q.ypx = load_fe25(pb);
      q.ymx = load_fe25(pb + 8);
      q.xy2d = load_fe25(pb + 16);
      r = ed_madd(load_ed(pa), q);
      break;
    }
    default: break;
  }
  uint32_t* o = out + (size_t)item * 32u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] = r.X.v[i];
    o[8 + i] = r.Y.v[i];
    o[16 + i] = r.Z.v[i];
    o[24 + i] = r.T.v[i];
  }
}

}  // namespace mpcx

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ed_probe(uint32_t op, const uint32_t* a,
                                                                      const uint32_t* b, uint32_t* out,
                                                                      uint32_t count, hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ed_probe, dim3(blocks), dim3(64), 0, st, op, a, b, out, count);
  return hipGetLastError();
}
