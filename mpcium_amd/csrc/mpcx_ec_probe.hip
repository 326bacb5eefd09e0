// mpcx_ec_probe.hip -- one secp256k1 field or point operation per thread, for
// tests and tools (C-ABI mpcx_ec_probe): the device functions k_ec_combine is
// made of (mpcx_ec_fe.hpp), reachable one at a time so that their carry and
// exceptional-case branches can be driven with chosen operands and compared
// with integer arithmetic. Not on any hot path.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcx.h"
#include "mpcx_ec_fe.hpp"

namespace mpcx {
namespace {

__device__ __forceinline__ Jac load_jac(const uint32_t* w) {
  Jac p;
  p.X = load_fe(w);
  p.Y = load_fe(w + 8);
  p.Z = load_fe(w + 16);
  return p;
}

}  // namespace

// a, b: count x 24 words (a Jacobian point X, Y, Z, or a field element in the
// first 8 words; jac_madd reads b's X, Y as the affine point), out: count x 24
// words (a field result in the first 8, the rest zero). Every input limb
// string is < p (checked by the host entry).
__global__ __launch_bounds__(64) void k_ec_probe(uint32_t op, const uint32_t* __restrict__ a,
                                                 const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                                 uint32_t count) {
  const uint32_t item = blockIdx.x * 64u + threadIdx.x;
  if (item >= count) return;
  const uint32_t* pa = a + (size_t)item * 24u;
  const uint32_t* pb = b + (size_t)item * 24u;
  Jac r = {};
  switch (op) {
    case MPCX_EC_OP_ADD: r.X = fe_add(load_fe(pa), load_fe(pb)); break;
    case MPCX_EC_OP_SUB: r.X = fe_sub(load_fe(pa), load_fe(pb)); break;
    case MPCX_EC_OP_MUL: r.X = fe_mul(load_fe(pa), load_fe(pb)); break;
    case MPCX_EC_OP_SQR: r.X = fe_sqr(load_fe(pa)); break;
    case MPCX_EC_OP_INV: r.X = fe_inv(load_fe(pa)); break;
    case MPCX_EC_OP_JAC_DBL: r = jac_dbl(load_jac(pa)); break;
    case MPCX_EC_OP_JAC_ADD: r = jac_add(load_jac(pa), load_jac(pb)); break;
    case MPCX_EC_OP_JAC_MADD: r = jac_madd(load_jac(pa), load_fe(pb), load_fe(pb + 8)); break;
    default: break;
  }
  uint32_t* o = out + (size_t)item * 24u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] = r.X.v[i];
    o[8 + i] = r.Y.v[i];
    o[16 + i] = r.Z.v[i];
  }
}

}  // namespace mpcx

extern "C" __attribute__((visibility("hidden"))) hipError_t mpcx_launch_ec_probe(uint32_t op, const uint32_t* a,
                                                                      const uint32_t* b, uint32_t* out,
                                                                      uint32_t count, hipStream_t st) {
  const uint32_t blocks = (count + 63u) / 64u;
  if (!blocks) return hipSuccess;
  hipLaunchKernelGGL(mpcx::k_ec_probe, dim3(blocks), dim3(64), 0, st, op, a, b, out, count);
  return hipGetLastError();
}
