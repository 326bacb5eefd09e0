// mpcx_device.hpp -- gfx950 (MI355X, CDNA4) batched modular exponentiation:
// device code shared by the per-geometry translation units (mpcx_geom.hip)
// and the primality kernels (mpcx_prime.hip).
//
// Replaces the arithmetic of Go math/big (*Int).Exp -> nat.expNNMontgomery
// (go1.23.5, go:src/math/big/nat.go) as reached through tss-lib v2.0.2
// common.ModInt(m).Exp (up:common/int.go) on mpcium's hot path
// (/root/reference/pkg/mpc/session.go:199 -> party.UpdateFromBytes -> Paillier /
// MtA proofs; /root/reference/pkg/mpc/node.go:69 -> GeneratePreParams).
//
// Design (DESIGN.md section "Kernels"):
//  * Radix 2^28 digits held in 64-bit lazy accumulators. A 28x28-bit product
//    is < 2^56, so an accumulator absorbs > 100 products before it can
//    overflow: every multiply-accumulate is ONE v_mad_u64_u32 (half rate on
//    gfx950, measured ~33.8 T/s/GPU), with no per-MAC carry instruction --
//    the carry-writing v_add_co/v_addc are half rate as well, so a 32-bit-limb
//    carry chain would cost >= 2 half-rate ops per MAC.
//  * Wavefront-cooperative operands: one 64-lane wavefront holds G operands;
//    operand g is spread over P lanes, each lane holding K consecutive digits
//    (L = P*K digits, R = 2^(28L) > 4m so no conditional subtraction is ever
//    needed inside the exponentiation: almost-Montgomery, results < 2m).
//  * Row-wise (CIOS) Montgomery: per digit b_i of the multiplier, every lane
//    does K mads for a*b_i, the group's lane 0 derives m_i, one ds_bpermute
//    broadcasts it, K more mads for m_i*N, then the accumulator window shifts
//    one digit: within a lane by register renaming (the K-iteration block is
//    unrolled), across lanes by ONE DPP wave_shl of a 28-bit value (the slot's
//    high part is folded into the next slot first).
//  * Exponentiation: a shared exponent follows a sliding-window schedule (odd
//    powers, windows of up to 6 bits, built on the device by k_expsched);
//    per-operand exponents use Go's fixed 4-bit window. Tables (<= 33 entries
//    per operand) live in a global workspace, lane-coalesced; b operands are
//    staged in LDS and read as group-broadcast ds_read_b32.
//  * The per-operand product is not a dense contraction. The REDUCTION of a
//    batch that shares its modulus is (fixed Toeplitz matrices of m'' and m):
//    geometry 2 runs it on the i8 matrix cores, k_modexp_mx (mpcx_mx.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mpcx_internal.h"

#if defined(MX_EMIT) || defined(MX_ITER_FENCE) || defined(MX_SPLIT_MAD) || defined(MX_READ_FENCE) ||          \
    defined(MX_PRIO) || defined(MX_PRIO_P) || defined(MX_PRIO_F) || defined(MX_PRIO_R) || defined(MX_PRIO_R2) || \
    defined(MX_PRIO_C) || defined(MX_CARRY_SKIP) || defined(MPCX_SCHED_BARRIER) || defined(MPCX_SQR_OPT) ||      \
    defined(MPCX_PREFETCH_B) || defined(MPCX_SQR_B2) || defined(MPCX_PRIME2C_DBL_FOLD)
#error "retired A/B switch; see DESIGN.md 5.2g"
#endif

#ifndef MPCX_PREFETCH2_KMAX
#define MPCX_PREFETCH2_KMAX 24  // montmul reads b two digits ahead for K below this
#endif
#ifndef MPCX_BLOCK_FENCE
#define MPCX_BLOCK_FENCE 0  // 1: scheduling fence between montmul's P blocks (the prime kernels' TU sets it)
#endif
#ifndef MPCX_WAVES_PER_EU_PRIME2C
#define MPCX_WAVES_PER_EU_PRIME2C 3
#endif
#ifndef MPCX_WAVES_PER_EU_MRC
#define MPCX_WAVES_PER_EU_MRC 3
#endif

namespace mpcx {

// Compile-time loop: f(std::integral_constant<int, i>) for i in [B, E).
// Guarantees constant register-array indices (a partially unrolled loop
// would demote the accumulators to scratch memory).
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

constexpr int DB = 28;
constexpr uint32_t M28 = (1u << DB) - 1u;

// lane l receives lane l+1's value; lane 63 receives 0 (DPP wave_shl:1, bound_ctrl zero).
__device__ __forceinline__ uint32_t from_next_lane(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true);
}
// lane l receives lane l-1's value; lane 0 receives 0 (DPP wave_shr:1).
__device__ __forceinline__ uint32_t from_prev_lane(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}

// Broadcast lane 0 of each P-lane operand group to the whole group. Quads
// (P = 4) and pairs (P = 2) use a DPP quad_perm, 8-lane groups a quad_perm plus
// row_shr:4 into the upper quad, 16-lane groups (one DPP row)
// DPP row_newbcast, 32-lane groups row_newbcast + row_bcast:15 -- a VALU move with a few cycles of latency on the
// per-iteration serial path; other group widths go through the LDS crossbar
// (ds_bpermute, ~100+ cycles of latency).
template <int P>
__device__ __forceinline__ uint32_t group_bcast(uint32_t v, int src_addr) {
  if constexpr (P == 4) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xF, 0xF, false);  // quad_perm [0,0,0,0]
  } else if constexpr (P == 2) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xF, 0xF, false);  // quad_perm [0,0,2,2]
  } else if constexpr (P == 8) {
    // each quad takes its lane 0, then the upper quad of every 8-lane group
    // (DPP banks 1 and 3) takes the lower quad's value by row_shr:4
    const int t = __builtin_amdgcn_mov_dpp((int)v, 0x00, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(t, t, 0x114, 0xF, 0xA, false);
  } else if constexpr (P == 16) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x150, 0xF, 0xF, false);  // row_newbcast:0
  } else if constexpr (P == 32) {
    // every row takes its lane 0, then rows 1 and 3 take lane 15 of the row
    // below (= lane 0 of rows 0 and 2) by row_bcast:15
    const int t = __builtin_amdgcn_mov_dpp((int)v, 0x150, 0xF, 0xF, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(t, t, 0x142, 0xA, 0xF, false);
  } else {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_addr, (int)v);
  }
}

// acc += a * b (32x32 -> 64 plus 64-bit addend): hipcc lowers this to ONE
// v_mad_u64_u32. (Inline asm would force ~20 s_nop hazard pads per digit
// iteration around its SGPR carry-out.)
__device__ __forceinline__ void mad64(uint64_t& acc, uint32_t a, uint32_t b) {
  acc += (uint64_t)a * b;
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One carry pass over 64-bit redundant digits: digit k keeps its low 28 bits
// and receives the high part of digit k-1 (across lanes via DPP). The carry
// out of a group's top digit is provably zero (value < R), so group
// boundaries need no masking.
template <int P, int K>
__device__ __forceinline__ void carry_pass64(uint64_t (&acc)[K]) {
  // in place, top slot first, so only one carry is live at a time
  const uint64_t ctop = acc[K - 1] >> DB;
#pragma unroll
  for (int k = K - 1; k >= 1; --k) acc[k] = (acc[k] & M28) + (acc[k - 1] >> DB);
  acc[0] &= M28;
  if constexpr (P > 1) {
    const uint32_t clo = from_prev_lane((uint32_t)ctop);
    const uint32_t chi = from_prev_lane((uint32_t)(ctop >> 32));
    acc[0] += ((uint64_t)chi << 32) | clo;
  }
}

template <int P, int K>
__device__ __forceinline__ void carry_pass32(uint32_t (&d)[K]) {
  const uint32_t ctop = d[K - 1] >> DB;
#pragma unroll
  for (int k = K - 1; k >= 1; --k) d[k] = (d[k] & M28) + (d[k - 1] >> DB);
  d[0] &= M28;
  if constexpr (P > 1) d[0] += from_prev_lane(ctop);
}

// A <- A * B * R^-1 (almost Montgomery, result < 2N given A, B < 2N), with
// B's L digits in LDS at bl[0..L) (p = this lane's index in its group).
// Digits: A's and B's are accepted in [0, 2^28 + 2^16): montmul's own results
// (<= 2^28 + 2^8, below) and montmul_mx's (< 2^28 + 2^16, mpcx_mx.hpp); N's are
// canonical and m_i < 2^28. For K <= 37:
//  * a product a*b is < 2^56.001, a squaring's doubled a*(2b) < 2^57.001, and
//    with k_prime2c's B = 2^bit x (its digits are montmul's own, doubled twice)
//    a*(4b) < 2^58.001; m_i*N is < 2^56;
//  * an accumulator register restarts every K iterations (see the end of the
//    block loop). In between it takes K products a*b and K products m_i*N, or
//    for a squaring (K + 1) / 2 doubled products and K products m_i*N, plus a
//    < 2^35 fold per iteration: < 37 * 2^57.001 + 2^41 < 2^62.3, squaring
//    < 19 * 2^58.001 + 37 * 2^56 + 2^41 < 2^62.9. No carry pass inside the
//    product;
//  * the two carry passes at the end leave < 2^28 + 2^35, then <= 2^28 + 2^8.
//
// SQR (B == A, squaring): each unordered digit pair {i, j} needs ONE product
// 2*a_i*a_j (plus a_i^2 on the diagonal). In iteration t the product of
// multiplicand register k (digit s = p*K + k) is needed iff d = (k - t) mod K
// lies in [1, (K-1)/2] (doubled), or d == 0 with a per-lane factor
// (2 above the diagonal lane, 1 on it, 0 below); every other register is
// skipped for ALL lanes -- a compile-time decision, since t mod K is the
// unrolled index. Each pair lands in its column before that column is
// reduced (both orientations use an iteration <= i + j). K must be odd.
// Saves (K-1)/2 of the K a*b mads of every squaring iteration.
// B2IN (squarings only): the LDS row holds 2*b (digits < 2^30.01), stored so
// by the caller, which saves the per-iteration doubling.
template <int P, int K, bool SQR, bool B2IN = false>
__device__ __forceinline__ void montmul(uint32_t (&A)[K], const uint32_t* bl, const uint32_t (&Nd)[K],
                                        uint32_t n0inv, int m_src_addr, int p) {
  static_assert(SQR || !B2IN, "doubled multiplier rows are for squarings");
  static_assert(!SQR || (K % 2) == 1, "squaring schedule needs an odd digit count per lane");
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0;
  // b digits are read from LDS ahead of use: one iteration ahead, or two for
  // short iterations (K < MPCX_PREFETCH2_KMAX: half an iteration of a K = 19
  // squaring is ~60 cycles, under the LDS read latency). Rows carry 2 digits
  // of padding for the reads past their end.
  constexpr bool PF2 = K < MPCX_PREFETCH2_KMAX;
  uint32_t bnext = bl[0];
  uint32_t bnext2 = PF2 ? bl[1] : 0u;
  // one copy of the K-iteration block (unrolling the P blocks would multiply
  // the code and the live ranges: k_prime2c spilled with P = 2 unrolled)
#pragma nounroll
  for (int o = 0; o < P; ++o) {
    const uint32_t* bo = bl + o * K;
    // diagonal-register factor of this lane for the whole block (2 above the
    // diagonal lane, 1 on it, 0 below) as a right shift of b2 = 2*b_i: digits
    // are < 2^29, so b2 < 2^30 and b2 >> 31 == 0. One v_lshrrev_b32 instead of
    // a v_mul_lo_u32 (which issues at MAD rate) per squaring iteration.
    const uint32_t dsh = p > o ? 0u : (p == o ? 1u : 31u);
    static_for<0, K>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const uint32_t bi = bnext;
      if constexpr (PF2) {
        bnext = bnext2;
        bnext2 = bo[u + 2];
      }
      const uint32_t b2 = B2IN ? bi : bi << 1;
      const uint32_t bd = b2 >> dsh;
      auto ab = [&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        if constexpr (!SQR) {
          mad64(acc[(k + u) % K], A[k], bi);
        } else {
          constexpr int d = ((k - u) % K + K) % K;
          if constexpr (d == 0) {
            mad64(acc[(k + u) % K], A[k], bd);
          } else if constexpr (d <= (K - 1) / 2) {
            mad64(acc[(k + u) % K], A[k], b2);
          }
        }
      };
      // slot 0 first: it feeds m_i, the only serial dependency of the iteration
      ab(std::integral_constant<int, 0>{});
      uint32_t m = ((uint32_t)acc[u] * n0inv) & M28;
      if constexpr (P > 1) m = group_bcast<P>(m, m_src_addr);
      // next digit of b, in flight behind the bpermute and the a*b_i mads
      // (the last read of the last block touches the neighbour row: unused)
      if constexpr (!PF2) bnext = bo[u + 1];
      static_for<1, K>(ab);
      static_for<0, K>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        mad64(acc[(k + u) % K], m, Nd[k]);
      });
      const uint64_t a0 = acc[u];
      acc[(u + 1) % K] += a0 >> DB;
      if constexpr (P > 1) {
        acc[u] = from_next_lane((uint32_t)a0 & M28);
      } else {
        acc[u] = 0;
      }
    });
    // No mid-way carry pass is needed: a register is reset (slot 0 retires to
    // a 28-bit value) once every K iterations, so it stays below 2^62.9 for
    // K <= 37 (the bounds above montmul). profiles/r03/kernel_ab: dropping the
    // pass took the config-2 kernel from 176.3 to 171.7 ms.
    // block boundary as a scheduling fence (mpcx_prime.hip: without it
    // k_prime2c's live ranges grew past its 3-wave budget and spilled; the
    // k_modexp geometries fit better without it).
    if constexpr (MPCX_BLOCK_FENCE == 1) __builtin_amdgcn_sched_barrier(0);
  }
  carry_pass64<P, K>(acc);
  // digits are now < 2^28 + 2^35: one more pass brings them to <= 2^28 + 2^8
  const uint32_t ctop = (uint32_t)(acc[K - 1] >> DB);
#pragma unroll
  for (int k = K - 1; k >= 1; --k) A[k] = ((uint32_t)acc[k] & M28) + (uint32_t)(acc[k - 1] >> DB);
  A[0] = (uint32_t)acc[0] & M28;
  if constexpr (P > 1) A[0] += from_prev_lane(ctop);
}

// Canonical digits (< 2^28): repeat carry passes until no digit overflows.
template <int P, int K>
__device__ __forceinline__ void canonicalize(uint32_t (&A)[K]) {
  for (int it = 0; it < P * K + 2; ++it) {
    bool over = false;
#pragma unroll
    for (int k = 0; k < K; ++k) over |= A[k] > M28;
    if (!__any(over)) break;
    carry_pass32<P, K>(A);
  }
}

template <int K>
__device__ __forceinline__ void lds_store_digits(uint32_t* bl, int p, const uint32_t (&A)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) bl[p * K + k] = A[k];
}

// the squaring's multiplier row: 2*A, which montmul reads as B2IN (no
// per-iteration doubling)
template <int K>
__device__ __forceinline__ void lds_store_sqr(uint32_t* bl, int p, const uint32_t (&A)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) bl[p * K + k] = A[k] << 1;
}

// bits [wb*j, wb*j + wb) of the ew-word exponent e (wb <= 32; bits past the
// top word read as 0)
__device__ __forceinline__ uint32_t window_of(const uint32_t* e, uint32_t j, uint32_t wb, uint32_t ew) {
  const uint32_t bit = wb * j, w = bit >> 5, sh = bit & 31u;
  uint32_t v = e[w] >> sh;
  if (sh + wb > 32u && w + 1u < ew) v |= e[w + 1u] << (32u - sh);
  return v & ((1u << wb) - 1u);
}

// Leaves A (<= m after the Montgomery-domain exit mont(z R, 1)) canonical,
// maps m -> 0, and writes the operand's out_words words (digits -> words
// through the group's LDS row).
template <int P, int K>
__device__ __forceinline__ void store_result(uint32_t (&A)[K], const uint32_t (&Nd)[K], uint32_t* bl, int p,
                                             int g_raw, bool idle, bool active, uint32_t* o, uint32_t out_words) {
  constexpr int L = P * K;
  canonicalize<P, K>(A);
  bool eq = true;
#pragma unroll
  for (int k = 0; k < K; ++k) eq &= (A[k] == Nd[k]);
  const uint64_t bal = __ballot(eq || idle);
  const uint64_t gmask = (P == 64 ? ~0ull : (((1ull << P) - 1ull) << (g_raw * P)));
  if (!idle && (bal & gmask) == gmask) {
#pragma unroll
    for (int k = 0; k < K; ++k) A[k] = 0;
  }
  wave_lds_fence();
  lds_store_digits<K>(bl, p, A);
  wave_lds_fence();
  if (active) {
    for (uint32_t w = (uint32_t)p; w < out_words; w += P) {
      const uint32_t bit = w * 32u;
      const uint32_t d0 = bit / DB, s0 = bit % DB;
      uint32_t v = 0;
      if (d0 < (uint32_t)L) {
        // s0 = 32w mod 28 <= 24, so bits [s0, s0+32) lie in two digits
        const uint64_t lo = bl[d0];
        const uint64_t hi = (d0 + 1 < (uint32_t)L) ? bl[d0 + 1] : 0u;
        v = (uint32_t)((lo | (hi << DB)) >> s0);
      }
      o[w] = v;
    }
  }
}

}  // namespace mpcx
#include "mpcx_mx.hpp"
namespace mpcx {

// Batched x_i^e_i mod m for one registered odd modulus m: wavefront `blk` of
// the batch described by a (k_modexp: one batch per launch; k_modexp_multi:
// several batches, each its own segment of the launch's wavefronts).
// MX (geometry 2 only, a.mx_img set; MX_WG wavefronts per workgroup): every
// product but the final exit runs as montmul_mx (reduction on the matrix cores,
// mpcx_mx.hpp) with the workgroup's LDS copy of the Toeplitz tables; the
// multiplier row is montmul_mx's scratch, so a row that the state machine reuses
// across products is staged again before each (`restage`).
template <int P, int K, int G, bool MX = false>
__device__ __forceinline__ void modexp_wave(const ModexpArgs& a, const uint32_t blk) {
  constexpr int L = P * K;
  using S = MxShape<P, K, G>;
  static_assert(!MX || (P == 4 && K == 37 && G == 16) || (P == 2 && K == 37 && G == 32),
                "montmul_mx serves geometries 2 and 5");
  // +2: the b prefetch reads up to two past a row; MX: tables, m's digits, rows
  __shared__ __attribute__((aligned(16))) uint32_t lds_all[MX ? S::LDS_WORDS_WG : (G + 1) * L + 2];
  uint32_t* lds = lds_all;
  if constexpr (MX) {
    // the workgroup's tables and m's digits, then the wavefronts part
    const uint32_t* img = static_cast<const uint32_t*>(a.mx_img);
    for (int i = (int)threadIdx.x; i < S::IMG_BYTES / 4; i += 64 * MX_WG) lds_all[i] = img[i];
    for (int i = (int)threadIdx.x; i < L; i += 64 * MX_WG) lds_all[S::IMG_BYTES / 4 + i] = a.nd[i];
    __syncthreads();
    if (blk >= a.nwaves) return;  // the last workgroup's spare wavefronts
    lds = lds_all + S::IMG_BYTES / 4 + L + 4 + (threadIdx.x >> 6) * S::WAVE_WORDS;
  }
  const int lane = MX ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
  const int g_raw = lane / P;
  const bool idle = g_raw >= G;  // lanes beyond G*P carry zeros
  const int g = idle ? G : g_raw;
  const int p = lane - g_raw * P;
  const uint32_t op = blk * G + (idle ? 0 : g_raw);
  const bool active = !idle && op < a.count;
  uint32_t* bl = lds + g * (MX ? S::ROW : L);
  const int m_src_addr = (idle ? lane : g_raw * P) * 4;

  uint32_t Nd[K], A[K];
  // L digits of a constant (m, R^2 mod m) into registers; MX: through an opaque
  // pointer and lane index, so the per-digit addresses are not hoisted out of
  // the step loop and held live across every product (as load_digits)
  auto load_const = [&] __attribute__((always_inline))(const uint32_t* src, uint32_t (&v)[K]) {
    if constexpr (MX) asm volatile("" : "+s"(src));
    int pp = p;
    if constexpr (MX) asm volatile("" : "+v"(pp));
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = idle ? 0u : src[pp * K + k];
  };
  auto load_nd = [&] __attribute__((always_inline))() { load_const(a.nd, Nd); };
  if constexpr (!MX) load_nd();  // MX: only the exit product and store_result need m in registers
  MxConsts mxc{};
  const uint32_t* mx_md = lds_all + S::IMG_BYTES / 4;  // MX: m's digits (LDS)
  if constexpr (MX) mxc = mx_consts<S>(reinterpret_cast<const uint8_t*>(lds_all), lane);

  // operand words -> radix-2^28 digits (inactive operands compute on zero)
  auto load_digits = [&] __attribute__((always_inline))(const uint32_t* src, uint32_t words) {
    // opaque pointer and lane index: keeps the per-digit address/shift math
    // from being hoisted out of the step loop and held live across every
    // montmul (it cost ~3K registers and forced spills)
    asm volatile("" : "+s"(src));
    int pp = p;
    asm volatile("" : "+v"(pp));
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t bit = (uint32_t)(pp * K + k) * DB;
      const uint32_t w = bit >> 5, sh = bit & 31u;
      uint64_t v = 0;
      if (active) {
        const uint32_t* x = src + (size_t)op * words;
        const uint32_t lo = w < words ? x[w] : 0u;
        const uint32_t hi = (w + 1) < words ? x[w + 1] : 0u;
        v = ((uint64_t)hi << 32) | lo;
      }
      A[k] = (uint32_t)(v >> sh) & M28;
    }
  };

  // fixed window of wb bits (4, or 5 for long per-operand exponents): a step is
  // wb squarings and one multiply by the operand's own window's table entry
  const uint32_t wb = a.win_bits;
  const uint32_t nw = (a.exp_bits + wb - 1u) / wb;
  const uint32_t* ex = a.exp_shared ? a.exps : a.exps + (size_t)(active ? op : 0) * a.exp_words;
  // Per-wavefront table of MPCX_TABLE_ENTRIES entries x K digit-slots x 64 lanes, accessed
  // through a buffer descriptor: lane offset in one VGPR, entry/slot offset
  // in an SGPR (no per-slot address registers live across the montmuls).
  uint32_t* tbl = a.table + (size_t)blk * MPCX_TABLE_ENTRIES * K * 64u;
  const auto tbl_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(tbl, (short)0, (int)(MPCX_TABLE_ENTRIES * K * 64u * 4u), 0x00020000);
  const int tbl_lane_off = lane * 4;
  // entry offset (possibly per-lane) in voffset, slot offset k*256 as a constant soffset
  auto tbl_store = [&](uint32_t e, const uint32_t (&v)[K]) __attribute__((always_inline)) {
    const int voff = tbl_lane_off + (int)(e * K * 256u);
#pragma unroll
    for (int k = 0; k < K; ++k) __builtin_amdgcn_raw_buffer_store_b32(v[k], tbl_rsrc, voff, k * 256, 0);
  };
  auto tbl_load = [&](uint32_t e, uint32_t (&v)[K]) __attribute__((always_inline)) {
    const int voff = tbl_lane_off + (int)(e * K * 256u);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, voff, k * 256, 0);
  };
  auto lds_from_table = [&] __attribute__((always_inline))(uint32_t e) {
    uint32_t tv[K];
    tbl_load(e, tv);
    lds_store_digits<K>(bl, p, tv);
  };
  auto lds_one = [&] __attribute__((always_inline))() {
    uint32_t one[K];
#pragma unroll
    for (int k = 0; k < K; ++k) one[k] = (p == 0 && k == 0 && !idle) ? 1u : 0u;
    lds_store_digits<K>(bl, p, one);
  };

  // table[0] = R mod m (Montgomery one); LDS <- R^2 mod m for the conversions
  {
    uint32_t r1[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r1[k] = idle ? 0u : a.r1d[p * K + k];
    tbl_store(0, r1);
  }
  {
    uint32_t r2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r2[k] = idle ? 0u : a.r2d[p * K + k];
    lds_store_digits<K>(bl, p, r2);
  }
  const bool has_mul = a.mul != nullptr;
  // Control state must stay provably wave-uniform (SGPRs): the schedule and a
  // shared exponent are read through readfirstlane, so the compiler keeps the
  // step machine and the table offsets off the VGPR file.
  //
  // A shared exponent e >= 1 follows the sliding-window schedule k_expsched
  // built from it on the same stream (ExpSched layout in mpcx_internal.h):
  // odd powers x^1, x^3, ..., x^(2 Tn + 1) in table[0..Tn], z = x^top, then
  // per entry s squarings and one multiply by an odd power. Windows of up to
  // 6 bits cost ~E/7 multiplies against Go's E/4 * 15/16; every decision
  // depends on e only, so the wave stays uniform. Per-operand exponents (and
  // e = 0) keep a fixed window (wb bits, every operand multiplies every step):
  // sliding windows would diverge.
  const bool sched = a.exp_shared != 0 && a.sched != nullptr &&
                     __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_TOP]) != MPCX_SCHED_NONE;
  const uint32_t wt = nw > 0 ? window_of(ex, nw - 1u, wb, a.exp_words) : 0u;
  // table entries built: fixed window p_1..p_T (a shared e < 2^wb needs p_1..p_e only)
  const uint32_t wt_u = __builtin_amdgcn_readfirstlane(wt);
  const uint32_t T = sched ? __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_TN])
                           : (a.exp_shared && nw <= 1u ? (wt_u > 1u ? wt_u : 1u) : (1u << wb) - 1u);
  // exponent steps: schedule entries, or windows below the top one
  const uint32_t nsteps = sched ? __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_N]) : (nw > 0 ? nw - 1u : 0u);

  // Montgomery-step state machine (ONE montmul call site keeps the code small):
  //   PRE : mul*R   = mont(mul, R^2)           -> table[MPCX_MUL_ENTRY]   (only with a multiplier)
  //   TAB : fixed window: p_i = mont(x, R^2), mont(p_{i-1}, p_1)  i = 1..T -> table[i]
  //         schedule:     x R = mont(x, R^2) -> table[0]
  //   TSQ : x^2 R (schedule, Tn > 0)
  //   STAB: x^(2i+1) R = mont(x^(2i-1) R, x^2 R) -> table[i], i = 1..Tn
  //   EXP : per step: s squarings, then mont(z, table entry)
  //         (fixed window: s = 4 and the operand's window, p_0 = R mod m)
  //   MULF: z*mul*R = mont(z*R, mul*R)                          (only with a multiplier)
  //   FIN : z       = mont(z*R, 1) <= m
  enum { ST_PRE, ST_TAB, ST_TSQ, ST_STAB, ST_EXP, ST_MULF, ST_FIN };
  int st;
  uint32_t idx = 1;
  bool sqr = false;  // next montmul is a squaring (B == A)
  if (has_mul) {
    load_digits(a.mul, a.mul_words);
    st = ST_PRE;
  } else {
    load_digits(a.base, a.base_words);
    st = ST_TAB;
  }
  wave_lds_fence();

  // Exponent steps (one inlined instance): a step is sq_left squarings, then
  // one multiply by table[pend] (pend < 0: none).
  uint32_t sq_left = 0;
  int pend = -1;  // uniform: table entry, or 0x100 for the operand's own window
  auto prepare_exp = [&] __attribute__((always_inline))() {
    for (;;) {
      if (sq_left) {
        --sq_left;
        lds_store_sqr<K>(bl, p, A);
        sqr = true;
        return;
      }
      if (pend >= 0) {
        // fixed window: the operand's window of the step just scheduled (idx - 1)
        lds_from_table(pend == 0x100 ? window_of(ex, nw - 1u - idx, wb, a.exp_words) : (uint32_t)pend);
        pend = -1;
        return;
      }
      if (idx == nsteps) {
        if (has_mul) {
          st = ST_MULF;
          lds_from_table(MPCX_MUL_ENTRY);
        } else {
          st = ST_FIN;
          lds_one();
        }
        return;
      }
      if (sched) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_STEPS + idx]);
        sq_left = s >> 8;
        pend = (s & 0xFFu) == 0xFFu ? -1 : (int)(s & 0xFFu);
      } else {
        sq_left = wb;
        pend = 0x100;
      }
      ++idx;
    }
  };

  int restage = -1;  // MX: table entry (or MX_RESTAGE_R2) to put back in the row before the next product
  constexpr int MX_RESTAGE_R2 = -2;
  for (;;) {
    if constexpr (MX) {
      if (restage != -1) {
        if (restage == MX_RESTAGE_R2) {
          uint32_t r2[K];
          load_const(a.r2d, r2);
          lds_store_digits<K>(bl, p, r2);
        } else {
          lds_from_table((uint32_t)restage);
        }
        restage = -1;
        wave_lds_fence();
      }
      if (st == ST_FIN) break;  // the exit product runs after the loop (m's digits live only there)
      if (sqr) {
        montmul_mx<S, true, true>(A, lds, mx_md, mxc, lane);
      } else {
        montmul_mx<S, false, false>(A, lds, mx_md, mxc, lane);
      }
    } else if (sqr) {
      montmul<P, K, true, true>(A, bl, Nd, a.n0inv, m_src_addr, p);
    } else {
      montmul<P, K, false>(A, bl, Nd, a.n0inv, m_src_addr, p);
    }
    sqr = false;
    wave_lds_fence();
    bool start_exp = false, run_exp = false;
    if (st == ST_PRE) {
      tbl_store(MPCX_MUL_ENTRY, A);
      load_digits(a.base, a.base_words);  // LDS still holds R^2
      if constexpr (MX) restage = MX_RESTAGE_R2;
      st = ST_TAB;
      idx = 1;
    } else if (st == ST_TAB) {
      tbl_store(sched ? 0u : idx, A);
      if (sched && T > 0u) {
        lds_store_sqr<K>(bl, p, A);
        sqr = true;
        st = ST_TSQ;
      } else if (!sched && idx == 1) {
        lds_store_digits<K>(bl, p, A);  // B = p_1 for the remaining table steps
      } else if (MX && !sched && idx < T) {
        restage = 1;  // the next table step multiplies by p_1 again
      }
      if (!sched && idx < T) {
        ++idx;
      } else if (st == ST_TAB) {
        start_exp = true;  // table complete
      }
    } else if (st == ST_TSQ) {
      lds_store_digits<K>(bl, p, A);  // B = x^2 R for the odd-power chain
      if constexpr (MX) tbl_store(MPCX_SQ_ENTRY, A);
      tbl_load(0, A);
      st = ST_STAB;
      idx = 1;
    } else if (st == ST_STAB) {
      tbl_store(idx, A);
      if (MX && idx < T) restage = MPCX_SQ_ENTRY;  // the next odd power multiplies by x^2 R again
      if (idx < T) {
        ++idx;
      } else {
        start_exp = true;
      }
    } else if (st == ST_EXP) {
      run_exp = true;
    } else if (st == ST_MULF) {
      st = ST_FIN;
      lds_one();
    } else {
      break;  // ST_FIN done
    }
    if (start_exp) {
      // z = x^top (schedule) or p_top (fixed window; Montgomery one if e = 0)
      tbl_load(sched ? __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_TOP]) : wt, A);
      st = ST_EXP;
      idx = 0;
      run_exp = true;
    }
    if (run_exp) prepare_exp();
    wave_lds_fence();
  }

  if constexpr (MX) {
    load_nd();  // exit product mont(z R, 1) <= m by the CIOS loop: canonical as store_result needs
    montmul<P, K, false>(A, bl, Nd, a.n0inv, m_src_addr, p);
  }
  store_result<P, K>(A, Nd, bl, p, g_raw, idle, active, a.out + (size_t)op * a.out_words, a.out_words);
}

template <int P, int K, int G, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_modexp(const ModexpArgs a) {
  modexp_wave<P, K, G>(a, blockIdx.x);
}

// k_modexp_multi with the reduction on the matrix cores: every segment starts on
// a workgroup boundary (first[] counts MX_WG-wavefront workgroups), so the
// workgroup's waves share the segment's tables
template <int P, int K, int G, int WPE>
__global__ __launch_bounds__(64 * MX_WG) __attribute__((amdgpu_waves_per_eu(WPE))) void k_modexp_multi_mx(
    const ModexpArgs* __restrict__ segs, const uint32_t* __restrict__ first, uint32_t nsegs) {
  const uint32_t b = blockIdx.x;
  uint32_t s = 0;
  while (s + 1u < nsegs && __builtin_amdgcn_readfirstlane(first[s + 1u]) <= b) ++s;
  s = __builtin_amdgcn_readfirstlane(s);
  modexp_wave<P, K, G, true>(segs[s], (b - __builtin_amdgcn_readfirstlane(first[s])) * MX_WG + (threadIdx.x >> 6));
}

// geometry 2 with the reduction on the matrix cores (a.mx_img set): MX_WG
// wavefronts per workgroup share the tables in LDS
template <int P, int K, int G, int WPE>
__global__ __launch_bounds__(64 * MX_WG) __attribute__((amdgpu_waves_per_eu(WPE))) void k_modexp_mx(
    const ModexpArgs a) {
  modexp_wave<P, K, G, true>(a, blockIdx.x * MX_WG + (threadIdx.x >> 6));
}

#ifndef MX_PROF
// x^e mod N^2 for a shared exponent e and a public N (Paillier: config 2's r^N mod
// N^2), on N-adic pairs: y is held as (u, v) with y R = u + v N (mod N^2),
// R = 2^2128, u and v within 2^-9 of (N/2, 3N/2) as 76 digits each (a quad of 19, as
// geometry 1), and a product is pairmul_mx (mpcx_mx.hpp): one 76-digit squaring and
// one 76-digit product per squaring instead of a 148-digit squaring, and two
// reductions mod N (R = 2^2128) instead of one mod N^2 (R = 2^4144). DESIGN.md 5.2h.
//  * entry: x = x0 + x1 2^2072 -> (x0, 0) x (a0, b0) + (x1, 0) x (a1, b1), the pairs of
//    R^2 and 2^2072 R^2 mod N^2 (a.nsq), added componentwise: u, v < 3.01 N;
//  * the schedule of k_expsched as in modexp_wave, odd powers as pairs in the table;
//  * exit: (u, v) x (1, 0) = (a, b) with y = a + b N mod N^2; a + b N < 2 N^2 is formed
//    by one more product loop and N^2 (a.nd, geometry 2's digits) subtracted once if
//    it is not below it.
// ONE call site per pairmul_mx variant, as modexp_wave's.
__device__ __forceinline__ void modexp_nsq_wave(const ModexpArgs& a, const uint32_t blk) {
  using S = MxN2;
  constexpr int P = S::P, K = S::K, L = S::L, G = S::G, ROW = S::ROW;
  constexpr int KT = MPCX_NSQ_TABLE_SLOTS;
  // per wave: the row sets a and b, +4 (the product loop reads one past a row), the
  // product loop's trash slots
  constexpr int WAVE_WORDS = 2 * G * ROW + 4 + ((64 + L + 3) / 4) * 4;
  constexpr int WAVES_OFF = S::IMG_BYTES / 4 + L + 4;
  __shared__ __attribute__((aligned(16))) uint32_t lds_all[WAVES_OFF + MPCX_NSQ_WG * WAVE_WORDS];
  {
    const uint32_t* img = static_cast<const uint32_t*>(a.mx_img);
    for (int i = (int)threadIdx.x; i < S::IMG_BYTES / 4; i += 64 * MPCX_NSQ_WG) lds_all[i] = img[i];
    for (int i = (int)threadIdx.x; i < L; i += 64 * MPCX_NSQ_WG) lds_all[S::IMG_BYTES / 4 + i] = a.nsq[i];
    __syncthreads();
    if (blk >= a.nwaves) return;  // the last workgroup's spare wavefronts
  }
  const int lane = (int)(threadIdx.x & 63u);
  const int g = lane / P, p = lane % P;
  const uint32_t op = blk * G + (uint32_t)g;
  const bool active = op < a.count;
  const uint32_t* md = lds_all + S::IMG_BYTES / 4;  // N's digits
  uint32_t* ra = lds_all + WAVES_OFF + (blk % MPCX_NSQ_WG) * WAVE_WORDS;
  uint32_t* rb = ra + G * ROW;
  uint32_t* tr = ra + 2 * G * ROW + 4 + lane;
  uint32_t* ga = ra + g * ROW;
  uint32_t* gb = rb + g * ROW;
  const MxConsts mxc = mx_consts<S>(reinterpret_cast<const uint8_t*>(lds_all), lane);
  uint32_t* out = a.out + (size_t)op * a.out_words;

  const uint32_t top = __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_TOP]);
  if (top == MPCX_SCHED_NONE) {  // e = 0
    if (active)
      for (uint32_t w = (uint32_t)p; w < a.out_words; w += P) out[w] = w == 0 ? 1u : 0u;
    return;
  }
  const uint32_t T = __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_TN]);
  const uint32_t nsteps = __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_N]);

  uint32_t U[K], V[K];
  uint32_t* tbl = a.table + (size_t)blk * MPCX_TABLE_ENTRIES * KT * 64u;
  const auto tbl_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(tbl, (short)0, (int)(MPCX_TABLE_ENTRIES * KT * 64u * 4u), 0x00020000);
  auto tbl_store = [&](uint32_t e) __attribute__((always_inline)) {
    const int voff = lane * 4 + (int)(e * KT * 256u);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      __builtin_amdgcn_raw_buffer_store_b32(U[k], tbl_rsrc, voff, k * 256, 0);
      __builtin_amdgcn_raw_buffer_store_b32(V[k], tbl_rsrc, voff, (K + k) * 256, 0);
    }
  };
  auto tbl_load = [&](uint32_t e, uint32_t (&u)[K], uint32_t (&v)[K]) __attribute__((always_inline)) {
    const int voff = lane * 4 + (int)(e * KT * 256u);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      u[k] = __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, voff, k * 256, 0);
      v[k] = __builtin_amdgcn_raw_buffer_load_b32(tbl_rsrc, voff, (K + k) * 256, 0);
    }
  };
  // the multiplier rows: a table entry, a pair of a.nsq's constants, 2u twice, (1, 0)
  auto stage_entry = [&](uint32_t e) __attribute__((always_inline)) {
    uint32_t u[K], v[K];
    tbl_load(e, u, v);
    lds_store_digits<K>(ga, p, u);
    lds_store_digits<K>(gb, p, v);
  };
  auto stage_const = [&](const uint32_t* src) __attribute__((always_inline)) {
    asm volatile("" : "+s"(src));
    int pp = p;
    asm volatile("" : "+v"(pp));
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ga[pp * K + k] = src[pp * K + k];
      gb[pp * K + k] = src[L + pp * K + k];
    }
  };
  auto stage_sqr = [&]() __attribute__((always_inline)) {
    lds_store_sqr<K>(ga, p, U);
    lds_store_sqr<K>(gb, p, U);
  };
  auto stage_unit = [&](uint32_t* row1, uint32_t* row0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      row1[p * K + k] = (p == 0 && k == 0) ? 1u : 0u;
      row0[p * K + k] = 0u;
    }
  };
  // (U, V) <- (74 digits of the base from digit d0 on, 0); inactive operands: 0
  auto load_half = [&](uint32_t d0) __attribute__((always_inline)) {
    const uint32_t* src = a.base;
    asm volatile("" : "+s"(src));
    int pp = p;
    asm volatile("" : "+v"(pp));
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t d = (uint32_t)(pp * K + k);
      const uint32_t bit = (d0 + d) * DB;
      const uint32_t w = bit >> 5, sh = bit & 31u;
      uint64_t v = 0;
      if (active && d < (uint32_t)MPCX_NSQ_SPLIT_DIGITS) {
        const uint32_t* x = src + (size_t)op * a.base_words;
        const uint32_t lo = w < a.base_words ? x[w] : 0u;
        const uint32_t hi = (w + 1) < a.base_words ? x[w + 1] : 0u;
        v = ((uint64_t)hi << 32) | lo;
      }
      U[k] = (uint32_t)(v >> sh) & M28;
      V[k] = 0u;
    }
  };

  enum { ST_IN0, ST_IN1, ST_TSQ, ST_STAB, ST_EXP, ST_OUT };
  int st = ST_IN0;
  uint32_t idx = 1, sq_left = 0;
  int pend = -1, restage = -1;
  bool sqr = false;
  stage_const(a.nsq + L);
  load_half(0);
  wave_lds_fence();
  for (;;) {
    if (restage != -1) {
      stage_entry((uint32_t)restage);
      restage = -1;
      wave_lds_fence();
    }
    if (sqr) {
      pairmul_mx<S, true>(U, V, ra, rb, tr, md, mxc, lane);
    } else {
      pairmul_mx<S, false>(U, V, ra, rb, tr, md, mxc, lane);
    }
    sqr = false;
    wave_lds_fence();
    bool start_exp = false, run_exp = false;
    if (st == ST_IN0) {
      tbl_store(0);
      stage_const(a.nsq + 3 * L);
      load_half(MPCX_NSQ_SPLIT_DIGITS);
      st = ST_IN1;
    } else if (st == ST_IN1) {
      // the pair of x: the two halves' pairs added, one carry pass (digits <= 2^28 + 2)
      uint32_t u0[K], v0[K];
      tbl_load(0, u0, v0);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        U[k] += u0[k];
        V[k] += v0[k];
      }
      carry_pass32<P, K>(U);
      carry_pass32<P, K>(V);
      tbl_store(0);
      if (T > 0u) {
        stage_sqr();
        sqr = true;
        st = ST_TSQ;
      } else {
        start_exp = true;
      }
    } else if (st == ST_TSQ) {
      lds_store_digits<K>(ga, p, U);  // the odd-power chain multiplies by x^2
      lds_store_digits<K>(gb, p, V);
      tbl_store(MPCX_SQ_ENTRY);
      tbl_load(0, U, V);
      st = ST_STAB;
      idx = 1;
    } else if (st == ST_STAB) {
      tbl_store(idx);
      if (idx < T) {
        restage = MPCX_SQ_ENTRY;
        ++idx;
      } else {
        start_exp = true;
      }
    } else if (st == ST_EXP) {
      run_exp = true;
    } else {
      break;  // ST_OUT done
    }
    if (start_exp) {
      tbl_load(top, U, V);
      st = ST_EXP;
      idx = 0;
      run_exp = true;
    }
    if (run_exp) {
      for (;;) {
        if (sq_left) {
          --sq_left;
          stage_sqr();
          sqr = true;
          break;
        }
        if (pend >= 0) {
          stage_entry((uint32_t)pend);
          pend = -1;
          break;
        }
        if (idx == nsteps) {
          st = ST_OUT;
          stage_unit(ga, gb);
          break;
        }
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.sched[MPCX_SCHED_STEPS + idx]);
        sq_left = s >> 8;
        pend = (s & 0xFFu) == 0xFFu ? -1 : (int)(s & 0xFFu);
        ++idx;
      }
    }
    wave_lds_fence();
  }

  // a + b N = U x (row b = 1) + V x (row a = N): low digits -> row b, high -> V -> row a
  stage_unit(gb, ga);
#pragma unroll
  for (int k = 0; k < K; ++k) ga[p * K + k] = md[p * K + k];
  wave_lds_fence();
  mx_product2<P, K>(U, V, ga, gb, tr, p);
  canonicalize<P, K>(V);
  wave_lds_fence();
  lds_store_digits<K>(ga, p, V);
  wave_lds_fence();
  auto digit = [&](uint32_t d) __attribute__((always_inline)) -> uint32_t {
    // row b: the product loop's low words, the digit in bits 0..27 (mx_product)
    return d < (uint32_t)L ? gb[d] & M28 : (d < 2u * L ? ga[d - L] : 0u);
  };
  if (p == 0) {  // one lane per operand, once per exponentiation: y - N^2 if y >= N^2
    constexpr uint32_t L2 = (uint32_t)MPCX_GEOM_L(2);
    int c = 0;
    for (int d = 2 * L - 1; d >= 0; --d) {
      const uint32_t x = digit((uint32_t)d), m = (uint32_t)d < L2 ? a.nd[d] : 0u;
      if (c == 0 && x != m) c = x > m ? 1 : -1;
    }
    if (c >= 0) {
      uint32_t borrow = 0;
      for (uint32_t d = 0; d < 2u * L; ++d) {
        const uint32_t m = d < L2 ? a.nd[d] : 0u;
        const uint32_t t = digit(d) - m - borrow;
        borrow = t >> 31;
        (d < (uint32_t)L ? gb[d] : ga[d - L]) = t & M28;
      }
    }
  }
  wave_lds_fence();
  if (active) {
    for (uint32_t w = (uint32_t)p; w < a.out_words; w += P) {
      const uint32_t bit = w * 32u;
      const uint32_t d0 = bit / DB, s0 = bit % DB;
      const uint64_t lo = digit(d0), hi = digit(d0 + 1u);
      out[w] = (uint32_t)((lo | (hi << DB)) >> s0);
    }
  }
}

// MPCX_NSQ_WG wavefronts per workgroup share N's tables; the wave index goes through
// readfirstlane so that the window table's buffer descriptor is provably uniform
template <int WPE>
__global__ __launch_bounds__(64 * MPCX_NSQ_WG) __attribute__((amdgpu_waves_per_eu(WPE))) void k_modexp_nsq(
    const ModexpArgs a) {
  modexp_nsq_wave(a, blockIdx.x * MPCX_NSQ_WG + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}
#endif  // MX_PROF

// Several batches of one modulus class in one launch (mpcx_modexp_multi_batch:
// different moduli, shared or per-operand exponents, multipliers): segment s
// owns wavefronts [first[s], first[s+1]) and its own ModexpArgs (constants,
// schedule, window-table region), read wave-uniformly.
template <int P, int K, int G, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_modexp_multi(
    const ModexpArgs* __restrict__ segs, const uint32_t* __restrict__ first, uint32_t nsegs) {
  const uint32_t b = blockIdx.x;
  uint32_t s = 0;
  while (s + 1u < nsegs && __builtin_amdgcn_readfirstlane(first[s + 1u]) <= b) ++s;
  s = __builtin_amdgcn_readfirstlane(s);
  modexp_wave<P, K, G>(segs[s], b - __builtin_amdgcn_readfirstlane(first[s]));
}

// Fixed-base multi-exponentiation: out_i = mul_i * prod_t b_t^(e_t,i) mod m
// for up to MPCX_FB_MAX_BASES registered bases (h1, h2 of a node's N~;
// up:crypto/mta/range_proof.go z = h1^m h2^rho, up:crypto/dlnproof/proof.go
// alpha_i = h1^a_i). With the comb table b^(v 2^(wj)) per w-bit window there
// are no squarings at all: one Montgomery product per window of each
// exponent, z <- mont(z, T[j][v]), against Go's E squarings + E/4 multiplies
// for the same Exp. Every operand multiplies in every window (v = 0 reads
// the Montgomery one), so the wave never diverges; windows above every
// operand's exponent are skipped by a wave-uniform ballot.
//
// Window split: a workgroup is S = blockDim.x / 64 wavefronts (1, 2 or 4) for
// the SAME G operands; wave w takes windows j = w, w + S, ... of every base
// (interleaved: balanced for short exponents too), waves 1..S-1 leave their
// partial products (Montgomery form) in their LDS rows, and wave 0 multiplies
// them in before leaving the Montgomery domain: S - 1 extra products per
// operand for S times the wavefronts of a launch below a resident round.
// LDS: S slices of (G + 1) L + 2 words (dynamic, sized by the launch).
template <int P, int K, int G>
constexpr uint32_t fb_lds_slice_words() {
  return (uint32_t)((G + 1) * P * K + 2);
}

template <int P, int K, int G>
__device__ __forceinline__ void fixedbase_wave(const FixedBaseArgs& a, const uint32_t blk) {
  constexpr int L = P * K;
  constexpr uint32_t kSlice = fb_lds_slice_words<P, K, G>();
  extern __shared__ uint32_t fb_lds[];
  const uint32_t S = __builtin_amdgcn_readfirstlane(blockDim.x >> 6);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // lane id from mbcnt: threadIdx.x & 63 made these kernels spill 48-264 B
  const int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int g_raw = lane / P;
  const bool idle = g_raw >= G;
  const int g = idle ? G : g_raw;
  const int p = lane - g_raw * P;
  const uint32_t op = blk * G + (idle ? 0 : g_raw);
  const bool active = !idle && op < a.count;
  uint32_t* bl = fb_lds + wv * kSlice + g * L;
  const int m_src_addr = (idle ? lane : g_raw * P) * 4;

  uint32_t Nd[K], A[K];
#pragma unroll
  for (int k = 0; k < K; ++k) Nd[k] = idle ? 0u : a.nd[p * K + k];
  auto lds_digits = [&](const uint32_t* src) __attribute__((always_inline)) {  // L digits, [p*K + k]
    uint32_t t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = idle ? 0u : src[p * K + k];
    lds_store_digits<K>(bl, p, t);
  };
  // ONE montmul call site (three would triple the unrolled product and its
  // register allocation); its B operand is this wave's LDS row. The next
  // product's table entry is
  // loaded after the current product: loading it during the product into
  // registers measured 6% slower on config 5 (profiles/r03/fb_prefetch), and
  // staging it into a second LDS row set by LDS DMA (global_load_lds) 5-15%
  // slower in isolation (profiles/r04/fb_dma_ab/isolated). Issue priority for
  // the fetch or for the products: no change (profiles/r06/fbab).
  uint32_t t = 0, j = wv;  // next window: base t, window j
  uint32_t part = 1;  // wave 0: next partial to multiply in
  bool own = true, fin = false;
  // B <- the next window's entry (some operand of the wave has bits there),
  // then the other waves' partials (wave 0), then the exit multiplier 1; false
  // once the exit product has been handed out (waves > 0: once their windows
  // are done). Stored at once: no digits held in registers across a product.
  auto fetch = [&] __attribute__((always_inline))() -> bool {
    for (; t < a.nbases; ++t, j = wv) {
      const uint32_t ew = a.exp_words[t], wb = a.wbits[t];
      const uint32_t* ex = a.exps[t] + (size_t)(active ? op : 0) * ew;
      for (; j < a.nwin[t]; j += S) {
        const uint32_t v = (active && ew) ? window_of(ex, j, wb, ew) : 0u;
        if (__ballot(v != 0u) == 0ull) continue;  // no operand of the wave has bits here
        const uint32_t* e = a.tables[t] + (((size_t)j << wb) + v) * L;
        uint32_t nx[K];
#pragma unroll
        for (int k = 0; k < K; ++k) nx[k] = idle ? 0u : e[k * P + p];
        lds_store_digits<K>(bl, p, nx);
        j += S;
        return true;
      }
    }
    if (own) {  // this wave's windows are done
      own = false;
      if (S > 1u) {
        if (wv) lds_store_digits<K>(bl, p, A);  // the partial, for wave 0
        __syncthreads();
        if (wv) return false;
      }
    }
    if (part < S) {  // wave 0: B <- wave part's partial (copied into this wave's row)
      const uint32_t* src = fb_lds + part * kSlice + g * L;
      uint32_t nx[K];
#pragma unroll
      for (int k = 0; k < K; ++k) nx[k] = src[p * K + k];
      lds_store_digits<K>(bl, p, nx);
      ++part;
      return true;
    }
    if (fin) return false;
    fin = true;  // leave the Montgomery domain: z = mont(z R, 1) <= m
    uint32_t one[K];
#pragma unroll
    for (int k = 0; k < K; ++k) one[k] = (p == 0 && k == 0 && !idle) ? 1u : 0u;
    lds_store_digits<K>(bl, p, one);
    return true;
  };

  // B of the first product: R^2 already in LDS (z = mul R = mont(mul, R^2),
  // wave 0), or the first fetched entry
  bool more = true;
  if (a.mul && wv == 0u) {
    lds_digits(a.r2d);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t bit = (uint32_t)(p * K + k) * DB;
      const uint32_t w = bit >> 5, sh = bit & 31u;
      uint64_t v = 0;
      if (active) {
        const uint32_t* x = a.mul + (size_t)op * a.mul_words;
        const uint32_t lo = w < a.mul_words ? x[w] : 0u;
        const uint32_t hi = (w + 1) < a.mul_words ? x[w + 1] : 0u;
        v = ((uint64_t)hi << 32) | lo;
      }
      A[k] = (uint32_t)(v >> sh) & M28;
    }
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) A[k] = idle ? 0u : a.r1d[p * K + k];  // z = R mod m
    more = fetch();
  }
  while (more) {
    wave_lds_fence();
    montmul<P, K, false>(A, bl, Nd, a.n0inv, m_src_addr, p);
    wave_lds_fence();
    more = fetch();
  }
  if (wv == 0u)
    store_result<P, K>(A, Nd, bl, p, g_raw, idle, active, a.out + (size_t)op * a.out_words, a.out_words);
}

template <int P, int K, int G, int WPE>
__global__ __launch_bounds__(64 * MPCX_FB_MAX_SPLIT) __attribute__((amdgpu_waves_per_eu(WPE))) void k_fixedbase(
    const FixedBaseArgs a) {
  fixedbase_wave<P, K, G>(a, blockIdx.x);
}

// Several comb batches in one launch (mpcx_fixedbase_multi_batch: concurrent
// callers' batches -- other tables, other moduli of the class, muls or not):
// segment s owns workgroups [first[s], first[s+1]) and its own FixedBaseArgs,
// read wave-uniformly, as k_modexp_multi does for exponentiations.
template <int P, int K, int G, int WPE>
__global__ __launch_bounds__(64 * MPCX_FB_MAX_SPLIT) __attribute__((amdgpu_waves_per_eu(WPE))) void k_fixedbase_multi(
    const FixedBaseArgs* __restrict__ segs, const uint32_t* __restrict__ first, uint32_t nsegs) {
  const uint32_t b = blockIdx.x;
  uint32_t s = 0;
  while (s + 1u < nsegs && __builtin_amdgcn_readfirstlane(first[s + 1u]) <= b) ++s;
  s = __builtin_amdgcn_readfirstlane(s);
  fixedbase_wave<P, K, G>(segs[s], b - __builtin_amdgcn_readfirstlane(first[s]));
}

// ------------------------------------------------- primality-test kernels
// The modulus is the candidate itself, so every Montgomery constant is derived
// on the device. Serial digit helpers first (all K digits of a value in one
// thread's registers): the thread-per-item prep kernels use them to work out
// each candidate's constants once.
template <int K>
__device__ __forceinline__ bool ge_digits(const uint32_t (&x)[K], const uint32_t (&y)[K]) {
  // branch-free lexicographic compare from the top digit
  int r = 0;  // 0 = equal so far, 1 = x > y, -1 = x < y
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    const int c = (x[k] > y[k]) - (x[k] < y[k]);
    r = r != 0 ? r : c;
  }
  return r >= 0;
}
template <int K>
__device__ __forceinline__ void sub_digits(uint32_t (&x)[K], const uint32_t (&y)[K]) {
  uint32_t br = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t t = x[k] - y[k] - br;
    br = (t >> 31) & 1u;  // digits < 2^28: a borrow shows as the sign bit
    x[k] = t & M28;
  }
}
template <int K>
__device__ __forceinline__ void norm_serial(uint32_t (&x)[K]) {
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t t = x[k] + c;
    x[k] = t & M28;
    c = t >> DB;
  }
}
// x = (x + y) mod-lazy: digit sum, normalised (no reduction)
template <int K>
__device__ __forceinline__ void add_digits(uint32_t (&x)[K], const uint32_t (&y)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) x[k] += y[k];
  norm_serial<K>(x);
}
// candidate words -> radix-2^28 digits
template <int K>
__device__ __forceinline__ void load_candidate(const uint32_t* w, uint32_t words, uint32_t (&Nd)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t bit = (uint32_t)k * DB, wi = bit >> 5, sh = bit & 31u;
    const uint64_t v = ((uint64_t)((wi + 1) < words ? w[wi + 1] : 0u) << 32) | (wi < words ? w[wi] : 0u);
    Nd[k] = (uint32_t)(v >> sh) & M28;
  }
}
// -n^-1 mod 2^28 (Newton on 32 bits)
__device__ __forceinline__ uint32_t neg_inv28(uint32_t n0) {
  uint32_t inv = n0;
  for (int i = 0; i < 5; ++i) inv *= 2u - n0 * inv;
  return (0u - inv) & M28;
}
template <int K>
__device__ __forceinline__ int bitlen_digits(const uint32_t (&Nd)[K]) {
  int nbits = 1;  // unrolled: no dynamic register indexing
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (Nd[k] != 0u) nbits = k * DB + (32 - __builtin_clz(Nd[k]));
  return nbits;
}
// R mod n (canonical), R = 2^(28K): 2^nbits - n (< n), then doublings mod n
template <int K>
__device__ __forceinline__ void r_mod(const uint32_t (&Nd)[K], int nbits, uint32_t (&A)[K]) {
  uint32_t c = 1;  // two's complement of n within nbits bits
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int lo = k * DB;
    uint32_t maskk = 0;
    if (nbits >= lo + DB) maskk = M28;
    else if (nbits > lo) maskk = (1u << (nbits - lo)) - 1u;
    const uint32_t t = ((~Nd[k]) & maskk) + c;
    c = t >> DB;
    A[k] = t & maskk;
  }
  for (int i = nbits; i < DB * K; ++i) {
#pragma unroll
    for (int k = 0; k < K; ++k) A[k] <<= 1;
    norm_serial<K>(A);
    if (ge_digits<K>(A, Nd)) sub_digits<K>(A, Nd);
  }
}
// bit j of the candidate (from its words in memory: no dynamic register index)
__device__ __forceinline__ uint32_t word_bit(const uint32_t* w, int j) { return (w[j >> 5] >> (j & 31)) & 1u; }

// ------------------------------------------ P lanes per candidate
// Each test runs as two launches. A thread-per-item prep kernel (k_pprep_*)
// writes the candidate's constants with the serial helpers above; the test
// kernel then gives each candidate P lanes of K digits each and runs the
// k_modexp montmul with a per-group modulus and -n^-1: P = 2 x K = 19 for the
// base-2 throughput tests (32 candidates per wave, 3 waves per SIMD),
// P = 16 x K = 3 for general-base Miller-Rabin and strong Lucas (4 tests per
// wave, 1/8 of one thread's serial chain; K = 5 for Lucas candidates above
// 1024 bits). Round 1 held one candidate per lane (1 x 37); that ran one
// wavefront per SIMD at ~45% of the v_mad_u64_u32 peak and made a small batch
// wait for one thread's full serial chain, so P lanes per candidate won
// (DESIGN.md 5.3).

// R mod n (canonical, L digits), -n^-1 mod 2^28 and nbits | s << 16
// (s = v2(n - 1)) of one odd n >= 5 for R = 2^(28 L): 28 L - nbits doublings,
// a few % of the exponentiation that follows.
template <int L>
__device__ __forceinline__ void pprep_item(const uint32_t* nw, uint32_t n_words, uint32_t* r1_out, uint32_t* meta_out) {
  uint32_t Nd[L], R1[L];
  load_candidate<L>(nw, n_words, Nd);
  const int nbits = bitlen_digits<L>(Nd);
  r_mod<L>(Nd, nbits, R1);
  int s = 1;
  while (s < nbits && !word_bit(nw, s)) ++s;
#pragma unroll
  for (int d = 0; d < L; ++d) r1_out[d] = R1[d];
  meta_out[0] = neg_inv28(Nd[0]);
  meta_out[1] = (uint32_t)nbits | ((uint32_t)s << 16);
}

template <int L>
__global__ __launch_bounds__(64) void k_pprep_prime2(const Prime2Args a) {
  const bool strong = blockIdx.x >= a.fp_blocks;
  uint32_t cnt, i;
  const uint32_t* src;
  size_t base;
  if (!strong) {
    cnt = a.count_dev ? min(a.count_f, *a.count_dev) : a.count_f;
    i = blockIdx.x * 64u + threadIdx.x;
    src = a.nf;
    base = 0;
  } else {
    cnt = a.count_s;
    i = (blockIdx.x - a.fp_blocks) * 64u + threadIdx.x;
    src = a.ns;
    base = a.count_f;
  }
  if (i >= cnt) return;
  pprep_item<L>(src + (size_t)i * a.n_words, a.n_words, a.r1 + (base + i) * L, a.meta + (base + i) * 2);
}

template <int L>
__global__ __launch_bounds__(64) void k_pprep_mr(const MrArgs a) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.count) return;
  pprep_item<L>(a.n + (size_t)i * a.n_words, a.n_words, a.r1 + (size_t)i * L, a.meta + (size_t)i * 2);
}

// digits p*K .. p*K+K-1 of a little-endian word array (radix 2^28)
template <int K>
__device__ __forceinline__ void load_group_digits(const uint32_t* w, uint32_t words, int p, uint32_t (&D)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t bit = (uint32_t)(p * K + k) * DB, wi = bit >> 5, sh = bit & 31u;
    const uint64_t v = ((uint64_t)((wi + 1) < words ? w[wi + 1] : 0u) << 32) | (wi < words ? w[wi] : 0u);
    D[k] = (uint32_t)(v >> sh) & M28;
  }
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

// all P lanes of this lane's group have v set
template <int P>
__device__ __forceinline__ bool group_all(bool v, int g) {
  const uint64_t bal = __ballot(v);
  const uint64_t gmask = (P == 64 ? ~0ull : (((1ull << P) - 1ull) << (g * P)));
  return (bal & gmask) == gmask;
}

// Leave the Montgomery domain on a copy and compare with 1 and n - 1:
// Y = mont(X, 1) <= n, canonical digits (uses the group's LDS row bl).
template <int P, int K>
__device__ __forceinline__ void exit_compare(const uint32_t (&X)[K], const uint32_t (&Nd)[K], uint32_t n0inv,
                                             uint32_t* bl, int p, int g, bool* is_one, bool* is_nm1) {
  uint32_t Y[K], one[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Y[k] = X[k];
    one[k] = (p == 0 && k == 0) ? 1u : 0u;
  }
  wave_lds_fence();
  lds_store_digits<K>(bl, p, one);
  wave_lds_fence();
  montmul<P, K, false>(Y, bl, Nd, n0inv, 0, p);
  wave_lds_fence();
  canonicalize<P, K>(Y);
  bool e1 = true, em = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const bool d0 = p == 0 && k == 0;
    e1 &= Y[k] == (d0 ? 1u : 0u);
    em &= Y[k] == (d0 ? Nd[0] - 1u : Nd[k]);  // n odd: n - 1 only changes digit 0
  }
  *is_one = group_all<P>(e1, g);
  *is_nm1 = group_all<P>(em, g);
}

// x <- 2x (digits doubled, one carry pass; values stay < R / 4)
template <int P, int K>
__device__ __forceinline__ void double_digits(uint32_t (&A)[K], bool on) {
  const uint32_t sh = on ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < K; ++k) A[k] <<= sh;
  carry_pass32<P, K>(A);
}

// Base-2 tests of the safe-prime search, P lanes per candidate, one
// wave-uniform mode per block.
// Fermat items, blocks [0, f_blocks): ok = 2^(n-1) == 1 (mod n) -- tss-lib's
// Pocklington check on p = 2q+1 (up:common/safe_prime.go
// isPocklingtonCriterionSatisfied).
// Strong items, the blocks after them: n - 1 = 2^s d, x = 2^d; ok iff x == 1,
// or x^(2^j) == n - 1 for some j < s -- the base-2 Miller-Rabin round of
// q.ProbablyPrime (go:src/math/big/prime.go, its forced last base), run first
// so the other rounds only see its survivors.
// Square-and-double: squarings are Montgomery squarings and the "multiply by
// 2" a digit doubling without reduction (values < 4n, and R > 16n keeps every
// almost-Montgomery output below 2n); the exponent bits differ per candidate,
// so the doubling is a per-lane shift by 0 or 1.
template <int P, int K, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_prime2c(const Prime2Args a) {
  constexpr int L = P * K, G = 64 / P;
  __shared__ uint32_t lds[2 * G * L + 2];  // per group: work row, saved-x row
  const int lane = threadIdx.x, g = lane / P, p = lane - g * P;
  const bool strong = blockIdx.x >= a.f_blocks;
  uint32_t cnt, item;
  const uint32_t* src;
  size_t base;
  if (!strong) {
    cnt = a.count_dev ? min(a.count_f, *a.count_dev) : a.count_f;
    if (blockIdx.x * (uint32_t)G >= cnt) return;  // whole wave beyond the sieve's survivors
    item = blockIdx.x * G + g;
    src = a.nf;
    base = 0;
  } else {
    cnt = a.count_s;
    if ((blockIdx.x - a.f_blocks) * (uint32_t)G >= cnt) return;
    item = (blockIdx.x - a.f_blocks) * G + g;
    src = a.ns;
    base = a.count_f;
  }
  const bool active = item < cnt;
  const uint32_t it = active ? item : item - g;  // idle groups recompute the block's first item
  uint32_t* bl = lds + 2 * g * L;
  uint32_t* sv = bl + L;
  const uint32_t* nw = src + (size_t)it * a.n_words;
  uint32_t Nd[K], A[K];
  load_group_digits<K>(nw, a.n_words, p, Nd);
  {
    const uint32_t* r1 = a.r1 + (base + it) * L + p * K;
#pragma unroll
    for (int k = 0; k < K; ++k) A[k] = r1[k];  // Montgomery 1
  }
  const uint32_t n0inv = a.meta[(base + it) * 2];
  const uint32_t mt = a.meta[(base + it) * 2 + 1];
  const int nbits = (int)(mt & 0xFFFFu), s = (int)(mt >> 16);
  const int sh = strong ? s : 0;  // strong: e = (n - 1) >> s; Fermat: e = n - 1
  // Left to right from the wave's highest exponent bit, starting at
  // Montgomery 1: above a candidate's own top bit its exponent bits are 0 and
  // squaring 1 changes nothing, so no lane needs a predicated select.
  // Two montmul call sites (squaring, exit product) as in k_modexp: states
  //   SQ : x <- x^2, then x <- 2x on an exponent bit
  //   EX : y = mont(x, 1) <= n (x saved in the group's second row), compare
  //        y with 1 and n - 1, restore x
  //   SS : strong-test squaring x <- x^2, then EX again
  enum { SQ, EX, SS };
  int st = SQ;
  int i = wave_max(nbits - sh - 1), j = 0;
  const int smax = strong ? wave_max(s) : 1;
  bool pass = false, done = false;
  for (;;) {
    wave_lds_fence();
    if (st == EX) {
      uint32_t one[K];
#pragma unroll
      for (int k = 0; k < K; ++k) one[k] = (p == 0 && k == 0) ? 1u : 0u;
      lds_store_digits<K>(sv, p, A);
      lds_store_digits<K>(bl, p, one);
    } else if (st == SQ) {
      // x <- 2^bit x^2 as ONE squaring product: B = 2^bit x in LDS, x in
      // registers -- the half-product schedule then sums x_i (2 x_j) pairs
      // (digits of B < 2^29 + 2^11, b2 < 2^31: the schedule's bounds hold, and
      // x (2x) < 8n^2 < nR keeps the result < 2n); no separate doubling pass
      const int jb = i + sh;  // bit jb of n - 1: bit jb of n except bit 0 (n odd)
      const uint32_t dsh = (jb > 0 && jb < nbits && word_bit(nw, jb)) ? 1u : 0u;
      uint32_t B2[K];
#pragma unroll
      for (int k = 0; k < K; ++k) B2[k] = A[k] << (dsh + 1u);  // montmul reads 2B
      lds_store_digits<K>(bl, p, B2);
    } else {
      lds_store_sqr<K>(bl, p, A);  // SS: a plain squaring
    }
    wave_lds_fence();
    if (st == EX) {
      montmul<P, K, false>(A, bl, Nd, n0inv, 0, p);
    } else {
      montmul<P, K, true, true>(A, bl, Nd, n0inv, 0, p);
    }
    if (st == SQ) {
      if (--i < 0) st = EX;
    } else if (st == SS) {
      st = EX;
    } else {
      canonicalize<P, K>(A);
      bool e1 = true, em = true;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool d0 = p == 0 && k == 0;
        e1 &= A[k] == (d0 ? 1u : 0u);
        em &= A[k] == (d0 ? Nd[0] - 1u : Nd[k]);  // n odd: n - 1 only changes digit 0
      }
      const bool one = group_all<P>(e1, g), nm1 = group_all<P>(em, g);
      if (j == 0) {
        pass = one || (strong && nm1);
        done = pass;
      } else if (!done && j < s) {
        if (one) {
          done = true;  // nontrivial square root of 1: composite
        } else if (nm1) {
          pass = true;
          done = true;
        }
      }
      if (++j >= smax) break;
      wave_lds_fence();
#pragma unroll
      for (int k = 0; k < K; ++k) A[k] = sv[p * K + k];
      st = SS;
    }
  }
  if (!active || p != 0) return;
  if (strong) {
    a.ok_s[item] = pass ? 1 : 0;
    return;
  }
  if (a.ok_f) a.ok_f[item] = pass ? 1 : 0;
  if (pass && a.pass_count) {
    const uint32_t slot = atomicAdd(a.pass_count, 1u);
    a.pass_idx[slot] = a.sieve_idx ? a.sieve_idx[item] : item;
    for (uint32_t w = 0; w < a.n_words; ++w) a.pass_n[(size_t)slot * a.n_words + w] = nw[w];
  }
}

// Miller-Rabin to arbitrary bases, P lanes per test: ok[i] = n_i is a strong
// probable prime to base a_i, that is, with n - 1 = 2^s d and x = a^d, x == 1
// or x^(2^j) == n - 1 for some j < s. Serves the random-base rounds of
// q.ProbablyPrime(20) in the safe-prime search (up:common/safe_prime.go).
// R^2 mod n = Mont(2^(28 L)) by square-and-double from Mont(2),
// a R = mont(a, R^2), a 16-entry table T[v] = a^v R in the group's LDS rows,
// then x = a^d by Go's 4-bit fixed window (4 squarings and one table product
// per window for every lane: the wave never diverges) and the strong check.
template <int P, int K, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_mrc(const MrArgs a) {
  constexpr int L = P * K, G = 64 / P, ROWS = 17;  // table rows 0..15, work row 16
  __shared__ uint32_t lds[G * ROWS * L + 2];
  const int lane = threadIdx.x, g = lane / P, p = lane - g * P;
  if (blockIdx.x * (uint32_t)G >= a.count) return;
  const uint32_t item = blockIdx.x * G + g;
  const bool active = item < a.count;
  const uint32_t it = active ? item : item - g;
  uint32_t* rows = lds + g * ROWS * L;
  uint32_t* wl = rows + 16 * L;
  const uint32_t* nw = a.n + (size_t)it * a.n_words;
  uint32_t Nd[K], R1[K], A[K], X[K];
  load_group_digits<K>(nw, a.n_words, p, Nd);
  load_group_digits<K>(a.a + (size_t)it * a.n_words, a.n_words, p, X);
  const uint32_t* r1 = a.r1 + (size_t)it * L + p * K;
#pragma unroll
  for (int k = 0; k < K; ++k) R1[k] = r1[k];
  const uint32_t n0inv = a.meta[(size_t)it * 2];
  const uint32_t mt = a.meta[(size_t)it * 2 + 1];
  const int nbits = (int)(mt & 0xFFFFu), s = (int)(mt >> 16);
  auto sqr = [&] __attribute__((always_inline))() {
    wave_lds_fence();
    lds_store_digits<K>(wl, p, A);
    wave_lds_fence();
    montmul<P, K, true>(A, wl, Nd, n0inv, 0, p);
  };
  // R^2 mod n = Mont(2^(28 L)): square-and-double over E = 28 L from Mont(2)
  constexpr int E = DB * L;
  constexpr int ETOP = 31 - __builtin_clz((unsigned)E);
#pragma unroll
  for (int k = 0; k < K; ++k) A[k] = R1[k];
  double_digits<P, K>(A, true);
  for (int i = ETOP - 1; i >= 0; --i) {
    sqr();
    double_digits<P, K>(A, ((E >> i) & 1) != 0);
  }
  // T[1] = a R = mont(a, R^2); T[0] = R mod n; T[v] = mont(T[v-1], T[1])
  wave_lds_fence();
  lds_store_digits<K>(wl, p, A);
  wave_lds_fence();
  montmul<P, K, false>(X, wl, Nd, n0inv, 0, p);
  wave_lds_fence();
  lds_store_digits<K>(rows, p, R1);
  lds_store_digits<K>(rows + L, p, X);
#pragma unroll
  for (int k = 0; k < K; ++k) A[k] = X[k];
  for (int v = 2; v < 16; ++v) {
    wave_lds_fence();
    montmul<P, K, false>(A, rows + L, Nd, n0inv, 0, p);
    wave_lds_fence();
    lds_store_digits<K>(rows + v * L, p, A);
  }
  // x = a^d, d = (n - 1) >> s = bits [s, nbits) of n, 4-bit windows from the top
  const int dbits = nbits - s;
  const int nwin = (dbits + 3) / 4;
#pragma unroll
  for (int k = 0; k < K; ++k) A[k] = R1[k];  // Montgomery one: leading zero windows keep it
  for (int w = wave_max(nwin) - 1; w >= 0; --w) {
#pragma unroll 1
    for (int q = 0; q < 4; ++q) sqr();
    uint32_t v = 0;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
      const int j = s + 4 * w + b;
      v = (v << 1) | ((j < nbits) ? word_bit(nw, j) : 0u);
    }
    wave_lds_fence();
    montmul<P, K, false>(A, rows + v * L, Nd, n0inv, 0, p);
  }
  bool one, nm1;
  exit_compare<P, K>(A, Nd, n0inv, wl, p, g, &one, &nm1);
  bool pass = one || nm1, done = pass;
  const int smax = wave_max(s);
  for (int j = 1; j < smax; ++j) {
    sqr();
    exit_compare<P, K>(A, Nd, n0inv, wl, p, g, &one, &nm1);
    const bool live = !done && j < s;
    if (live && one) done = true;  // nontrivial square root of 1: composite
    else if (live && nm1) {
      pass = true;
      done = true;
    }
  }
  if (active && p == 0) a.ok[item] = pass ? 1 : 0;
}

// Strong Lucas test, P lanes per candidate: Go math/big probablyPrimeLucas
// (go:src/math/big/prime.go), the last step of ProbablyPrime. With P from
// Baillie-OEIS method C (the smallest P >= 3 with Jacobi(P^2 - 4, n) = -1,
// found by the caller; Q = 1) and n + 1 = 2^r s (s odd), n passes iff
// V_s == +-2 and U_s == 0 (checked as P V_s == 2 V_{s+1}, Crandall-Pomerance
// 3.13), or V_{2^t s} == 0 for some 0 <= t < r - 1.
// V is built by the binary ladder V_2k = V_k^2 - 2, V_2k+1 = V_k V_k+1 - P in
// the Montgomery domain: every bit is one product and one squaring for every
// lane (the bit only selects where the two results go); bits above a
// candidate's own top keep (V_0, V_1) = (2, P) fixed (2^2 - 2 = 2,
// 2P - P = P), so the wave needs no predication. The subtractions are
// additions of 2n - c (c = P R or 2 R, canonical): an almost-Montgomery value
// (< 2n) may be below c, and the sum is never negative and stays < 4n. The
// checks compare canonical values after leaving the Montgomery domain.
// k_pprep_lucas, thread per item, does the serial Horner / doubling steps that
// give each candidate's Montgomery constants.
template <int L>
__global__ __launch_bounds__(64) void k_pprep_lucas(const LucasArgs a) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= a.count) return;
  const uint32_t* nw = a.n + (size_t)i * a.n_words;
  uint32_t Nd[L], R1[L], PR[L], T[L];
  load_candidate<L>(nw, a.n_words, Nd);
  const int nbits = bitlen_digits<L>(Nd);
  r_mod<L>(Nd, nbits, R1);
  const uint32_t P = a.P[i];
#pragma unroll
  for (int k = 0; k < L; ++k) PR[k] = 0;
  for (int b = 13; b >= 0; --b) {  // P R mod n, Horner over P's bits
#pragma unroll
    for (int k = 0; k < L; ++k) PR[k] <<= 1;
    norm_serial<L>(PR);
    if (ge_digits<L>(PR, Nd)) sub_digits<L>(PR, Nd);
    if ((P >> b) & 1u) {
      add_digits<L>(PR, R1);
      if (ge_digits<L>(PR, Nd)) sub_digits<L>(PR, Nd);
    }
  }
  uint32_t* c = a.consts + (size_t)i * 4 * L;
  // [0] P R, [1] 2 R, [2] 2n - P R, [3] 2n - 2 R (all canonical, < 2n)
#pragma unroll
  for (int k = 0; k < L; ++k) c[k] = PR[k];
#pragma unroll
  for (int k = 0; k < L; ++k) T[k] = R1[k] << 1;
  norm_serial<L>(T);
  if (ge_digits<L>(T, Nd)) sub_digits<L>(T, Nd);
#pragma unroll
  for (int k = 0; k < L; ++k) c[L + k] = T[k];
  uint32_t N2[L];
#pragma unroll
  for (int k = 0; k < L; ++k) N2[k] = Nd[k] << 1;
  norm_serial<L>(N2);
  {
    uint32_t X[L];
#pragma unroll
    for (int k = 0; k < L; ++k) X[k] = N2[k];
    sub_digits<L>(X, PR);
#pragma unroll
    for (int k = 0; k < L; ++k) c[2 * L + k] = X[k];
#pragma unroll
    for (int k = 0; k < L; ++k) X[k] = N2[k];
    sub_digits<L>(X, T);
#pragma unroll
    for (int k = 0; k < L; ++k) c[3 * L + k] = X[k];
  }
  int r = 0;  // n + 1 = 2^r s: r = trailing ones of n
  while (r < nbits && word_bit(nw, r)) ++r;
  a.meta[(size_t)i * 2] = neg_inv28(Nd[0]);
  a.meta[(size_t)i * 2 + 1] = (uint32_t)nbits | ((uint32_t)r << 16);
}

// canonical value of Montgomery-form X in [0, n): y = mont(X, 1) <= n, with
// n mapped to 0
template <int P, int K>
__device__ __forceinline__ void exit_canonical(const uint32_t (&X)[K], const uint32_t (&Nd)[K], uint32_t n0inv,
                                               uint32_t* bl, int p, int g, uint32_t (&Y)[K]) {
  uint32_t one[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Y[k] = X[k];
    one[k] = (p == 0 && k == 0) ? 1u : 0u;
  }
  wave_lds_fence();
  lds_store_digits<K>(bl, p, one);
  wave_lds_fence();
  montmul<P, K, false>(Y, bl, Nd, n0inv, 0, p);
  wave_lds_fence();
  canonicalize<P, K>(Y);
  bool en = true;
#pragma unroll
  for (int k = 0; k < K; ++k) en &= Y[k] == Nd[k];
  if (group_all<P>(en, g)) {
#pragma unroll
    for (int k = 0; k < K; ++k) Y[k] = 0;
  }
}

// canonical Y equals the small constant c
template <int P, int K>
__device__ __forceinline__ bool group_eq_small(const uint32_t (&Y)[K], uint32_t c, int p, int g) {
  bool e = true;
#pragma unroll
  for (int k = 0; k < K; ++k) e &= Y[k] == ((p == 0 && k == 0) ? c : 0u);
  return group_all<P>(e, g);
}

// the ladder and the checks of the strong Lucas test (see k_pprep_lucas)
template <int P, int K, int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_lucasc(const LucasArgs a) {
  constexpr int L = P * K, G = 64 / P;
  __shared__ uint32_t lds[G * L + 2];
  const int lane = threadIdx.x, g = lane / P, p = lane - g * P;
  if (blockIdx.x * (uint32_t)G >= a.count) return;
  const uint32_t item = blockIdx.x * G + g;
  const bool active = item < a.count;
  const uint32_t it = active ? item : item - g;
  uint32_t* bl = lds + g * L;
  const uint32_t* nw = a.n + (size_t)it * a.n_words;
  uint32_t Nd[K], PR[K], CP[K], C2[K], vk[K], vk1[K];
  load_group_digits<K>(nw, a.n_words, p, Nd);
  {
    const uint32_t* c = a.consts + (size_t)it * 4 * L + p * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      PR[k] = c[k];
      vk[k] = c[L + k];  // V_0 = 2
      CP[k] = c[2 * L + k];
      C2[k] = c[3 * L + k];
      vk1[k] = PR[k];  // V_1 = P
    }
  }
  const uint32_t n0inv = a.meta[(size_t)it * 2];
  const uint32_t mt = a.meta[(size_t)it * 2 + 1];
  const int nbits = (int)(mt & 0xFFFFu), r = (int)(mt >> 16);
  const int sbits = (r == nbits) ? 1 : nbits - r;  // bit length of s = (n + 1) >> r
  auto add_const = [&](uint32_t (&X)[K], const uint32_t (&C)[K]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < K; ++k) X[k] += C[k];
    carry_pass32<P, K>(X);  // < 4n < R: no carry leaves the group
  };
  for (int i = wave_max(sbits) - 1; i >= 0; --i) {
    const int j = i + r;  // bit i of s = bit j of n + 1: 1 at j == r, n's bit above
    const bool bit = i < sbits && (j == r || (j < nbits && word_bit(nw, j)));
    // X = V_k V_k+1 - P; Y = (bit ? V_k+1 : V_k)^2 - 2
    uint32_t X[K], Y[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      X[k] = vk[k];
      Y[k] = bit ? vk1[k] : vk[k];
    }
    wave_lds_fence();
    lds_store_digits<K>(bl, p, vk1);
    wave_lds_fence();
    montmul<P, K, false>(X, bl, Nd, n0inv, 0, p);
    add_const(X, CP);
    wave_lds_fence();
    lds_store_digits<K>(bl, p, Y);
    wave_lds_fence();
    montmul<P, K, true>(Y, bl, Nd, n0inv, 0, p);
    add_const(Y, C2);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      vk[k] = bit ? X[k] : Y[k];
      vk1[k] = bit ? Y[k] : X[k];
    }
  }
  // V_s == +-2 and U_s == 0 (P V_s == 2 V_s+1), or V_(2^t s) == 0, t < r - 1
  uint32_t Y[K];
  exit_canonical<P, K>(vk, Nd, n0inv, bl, p, g, Y);
  bool pass = false;
  {
    const bool is2 = group_eq_small<P, K>(Y, 2u, p, g);
    uint32_t Z[K];  // Y + 2 == n  <=>  V_s == n - 2
#pragma unroll
    for (int k = 0; k < K; ++k) Z[k] = Y[k] + ((p == 0 && k == 0) ? 2u : 0u);
    carry_pass32<P, K>(Z);
    bool en = true;
#pragma unroll
    for (int k = 0; k < K; ++k) en &= Z[k] == Nd[k];
    const bool isn2 = group_all<P>(en, g);
    uint32_t U1[K], U2[K], A1[K], A2[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      U1[k] = vk[k];
      U2[k] = vk1[k] << 1;  // 2 V_s+1 R (< 4n)
    }
    carry_pass32<P, K>(U2);
    wave_lds_fence();
    lds_store_digits<K>(bl, p, PR);
    wave_lds_fence();
    montmul<P, K, false>(U1, bl, Nd, n0inv, 0, p);  // P V_s R
    exit_canonical<P, K>(U1, Nd, n0inv, bl, p, g, A1);
    exit_canonical<P, K>(U2, Nd, n0inv, bl, p, g, A2);
    bool eu = true;
#pragma unroll
    for (int k = 0; k < K; ++k) eu &= A1[k] == A2[k];
    pass = (is2 || isn2) && group_all<P>(eu, g);
  }
  bool done = pass;
  const int tmax = wave_max(r - 1);
  for (int t = 0; t < tmax; ++t) {
    const bool live = !done && t < r - 1;
    exit_canonical<P, K>(vk, Nd, n0inv, bl, p, g, Y);
    if (live && group_eq_small<P, K>(Y, 0u, p, g)) {
      pass = true;
      done = true;
    } else if (live && group_eq_small<P, K>(Y, 2u, p, g)) {
      done = true;  // V = 2 is a fixed point of V^2 - 2: never 0
    }
    wave_lds_fence();
    lds_store_digits<K>(bl, p, vk);
    wave_lds_fence();
    montmul<P, K, true>(vk, bl, Nd, n0inv, 0, p);
    add_const(vk, C2);
  }
  if (active && p == 0) a.ok[item] = pass ? 1 : 0;
}

}  // namespace mpcx

