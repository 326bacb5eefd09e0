// mpcx_mx.hpp -- gfx950 Montgomery products with the REDUCTION on the matrix
// cores (v_mfma_i32_16x16x64_i8) and the product A*B on the VALU, for the two
// main geometries whose batches share one modulus: geometry 2 (4 x 37 lanes,
// 16 operands per wave, 4096-bit class: Paillier N^2) and geometry 5 (2 x 37,
// 32 operands per wave, 2048-bit class: N, N~).
//
// Every operand of a k_modexp batch shares the modulus m (config 2: 65,536 x
// r^N mod N^2; ModProof's Z_i^N mod N in keygen), so the two reduction products
// of a Montgomery multiplication in separated form,
//     q = (T mod R) * m'' mod R     (m'' = -m^-1 mod R)
//     U = (T + q m) / R,
// are products of a batch of rows with FIXED Toeplitz matrices of m'' and m:
// dense contractions. The VALU keeps what is per operand -- T = A*B, the same
// lazy radix-2^28 row loop as montmul<P, 37> (mpcx_device.hpp) without its
// m_i N half -- and the matrix cores take the reduction (two thirds of a
// CIOS squaring's multiply-accumulates).
//
// Layout (R = 2^(28 L), the same Montgomery domain as the CIOS geometry, so
// tables, constants and the CIOS exit product mix):
//  * VALU ("block") layout: operand g on lanes Pg..Pg+P-1, lane p holds radix-2^28
//    digits 37p..37p+36 -- montmul's layout.
//  * MFMA layout, per 16 operands (a geometry-5 wave runs two halves): operand
//    n = lane & 15, quarter h = lane >> 4. Radix-2^7 digits (4 per radix-2^28
//    digit, one byte each, so the conversion is a bit spread) are the K index; a
//    16x16x64 MFMA takes B = 64 digits of 16 operands (lane (n, h): bytes
//    16h..16h+15 of the K block -- one ds_read_b128 of radix-2^28 digits
//    16kb + 4h .. +3) and A = the Toeplitz block of m'' or m for output positions
//    16o..16o+15 (precomputed per modulus in the same lane map, so the hardware's
//    k order inside a lane never matters), and accumulates column sums
//    C[4h + r][n] = output position 16o + 4h + r of operand n: one lane holds 4
//    consecutive radix-2^7 positions = ONE radix-2^28 digit.
//  * Column sums are exact in i32: <= 4L products of 7-bit digits.
//  * q is normalised to balanced radix-2^28 digits in [-2^27 - 2^17, 2^27 + 2^17]
//    (one carry step, the neighbour digit's carry by ds_bpermute), whose top
//    radix-2^7 digit is in [-65, 64]: a valid signed i8, so |q| <= R/2 and
//    U + m, not U, is the result: U + m in (m/2, 3m/2) for A, B < 2m, the
//    bound the VALU product needs.
//  * The carry out of the low half of T + q m (an exact multiple of R) is the
//    rounded value of its top four column sums (the rest is < 2^-5 of a unit).
//
// One LDS row per operand: the multiplier (2A for squarings), overwritten by T's
// low digits as the product loop passes them, then T's high digits + m, then
// U + m. q goes from the accumulator layout to B fragments by permlane swaps.
// Included by mpcx_device.hpp (after montmul, before modexp_wave); not on its own.
#pragma once

namespace mpcx {

typedef int mx_v4i __attribute__((ext_vector_type(4)));

// MxShape, MxG2, MxG5, MX_WG: mpcx_internal.h (the C-ABI builds the tables with them)

struct MxConsts {
  const uint8_t* t1;  // LDS: table of m'' = -m^-1 mod R, pre-offset to this lane's row copy
  const uint8_t* t2;  // LDS: table of m, likewise
};
// lane (i = lane & 15, h = lane >> 4): fragment j at t + 16 (JMAX - j)
template <class S>
__device__ __forceinline__ MxConsts mx_consts(const uint8_t* img, int lane) {
  const int off = (lane & 15) * S::TAB_STRIDE + 16 * (lane >> 4);
  return MxConsts{img + off, img + S::TAB_BYTES + off};
}

// radix-2^28 digit (two's complement, |x| < 2^28) -> 4 radix-2^7 digits, one per
// byte (the top one signed), in five instructions: a 2-bit gap above bit 13 first
// (x + 3 t for t = x's bits 14 and up, as a shift-add and a subtract), then the 1-bit
// gaps above bits 6 and 22 of that with one mask and one add (no carry crosses the
// halves: bits 14 and 15 are clear). Equal for every 32-bit x to the three
// add-the-upper-part steps x += x & ~(2^7 - 1), ~(2^15 - 1), ~(2^23 - 1) it replaces
// (six instructions; tests/test_mx_spread_cpu.py).
// (round 6: the closed form x + 2^7 (x >> 7) + 2^15 (x >> 14) + 2^23 (x >> 21) on the
// MAD pipe measured slower, profiles/r06/spab/; round 8: x + 3 2^14 (x >> 14) as one
// v_mad_i32_i24, four instructions, won alone and lost together with the unmasked
// stores of the product loops, profiles/r08/valu/)
//
// The empty asm statements here, in mx_spread7_low28 and in mx_retire_mask emit no
// instruction: they only hide a value's origin from hipcc, whose canonical forms of
// these expressions are one instruction longer (no builtin states the shorter
// shape). They cannot change a result, only the instruction count, and that rests on
// this compiler's behaviour: with every ROCm upgrade regenerate the listing and
// compare the counts with DESIGN.md 5.2i (tools/isa_loops.py, tools/isa_census.py).
__device__ __forceinline__ uint32_t mx_spread7(uint32_t x) {
  uint32_t t = x & 0xFFFFC000u;
  asm("" : "+v"(t));  // opaque: or hipcc rewrites x - t as x & 0x3FFF and is back at six
  x = ((t << 2) + x) - t;
  x += x & 0xFF80FF80u;
  return x;
}
// The same for a digit of T as the product loops store it: bits 0..27 are the
// digit (>= 0), bits 28..31 whatever the column sum held above it. The two masks of
// the 14 | 14 split drop those bits, so the loops store the low word unmasked
// (five instructions here for one saved at each of the L stores).
__device__ __forceinline__ uint32_t mx_spread7_low28(uint32_t x) {
  uint32_t t = x & 0x0FFFC000u;
  asm("" : "+v"(t));  // opaque: one v_lshl_add_u32; hipcc's own form is a shift and two bit operations
  x = (t << 2) + (x & 0x00003FFFu);
  x += x & 0xFF80FF80u;
  return x;
}

// The retire step of the product loops hands a column's low 28 bits to the lane
// below as its new top column, except across a group boundary: lane 0's digit
// leaves the window and must not shift into the previous group's top slot. The
// RECEIVING lane masks what it pulls through DPP (one v_and_b32 with a DPP source):
// 2^28 - 1 inside a group, 0 in the group's top lane (lane 63 reads 0 anyway).
template <int P>
__device__ __forceinline__ uint32_t mx_retire_mask(int p) {
  uint32_t m = p == P - 1 ? 0u : M28;
  asm volatile("" : "+v"(m));  // opaque: or the select comes back into every retire step
  return m;
}

// T = A * B (B == A for SQR; B2IN: the row holds 2B) in montmul's row loop without
// the m_i N half: T's low L digits are emitted to tl[] as the window passes them
// (lane p == 0 of the group), the high L digits end in A (<= 2^28 + 2^10).
// A word of tl[] is the retiring column's low 32 bits: T's digit (< 2^28) in bits
// 0..27 and the low bits of its carry above. Every reader drops them: the fragment
// build (mx_spread7_low28) and ttop in mx_reduce, digit() at k_modexp_nsq's exit.
//
// Every lane stores, lanes p != 0 into a per-lane trash slot of the wave's LDS
// area (tr: that lane's slots, L words from lane + 0), so that the loop body has
// no exec-mask changes (their SALU mask ops serialise against the MADs' carry-out
// SGPRs).
template <int P, int K, bool SQR, bool B2IN>
__device__ __forceinline__ void mx_product(uint32_t (&A)[K], const uint32_t* bl, uint32_t* tl, uint32_t* tr, int p) {
  static_assert(!SQR || (K % 2) == 1, "squaring schedule needs an odd digit count per lane");
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0;
  uint32_t bnext = bl[0];
  const uint32_t rmask = mx_retire_mask<P>(p);
#pragma nounroll
  for (int o = 0; o < P; ++o) {
    const uint32_t* bo = bl + o * K;
    uint32_t* to = (p == 0 ? tl : tr) + o * K;
    const uint32_t dsh = p > o ? 0u : (p == o ? 1u : 31u);
    static_for<0, K>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const uint32_t bi = bnext;
      bnext = bo[u + 1];
      const uint32_t b2 = B2IN ? bi : bi << 1;
      const uint32_t bd = b2 >> dsh;
      static_for<0, K>([&](auto kc) {
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
      });
      const uint64_t a0 = acc[u];
      acc[(u + 1) % K] += a0 >> DB;
      // lane 0's digit leaves the window as T's digit i (in CIOS it is zero): the
      // low word as it is, bits 28..31 are the readers' to drop (above mx_product)
      to[u] = (uint32_t)a0;
      acc[u] = from_next_lane((uint32_t)a0) & rmask;
    });
  }
  carry_pass64<P, K>(acc);
  const uint32_t ctop = (uint32_t)(acc[K - 1] >> DB);
#pragma unroll
  for (int k = K - 1; k >= 1; --k) A[k] = ((uint32_t)acc[k] & M28) + (uint32_t)(acc[k - 1] >> DB);
  A[0] = (uint32_t)acc[0] & M28;
  A[0] += from_prev_lane(ctop);
}

// Z = U * B + V * A for the rows A (al) and B (bl) in ONE row loop (2 K MADs per row
// step; k_modexp_nsq's cross term u v' + v u'): Z's low L digits overwrite row B
// behind the digits the loop has read (as mx_product's: the digit in bits 0..27 of
// the word), the high L digits end in V (<= 2^28 + 2^10).
// Accumulators: 2 K products < 2^56.001 between two restarts, < 2^61.3 for K = 19.
template <int P, int K>
__device__ __forceinline__ void mx_product2(const uint32_t (&U)[K], uint32_t (&V)[K], const uint32_t* al,
                                            uint32_t* bl, uint32_t* tr, int p) {
  uint64_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0;
  uint32_t anext = al[0], bnext = bl[0];
  const uint32_t rmask = mx_retire_mask<P>(p);
#pragma nounroll
  for (int o = 0; o < P; ++o) {
    const uint32_t* ao = al + o * K;
    const uint32_t* bo = bl + o * K;
    uint32_t* to = (p == 0 ? bl : tr) + o * K;
    static_for<0, K>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const uint32_t ai = anext, bi = bnext;
      anext = ao[u + 1];
      bnext = bo[u + 1];
      static_for<0, K>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        mad64(acc[(k + u) % K], U[k], bi);
        mad64(acc[(k + u) % K], V[k], ai);
      });
      const uint64_t a0 = acc[u];
      acc[(u + 1) % K] += a0 >> DB;
      to[u] = (uint32_t)a0;
      acc[u] = from_next_lane((uint32_t)a0) & rmask;
    });
  }
  carry_pass64<P, K>(acc);
  const uint32_t ctop = (uint32_t)(acc[K - 1] >> DB);
#pragma unroll
  for (int k = K - 1; k >= 1; --k) V[k] = ((uint32_t)acc[k] & M28) + (uint32_t)(acc[k - 1] >> DB);
  V[0] = (uint32_t)acc[0] & M28;
  V[0] += from_prev_lane(ctop);
}

// lane (n, h) <- lane (n, h - 1) (h = 0: lane (n, 3)); one LDS-crossbar permute
__device__ __forceinline__ int mx_from_prev_quarter(int v, int lane) {
  return __builtin_amdgcn_ds_bpermute(((lane - 16) & 63) << 2, v);
}

// the radix-2^28 digit sum of four column sums as one 64-bit value V = c0 + add +
// c1 2^7 + c2 2^14 + c3 2^21, built by three v_mad_i64_i32 (the MAD pipe idles
// during the reduction) instead of masks, shifts and adds on the VALU; the digit
// V mod 2^28 and the carry V >> 28 (arithmetic) follow from V directly.
// Multipliers in SGPRs (VOP3 takes no literal), so the compiler cannot turn them
// back into shifts.
__device__ __forceinline__ int64_t mx_sum64(const mx_v4i c, int add) {
  int64_t v = (int64_t)(c[0] + add);
  uint64_t cy;
  asm("v_mad_i64_i32 %0, %1, %2, %3, %0" : "+v"(v), "=s"(cy) : "v"(c[1]), "s"(1 << 7));
  asm("v_mad_i64_i32 %0, %1, %2, %3, %0" : "+v"(v), "=s"(cy) : "v"(c[2]), "s"(1 << 14));
  asm("v_mad_i64_i32 %0, %1, %2, %3, %0" : "+v"(v), "=s"(cy) : "v"(c[3]), "s"(1 << 21));
  return v;
}
// V >> 28 as a 32-bit int (|V| < 2^59): one v_alignbit_b32 of the two halves
__device__ __forceinline__ int mx_hi28(int64_t v) {
  return (int)__builtin_amdgcn_alignbit((uint32_t)((uint64_t)v >> 32), (uint32_t)v, 28);
}

// acc[o - O0] += sum over K blocks kb of F_j (j = o - 4 kb) x bf[kb], for output
// blocks O0 <= o < O1; Toeplitz block j is read once and used for every kb it
// pairs with (one block ahead of its MFMAs)
// (ACCUM: on top of what acc holds)
template <class S, int NJ, int O0, int O1, bool ACCUM = false>
__device__ __forceinline__ void mx_toeplitz(mx_v4i (&acc)[O1 - O0], const uint8_t* f, const mx_v4i (&bf)[S::KB]) {
  // one ds_read_b128 per block: lane base in a VGPR, block offset an immediate
  auto ld = [&](int j) __attribute__((always_inline)) {
    return *reinterpret_cast<const mx_v4i*>(f + 16 * (S::JMAX - j));
  };
  // (hipcc folds this zero fill into the first MFMA of each block as the inline
  // constant 0 for C: no v_mov is issued for it)
  if constexpr (!ACCUM) static_for<0, O1 - O0>([&](auto oc) { acc[decltype(oc)::value] = mx_v4i{0, 0, 0, 0}; });
  // first and last Toeplitz block with an MFMA in this chunk
  constexpr int JLO = (O0 - 4 * (S::KB - 1)) > 0 ? (O0 - 4 * (S::KB - 1)) : 0;
  constexpr int JHI = (O1 - 1) < (NJ - 1) ? (O1 - 1) : (NJ - 1);
  mx_v4i fnext = ld(JLO);
  static_for<JLO, JHI + 1>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const mx_v4i fj = fnext;
    if constexpr (j + 1 <= JHI) fnext = ld(j + 1);
    // the next block's read stays one block ahead: ALU and MFMA may move
    // across, LDS reads may not (hoisting them all costs 4 VGPRs per block)
    __builtin_amdgcn_sched_barrier(0x000F);
    static_for<0, S::KB>([&](auto kc) {
      constexpr int kb = decltype(kc)::value;
      constexpr int o = j + 4 * kb;
      if constexpr (o >= O0 && o < O1) acc[o - O0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fj, bf[kb], acc[o - O0], 0, 0, 0);
    });
  });
}

// 4x4 transpose between the register index and the lane quarter (h): on return
// y[i] in lane (n, h) is x[h] of lane (n, i). Two permlane32 and two permlane16
// swaps (gfx950), no LDS.
__device__ __forceinline__ mx_v4i mx_transpose4(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
  auto r02 = __builtin_amdgcn_permlane32_swap(x0, x2, false, false);
  auto r13 = __builtin_amdgcn_permlane32_swap(x1, x3, false, false);
  auto r01 = __builtin_amdgcn_permlane16_swap(r02[0], r13[0], false, false);
  auto r23 = __builtin_amdgcn_permlane16_swap(r02[1], r13[1], false, false);
  return mx_v4i{(int)r01[0], (int)r01[1], (int)r23[0], (int)r23[1]};
}

// Round 6 measured and removed: a workgroup barrier pairing one
// wave's product loop with its SIMD partner's reduction (slower), and each chunk's
// normalisation interleaved with the next chunk's MFMAs (equal).
// A <- A * B * R^-1 + m (mod-m class preserved; result in (m/2, 3m/2) for A, B < 2m).
// Postcondition: every digit of A is in [0, 2^28 + 2^16). The reduction emits
// digits in (-2^16, 2^28 + 2^16) and the signed carry passes at the end run only
// while some digit of the wave is negative; mx_product and montmul take such
// digits as they are (bounds above montmul, mpcx_device.hpp).
// rows: this wavefront's G operand rows (S::ROW words each); operand g's row holds
// B (2B for squarings) on entry and is the scratch of the whole product: T's low
// digits overwrite B as the loop consumes it, then T's high digits + m, then
// U + m. md: m's L radix-2^28 digits (LDS).
// MX_PROF (microbench builds only): s_memtime stamps at the phase boundaries,
// accumulated per wave in MxProf (the stamps fence the scheduler around them)
#ifdef MX_PROF
struct MxProf {
  uint64_t t[7];
  uint64_t last;
};
#define MX_STAMP(i)                                          \
  do {                                                       \
    __builtin_amdgcn_sched_barrier(0);                       \
    const uint64_t now_ = __builtin_amdgcn_s_memtime();      \
    if ((i) > 0) pf->t[(i) - 1] += now_ - pf->last;          \
    pf->last = now_;                                         \
    __builtin_amdgcn_sched_barrier(0);                       \
  } while (0)
#define MX_PROF_ARG , MxProf* pf
#define MX_PROF_PASS , pf
#else
#define MX_STAMP(i) \
  do {              \
  } while (0)
#define MX_PROF_ARG
#define MX_PROF_PASS
#endif
#ifndef MPCX_MX_TIMING
#define MPCX_MX_TIMING 0  // microbench builds only: 1 = product loop alone, 2 = reduction alone
#endif

// The wave's issue priority by phase of the Montgomery product (s_setprio; the
// two waves of a SIMD are mostly in different phases). The levels fall along
// the product, so whenever the two waves are in different phases the one that
// is earlier in its product issues first and the other fills the slots it
// leaves: config 2 at 123.3 ms, the fastest of the orders tried
// (profiles/r06/prioab2..5).
constexpr int PRIO_PRODUCT = 3;  // product loop
constexpr int PRIO_FRAG = 2;     // fragment build
constexpr int PRIO_Q = 1;        // q products
constexpr int PRIO_QM = 0;       // q m products
constexpr int PRIO_CARRY = 0;    // carry passes

// The quotient of one reduction, handed to a second one (k_modexp_nsq, below): its
// bytes NEGATED, as B fragments, and its top radix-2^28 digit L - 1 (in the lane
// that estimates the carry out of the low half)
template <class S>
struct MxQ {
  mx_v4i f[S::KB];
  int top;
};

// every byte b of x (|b| <= 127) -> -b, no borrow between bytes
__device__ __forceinline__ int mx_neg_bytes(int x) {
  const uint32_t b = (uint32_t)x, H = 0x80808080u;
  return (int)((H - (b & ~H)) ^ (~b & H));
}

// The end of a reduction: U + m from the row back to the block layout, and signed
// carry passes until every digit is >= 0 (k_modexp_nsq reads both halves back after
// the second reduction, so neither is live during the other's)
template <class S>
__device__ __forceinline__ void mx_readback(uint32_t (&A)[S::K], const uint32_t* rg, int p MX_PROF_ARG) {
  constexpr int P = S::P, K = S::K, L = S::L;
  wave_lds_fence();
  // ---- back to the block layout; signed carry passes until every digit is >= 0
#pragma unroll
  for (int k = 0; k < K; ++k) A[k] = rg[p * K + k];
  MX_STAMP(5);
  // the emitted digits lie in (-2^16, 2^28 + 2^16) (one carry step of |carry| <
  // 2^16); the next product takes any non-negative digits of that size, so the
  // passes run only when some digit of the wave is negative (~1 wave in 4)
  uint32_t sg = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) sg |= A[k];
  const bool need = __any((int)sg < 0);
  for (int it = 0; need && it < L + 2; ++it) {
    const int top = (int)A[K - 1];
    const int ctop = (p == P - 1) ? 0 : (top >> DB);
#pragma unroll
    for (int k = K - 1; k >= 1; --k) {
      const int cur = (int)A[k];
      const bool keep = (k == K - 1) && (p == P - 1);
      A[k] = (uint32_t)((keep ? cur : (cur & (int)M28)) + ((int)A[k - 1] >> DB));
    }
    const int c0 = (int)from_prev_lane((uint32_t)ctop);
    A[0] = (uint32_t)(((int)A[0] & (int)M28) + (p == 0 ? 0 : c0));
    bool neg = false;
#pragma unroll
    for (int k = 0; k < K; ++k) neg |= (int)A[k] < 0;
    if (!__any(neg)) break;
  }
  MX_STAMP(6);
}

// The reduction of montmul_mx: T's low digits in the rows, its high digits in A;
// A <- (T + q m) / R + m, q balanced. MODE 0: that alone. The pair of reductions of
// a product mod m^2 in m-adic form (mpcx_device.hpp, k_modexp_nsq):
// MODE 1 also hands out its q; MODE 2 reduces T - q1 - R for the q1 handed in:
//  * its q is ((T mod R) - q1) m'' mod R: a second Toeplitz pass over q1's negated
//    bytes into the same column sums (|sum| < 2 * 4 L * 127^2 < 2^24 for L = 76);
//  * the carry out of the low half T_low - q1 + (q m)_low takes q1's top digit too
//    (q1's lower digits weigh < 2^-28 of a carry unit);
//  * the high half adds m - 1: - R is one unit there, and with |q|, |q1| <= R/2
//    (1 + 2^-10) the result (T - q1 + q m) / R - 1 + m stays within m/2 (1 - 2^-10) - 2
//    and 3m/2 (1 + 2^-10) + 2 + T/R.
template <class S, int MODE>
__device__ __forceinline__ void mx_reduce(uint32_t (&A)[S::K], uint32_t* rows, const uint32_t* md,
                                          const MxConsts& c, int lane, MxQ<S>& q1 MX_PROF_ARG) {
  static_assert(MODE == 0 || S::HALVES == 1, "the pair of reductions serves 16 operands per wave");
  constexpr int P = S::P, K = S::K, L = S::L, ROW = S::ROW, KB = S::KB;
  const int g = lane / P, p = lane % P;    // block layout
  const int n = lane & 15, h = lane >> 4;  // MFMA layout
  uint32_t* rg = rows + g * ROW;
  __builtin_amdgcn_s_setprio(PRIO_FRAG);
  MX_STAMP(1);
  if constexpr (MPCX_MX_TIMING == 1) return;
  wave_lds_fence();
  // ---- T's low half as B fragments (radix-2^7 bytes), every half of the wave
  mx_v4i bf[S::HALVES][KB];
  int ttop[S::HALVES];  // T's digit L - 1: the top 4 positions of the carry estimate
  static_for<0, S::HALVES>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    const uint32_t* rn = rows + (16 * s + n) * ROW;
    static_for<0, KB>([&](auto kc) {
      constexpr int kb = decltype(kc)::value;
      mx_v4i v = {0, 0, 0, 0};
      if (16 * kb + 4 * h < L) v = *reinterpret_cast<const mx_v4i*>(rn + 16 * kb + 4 * h);
      if constexpr (16 * kb + 15 >= L) {  // the digits past L in the last K block
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (16 * kb + 4 * h + i >= L) v[i] = 0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (int)mx_spread7_low28((uint32_t)v[i]);
      bf[s][kb] = v;
    });
    ttop[s] = (int)(rn[L - 1] & M28);
  });
  wave_lds_fence();
  MX_STAMP(2);
  // ---- the row <- T's high digits + m (block layout)
#pragma unroll
  for (int k = 0; k < K; ++k) rg[p * K + k] = A[k] + md[p * K + k] - (MODE == 2 && k == 0 && p == 0 ? 1u : 0u);
  __builtin_amdgcn_s_setprio(PRIO_Q);
  static_for<0, S::HALVES>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    uint32_t* rn = rows + (16 * s + n) * ROW;
    if constexpr (s > 0) __builtin_amdgcn_s_setprio(PRIO_Q);  // the first half left it at PRIO_QM
    // ---- q column sums (o = j + 4 kb; chunks of output blocks bound the live
    // accumulators), balanced radix-2^28 digits with one carry step, as bytes;
    // every 4 blocks transposed in registers into one B fragment of phase 2
    mx_v4i qf_own[KB];
    mx_v4i(&qf)[KB] = MODE == 1 ? q1.f : qf_own;
    {
      int xprev = 0;
      uint32_t X[4] = {0u, 0u, 0u, 0u};
      auto norm = [&](const mx_v4i& cs, int o) __attribute__((always_inline)) -> uint32_t {
        const int64_t v = mx_sum64(cs, 1 << 27);
        const int lo = ((int)(uint32_t)v & (int)M28) - (1 << 27);
        const int hi = mx_hi28(v);
        const int x = mx_from_prev_quarter(hi, lane);
        int e = lo + (h == 0 ? xprev : x);
        xprev = x;
        if (4 * o + 3 >= L && 4 * o + h >= L) e = 0;  // digits past L: q is mod R
        if (MODE == 1 && o == (L - 1) / 4) q1.top = e;  // lane h = (L - 1) % 4: digit L - 1
        return mx_spread7((uint32_t)e);
      };
      auto norm_block = [&](const mx_v4i& cs, auto oc) __attribute__((always_inline)) {
        constexpr int o = decltype(oc)::value;
        X[o & 3] = norm(cs, o);
        if constexpr ((o & 3) == 3) {
          qf[o >> 2] = mx_transpose4(X[0], X[1], X[2], X[3]);
        } else if constexpr (o == S::O1 - 1) {
          qf[o >> 2] = mx_transpose4(X[0], (o & 3) >= 1 ? X[1] : 0u, (o & 3) >= 2 ? X[2] : 0u, 0u);
        }
      };
      constexpr int NC = (S::O1 + S::CS1 - 1) / S::CS1;
      static_for<0, NC>([&](auto cc) {
        constexpr int O0 = S::CS1 * decltype(cc)::value;
        constexpr int O1 = O0 + S::CS1 < S::O1 ? O0 + S::CS1 : S::O1;
        mx_v4i acc[O1 - O0];
        mx_toeplitz<S, S::NJ1, O0, O1>(acc, c.t1, bf[s]);
        if constexpr (MODE == 2) mx_toeplitz<S, S::NJ1, O0, O1, true>(acc, c.t1, q1.f);
        static_for<0, O1 - O0>([&](auto oc) {
          norm_block(acc[decltype(oc)::value], std::integral_constant<int, O0 + decltype(oc)::value>{});
        });
        __builtin_amdgcn_sched_barrier(0);  // one chunk's accumulators live at a time
      });
    }
    MX_STAMP(3);
    __builtin_amdgcn_s_setprio(PRIO_QM);
    // ---- q m column sums for blocks O2LO.. : the lane whose 4 positions are the
    // low half's top (N7 - 4 .. N7 - 1) gives the carry out of the low half, the
    // lanes at positions N7 + 4d the digits d of U + m, adding T's high digit + m
    // from the row; the carry chain runs through the quarters as in q
    {
      int xprev = 0;
      auto emit = [&](const mx_v4i& cs, int o) __attribute__((always_inline)) {
        const int pos = 16 * o + 4 * h;
        const bool carry_lane = pos == S::N7 - 4;
        const int d = (pos - S::N7) >> 2;  // U's digit (< 0: the low half)
        const int dc = d < 0 ? 0 : d;
        const int add = carry_lane ? ttop[s] + (1 << 27) - (MODE == 2 ? q1.top : 0) : (int)rn[dc];
        const int64_t v = mx_sum64(cs, add);
        const int hi = mx_hi28(v);        // on the carry lane: round(low half / R)
        const int top = (int)(uint32_t)v;  // the sum mod 2^32
        const int dig = top & (int)M28;    // the sum's bits 0..27
        const int x = mx_from_prev_quarter(hi, lane);
        const int cin = h == 0 ? xprev : x;
        xprev = x;
        // the top digit keeps its carry (the value is < 2m < 2^(28 L - 47))
        const int u = d == L - 1 ? top + cin : dig + cin;
        if (d >= 0) rn[dc] = (uint32_t)u;
      };
      constexpr int NC = (S::O2HI - S::O2LO + S::CS2 - 1) / S::CS2;
      static_for<0, NC>([&](auto cc) {
        constexpr int O0 = S::O2LO + S::CS2 * decltype(cc)::value;
        constexpr int O1 = O0 + S::CS2 < S::O2HI ? O0 + S::CS2 : S::O2HI;
        mx_v4i acc[O1 - O0];
        mx_toeplitz<S, S::NJ2, O0, O1>(acc, c.t2, qf);
        static_for<0, O1 - O0>([&](auto oc) { emit(acc[decltype(oc)::value], O0 + decltype(oc)::value); });
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    if constexpr (MODE == 1) {  // the second reduction subtracts this q
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) q1.f[kb][i] = mx_neg_bytes(q1.f[kb][i]);
    }
  });
  __builtin_amdgcn_s_setprio(PRIO_CARRY);
  MX_STAMP(4);
  if constexpr (MODE == 0) mx_readback<S>(A, rg, p MX_PROF_PASS);
}

template <class S, bool SQR, bool B2IN>
__device__ __forceinline__ void montmul_mx(uint32_t (&A)[S::K], uint32_t* rows, const uint32_t* md,
                                           const MxConsts& c, int lane MX_PROF_ARG) {
  uint32_t* rg = rows + (lane / S::P) * S::ROW;
  // ---- T = A B on the VALU: low digits -> the row (behind the multiplier digits
  // the loop has read), high digits -> A
  MX_STAMP(0);
  __builtin_amdgcn_s_setprio(PRIO_PRODUCT);
  if constexpr (MPCX_MX_TIMING != 2)
    mx_product<S::P, S::K, SQR, B2IN>(A, rg, rg, rows + S::TRASH_OFF + lane, lane % S::P);
  MxQ<S> q;  // unused
  mx_reduce<S, 0>(A, rows, md, c, lane, q MX_PROF_PASS);
}

// (u, v) <- (u, v) x (a, b) mod m^2 in m-adic Montgomery form (k_modexp_nsq,
// mpcx_device.hpp): u <- montmul_mx(u, a) = (u a + q m) / R + m and
// v <- (u b + v a - q - R) / R mod m, the second reduction taking the first one's q
// (u a = R u' - (q + R) m, so the pair stands for (u + v m)(a + b m) / R mod m^2; the
// v b m^2 term is never formed). ra / rb: the wave's row sets with a and b
// (operand g's rows at g * ROW), both scratch as montmul_mx's row.
// SQR: (a, b) = (u, v) with 2u in BOTH rows: u^2 on row a and 2 u v = v x row b.
template <class S, bool SQR>
__device__ __forceinline__ void pairmul_mx(uint32_t (&U)[S::K], uint32_t (&V)[S::K], uint32_t* ra, uint32_t* rb,
                                           uint32_t* tr, const uint32_t* md, const MxConsts& c, int lane) {
  constexpr int P = S::P, K = S::K;
  const int g = lane / P, p = lane % P;
  uint32_t* ga = ra + g * S::ROW;
  uint32_t* gb = rb + g * S::ROW;
  __builtin_amdgcn_s_setprio(PRIO_PRODUCT);
  if constexpr (SQR) {
    mx_product<P, K, false, false>(V, gb, gb, tr, p);
    mx_product<P, K, true, true>(U, ga, ga, tr, p);
  } else {
    mx_product2<P, K>(U, V, ga, gb, tr, p);
    mx_product<P, K, false, false>(U, ga, ga, tr, p);
  }
  MxQ<S> q;
  mx_reduce<S, 1>(U, ra, md, c, lane, q);
  mx_reduce<S, 2>(V, rb, md, c, lane, q);
  mx_readback<S>(U, ga, p);
  mx_readback<S>(V, gb, p);
}

}  // namespace mpcx
