// edvss.hpp -- Feldman VSS over Ed25519, batched: vss.hpp function for function
// over ed::Point, as tss-lib v2's crypto/vss runs under up:eddsa/keygen and
// up:eddsa/resharing (the curve is a parameter upstream). Scalars are mod
// L = ed::OrderL() and stay on the host; the point sums run on the GPU as
// multi-scalar sums (eddsa::MsmBatch, libmpcx's k_ed_msm). Restated as recalled
// and marked "upstream, verify" as vss.hpp is; tests/eddsa_keygen_model.py
// restates the same functions and is pinned by its algebra and by OpenSSL.
//
// AdmitBatch is what a receiver does to every commitment point before using it:
// crypto.NewECPoint's check, then EightInvEight (mpcx_ed_admit_batch, libmpcx's
// k_ed_admit).
#pragma once

#include <cstdint>
#include <vector>

#include "bignum.hpp"
#include "ed25519.hpp"
#include "tsscommon.hpp"

namespace mpcx::host::edvss {

constexpr uint32_t kMaxTerms = 16;  // threshold + 1 and the number of ids of one call

// CheckIndexes (upstream, verify): every id is nonzero mod L and no two are
// equal mod L. Returns the ids reduced mod L; throws std::invalid_argument.
std::vector<Nat> CheckIndexes(const std::vector<Nat>& ids);

struct Created {
  std::vector<ed::Point> Vs;  // V_k = a_k B, k = 0..threshold
  std::vector<Nat> shares;    // s_j = sum_k a_k id_j^k mod L, one per id
};
// vss.Create per session (upstream, verify): a_0 = secrets[i], a_1..a_t =
// GetRandomPositiveInt(readers[i], L) in that order. Every V_k of the call is one
// GPU batch of plain base-point multiples (n_points = 0). Requires
// threshold + 1 <= 16, 1 <= ids.size() <= 16 and threshold < ids.size(); throws
// std::invalid_argument otherwise.
std::vector<Created> CreateBatch(uint32_t threshold, const std::vector<Nat>& ids, const std::vector<Nat>& secrets,
                                 const std::vector<RandFn>& readers);

struct VerifyItem {
  std::vector<ed::Point> Vs;
  Nat id, share;
};
// (*Share).Verify per item (upstream, verify): share B == sum_k id^k V_k, as the
// multi-scalar sum (L - share) B + sum_k id^k V_k == the identity. An item whose
// Vs is not threshold + 1 points, holds an off-curve point, or whose id is 0 mod
// L fails without GPU work; the rest are one GPU batch.
std::vector<uint8_t> VerifyBatch(uint32_t threshold, const std::vector<VerifyItem>& items);

struct PublicShares {
  std::vector<ed::Point> Vc;  // Vc_k = sum_i V_ik; Vc_0 is the public key
  std::vector<ed::Point> X;   // X_j = sum_k id_j^k Vc_k, one per id
};
// Vs[session][party][k], party i's commitments (any number of parties up to
// 16); ids are the receivers'. Two GPU batches: the sums over parties (scalars
// 1), then the public shares.
std::vector<PublicShares> PublicSharesBatch(uint32_t threshold, const std::vector<Nat>& ids,
                                            const std::vector<std::vector<std::vector<ed::Point>>>& Vs);

struct Reconstructed {
  Nat secret;
  bool ok = false;
};
// (Shares).ReConstruct per item (upstream, verify): Lagrange interpolation at 0
// over the item's (id, share) pairs, on the host. ok = false on an id that is 0
// mod L or on two ids equal mod L.
std::vector<Reconstructed> ReconstructBatch(const std::vector<std::vector<Nat>>& ids,
                                            const std::vector<std::vector<Nat>>& shares);

// prod_{j != i} id_j / (id_j - id_i) mod L for every i (ids already checked and
// reduced); false when a difference has no inverse
bool LagrangeAtZero(const std::vector<Nat>& idq, std::vector<Nat>* out);

struct Admitted {
  std::vector<ed::Point> out;   // the admitted point; the identity for a rejected item
  std::vector<uint8_t> status;  // MPCX_ED_ADMIT_*
};
// crypto.NewECPoint's check and, with clear, EightInvEight per point, on the GPU.
// Coordinates are any values below 2^256 (wider ones throw).
Admitted AdmitBatch(const std::vector<ed::Point>& points, bool clear);

}  // namespace mpcx::host::edvss
