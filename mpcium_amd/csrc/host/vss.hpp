// vss.hpp -- batched mirror of tss-lib v2.0.2's Feldman VSS
// (up:crypto/vss/feldman_vss.go: Create, (*Share).Verify, (Shares).ReConstruct,
// CheckIndexes) and of the public-share derivation of keygen round 3 /
// resharing round 4-5 (BigXj = sum_k id_j^k * sum_i V_ik), at any threshold up
// to 15. The point sums run on the GPU as multi-scalar sums (secp::MsmBatch,
// libmpcx's k_ec_msm); the scalar arithmetic mod q = secp::CurveN() stays on
// the host. Restated as recalled and marked "upstream, verify": the upstream
// text cannot be checked in this image; tests/vss_model.py
// restates the same functions over oracle/tss_ref.py and is pinned by its algebra.
#pragma once

#include <cstdint>
#include <vector>

#include "bignum.hpp"
#include "secp256k1.hpp"
#include "tsscommon.hpp"

namespace mpcx::host::vss {

constexpr uint32_t kMaxTerms = 16;  // threshold + 1 and the number of ids of one call

// CheckIndexes (upstream, verify): every id is nonzero mod q and no two are
// equal mod q. Returns the ids reduced mod q; throws std::invalid_argument.
std::vector<Nat> CheckIndexes(const std::vector<Nat>& ids);

struct Created {
  std::vector<secp::Affine> Vs;  // V_k = a_k G, k = 0..threshold
  std::vector<Nat> shares;       // s_j = sum_k a_k id_j^k mod q, one per id
};
// vss.Create per session (upstream, verify): a_0 = secrets[i], a_1..a_t =
// GetRandomPositiveInt(readers[i], q) in that order. Every V_k of the call is one
// GPU batch. Requires threshold + 1 <= 16, 1 <= ids.size() <= 16 and
// threshold < ids.size(); throws std::invalid_argument otherwise.
std::vector<Created> CreateBatch(uint32_t threshold, const std::vector<Nat>& ids, const std::vector<Nat>& secrets,
                                 const std::vector<RandFn>& readers);

struct VerifyItem {
  std::vector<secp::Affine> Vs;
  Nat id, share;
};
// (*Share).Verify per item (upstream, verify): share G == sum_k id^k V_k, as the
// multi-scalar sum -share G + sum_k id^k V_k == infinity. An item whose Vs is
// not threshold + 1 points, holds an infinite or off-curve point, or whose id is
// 0 mod q fails without GPU work; the rest are one GPU batch.
std::vector<uint8_t> VerifyBatch(uint32_t threshold, const std::vector<VerifyItem>& items);

struct PublicShares {
  std::vector<secp::Affine> Vc;  // Vc_k = sum_i V_ik; Vc_0 is the public key
  std::vector<secp::Affine> X;   // X_j = sum_k id_j^k Vc_k, one per id
};
// Vs[session][party][k], party i's commitments in the order of ids. Two GPU
// batches: the sums over parties (scalars 1), then the public shares.
std::vector<PublicShares> PublicSharesBatch(uint32_t threshold, const std::vector<Nat>& ids,
                                            const std::vector<std::vector<std::vector<secp::Affine>>>& Vs);

struct Reconstructed {
  Nat secret;
  bool ok = false;
};
// (Shares).ReConstruct per item (upstream, verify): Lagrange interpolation at 0
// over the item's (id, share) pairs, on the host. ok = false on an id that is 0
// mod q or on two ids equal mod q.
std::vector<Reconstructed> ReconstructBatch(const std::vector<std::vector<Nat>>& ids,
                                            const std::vector<std::vector<Nat>>& shares);

}  // namespace mpcx::host::vss
