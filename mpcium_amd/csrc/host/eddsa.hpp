// eddsa.hpp -- threshold EdDSA over Ed25519 for many wallets at once: what
// mpcium runs beside GG18 for every wallet (tss-lib v2 up:eddsa/signing through
// /root/reference/pkg/mpc/eddsa_signing_session.go, every result checked with
// decred's edwards.Verify). Every point equation of a step is ONE multi-scalar
// batch on the GPU over all wallets and signers of the call (MsmBatch:
// mpcx_ed_msm_batch, libmpcx's k_ed_msm); scalars mod L and the hashes stay on
// the host (ed25519.hpp).
//
// VerifyBatch -- edwards.Verify per item: A on the curve, s < L (RFC 8032 and
// OpenSSL; whether decred's Verify also rejects s >= L is "upstream, verify"),
// and enc(s B - h A) equal to the signature's first 32 bytes byte for byte,
// h = SHA-512(R || enc(A) || M) mod L. One batch: a = s, one point A with
// scalar L - h.
//
// SignBatch -- up:eddsa/signing rounds 1-3 and finalize, every one of the t + 1
// signers of every wallet replayed in process (as signing::RunSigning does for
// GG18). Restated as recalled; the draw order and the hash inputs are marked
// "upstream, verify" (they cannot be checked in this image);
// tests/eddsa_model.py restates the same steps in Python and OpenSSL verifies
// the signatures. Per wallet and signer i, from the signer's own reader:
//   round 1: r_i = GetRandomPositiveInt(rd, L); R_i = r_i B            [batch 1]
//            (C_i, D_i) = commitments.NewHashCommitment(rd, R_i.x, R_i.y)
//   round 2: D_i sent; schnorr.NewZKProof(Session_i, r_i, R_i, rd):
//            a = GetRandomPositiveInt(rd, L), alpha = a B               [batch 2]
//            c = SHA512_256i_TAGGED(Session_i, R_i.x, R_i.y, B.x, B.y, alpha.x, alpha.y) mod L, t = a + c r_i
//            Session_i = the wallet's session bytes || big.Int(i).Bytes()
//   round 3: every signer i opens every other D_j against C_j, takes R_j
//            through NewECPoint and checks t_j B - c_j R_j == alpha_j    [batch 3]
//            R = R_i + sum_j R_j (scalars 1)                            [batch 4]
//            lambda = SHA-512(enc(R) || enc(pk) || M) mod L
//            s_i = r_i + lambda w_i, w_i = x_i prod_{j != i} id_j / (id_j - id_i)
//   finalize: s = sum s_i; signature enc(R) || LE32(s); VerifyBatch by every signer  [batch 5]
// Not restated: tss-lib clears the cofactor of a received R_j (EightInvEight)
// before using it; for the honest R_j = r_j B that is the identity map.
// A wallet that fails a check aborts alone, with the round reported.
#pragma once

#include <cstdint>
#include <vector>

#include "ed25519.hpp"
#include "tsscommon.hpp"

namespace mpcx::host::eddsa {

constexpr uint32_t kMaxSigners = 16;

struct Msm {
  Nat a;  // scalar of B, used as it is (< 2^256)
  bool has_a = false;
  std::vector<Nat> b;
  std::vector<ed::Point> P;  // b.size() points, at most 16
};
// a B + sum_k b_k P_k per item on the GPU (mpcx_ed_msm_batch). Scalars must be
// below 2^256 and are not reduced; items are padded to the batch's widest
// with zero scalars. Throws without a bound device.
std::vector<ed::Point> MsmBatch(const std::vector<Msm>& items);

struct VerifyItem {
  ed::Point A;
  std::vector<uint8_t> msg;
  uint8_t sig[64];
};
std::vector<uint8_t> VerifyBatch(const std::vector<VerifyItem>& items);

struct Wallet {
  std::vector<Nat> ids;     // the signers' ids (any width, used mod L), one per signer
  std::vector<Nat> shares;  // their Shamir shares x_i
  ed::Point pk;
  std::vector<uint8_t> msg;      // taken as given (mpcium passes tx.Bytes(): no leading zero bytes)
  std::vector<uint8_t> session;  // Session of the Schnorr proofs
  std::vector<RandFn> readers;   // one per signer
  bool trace = false;
};

// status of a wallet: 0, or the round that aborted it
constexpr uint8_t kOk = 0, kAbortRound3 = 3, kAbortFinalize = 4;
// Test hooks on signer 0 of wallet `tamper_wallet`: shift its Schnorr response
// by one, or swap the two coordinates of its decommitment.
constexpr int kTamperSchnorr = 1, kTamperDecommit = 2;

// Per traced wallet, kTraceSignerWords per signer -- r_i (8), R_i.x, R_i.y (16),
// C_i (8), alpha.x, alpha.y (16), t (8), s_i (8) -- then 8 words of
// SHA512_256i(per signer: C_i, R_i.x, R_i.y, alpha.x, alpha.y, t, s_i; then R.x, R.y, s);
// an aborted wallet's s_i and digest are zero.
constexpr uint32_t kTraceSignerWords = 64, kTraceDigestWords = 8;

struct SignResult {
  std::vector<std::array<uint8_t, 64>> sig;  // zero for an aborted wallet
  std::vector<uint8_t> status;
  std::vector<std::vector<uint32_t>> trace;  // one per traced wallet, in wallet order
  double gpu_s = 0;                          // wall time inside the five MsmBatch calls
};
// Every wallet of a call has the same number of signers (2..16).
SignResult SignBatch(const std::vector<Wallet>& wallets, int64_t tamper_wallet = -1, int tamper_kind = 0);

}  // namespace mpcx::host::eddsa
