// eddsa_keygen.hpp -- threshold EdDSA key generation and resharing over Ed25519
// for many wallets at once: the other two EdDSA sessions mpcium runs
// (/root/reference/pkg/mpc/eddsa_keygen_session.go, eddsa_resharing_session.go
// over tss-lib v2 up:eddsa/keygen and up:eddsa/resharing), beside eddsa.hpp's
// signing. Every party is replayed in process; every point equation of a step
// is ONE GPU batch over all sessions and parties of the call (eddsa::MsmBatch,
// edvss::AdmitBatch); scalars mod L and the hashes stay on the host. What
// several receivers would compute alike is computed once per session: the
// opening of a broadcast, the admission of its points, a dealer's Schnorr check.
//
// Restated as recalled; the draw order, the hash inputs and the points below
// are marked "upstream, verify" (they cannot be checked in this image,
// SURVEY.md 8(c)); tests/eddsa_keygen_model.py restates the same steps and
// OpenSSL verifies signatures made with the result.
//
// KeygenBatch, n parties and threshold t per session, party i on its own reader:
//   round 1: u_i = GetRandomPositiveInt(rd, L)
//            vss.Create(t, u_i, ids, rd): a_1..a_t, V_ik = a_k B         [batch 1]
//            (C_i, D_i) = NewHashCommitment(rd, V_i0.x, V_i0.y, ..., V_it.x, V_it.y)
//   round 2: the shares s_ij go out, D_i is opened;
//            schnorr.NewZKProof(Session_i, u_i, V_i0, rd): a = GetRandomPositiveInt(rd, L),
//            alpha = a B                                                 [batch 2]
//            c = SHA512_256i_TAGGED(Session_i, V_i0, B, alpha) mod L, t = a + c u_i,
//            Session_i = session || big.Int(i).Bytes() (signing's conventions)
//   round 3, per dealer i: D_i opens C_i and holds 2 (t + 1) values;
//            every V_ik is admitted: NewECPoint, EightInvEight           [admission]
//            t_i B - c_i V_i0 == alpha_i                                 [batch 3]
//            every j != i: (L - s_ij) B + sum_k id_j^k V_ik == identity  [batch 4]
//            Vc_k = sum_i V_ik, pk = Vc_0                                [batch 5]
//            X_j = sum_k id_j^k Vc_k                                     [batch 6]
//            x_j = sum_i s_ij mod L
// upstream, verify: the verifier's challenge is over the ADMITTED V_i0 (the
// prover's over its own, the same point when honest), and admission is done
// once per dealer and used by every party, the dealer included.
//
// ReshareBatch: every old party i deals w_i = lambda_i x_i (lambda_i the
// Lagrange weight at 0 over the old ids of the call) with vss.Create(t_new, w_i,
// ids_new, rd_i) and commits to its V_i; the new parties open and admit them,
// check every share, then require sum_i V_i0 == pk and derive x'_j and X'_j as
// above. tss-lib's resharing has no Schnorr proofs.
// A session that fails a check aborts alone.
#pragma once

#include <cstdint>
#include <vector>

#include "ed25519.hpp"
#include "tsscommon.hpp"

namespace mpcx::host::eddsa {

// status of a session: 0, or the round that aborted it; culprit: the dealer
// whose message failed, kNoCulprit when the public key did not come out
constexpr uint8_t kAbortKeygenRound3 = 3, kAbortReshare = 4, kNoCulprit = 255;

// Test hooks on dealer 0 of session `tamper_session`: 1 shifts its Schnorr
// response by one, 2 swaps two coordinates of its decommitment, 3 shifts the
// share s_01 by one, 4 adds the point (sqrt(-1), 0) of order four to V_01 before
// committing (admission clears it: the session succeeds with the untampered
// result; without it the share check of a receiver whose id is not 0 mod 4
// fails), 5 commits to an off-curve V_01.
constexpr int kTamperKgSchnorr = 1, kTamperKgDecommit = 2, kTamperKgShare = 3, kTamperKgSmallOrder = 4,
              kTamperKgOffCurve = 5;

struct KeygenSession {
  std::vector<uint8_t> session;  // Session of the Schnorr proofs
  std::vector<RandFn> readers;   // one per party
  bool trace = false;
};
struct KeygenParty {  // what party i sent, as sent
  Nat u, C, t;
  std::vector<ed::Point> V;
  ed::Point alpha;
  std::vector<Nat> shares;
};
struct KeygenResult {
  std::vector<uint8_t> status, culprit;
  std::vector<ed::Point> pk;               // the identity for an aborted session
  std::vector<std::vector<Nat>> x;         // x_j per party; empty when aborted
  std::vector<std::vector<ed::Point>> X;   // X_j per party; empty when aborted
  std::vector<std::vector<KeygenParty>> trace;  // one per traced session, in session order
  double gpu_s = 0;                        // wall time inside the GPU batches
};
// threshold < ids.size() <= 16, threshold >= 1; every session has ids.size() readers.
KeygenResult KeygenBatch(const std::vector<KeygenSession>& sessions, uint32_t threshold, const std::vector<Nat>& ids,
                         int64_t tamper_session = -1, int tamper_kind = 0);

struct ReshareSession {
  std::vector<Nat> shares;      // x_i of the old parties, in the order of old_ids
  ed::Point pk;
  std::vector<RandFn> readers;  // one per old party
};
// old_ids: 1..16 old parties (at least the old threshold + 1 of them, or the
// public key does not come out); new_threshold < new_ids.size() <= 16.
KeygenResult ReshareBatch(const std::vector<ReshareSession>& sessions, const std::vector<Nat>& old_ids,
                          uint32_t new_threshold, const std::vector<Nat>& new_ids);

}  // namespace mpcx::host::eddsa
