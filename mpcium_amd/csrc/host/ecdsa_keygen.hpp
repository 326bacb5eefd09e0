// ecdsa_keygen.hpp -- GG18 ECDSA key generation over secp256k1 for many wallets
// at once: tss-lib v2 up:ecdsa/keygen rounds 1-4 as mpcium runs them per wallet
// (/root/reference/pkg/mpc/ecdsa_keygen_session.go), with every party replayed
// in process, as eddsa_keygen.hpp does for Ed25519. The committee's
// LocalPreParams are the nodes' (shared across wallets,
// /root/reference/pkg/mpc/node.go:69), so every proof kind of a party is ONE
// batch over the sessions of the call, and every point equation of a step is
// ONE GPU batch over all sessions, dealers and receivers (vss::CreateBatch,
// VerifyBatch, PublicSharesBatch on k_ec_msm). What every receiver would
// compute alike -- the opening of a broadcast, a dealer's DLN, Mod and
// Paillier proofs -- is verified once per dealer.
//
// Restated as recalled; everything below is "upstream, verify" (DESIGN.md
// section 8; tests/ecdsa_keygen_model.py restates the same steps).
//
// Party i of n at threshold t, on its own reader, draws in this order:
//   u_i = GetRandomPositiveInt(rd, q); a_1..a_t of vss.Create; the commitment's
//   256-bit blinding value; the DLN proof (h1, h2, alpha); the DLN proof
//   (h2, h1, beta); the Fac proofs to its peers j != i, ascending (none to
//   itself: keygenload.hpp's mix); the Mod proof. The Paillier proof draws nothing.
//   round 1: V_ik = a_k G (a_0 = u_i), s_ij = f_i(id_j),
//            (C_i, D_i) = NewHashCommitment(rd, V_i0.x, V_i0.y, ..), both DLN proofs
//   round 2: the committee checks, once per call (N_j and N~_j of 2048 bits,
//            h1_j != h2_j, no N~ and no h1 / h2 used twice: std::invalid_argument);
//            every dealer's two DLN proofs verified; the Fac proofs and the Mod
//            proof built under Session_i = session || big.Int(i).Bytes()
//   round 3: per dealer j: D_j opens C_j to t + 1 points on the curve, its Mod
//            proof verifies, its Fac proof to every receiver verifies, and
//            s_ji G == sum_k id_i^k V_jk for every receiver i != j;
//            x_i = sum_j s_ji, Vc_k = sum_j V_jk, BigX_j = sum_k id_j^k Vc_k,
//            ECDSAPub = Vc_0; the Paillier proof with k = id_i and ECDSAPub
//   round 4: every dealer's Paillier proof verified.
// A session that fails a check aborts alone with the round and the lowest
// failing party; every message of the earlier rounds is still built for it (its
// readers make the same draws), the Paillier proofs only for sessions alive
// after round 3.
#pragma once

#include <cstdint>
#include <vector>

#include "keygenload.hpp"
#include "secp256k1.hpp"
#include "tsscommon.hpp"

namespace mpcx::host::ecdsa {

constexpr uint8_t kAbortRound2 = 2, kAbortRound3 = 3, kAbortRound4 = 4, kNoCulprit = 255;

// Test hooks on dealer 0 of session `tamper_session`: 1 shifts the first
// response of its DLN proof (h1, h2, alpha) by one (round 2), 2 swaps two
// coordinates of its decommitment (round 3), 3 shifts the share s_01 by one
// (round 3), 4 shifts y_0 of its Paillier proof by one (round 4).
constexpr int kTamperDLN = 1, kTamperDecommit = 2, kTamperShare = 3, kTamperPaillier = 4;

struct KeygenSession {
  std::vector<uint8_t> session;
  std::vector<RandFn> readers;  // one per party
  bool trace = false;
};
struct KeygenParty {  // what party i sent, as sent
  Nat u, C;
  std::vector<secp::Affine> V;
  std::vector<Nat> shares;
  // SHA512_256i digests: the DLN, Mod and Fac ones as keygenload.hpp's trace,
  // fac[j] zero for j == i, paillier = SHA512_256i(y_0..y_12) (zero when not built)
  Nat dln1, dln2, mod, paillier;
  std::vector<Nat> fac;
};
struct KeygenResult {
  std::vector<uint8_t> status, culprit;
  std::vector<secp::Affine> pub;             // ECDSAPub; infinity for an aborted session
  std::vector<std::vector<Nat>> x;           // x_j per party; empty when aborted
  std::vector<std::vector<secp::Affine>> X;  // BigX_j per party; empty when aborted
  std::vector<std::vector<KeygenParty>> trace;  // one per traced session, in session order
  double gpu_s = 0;                          // wall time inside the GPU batch calls
};
// words per party of a traced session: u (8), C (8), V_0..V_t (16 each), the
// shares (8 each), then the digests dln1, dln2, mod, fac[0..n) and paillier (8 each)
inline size_t TracePartyWords(size_t t, size_t n) { return 16 + 16 * (t + 1) + 8 * n + 8 * (4 + n); }

// parties.size() == ids.size() in [2, 16], 1 <= threshold < parties.size();
// every session has one reader per party. The parties' proof batches of a step
// (different moduli, different readers) run side by side, one thread each.
// serial_launches: every launch of the call is issued after the one before (no
// two in flight), so the number of kernel launches depends on the inputs alone:
// concurrent launches meet in the coalescer (engine.cpp), which merges whatever
// waits when a dispatch slot frees, by timing. For launch-count checks; DESIGN.md
// section 6 has what it costs.
KeygenResult KeygenBatch(const std::vector<keygenload::PartyKeys>& parties, const std::vector<KeygenSession>& sessions,
                         uint32_t threshold, const std::vector<Nat>& ids, int64_t tamper_session = -1,
                         int tamper_kind = 0, bool serial_launches = false);

}  // namespace mpcx::host::ecdsa
