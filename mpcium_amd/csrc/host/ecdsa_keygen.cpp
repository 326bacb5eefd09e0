// ecdsa_keygen.cpp -- see ecdsa_keygen.hpp
#include "ecdsa_keygen.hpp"

#include <algorithm>
#include <chrono>
#include <functional>
#include <memory>
#include <stdexcept>

#include "expset.hpp"
#include "hostprof.hpp"
#include "proofs.hpp"
#include "vss.hpp"

namespace mpcx::host::ecdsa {

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Timed {  // adds the enclosing scope's wall time to *acc
  double* acc;
  double t0 = now();
  explicit Timed(double* a) : acc(a) {}
  ~Timed() { *acc += now() - t0; }
};

std::vector<uint8_t> session_of(const std::vector<uint8_t>& session, size_t i) {
  std::vector<uint8_t> s = session;
  const std::vector<uint8_t> ib = Nat((uint64_t)i).to_bytes_be();
  s.insert(s.end(), ib.begin(), ib.end());
  return s;
}

Nat hash_all(const std::vector<Nat>& D) {
  std::vector<const Nat*> in;
  for (const Nat& v : D) in.push_back(&v);
  return SHA512_256i(in);
}

// the digests of keygenload.cpp's trace (oracle/keygen_ref.py)
Nat dln_digest(const proofs::DLNProof& p) {
  std::vector<const Nat*> v;
  for (const auto& x : p.Alpha) v.push_back(&x);
  for (const auto& x : p.T) v.push_back(&x);
  return SHA512_256i(v);
}
Nat mod_digest(const proofs::ModProof& p) {
  std::vector<const Nat*> v{&p.W, &p.A, &p.B};
  for (const auto& x : p.X) v.push_back(&x);
  for (const auto& x : p.Z) v.push_back(&x);
  return SHA512_256i(v);
}
Nat fac_digest(const proofs::FacProof& p) {
  const Nat vabs = p.V.mag, vneg(p.V.neg ? 1u : 0u);
  return SHA512_256i({&p.P, &p.Q, &p.A, &p.B, &p.T, &p.Sigma, &p.Z1, &p.Z2, &p.W1, &p.W2, &vabs, &vneg});
}

// round 2's checks of the committee's parameters, the same for every session
void check_committee(const std::vector<keygenload::PartyKeys>& ps) {
  for (size_t i = 0; i < ps.size(); ++i) {
    const keygenload::PartyKeys& p = ps[i];
    if (p.sk.pub.N.bit_len() != 2048) throw std::invalid_argument("ecdsa keygen: a Paillier N is not 2048 bits");
    if (p.NTilde.bit_len() != 2048) throw std::invalid_argument("ecdsa keygen: an NTilde is not 2048 bits");
    if (p.h1 == p.h2) throw std::invalid_argument("ecdsa keygen: h1 == h2");
    if (p.sk.P * p.sk.Q != p.sk.pub.N) throw std::invalid_argument("ecdsa keygen: N != P Q");
    for (size_t j = 0; j < i; ++j) {
      const keygenload::PartyKeys& o = ps[j];
      if (o.NTilde == p.NTilde) throw std::invalid_argument("ecdsa keygen: an NTilde is used by two parties");
      if (o.h1 == p.h1 || o.h1 == p.h2 || o.h2 == p.h1 || o.h2 == p.h2)
        throw std::invalid_argument("ecdsa keygen: an h1 or h2 is used by two parties");
    }
  }
}

}  // namespace

KeygenResult KeygenBatch(const std::vector<keygenload::PartyKeys>& parties, const std::vector<KeygenSession>& sessions,
                         uint32_t threshold, const std::vector<Nat>& ids, int64_t tamper_session, int tamper_kind,
                         bool serial_launches) {
  MPCX_PROF("ecdsa.keygen");
  std::unique_ptr<SerialLaunches> one_launch_at_a_time;  // expset.hpp
  if (serial_launches) one_launch_at_a_time = std::make_unique<SerialLaunches>();
  const size_t S = sessions.size(), n = ids.size(), t1 = (size_t)threshold + 1;
  if (n < 2 || n > vss::kMaxTerms) throw std::invalid_argument("ecdsa keygen: 2..16 parties");
  if (parties.size() != n) throw std::invalid_argument("ecdsa keygen: one key set per party");
  if (threshold < 1 || threshold >= n) throw std::invalid_argument("ecdsa keygen: 1 <= threshold < parties");
  if (tamper_kind < 0 || tamper_kind > kTamperPaillier) throw std::invalid_argument("ecdsa keygen: unknown tamper kind");
  for (const KeygenSession& s : sessions)
    if (s.readers.size() != n) throw std::invalid_argument("ecdsa keygen: one reader per party");
  vss::CheckIndexes(ids);
  check_committee(parties);
  const Nat& q = secp::CurveN();
  const Nat& fp = secp::FieldP();
  KeygenResult res;
  if (!S) return res;
  const bool tamper = tamper_session >= 0 && (size_t)tamper_session < S && tamper_kind != 0;
  const size_t ts = tamper ? (size_t)tamper_session : 0;
  auto E = [n](size_t s, size_t i) { return s * n + i; };
  // one step of every party: the parties' batches are over different moduli and
  // readers, so they run side by side (one thread each, as keygenload.cpp's
  // chains) unless the launches are to be issued one after another
  auto per_party = [&](const std::function<void(size_t)>& step) {
    if (serial_launches) {
      for (size_t i = 0; i < n; ++i) step(i);
      return;
    }
    std::vector<std::function<void()>> fs;
    for (size_t i = 0; i < n; ++i) fs.push_back([&step, i] { step(i); });
    run_concurrently(fs);
  };

  // ---- round 1: u_i, the sharing polynomial, its commitment, both DLN proofs
  std::vector<Nat> u(S * n);
  std::vector<RandFn> rd(S * n);
  parallel_for(S, [&](size_t s) {
    for (size_t i = 0; i < n; ++i) {
      rd[E(s, i)] = sessions[s].readers[i];
      u[E(s, i)] = GetRandomPositiveInt(rd[E(s, i)], q);
    }
  });
  std::vector<vss::Created> cr;
  {
    Timed tm(&res.gpu_s);
    cr = vss::CreateBatch(threshold, ids, u, rd);  // V_ik of every session and party: one batch
  }
  std::vector<Nat> C(S * n);
  std::vector<std::vector<Nat>> D(S * n), shares(S * n);
  parallel_for(S * n, [&](size_t e) {
    D[e].push_back(MustGetRandomInt(rd[e], 256));
    for (const secp::Affine& v : cr[e].Vs) {
      D[e].push_back(secp::FeToNat(v.x));
      D[e].push_back(secp::FeToNat(v.y));
    }
    C[e] = hash_all(D[e]);
    shares[e] = cr[e].shares;
  });
  // party i's readers and proof sessions over the sessions of the call
  std::vector<std::vector<RandFn>> prd(n, std::vector<RandFn>(S));
  std::vector<std::vector<proofs::Bytes>> psess(n, std::vector<proofs::Bytes>(S));
  for (size_t i = 0; i < n; ++i)
    for (size_t s = 0; s < S; ++s) {
      prd[i][s] = rd[E(s, i)];
      psess[i][s] = session_of(sessions[s].session, i);
    }
  std::vector<std::vector<proofs::DLNProof>> dln1(n), dln2(n);
  {
    Timed tm(&res.gpu_s);
    per_party([&](size_t i) {
      const keygenload::PartyKeys& P = parties[i];
      dln1[i] = proofs::DLNProveBatch(P.h1, P.h2, P.alpha, P.p, P.q, P.NTilde, prd[i]);
      dln2[i] = proofs::DLNProveBatch(P.h2, P.h1, P.beta, P.p, P.q, P.NTilde, prd[i]);
    });
  }
  if (tamper && tamper_kind == kTamperDLN) dln1[0][ts].T[0] = dln1[0][ts].T[0] + Nat(1);

  // ---- round 2: every dealer's DLN proofs verified once; Fac and Mod proofs built
  std::vector<uint8_t> fail2(S * n, 0), fail3(S * n, 0), fail4(S * n, 0);
  std::vector<std::vector<std::vector<proofs::FacProof>>> fac(n, std::vector<std::vector<proofs::FacProof>>(n));
  std::vector<std::vector<proofs::ModProof>> mod(n);
  {
    Timed tm(&res.gpu_s);
    per_party([&](size_t i) {
      const keygenload::PartyKeys& P = parties[i];
      const std::vector<uint8_t> ok1 = proofs::DLNVerifyBatch(P.h1, P.h2, P.NTilde, dln1[i]);
      const std::vector<uint8_t> ok2 = proofs::DLNVerifyBatch(P.h2, P.h1, P.NTilde, dln2[i]);
      for (size_t s = 0; s < S; ++s) fail2[E(s, i)] = !(ok1[s] && ok2[s]);
    });
    per_party([&](size_t i) {
      const keygenload::PartyKeys& P = parties[i];
      for (size_t j = 0; j < n; ++j) {
        if (j == i) continue;
        const keygenload::PartyKeys& V = parties[j];
        fac[i][j] = proofs::FacProveBatch(psess[i], P.sk.pub.N, V.NTilde, V.h1, V.h2, P.sk.P, P.sk.Q, prd[i]);
      }
      mod[i] = proofs::ModProveBatch(psess[i], P.sk.pub.N, P.sk.P, P.sk.Q, prd[i]);
    });
  }
  if (tamper && tamper_kind == kTamperDecommit) std::swap(D[E(ts, 0)][1], D[E(ts, 0)][2]);
  if (tamper && tamper_kind == kTamperShare) shares[E(ts, 0)][1] = (shares[E(ts, 0)][1] + Nat(1)) % q;

  // ---- round 3: per dealer the opening, the points, the Mod and Fac proofs, the shares
  std::vector<std::vector<secp::Affine>> Vo(S * n);  // the opened points of a dealer
  parallel_for(S * n, [&](size_t e) {
    if (D[e].size() != 2 * t1 + 1 || hash_all(D[e]) != C[e]) {
      fail3[e] = 1;
      return;
    }
    std::vector<secp::Affine> pts(t1);
    for (size_t k = 0; k < t1; ++k) {
      const Nat &x = D[e][1 + 2 * k], &y = D[e][2 + 2 * k];
      if (!(x < fp) || !(y < fp)) {
        fail3[e] = 1;
        return;
      }
      pts[k].x = secp::NatToFe(x);
      pts[k].y = secp::NatToFe(y);
      pts[k].inf = false;
      if (!secp::IsOnCurve(pts[k])) {
        fail3[e] = 1;
        return;
      }
    }
    Vo[e] = std::move(pts);
  });
  {
    Timed tm(&res.gpu_s);
    per_party([&](size_t j) {
      const keygenload::PartyKeys& P = parties[j];
      const std::vector<uint8_t> okm = proofs::ModVerifyBatch(psess[j], P.sk.pub.N, mod[j]);
      for (size_t s = 0; s < S; ++s)
        if (!okm[s]) fail3[E(s, j)] = 1;
      for (size_t i = 0; i < n; ++i) {
        if (i == j) continue;
        const keygenload::PartyKeys& V = parties[i];
        const std::vector<uint8_t> okf = proofs::FacVerifyBatch(psess[j], P.sk.pub.N, V.NTilde, V.h1, V.h2, fac[j][i]);
        for (size_t s = 0; s < S; ++s)
          if (!okf[s]) fail3[E(s, j)] = 1;
      }
    });
    // s_ji G == sum_k id_i^k V_jk for every session, dealer j and receiver i != j: one batch
    std::vector<vss::VerifyItem> items;
    std::vector<size_t> owner;
    for (size_t e = 0; e < S * n; ++e) {
      if (Vo[e].empty()) continue;
      for (size_t i = 0; i < n; ++i) {
        if (i == e % n) continue;
        items.push_back({Vo[e], ids[i], shares[e][i]});
        owner.push_back(e);
      }
    }
    const std::vector<uint8_t> oks = vss::VerifyBatch(threshold, items);
    for (size_t k = 0; k < items.size(); ++k)
      if (!oks[k]) fail3[owner[k]] = 1;
  }
  res.status.assign(S, 0);
  res.culprit.assign(S, kNoCulprit);
  res.pub.assign(S, secp::Affine());
  res.x.assign(S, {});
  res.X.assign(S, {});
  auto settle = [&](const std::vector<uint8_t>& fail, uint8_t code) {
    for (size_t s = 0; s < S; ++s)
      for (size_t i = 0; i < n && res.status[s] == 0; ++i)
        if (fail[E(s, i)]) {
          res.status[s] = code;
          res.culprit[s] = (uint8_t)i;
        }
  };
  settle(fail2, kAbortRound2);
  settle(fail3, kAbortRound3);
  std::vector<size_t> live;
  std::vector<std::vector<std::vector<secp::Affine>>> Vs;
  for (size_t s = 0; s < S; ++s) {
    if (res.status[s]) continue;
    live.push_back(s);
    Vs.emplace_back();
    for (size_t i = 0; i < n; ++i) Vs.back().push_back(Vo[E(s, i)]);
  }
  std::vector<vss::PublicShares> ps;
  {
    Timed tm(&res.gpu_s);
    ps = vss::PublicSharesBatch(threshold, ids, Vs);  // Vc and BigX of every live session: two batches
  }
  // the Paillier proof of every party over the live sessions, k = id_i
  std::vector<std::vector<proofs::PaillierProof>> pai(n);
  {
    Timed tm(&res.gpu_s);
    per_party([&](size_t i) {
      std::vector<proofs::PaillierStatement> st(live.size());
      for (size_t l = 0; l < live.size(); ++l)
        st[l] = {ids[i], secp::FeToNat(ps[l].Vc[0].x), secp::FeToNat(ps[l].Vc[0].y)};
      const keygenload::PartyKeys& P = parties[i];
      std::vector<std::vector<Nat>> xs;  // GenerateXs once for the prover and the verifier played here
      pai[i] = proofs::PaillierProveBatch(P.sk.pub.N, P.sk.P, P.sk.Q, st, nullptr, &xs);
      if (i == 0 && tamper && tamper_kind == kTamperPaillier)
        for (size_t l = 0; l < live.size(); ++l)
          if (live[l] == ts) pai[0][l].Y[0] = pai[0][l].Y[0] + Nat(1);
      // ---- round 4: verified once per dealer
      const std::vector<uint8_t> okp = proofs::PaillierVerifyBatch(P.sk.pub.N, st, pai[i], &xs);
      for (size_t l = 0; l < live.size(); ++l)
        if (!okp[l]) fail4[E(live[l], i)] = 1;
    });
  }
  settle(fail4, kAbortRound4);
  for (size_t l = 0; l < live.size(); ++l) {
    const size_t s = live[l];
    if (res.status[s]) continue;
    res.pub[s] = ps[l].Vc[0];
    res.X[s] = ps[l].X;
    res.x[s].assign(n, Nat());
    for (size_t i = 0; i < n; ++i)
      for (size_t j = 0; j < n; ++j) res.x[s][i] = (res.x[s][i] + shares[E(s, j)][i]) % q;
  }
  // the traces hold what was sent
  std::vector<size_t> live_at(S, (size_t)-1);
  for (size_t l = 0; l < live.size(); ++l) live_at[live[l]] = l;
  for (size_t s = 0; s < S; ++s) {
    if (!sessions[s].trace) continue;
    std::vector<KeygenParty> tr(n);
    for (size_t i = 0; i < n; ++i) {
      const size_t e = E(s, i);
      KeygenParty& p = tr[i];
      p.u = u[e];
      p.C = C[e];
      p.V = cr[e].Vs;
      p.shares = shares[e];
      p.dln1 = dln_digest(dln1[i][s]);
      p.dln2 = dln_digest(dln2[i][s]);
      p.mod = mod_digest(mod[i][s]);
      p.fac.assign(n, Nat());
      for (size_t j = 0; j < n; ++j)
        if (j != i) p.fac[j] = fac_digest(fac[i][j][s]);
      if (live_at[s] != (size_t)-1) p.paillier = hash_all(pai[i][live_at[s]].Y);
    }
    res.trace.push_back(std::move(tr));
  }
  return res;
}

}  // namespace mpcx::host::ecdsa
