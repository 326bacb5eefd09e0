// eddsa_keygen.cpp -- see eddsa_keygen.hpp
#include "eddsa_keygen.hpp"

#include <algorithm>
#include <chrono>
#include <stdexcept>

#include "eddsa.hpp"
#include "edvss.hpp"
#include "hostprof.hpp"
#include "mpcx.h"

namespace mpcx::host::eddsa {

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the challenge of schnorr.ZKProof over Edwards and Session_i, as eddsa.cpp's (upstream, verify)
Nat zk_challenge(const std::vector<uint8_t>& session, const ed::Point& X, const ed::Point& alpha) {
  const ed::Point& B = ed::BasePoint();
  return RejectionSample(ed::OrderL(),
                         SHA512_256i_TAGGED(session, {&X.x, &X.y, &B.x, &B.y, &alpha.x, &alpha.y}));
}
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
// commitments.NewHashCommitment(rd, V_0.x, V_0.y, ..., V_t.x, V_t.y)
void commit_points(const RandFn& rd, const std::vector<ed::Point>& V, Nat* C, std::vector<Nat>* D) {
  D->clear();
  D->push_back(MustGetRandomInt(rd, 256));
  for (const ed::Point& p : V) {
    D->push_back(p.x);
    D->push_back(p.y);
  }
  *C = hash_all(*D);
}

// One dealer of one session: what it broadcast and sent, and what the receivers make of it.
struct Dealer {
  Nat C;
  std::vector<Nat> D, shares;   // shares: one per receiver
  std::vector<ed::Point> V;     // the admitted points, once ok
  bool ok = true;
};

// The receivers' side both protocols share, over dl[session * m + dealer] with
// t + 1 points each: open every D against its C and admit the points (one
// batch). A dealer that fails is marked and its V left empty.
void open_and_admit(std::vector<Dealer>& dl, uint32_t t, double* gpu_s) {
  const size_t t1 = (size_t)t + 1;
  std::vector<ed::Point> pts(dl.size() * t1);  // the identity stands in for what did not open
  parallel_for(dl.size(), [&](size_t e) {
    Dealer& d = dl[e];
    if (d.D.size() != 2 * t1 + 1 || hash_all(d.D) != d.C) {
      d.ok = false;
      return;
    }
    for (size_t k = 0; k < t1; ++k) {
      pts[e * t1 + k].x = d.D[1 + 2 * k];
      pts[e * t1 + k].y = d.D[2 + 2 * k];
    }
  });
  const double t0 = now();
  const edvss::Admitted adm = edvss::AdmitBatch(pts, true);
  *gpu_s += now() - t0;
  for (size_t e = 0; e < dl.size(); ++e) {
    if (!dl[e].ok) continue;
    for (size_t k = 0; k < t1; ++k)
      if (adm.status[e * t1 + k]) dl[e].ok = false;
    if (dl[e].ok) dl[e].V.assign(adm.out.begin() + (long)(e * t1), adm.out.begin() + (long)((e + 1) * t1));
  }
}

// (L - s_ij) B + sum_k id_j^k V_ik == identity for every dealer still ok and
// every receiver j but `skip_own` ones (j == dealer index within the session), one batch
void check_shares(std::vector<Dealer>& dl, size_t m, const std::vector<Nat>& idq, uint32_t t, bool skip_own,
                  double* gpu_s) {
  const size_t n = idq.size();
  std::vector<std::vector<Nat>> pw(n);
  for (size_t j = 0; j < n; ++j) {
    pw[j].resize(t + 1);
    pw[j][0] = Nat(1);
    for (uint32_t k = 1; k <= t; ++k) pw[j][k] = ed::ScMul(pw[j][k - 1], idq[j]);
  }
  std::vector<Msm> b(dl.size() * n);
  parallel_for(dl.size(), [&](size_t e) {
    const Dealer& d = dl[e];
    if (!d.ok) return;
    for (size_t j = 0; j < n; ++j) {
      if (skip_own && j == e % m) continue;
      Msm& it = b[e * n + j];
      it.a = ed::ScNeg(d.shares[j]);
      it.has_a = true;
      it.b = pw[j];
      it.P = d.V;
    }
  });
  const double t0 = now();
  const std::vector<ed::Point> r = MsmBatch(b);  // an item left empty comes back as the identity
  *gpu_s += now() - t0;
  for (size_t e = 0; e < dl.size(); ++e)
    for (size_t j = 0; j < n; ++j)
      if (!(r[e * n + j].x.is_zero() && r[e * n + j].y == Nat(1))) dl[e].ok = false;
}

// status and culprit of every session from its dealers; then Vc, X and x_j of the live ones
void finish(const std::vector<Dealer>& dl, size_t S, size_t m, const std::vector<Nat>& ids, uint32_t t,
            uint8_t abort_code, KeygenResult* res) {
  const size_t n = ids.size();
  res->status.assign(S, 0);
  res->culprit.assign(S, kNoCulprit);
  res->pk.assign(S, ed::Point());
  res->x.assign(S, {});
  res->X.assign(S, {});
  std::vector<size_t> live;
  std::vector<std::vector<std::vector<ed::Point>>> Vs;
  for (size_t s = 0; s < S; ++s) {
    for (size_t i = 0; i < m && res->status[s] == 0; ++i)
      if (!dl[s * m + i].ok) {
        res->status[s] = abort_code;
        res->culprit[s] = (uint8_t)i;
      }
    if (res->status[s]) continue;
    live.push_back(s);
    Vs.emplace_back();
    for (size_t i = 0; i < m; ++i) Vs.back().push_back(dl[s * m + i].V);
  }
  const double t0 = now();
  const std::vector<edvss::PublicShares> ps = edvss::PublicSharesBatch(t, ids, Vs);
  res->gpu_s += now() - t0;
  for (size_t q = 0; q < live.size(); ++q) {
    const size_t s = live[q];
    res->pk[s] = ps[q].Vc[0];
    res->X[s] = ps[q].X;
    res->x[s].assign(n, Nat());
    for (size_t j = 0; j < n; ++j)
      for (size_t i = 0; i < m; ++i) res->x[s][j] = ed::ScAdd(res->x[s][j], dl[s * m + i].shares[j]);
  }
}

}  // namespace

KeygenResult KeygenBatch(const std::vector<KeygenSession>& sessions, uint32_t threshold, const std::vector<Nat>& ids,
                         int64_t tamper_session, int tamper_kind) {
  MPCX_PROF("eddsa.keygen");
  const size_t S = sessions.size(), n = ids.size();
  if (n < 2 || n > edvss::kMaxTerms) throw std::invalid_argument("eddsa keygen: 2..16 parties");
  if (threshold < 1 || threshold >= n) throw std::invalid_argument("eddsa keygen: 1 <= threshold < parties");
  if (tamper_kind < 0 || tamper_kind > kTamperKgOffCurve) throw std::invalid_argument("eddsa keygen: unknown tamper kind");
  for (const KeygenSession& s : sessions)
    if (s.readers.size() != n) throw std::invalid_argument("eddsa keygen: one reader per party");
  const std::vector<Nat> idq = edvss::CheckIndexes(ids);
  const Nat& L = ed::OrderL();
  const Nat& p = ed::FieldP();
  KeygenResult res;
  if (!S) return res;
  auto tampered = [&](size_t s, int kind) { return (int64_t)s == tamper_session && tamper_kind == kind; };

  // ---- round 1: u_i, the sharing polynomial and its commitments
  std::vector<Nat> u(S * n);
  std::vector<RandFn> rd(S * n);
  parallel_for(S, [&](size_t s) {
    for (size_t i = 0; i < n; ++i) {
      rd[s * n + i] = sessions[s].readers[i];
      u[s * n + i] = GetRandomPositiveInt(rd[s * n + i], L);
    }
  });
  double t0 = now();
  std::vector<edvss::Created> cr = edvss::CreateBatch(threshold, ids, u, rd);
  res.gpu_s += now() - t0;
  std::vector<Dealer> dl(S * n);
  std::vector<Nat> a(S * n);
  std::vector<Msm> b2(S * n);
  parallel_for(S, [&](size_t s) {
    for (size_t i = 0; i < n; ++i) {
      const size_t e = s * n + i;
      std::vector<ed::Point>& V = cr[e].Vs;
      if (i == 0 && tampered(s, kTamperKgSmallOrder)) {  // + (sqrt(-1), 0), of order four: (x, y) -> (i y, i x)
        static const Nat sqrt_m1 = Nat::from_hex("2b8324804fc1df0b2b4d00993dfbd7a72f431806ad2fe478c4ee1b274a0ea0b0");
        const Nat x = (sqrt_m1 * V[1].y) % p, y = (sqrt_m1 * V[1].x) % p;
        V[1].x = x;
        V[1].y = y;
      }
      if (i == 0 && tampered(s, kTamperKgOffCurve)) V[1].y = (V[1].y + Nat(1)) % p;
      commit_points(rd[e], V, &dl[e].C, &dl[e].D);
      dl[e].shares = cr[e].shares;
      // ---- round 2: the Schnorr proof of u_i
      a[e] = GetRandomPositiveInt(rd[e], L);
      b2[e].a = a[e];
      b2[e].has_a = true;
    }
  });
  t0 = now();
  const std::vector<ed::Point> alpha = MsmBatch(b2);
  res.gpu_s += now() - t0;
  std::vector<Nat> tt(S * n);
  parallel_for(S, [&](size_t s) {
    for (size_t i = 0; i < n; ++i) {
      const size_t e = s * n + i;
      tt[e] = ed::ScAdd(a[e], ed::ScMul(zk_challenge(session_of(sessions[s].session, i), cr[e].Vs[0], alpha[e]), u[e]));
    }
    if (tampered(s, kTamperKgSchnorr)) tt[s * n] = ed::ScAdd(tt[s * n], Nat(1));
    if (tampered(s, kTamperKgDecommit)) std::swap(dl[s * n].D[1], dl[s * n].D[2]);
    if (tampered(s, kTamperKgShare)) dl[s * n].shares[1] = ed::ScAdd(dl[s * n].shares[1], Nat(1));
  });
  // the traces hold what was sent
  for (size_t s = 0; s < S; ++s) {
    if (!sessions[s].trace) continue;
    std::vector<KeygenParty> tr(n);
    for (size_t i = 0; i < n; ++i) {
      const size_t e = s * n + i;
      tr[i].u = u[e];
      tr[i].C = dl[e].C;
      tr[i].t = tt[e];
      tr[i].V = cr[e].Vs;
      tr[i].alpha = alpha[e];
      tr[i].shares = dl[e].shares;
    }
    res.trace.push_back(std::move(tr));
  }

  // ---- round 3
  open_and_admit(dl, threshold, &res.gpu_s);
  std::vector<Msm> b3(S * n);
  parallel_for(S * n, [&](size_t e) {
    Dealer& d = dl[e];
    if (!d.ok) return;
    if (!ed::IsOnCurve(alpha[e])) {  // crypto.NewECPoint on the proof's alpha
      d.ok = false;
      return;
    }
    b3[e].a = tt[e];
    b3[e].has_a = true;
    b3[e].b = {ed::ScNeg(zk_challenge(session_of(sessions[e / n].session, e % n), d.V[0], alpha[e]))};
    b3[e].P = {d.V[0]};
  });
  t0 = now();
  const std::vector<ed::Point> r3 = MsmBatch(b3);
  res.gpu_s += now() - t0;
  for (size_t e = 0; e < S * n; ++e)
    if (dl[e].ok && (r3[e].x != alpha[e].x || r3[e].y != alpha[e].y)) dl[e].ok = false;
  check_shares(dl, n, idq, threshold, true, &res.gpu_s);
  finish(dl, S, n, ids, threshold, kAbortKeygenRound3, &res);
  return res;
}

KeygenResult ReshareBatch(const std::vector<ReshareSession>& sessions, const std::vector<Nat>& old_ids,
                          uint32_t new_threshold, const std::vector<Nat>& new_ids) {
  MPCX_PROF("eddsa.reshare");
  const size_t S = sessions.size(), m = old_ids.size(), n = new_ids.size();
  if (m < 1 || m > edvss::kMaxTerms) throw std::invalid_argument("eddsa reshare: 1..16 old parties");
  if (n < 2 || n > edvss::kMaxTerms) throw std::invalid_argument("eddsa reshare: 2..16 new parties");
  if (new_threshold < 1 || new_threshold >= n) throw std::invalid_argument("eddsa reshare: 1 <= threshold < new parties");
  for (const ReshareSession& s : sessions)
    if (s.readers.size() != m || s.shares.size() != m)
      throw std::invalid_argument("eddsa reshare: one share and one reader per old party");
  const std::vector<Nat> oldq = edvss::CheckIndexes(old_ids), newq = edvss::CheckIndexes(new_ids);
  std::vector<Nat> lam;
  if (!edvss::LagrangeAtZero(oldq, &lam)) throw std::invalid_argument("eddsa reshare: old ids without Lagrange weights");
  KeygenResult res;
  if (!S) return res;
  // every old party deals w_i = lambda_i x_i to the new committee
  std::vector<Nat> w(S * m);
  std::vector<RandFn> rd(S * m);
  for (size_t s = 0; s < S; ++s)
    for (size_t i = 0; i < m; ++i) {
      rd[s * m + i] = sessions[s].readers[i];
      w[s * m + i] = ed::ScMul(sessions[s].shares[i], lam[i]);
    }
  double gpu_s = 0;
  double t0 = now();
  std::vector<edvss::Created> cr = edvss::CreateBatch(new_threshold, new_ids, w, rd);
  gpu_s += now() - t0;
  std::vector<Dealer> dl(S * m);
  parallel_for(S * m, [&](size_t e) {
    commit_points(rd[e], cr[e].Vs, &dl[e].C, &dl[e].D);
    dl[e].shares = cr[e].shares;
  });
  // the new parties
  open_and_admit(dl, new_threshold, &gpu_s);
  check_shares(dl, m, newq, new_threshold, false, &gpu_s);
  finish(dl, S, m, new_ids, new_threshold, kAbortReshare, &res);
  res.gpu_s += gpu_s;
  for (size_t s = 0; s < S; ++s) {
    if (res.status[s]) continue;
    if (res.pk[s].x != sessions[s].pk.x || res.pk[s].y != sessions[s].pk.y) {  // sum_i V_i0 != pk
      res.status[s] = kAbortReshare;
      res.pk[s] = ed::Point();
      res.x[s].clear();
      res.X[s].clear();
    }
  }
  return res;
}

}  // namespace mpcx::host::eddsa
