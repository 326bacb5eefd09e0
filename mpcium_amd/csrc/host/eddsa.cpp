// eddsa.cpp -- see eddsa.hpp
#include "eddsa.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>

#include "hostprof.hpp"
#include "mpcx.h"

namespace mpcx::host::eddsa {

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// commitments.NewHashCommitment(rand, secrets...): r = MustGetRandomInt(256),
// C = SHA512_256i(r, secrets...), D = [r, secrets...] (as signing.cpp's)
void hash_commit(const RandFn& rd, const Nat& s0, const Nat& s1, Nat* C, std::vector<Nat>* D) {
  D->clear();
  D->push_back(MustGetRandomInt(rd, 256));
  D->push_back(s0);
  D->push_back(s1);
  *C = SHA512_256i({&(*D)[0], &(*D)[1], &(*D)[2]});
}
bool hash_decommit(const Nat& C, const std::vector<Nat>& D) {
  if (D.size() != 3) return false;
  return SHA512_256i({&D[0], &D[1], &D[2]}) == C;
}
// the challenge of schnorr.ZKProof over Edwards (upstream, verify)
Nat zk_challenge(const std::vector<uint8_t>& session, const ed::Point& X, const ed::Point& alpha) {
  const ed::Point& B = ed::BasePoint();
  return RejectionSample(ed::OrderL(),
                         SHA512_256i_TAGGED(session, {&X.x, &X.y, &B.x, &B.y, &alpha.x, &alpha.y}));
}
// Session || big.Int(i).Bytes() (empty for i = 0)
std::vector<uint8_t> session_of(const std::vector<uint8_t>& session, size_t i) {
  std::vector<uint8_t> s = session;
  const std::vector<uint8_t> ib = Nat((uint64_t)i).to_bytes_be();
  s.insert(s.end(), ib.begin(), ib.end());
  return s;
}

// every id nonzero and distinct mod L (vss::CheckIndexes over L)
bool check_ids(const std::vector<Nat>& ids, std::vector<Nat>* out) {
  const Nat& L = ed::OrderL();
  out->resize(ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    (*out)[i] = ids[i] % L;
    if ((*out)[i].is_zero()) return false;
    for (size_t j = 0; j < i; ++j)
      if ((*out)[j] == (*out)[i]) return false;
  }
  return true;
}

struct Signer {
  Nat r, a, C, t, s;
  std::vector<Nat> D;
  ed::Point R, alpha;
  ed::Point Rsum;
  bool ok = true;
};

}  // namespace

std::vector<ed::Point> MsmBatch(const std::vector<Msm>& items) {
  MPCX_TRACE("gpu.ed", items.size());
  MPCX_PROF("ed.msm_batch");
  const size_t n = items.size();
  std::vector<ed::Point> out(n);
  if (!n) return out;
  size_t np = 0;
  bool any_a = false;
  for (const Msm& t : items) {
    if (t.b.size() != t.P.size()) throw std::invalid_argument("ed MsmBatch: scalars and points differ in number");
    np = std::max(np, t.b.size());
    any_a = any_a || t.has_a;
  }
  if (np > MPCX_ED_MSM_MAX_POINTS) throw std::invalid_argument("ed MsmBatch: more than 16 points in an item");
  if (!np && !any_a) return out;  // nothing in any item: identities
  auto put_scalar = [](const Nat& k, uint32_t* w) {
    if (k.bit_len() > 256) throw std::invalid_argument("ed MsmBatch: a scalar wider than 256 bits");
    k.to_words(w, 8);
  };
  std::vector<uint32_t> av(any_a || !np ? n * 8 : 0, 0), sc(n * np * 8, 0), pt(n * np * 16, 0), res(n * 16, 0);
  parallel_for((n + 255) / 256, [&](size_t blk) {
    for (size_t i = blk * 256; i < std::min(n, blk * 256 + 256); ++i) {
      const Msm& t = items[i];
      if (t.has_a) put_scalar(t.a, &av[i * 8]);
      for (size_t k = 0; k < t.b.size(); ++k) {
        put_scalar(t.b[k], &sc[(i * np + k) * 8]);
        t.P[k].x.to_words(&pt[(i * np + k) * 16], 8);
        t.P[k].y.to_words(&pt[(i * np + k) * 16 + 8], 8);
      }
    }
  });
  const int rc = mpcx_ed_msm_batch((uint32_t)n, (uint32_t)np, av.empty() ? nullptr : av.data(),
                                   np ? sc.data() : nullptr, np ? pt.data() : nullptr, res.data());
  if (rc != MPCX_OK) throw std::runtime_error(std::string("mpcx_ed_msm_batch: ") + mpcx_last_error());
  parallel_for((n + 255) / 256, [&](size_t blk) {
    for (size_t i = blk * 256; i < std::min(n, blk * 256 + 256); ++i) {
      out[i].x = Nat::from_words(&res[i * 16], 8);
      out[i].y = Nat::from_words(&res[i * 16 + 8], 8);
    }
  });
  return out;
}

std::vector<uint8_t> VerifyBatch(const std::vector<VerifyItem>& items) {
  MPCX_PROF("eddsa.verify");
  const size_t n = items.size();
  std::vector<uint8_t> ok(n, 0), sent(n, 0);
  std::vector<Msm> ms(n);
  parallel_for(n, [&](size_t i) {
    const VerifyItem& it = items[i];
    if (!ed::IsOnCurve(it.A)) return;
    const Nat s = ed::FromLe(it.sig + 32, 32);
    if (!(s < ed::OrderL())) return;
    const ed::Bytes32 Aenc = ed::Encode(it.A);
    const Nat h = ed::Hram(it.sig, Aenc.data(), it.msg.data(), it.msg.size());
    ms[i].a = s;
    ms[i].has_a = true;
    ms[i].b = {ed::ScNeg(h)};
    ms[i].P = {it.A};
    sent[i] = 1;
  });
  std::vector<Msm> batch;
  for (size_t i = 0; i < n; ++i)
    if (sent[i]) batch.push_back(std::move(ms[i]));
  const std::vector<ed::Point> r = MsmBatch(batch);
  for (size_t i = 0, k = 0; i < n; ++i)
    if (sent[i]) {
      const ed::Bytes32 e = ed::Encode(r[k++]);
      ok[i] = std::memcmp(e.data(), items[i].sig, 32) == 0 ? 1 : 0;
    }
  return ok;
}

SignResult SignBatch(const std::vector<Wallet>& wallets, int64_t tamper_wallet, int tamper_kind) {
  MPCX_PROF("eddsa.sign");
  const size_t W = wallets.size();
  SignResult res;
  res.sig.assign(W, {});
  res.status.assign(W, kOk);
  if (!W) return res;
  const size_t S = wallets[0].ids.size();
  if (S < 2 || S > kMaxSigners) throw std::invalid_argument("eddsa: 2..16 signers per wallet");
  for (const Wallet& w : wallets)
    if (w.ids.size() != S || w.shares.size() != S || w.readers.size() != S)
      throw std::invalid_argument("eddsa: every wallet needs the same number of ids, shares and readers");
  const Nat& L = ed::OrderL();
  std::vector<Signer> sg(W * S);
  auto at = [&](size_t w, size_t i) -> Signer& { return sg[w * S + i]; };
  auto timed = [&](const std::vector<Msm>& b) {
    const double t0 = now();
    std::vector<ed::Point> r = MsmBatch(b);
    res.gpu_s += now() - t0;
    return r;
  };

  // Lagrange-weighted shares w_i (PrepareForSigning); ids that are 0 or equal mod L are an argument error
  std::vector<Nat> wi(W * S);
  std::vector<uint8_t> bad_ids(W, 0);
  parallel_for(W, [&](size_t w) {
    std::vector<Nat> id;
    if (!check_ids(wallets[w].ids, &id)) {
      bad_ids[w] = 1;
      return;
    }
    for (size_t i = 0; i < S; ++i) {
      Nat num(1), den(1);
      for (size_t j = 0; j < S; ++j) {
        if (j == i) continue;
        num = ed::ScMul(num, id[j]);
        den = ed::ScMul(den, ed::ScAdd(id[j], ed::ScNeg(id[i])));
      }
      Nat inv;
      if (!ed::ScInv(den, &inv)) {
        bad_ids[w] = 1;
        return;
      }
      wi[w * S + i] = ed::ScMul(wallets[w].shares[i] % L, ed::ScMul(num, inv));
    }
  });
  for (size_t w = 0; w < W; ++w)
    if (bad_ids[w]) throw std::invalid_argument("eddsa: a wallet's ids are zero or equal mod L");

  // ---- round 1: r_i, R_i = r_i B, the commitment to R_i
  std::vector<Msm> b1(W * S);
  parallel_for(W, [&](size_t w) {
    for (size_t i = 0; i < S; ++i) {
      at(w, i).r = GetRandomPositiveInt(wallets[w].readers[i], L);
      b1[w * S + i].a = at(w, i).r;
      b1[w * S + i].has_a = true;
    }
  });
  const std::vector<ed::Point> R1 = timed(b1);
  // ---- round 2: the decommitment goes out with a Schnorr proof of r_i
  std::vector<Msm> b2(W * S);
  parallel_for(W, [&](size_t w) {
    for (size_t i = 0; i < S; ++i) {
      Signer& s = at(w, i);
      s.R = R1[w * S + i];
      hash_commit(wallets[w].readers[i], s.R.x, s.R.y, &s.C, &s.D);
      s.a = GetRandomPositiveInt(wallets[w].readers[i], L);
      b2[w * S + i].a = s.a;
      b2[w * S + i].has_a = true;
    }
  });
  const std::vector<ed::Point> A2 = timed(b2);
  parallel_for(W, [&](size_t w) {
    for (size_t i = 0; i < S; ++i) {
      Signer& s = at(w, i);
      s.alpha = A2[w * S + i];
      s.t = ed::ScAdd(s.a, ed::ScMul(zk_challenge(session_of(wallets[w].session, i), s.R, s.alpha), s.r));
    }
    if ((int64_t)w == tamper_wallet) {
      Signer& s0 = at(w, 0);
      if (tamper_kind == kTamperSchnorr) s0.t = ed::ScAdd(s0.t, Nat(1));
      if (tamper_kind == kTamperDecommit) std::swap(s0.D[1], s0.D[2]);
    }
  });
  // ---- round 3: every signer opens and checks every other signer's message,
  // then sums the R_j
  const size_t P = S - 1;
  std::vector<Msm> b3(W * S * P), b4(W * S);
  std::vector<ed::Point> Rj(W * S * P);
  parallel_for(W, [&](size_t w) {
    for (size_t i = 0; i < S; ++i) {
      Signer& s = at(w, i);
      Msm& sum = b4[w * S + i];
      sum.b.push_back(Nat(1));
      sum.P.push_back(s.R);
      size_t pj = 0;
      for (size_t j = 0; j < S; ++j) {
        if (j == i) continue;
        const Signer& o = at(w, j);
        const size_t e = (w * S + i) * P + pj++;
        if (!hash_decommit(o.C, o.D)) {
          s.ok = false;
          continue;
        }
        ed::Point& G = Rj[e];
        G.x = o.D[1];
        G.y = o.D[2];
        if (!ed::IsOnCurve(G) || !ed::IsOnCurve(o.alpha)) {  // crypto.NewECPoint
          s.ok = false;
          continue;
        }
        b3[e].a = o.t;
        b3[e].has_a = true;
        b3[e].b = {ed::ScNeg(zk_challenge(session_of(wallets[w].session, j), G, o.alpha))};
        b3[e].P = {G};
        sum.b.push_back(Nat(1));
        sum.P.push_back(G);
      }
    }
  });
  const std::vector<ed::Point> r3 = timed(b3);
  const std::vector<ed::Point> r4 = timed(b4);
  std::vector<ed::Bytes32> Renc(W), Aenc(W);
  std::vector<Nat> ssum(W);
  parallel_for(W, [&](size_t w) {
    for (size_t i = 0; i < S; ++i) {
      Signer& s = at(w, i);
      for (size_t pj = 0, j = 0; j < S; ++j) {
        if (j == i) continue;
        const ed::Point& got = r3[(w * S + i) * P + pj++];
        const Signer& o = at(w, j);
        // an item that was never filled comes back as the identity and its signer is already not ok
        if (got.x != o.alpha.x || got.y != o.alpha.y) s.ok = false;
      }
      s.Rsum = r4[w * S + i];
    }
    bool ok = true;
    for (size_t i = 0; i < S; ++i) ok = ok && at(w, i).ok;
    if (!ok) {
      res.status[w] = kAbortRound3;
      return;
    }
    Aenc[w] = ed::Encode(wallets[w].pk);
    Nat acc;
    for (size_t i = 0; i < S; ++i) {
      Signer& s = at(w, i);
      const ed::Bytes32 Re = ed::Encode(s.Rsum);
      if (i == 0) Renc[w] = Re;
      const Nat lambda = ed::Hram(Re.data(), Aenc[w].data(), wallets[w].msg.data(), wallets[w].msg.size());
      s.s = ed::ScAdd(s.r, ed::ScMul(lambda, wi[w * S + i]));
      acc = ed::ScAdd(acc, s.s);
    }
    ssum[w] = acc;
  });
  // ---- finalize: the signature, verified by every signer
  std::vector<VerifyItem> vi;
  std::vector<size_t> vw;
  for (size_t w = 0; w < W; ++w) {
    if (res.status[w] != kOk) continue;
    VerifyItem it;
    it.A = wallets[w].pk;
    it.msg = wallets[w].msg;
    const ed::Bytes32 sb = ed::ToLe32(ssum[w]);
    for (size_t i = 0; i < S; ++i) {
      const ed::Bytes32 Re = ed::Encode(at(w, i).Rsum);  // each signer's own R
      std::memcpy(it.sig, Re.data(), 32);
      std::memcpy(it.sig + 32, sb.data(), 32);
      vi.push_back(it);
      vw.push_back(w);
    }
  }
  {
    const double t0 = now();
    const std::vector<uint8_t> ok = VerifyBatch(vi);
    res.gpu_s += now() - t0;
    for (size_t k = 0; k < ok.size(); ++k)
      if (!ok[k]) res.status[vw[k]] = kAbortFinalize;
  }
  for (size_t w = 0; w < W; ++w) {
    if (res.status[w] != kOk) continue;
    const ed::Bytes32 sb = ed::ToLe32(ssum[w]);
    std::memcpy(res.sig[w].data(), Renc[w].data(), 32);
    std::memcpy(res.sig[w].data() + 32, sb.data(), 32);
  }
  // ---- traces
  for (size_t w = 0; w < W; ++w) {
    if (!wallets[w].trace) continue;
    std::vector<uint32_t> tr(S * kTraceSignerWords + kTraceDigestWords, 0);
    const bool live = res.status[w] == kOk;
    std::vector<Nat> vals;
    for (size_t i = 0; i < S; ++i) {
      const Signer& s = at(w, i);
      uint32_t* o = &tr[i * kTraceSignerWords];
      s.r.to_words(o, 8);
      s.R.x.to_words(o + 8, 8);
      s.R.y.to_words(o + 16, 8);
      s.C.to_words(o + 24, 8);
      s.alpha.x.to_words(o + 32, 8);
      s.alpha.y.to_words(o + 40, 8);
      s.t.to_words(o + 48, 8);
      if (live) s.s.to_words(o + 56, 8);
      for (const Nat* v : {&s.C, &s.R.x, &s.R.y, &s.alpha.x, &s.alpha.y, &s.t, &s.s}) vals.push_back(*v);
    }
    if (live) {
      vals.push_back(at(w, 0).Rsum.x);
      vals.push_back(at(w, 0).Rsum.y);
      vals.push_back(ssum[w]);
      std::vector<const Nat*> in;
      for (const Nat& v : vals) in.push_back(&v);
      SHA512_256i(in).to_words(&tr[S * kTraceSignerWords], 8);
    }
    res.trace.push_back(std::move(tr));
  }
  return res;
}

}  // namespace mpcx::host::eddsa
