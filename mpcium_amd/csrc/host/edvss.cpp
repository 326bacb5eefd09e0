// edvss.cpp -- see edvss.hpp
#include "edvss.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "eddsa.hpp"
#include "hostprof.hpp"
#include "mpcx.h"

namespace mpcx::host::edvss {

namespace {

// 1, id, id^2, ..., id^t mod L
std::vector<Nat> powers(const Nat& id, uint32_t t) {
  std::vector<Nat> p(t + 1);
  p[0] = Nat(1);
  for (uint32_t k = 1; k <= t; ++k) p[k] = ed::ScMul(p[k - 1], id);
  return p;
}

void check_threshold(uint32_t threshold) {
  if (threshold >= kMaxTerms) throw std::invalid_argument("edvss: threshold + 1 > 16");
}

bool is_identity(const ed::Point& P) { return P.x.is_zero() && P.y == Nat(1); }

}  // namespace

std::vector<Nat> CheckIndexes(const std::vector<Nat>& ids) {
  const Nat& L = ed::OrderL();
  std::vector<Nat> r(ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    r[i] = ids[i] % L;
    if (r[i].is_zero()) throw std::invalid_argument("edvss: an id is 0 mod L");
    for (size_t j = 0; j < i; ++j)
      if (r[j] == r[i]) throw std::invalid_argument("edvss: duplicate ids mod L");
  }
  return r;
}

std::vector<Created> CreateBatch(uint32_t threshold, const std::vector<Nat>& ids, const std::vector<Nat>& secrets,
                                 const std::vector<RandFn>& readers) {
  MPCX_PROF("edvss.create");
  check_threshold(threshold);
  if (ids.empty() || ids.size() > kMaxTerms) throw std::invalid_argument("edvss: 1..16 ids per call");
  if (threshold >= ids.size()) throw std::invalid_argument("edvss: threshold >= number of ids");
  if (readers.size() != secrets.size()) throw std::invalid_argument("edvss: one reader per secret");
  const std::vector<Nat> idq = CheckIndexes(ids);
  const Nat& L = ed::OrderL();
  const size_t m = secrets.size(), t = threshold;
  std::vector<Created> out(m);
  std::vector<eddsa::Msm> gs(m * (t + 1));
  parallel_for(m, [&](size_t s) {
    std::vector<Nat> a(t + 1);
    a[0] = secrets[s] % L;
    for (size_t k = 1; k <= t; ++k) a[k] = GetRandomPositiveInt(readers[s], L);
    out[s].shares.resize(idq.size());
    for (size_t j = 0; j < idq.size(); ++j) {  // Horner
      Nat v = a[t];
      for (size_t k = t; k-- > 0;) v = (v * idq[j] + a[k]) % L;
      out[s].shares[j] = v;
    }
    for (size_t k = 0; k <= t; ++k) {
      gs[s * (t + 1) + k].a = a[k];
      gs[s * (t + 1) + k].has_a = true;
    }
  });
  const std::vector<ed::Point> V = eddsa::MsmBatch(gs);  // V_k = a_k B
  for (size_t s = 0; s < m; ++s) out[s].Vs.assign(V.begin() + (long)(s * (t + 1)), V.begin() + (long)((s + 1) * (t + 1)));
  return out;
}

std::vector<uint8_t> VerifyBatch(uint32_t threshold, const std::vector<VerifyItem>& items) {
  MPCX_PROF("edvss.verify");
  check_threshold(threshold);
  const Nat& L = ed::OrderL();
  const size_t n = items.size();
  std::vector<uint8_t> ok(n, 0), sent(n, 0);
  std::vector<eddsa::Msm> ms(n);
  parallel_for(n, [&](size_t i) {
    const VerifyItem& it = items[i];
    if (it.Vs.size() != (size_t)threshold + 1) return;
    for (const auto& v : it.Vs)
      if (!ed::IsOnCurve(v)) return;
    const Nat id = it.id % L;
    if (id.is_zero()) return;
    ms[i].a = ed::ScNeg(it.share);
    ms[i].has_a = true;
    ms[i].b = powers(id, threshold);
    ms[i].P = it.Vs;
    sent[i] = 1;
  });
  std::vector<eddsa::Msm> batch;
  for (size_t i = 0; i < n; ++i)
    if (sent[i]) batch.push_back(std::move(ms[i]));
  const std::vector<ed::Point> r = eddsa::MsmBatch(batch);
  for (size_t i = 0, k = 0; i < n; ++i)
    if (sent[i]) ok[i] = is_identity(r[k++]) ? 1 : 0;
  return ok;
}

std::vector<PublicShares> PublicSharesBatch(uint32_t threshold, const std::vector<Nat>& ids,
                                            const std::vector<std::vector<std::vector<ed::Point>>>& Vs) {
  MPCX_PROF("edvss.public_shares");
  check_threshold(threshold);
  if (ids.empty() || ids.size() > kMaxTerms) throw std::invalid_argument("edvss: 1..16 ids per call");
  const std::vector<Nat> idq = CheckIndexes(ids);
  const size_t m = Vs.size(), n = idq.size(), t = threshold;
  for (const auto& sess : Vs) {
    if (sess.empty() || sess.size() > kMaxTerms) throw std::invalid_argument("edvss: 1..16 commitment vectors per session");
    for (const auto& v : sess)
      if (v.size() != t + 1) throw std::invalid_argument("edvss: a commitment vector is not threshold + 1 points");
  }
  std::vector<PublicShares> out(m);
  // Vc_k = sum_i V_ik
  std::vector<eddsa::Msm> sums(m * (t + 1));
  for (size_t s = 0; s < m; ++s)
    for (size_t k = 0; k <= t; ++k) {
      eddsa::Msm& it = sums[s * (t + 1) + k];
      it.b.assign(Vs[s].size(), Nat(1));
      it.P.resize(Vs[s].size());
      for (size_t i = 0; i < Vs[s].size(); ++i) it.P[i] = Vs[s][i][k];
    }
  const std::vector<ed::Point> vc = eddsa::MsmBatch(sums);
  // X_j = sum_k id_j^k Vc_k
  std::vector<std::vector<Nat>> pw(n);
  for (size_t j = 0; j < n; ++j) pw[j] = powers(idq[j], threshold);
  std::vector<eddsa::Msm> xs(m * n);
  for (size_t s = 0; s < m; ++s) {
    out[s].Vc.assign(vc.begin() + (long)(s * (t + 1)), vc.begin() + (long)((s + 1) * (t + 1)));
    for (size_t j = 0; j < n; ++j) {
      xs[s * n + j].b = pw[j];
      xs[s * n + j].P = out[s].Vc;
    }
  }
  const std::vector<ed::Point> X = eddsa::MsmBatch(xs);
  for (size_t s = 0; s < m; ++s) out[s].X.assign(X.begin() + (long)(s * n), X.begin() + (long)((s + 1) * n));
  return out;
}

bool LagrangeAtZero(const std::vector<Nat>& idq, std::vector<Nat>* out) {
  out->assign(idq.size(), Nat());
  for (size_t i = 0; i < idq.size(); ++i) {
    Nat num(1), den(1);
    for (size_t j = 0; j < idq.size(); ++j) {
      if (j == i) continue;
      num = ed::ScMul(num, idq[j]);
      den = ed::ScMul(den, ed::ScAdd(idq[j], ed::ScNeg(idq[i])));
    }
    Nat inv;
    if (!ed::ScInv(den, &inv)) return false;
    (*out)[i] = ed::ScMul(num, inv);
  }
  return true;
}

std::vector<Reconstructed> ReconstructBatch(const std::vector<std::vector<Nat>>& ids,
                                            const std::vector<std::vector<Nat>>& shares) {
  MPCX_PROF("edvss.reconstruct");
  if (ids.size() != shares.size()) throw std::invalid_argument("edvss: ids and shares differ in number");
  std::vector<Reconstructed> out(ids.size());
  parallel_for(ids.size(), [&](size_t x) {
    if (ids[x].size() != shares[x].size()) return;
    std::vector<Nat> id, lam;
    try {
      id = CheckIndexes(ids[x]);
    } catch (const std::invalid_argument&) {
      return;
    }
    if (!LagrangeAtZero(id, &lam)) return;
    // secret = sum_i s_i prod_{j != i} id_j / (id_j - id_i)
    Nat acc;
    for (size_t i = 0; i < id.size(); ++i) acc = ed::ScAdd(acc, ed::ScMul(shares[x][i], lam[i]));
    out[x].secret = acc;
    out[x].ok = true;
  });
  return out;
}

Admitted AdmitBatch(const std::vector<ed::Point>& points, bool clear) {
  MPCX_PROF("edvss.admit");
  const size_t n = points.size();
  Admitted r;
  r.out.assign(n, ed::Point());
  r.status.assign(n, 0);
  if (!n) return r;
  std::vector<uint32_t> in(n * 16, 0), res(n * 16, 0);
  for (size_t i = 0; i < n; ++i) {
    if (points[i].x.bit_len() > 256 || points[i].y.bit_len() > 256)
      throw std::invalid_argument("edvss AdmitBatch: a coordinate wider than 256 bits");
    points[i].x.to_words(&in[i * 16], 8);
    points[i].y.to_words(&in[i * 16 + 8], 8);
  }
  const int rc = mpcx_ed_admit_batch((uint32_t)n, clear ? 1u : 0u, in.data(), res.data(), r.status.data());
  if (rc != MPCX_OK) throw std::runtime_error(std::string("mpcx_ed_admit_batch: ") + mpcx_last_error());
  for (size_t i = 0; i < n; ++i) {
    if (r.status[i]) continue;
    r.out[i].x = Nat::from_words(&res[i * 16], 8);
    r.out[i].y = Nat::from_words(&res[i * 16 + 8], 8);
  }
  return r;
}

}  // namespace mpcx::host::edvss
