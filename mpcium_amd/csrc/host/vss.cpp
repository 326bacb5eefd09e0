// vss.cpp -- see vss.hpp
#include "vss.hpp"

#include <stdexcept>

#include "hostprof.hpp"

namespace mpcx::host::vss {

namespace {

// 1, id, id^2, ..., id^t mod q
std::vector<Nat> powers(const Nat& id, uint32_t t, const Nat& q) {
  std::vector<Nat> p(t + 1);
  p[0] = Nat(1);
  for (uint32_t k = 1; k <= t; ++k) p[k] = (p[k - 1] * id) % q;
  return p;
}

void check_threshold(uint32_t threshold) {
  if (threshold >= kMaxTerms) throw std::invalid_argument("vss: threshold + 1 > 16");
}

}  // namespace

std::vector<Nat> CheckIndexes(const std::vector<Nat>& ids) {
  const Nat& q = secp::CurveN();
  std::vector<Nat> r(ids.size());
  for (size_t i = 0; i < ids.size(); ++i) {
    r[i] = ids[i] % q;
    if (r[i].is_zero()) throw std::invalid_argument("vss: an id is 0 mod q");
    for (size_t j = 0; j < i; ++j)
      if (r[j] == r[i]) throw std::invalid_argument("vss: duplicate ids mod q");
  }
  return r;
}

std::vector<Created> CreateBatch(uint32_t threshold, const std::vector<Nat>& ids, const std::vector<Nat>& secrets,
                                 const std::vector<RandFn>& readers) {
  MPCX_PROF("vss.create");
  check_threshold(threshold);
  if (ids.empty() || ids.size() > kMaxTerms) throw std::invalid_argument("vss: 1..16 ids per call");
  if (threshold >= ids.size()) throw std::invalid_argument("vss: threshold >= number of ids");
  if (readers.size() != secrets.size()) throw std::invalid_argument("vss: one reader per secret");
  const std::vector<Nat> idq = CheckIndexes(ids);
  const Nat& q = secp::CurveN();
  const size_t m = secrets.size(), t = threshold;
  std::vector<Created> out(m);
  std::vector<secp::Msm> gs(m * (t + 1));
  parallel_for(m, [&](size_t s) {
    std::vector<Nat> a(t + 1);
    a[0] = secrets[s];
    for (size_t k = 1; k <= t; ++k) a[k] = GetRandomPositiveInt(readers[s], q);
    out[s].shares.resize(idq.size());
    for (size_t j = 0; j < idq.size(); ++j) {  // Horner
      Nat v = a[t] % q;
      for (size_t k = t; k-- > 0;) v = (v * idq[j] + a[k]) % q;
      out[s].shares[j] = v;
    }
    for (size_t k = 0; k <= t; ++k) gs[s * (t + 1) + k].a = a[k];
  });
  const std::vector<secp::Affine> V = secp::MsmBatch(gs);  // V_k = a_k G
  for (size_t s = 0; s < m; ++s) out[s].Vs.assign(V.begin() + (long)(s * (t + 1)), V.begin() + (long)((s + 1) * (t + 1)));
  return out;
}

std::vector<uint8_t> VerifyBatch(uint32_t threshold, const std::vector<VerifyItem>& items) {
  MPCX_PROF("vss.verify");
  check_threshold(threshold);
  const Nat& q = secp::CurveN();
  const size_t n = items.size();
  std::vector<uint8_t> ok(n, 0), sent(n, 0);
  std::vector<secp::Msm> ms(n);
  parallel_for(n, [&](size_t i) {
    const VerifyItem& it = items[i];
    if (it.Vs.size() != (size_t)threshold + 1) return;
    for (const auto& v : it.Vs)
      if (!secp::IsOnCurve(v)) return;  // infinity included
    const Nat id = it.id % q;
    if (id.is_zero()) return;
    const Nat s = it.share % q;
    ms[i].a = s.is_zero() ? s : q - s;
    ms[i].b = powers(id, threshold, q);
    ms[i].P = it.Vs;
    sent[i] = 1;
  });
  std::vector<secp::Msm> batch;
  for (size_t i = 0; i < n; ++i)
    if (sent[i]) batch.push_back(std::move(ms[i]));
  const std::vector<secp::Affine> r = secp::MsmBatch(batch);
  for (size_t i = 0, k = 0; i < n; ++i)
    if (sent[i]) ok[i] = r[k++].inf ? 1 : 0;
  return ok;
}

std::vector<PublicShares> PublicSharesBatch(uint32_t threshold, const std::vector<Nat>& ids,
                                            const std::vector<std::vector<std::vector<secp::Affine>>>& Vs) {
  MPCX_PROF("vss.public_shares");
  check_threshold(threshold);
  if (ids.empty() || ids.size() > kMaxTerms) throw std::invalid_argument("vss: 1..16 ids per call");
  const std::vector<Nat> idq = CheckIndexes(ids);
  const Nat& q = secp::CurveN();
  const size_t m = Vs.size(), n = idq.size(), t = threshold;
  for (const auto& sess : Vs) {
    if (sess.size() != n) throw std::invalid_argument("vss: one commitment vector per id");
    for (const auto& v : sess)
      if (v.size() != t + 1) throw std::invalid_argument("vss: a commitment vector is not threshold + 1 points");
  }
  std::vector<PublicShares> out(m);
  // Vc_k = sum_i V_ik
  std::vector<secp::Msm> sums(m * (t + 1));
  for (size_t s = 0; s < m; ++s)
    for (size_t k = 0; k <= t; ++k) {
      secp::Msm& it = sums[s * (t + 1) + k];
      it.b.assign(n, Nat(1));
      it.P.resize(n);
      for (size_t i = 0; i < n; ++i) it.P[i] = Vs[s][i][k];
    }
  const std::vector<secp::Affine> vc = secp::MsmBatch(sums);
  // X_j = sum_k id_j^k Vc_k
  std::vector<std::vector<Nat>> pw(n);
  for (size_t j = 0; j < n; ++j) pw[j] = powers(idq[j], threshold, q);
  std::vector<secp::Msm> xs(m * n);
  for (size_t s = 0; s < m; ++s) {
    out[s].Vc.assign(vc.begin() + (long)(s * (t + 1)), vc.begin() + (long)((s + 1) * (t + 1)));
    for (size_t j = 0; j < n; ++j) {
      xs[s * n + j].b = pw[j];
      xs[s * n + j].P = out[s].Vc;
    }
  }
  const std::vector<secp::Affine> X = secp::MsmBatch(xs);
  for (size_t s = 0; s < m; ++s) out[s].X.assign(X.begin() + (long)(s * n), X.begin() + (long)((s + 1) * n));
  return out;
}

std::vector<Reconstructed> ReconstructBatch(const std::vector<std::vector<Nat>>& ids,
                                            const std::vector<std::vector<Nat>>& shares) {
  MPCX_PROF("vss.reconstruct");
  if (ids.size() != shares.size()) throw std::invalid_argument("vss: ids and shares differ in number");
  const Nat& q = secp::CurveN();
  std::vector<Reconstructed> out(ids.size());
  parallel_for(ids.size(), [&](size_t x) {
    if (ids[x].size() != shares[x].size()) return;
    std::vector<Nat> id;
    try {
      id = CheckIndexes(ids[x]);
    } catch (const std::invalid_argument&) {
      return;
    }
    // secret = sum_i s_i prod_{j != i} id_j / (id_j - id_i)
    Nat acc;
    for (size_t i = 0; i < id.size(); ++i) {
      Nat num(1), den(1);
      for (size_t j = 0; j < id.size(); ++j) {
        if (j == i) continue;
        num = (num * id[j]) % q;
        den = (den * ((id[j] + q - id[i]) % q)) % q;
      }
      Nat inv;
      if (!mod_inverse(Int(den), q, &inv)) return;
      acc = (acc + (shares[x][i] % q) * ((num * inv) % q)) % q;
    }
    out[x].secret = acc;
    out[x].ok = true;
  });
  return out;
}

}  // namespace mpcx::host::vss
