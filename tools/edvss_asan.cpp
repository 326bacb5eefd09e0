// Property check of the host-only part of the Feldman VSS over Ed25519 (csrc/host/edvss.cpp: CheckIndexes,
// LagrangeAtZero, ReconstructBatch) under ASAN + UBSAN (CPU only; tools/edvss_asan.sh). The GPU entries the
// file also calls are stubbed below: nothing here reaches them.
//   deal: a random polynomial of degree t over ids of up to 16 words, shares by Horner mod L;
//   reconstruct: any t + 1 shares give the secret, a share changed by one gives another value;
//   weights: sum_i lambda_i = 1 (the constant polynomial), lambda_i (id_j - id_i) products invert;
//   refusals: an id that is 0 mod L, two ids equal mod L, ids and shares of different lengths.
#include <cstdio>
#include <random>
#include <stdexcept>

#include "eddsa.hpp"
#include "edvss.hpp"
#include "mpcx.h"
using namespace mpcx::host;

namespace mpcx::host::eddsa {
std::vector<ed::Point> MsmBatch(const std::vector<Msm>&) { throw std::logic_error("no device in this program"); }
}  // namespace mpcx::host::eddsa
extern "C" int mpcx_ed_admit_batch(uint32_t, uint32_t, const uint32_t*, uint32_t*, uint8_t*) { return MPCX_ENODEV; }
extern "C" const char* mpcx_last_error(void) { return "no device in this program"; }
extern "C" int mpcx_bound_devices(int* n, int*, int) {  // the worker pool sizes itself by it
  *n = 0;
  return MPCX_OK;
}

static Nat rand_words(std::mt19937_64& g, size_t words, bool ones) {
  std::vector<uint32_t> w(words);
  for (auto& x : w) x = ones ? 0xFFFFFFFFu : (uint32_t)g();
  return Nat::from_words(w.data(), words);
}

int main() {
  std::mt19937_64 g(0xED55);
  const Nat& L = ed::OrderL();
  long bad = 0, n = 0;
  for (int it = 0; it < 300; ++it) {
    const size_t k = 1 + g() % 16, t = k - 1;  // k shares of a degree-t polynomial
    std::vector<Nat> ids(k), coef(t + 1), shares(k);
    for (size_t i = 0; i < k; ++i) ids[i] = rand_words(g, 1 + g() % 16, false) + Nat(1);
    for (auto& c : coef) c = rand_words(g, 8, (g() % 8) == 0) % L;
    std::vector<Nat> idq;
    try {
      idq = edvss::CheckIndexes(ids);
    } catch (const std::invalid_argument&) {
      continue;  // a random collision mod L: not in this lifetime, but not an error of the code
    }
    for (size_t j = 0; j < k; ++j) {
      Nat v = coef[t];
      for (size_t q = t; q-- > 0;) v = (v * idq[j] + coef[q]) % L;
      shares[j] = v + (g() % 2 ? L : Nat());  // shares count mod L
    }
    auto r = edvss::ReconstructBatch({ids}, {shares});
    if (!r[0].ok || r[0].secret != coef[0]) ++bad;
    std::vector<Nat> lam;
    if (!edvss::LagrangeAtZero(idq, &lam)) ++bad;
    Nat s;
    for (const Nat& l : lam) s = ed::ScAdd(s, l);
    if (s != Nat(1)) ++bad;
    const size_t v = g() % k;
    shares[v] = ed::ScAdd(shares[v], Nat(1));
    r = edvss::ReconstructBatch({ids}, {shares});
    if (!r[0].ok || r[0].secret == coef[0]) ++bad;
    // refusals
    std::vector<Nat> z = ids, d = ids;
    z[g() % k] = L * Nat(g() % 5);
    if (edvss::ReconstructBatch({z}, {shares})[0].ok) ++bad;
    if (k > 1) {
      d[0] = d[k - 1] + L * Nat(1 + g() % 3);
      if (edvss::ReconstructBatch({d}, {shares})[0].ok) ++bad;
      std::vector<Nat> fewer(shares.begin(), shares.end() - 1);
      if (edvss::ReconstructBatch({ids}, {fewer})[0].ok) ++bad;
    }
    ++n;
  }
  bool threw = false;
  try {
    edvss::ReconstructBatch({{Nat(1)}}, {});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  if (!threw || !edvss::ReconstructBatch({}, {}).empty()) ++bad;
  std::printf("checked %ld, bad %ld\n", n, bad);
  return bad != 0 || n < 250;
}
