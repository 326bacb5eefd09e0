// Property check of the host Ed25519 arithmetic (csrc/host/ed25519.cpp) under ASAN + UBSAN (CPU only;
// tools/ed25519_asan.sh): random and all-ones operands through ScReduce, ScMul, ScInv, Decode and Encode.
//   reduce: r < L and r = v mod L for 1..64-byte little-endian values;   mul / inverse: a a^-1 = 1 mod L;
//   decode / encode: an accepted encoding is on the curve and encodes back to the same bytes (so y < p and
//   the sign rule hold), a refused one stays refused with the other sign bit unless x = 0 is the reason.
#include "ed25519.hpp"
#include <cstdio>
#include <cstring>
#include <random>
using namespace mpcx::host;
int main() {
  std::mt19937_64 g(25519);
  long bad = 0, n = 0, accepted = 0;
  const Nat& L = ed::OrderL();
  if (!ed::IsOnCurve(ed::BasePoint())) ++bad;
  for (int it = 0; it < 4000; ++it) {
    uint8_t buf[64];
    const bool ones = (g() % 16) == 0;
    for (auto& b : buf) b = ones ? 0xFF : (uint8_t)g();
    const size_t len = 1 + g() % 64;
    const Nat r = ed::ScReduce(buf, len), v = ed::FromLe(buf, len);
    if (!(r < L) || r != v % L) ++bad;
    const Nat a = ed::ScReduce(buf, 64), b = ed::ScReduce(buf + 7, 32);
    if (ed::ScMul(a, b) != (a * b) % L || ed::ScAdd(a, ed::ScNeg(a)) != Nat()) ++bad;
    Nat inv;
    if (ed::ScInv(a, &inv) ? ed::ScMul(a, inv) != Nat(1) : !a.is_zero()) ++bad;
    ed::Point P;
    if (ed::Decode(buf, &P)) {
      ++accepted;
      const ed::Bytes32 e = ed::Encode(P);
      if (!ed::IsOnCurve(P) || std::memcmp(e.data(), buf, 32) != 0) ++bad;
    } else if (!ones) {
      uint8_t other[32];
      std::memcpy(other, buf, 32);
      other[31] ^= 0x80;
      ed::Point Q;
      if (ed::Decode(other, &Q) && !Q.x.is_zero()) ++bad;
    }
    ++n;
  }
  Nat none;
  if (ed::ScInv(L, &none) || ed::ScInv(Nat(), &none)) ++bad;
  std::printf("checked %ld, decoded %ld, bad %ld\n", n, accepted, bad);
  return bad != 0 || accepted < n / 4;
}
