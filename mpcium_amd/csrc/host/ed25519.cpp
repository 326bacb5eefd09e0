// ed25519.cpp -- see ed25519.hpp
#include "ed25519.hpp"

#include <openssl/sha.h>

#include <algorithm>
#include <stdexcept>

namespace mpcx::host::ed {

namespace {

Nat fmul(const Nat& a, const Nat& b) { return (a * b) % FieldP(); }
Nat fadd(const Nat& a, const Nat& b) { return (a + b) % FieldP(); }
Nat fsub(const Nat& a, const Nat& b) { return (a + FieldP() - (b % FieldP())) % FieldP(); }
Nat fpow(const Nat& a, const Nat& e) {
  Nat r(1);
  for (uint32_t i = e.bit_len(); i-- > 0;) {
    r = fmul(r, r);
    if (e.bit(i)) r = fmul(r, a);
  }
  return r;
}
// sqrt(-1) = 2^((p - 1) / 4)
const Nat& SqrtM1() {
  static const Nat v = fpow(Nat(2), (FieldP() - Nat(1)) >> 2);
  return v;
}

}  // namespace

const Nat& FieldP() {
  static const Nat p = (Nat(1) << 255) - Nat(19);
  return p;
}
const Nat& OrderL() {
  static const Nat l = (Nat(1) << 252) + Nat::from_hex("14def9dea2f79cd65812631a5cf5d3ed");
  return l;
}
const Nat& CurveD() {
  static const Nat d = [] {
    Nat inv;
    if (!mod_inverse(Int(Nat(121666)), FieldP(), &inv)) throw std::logic_error("ed25519: 121666 has no inverse");
    return fmul(FieldP() - Nat(121665), inv);
  }();
  return d;
}
const Point& BasePoint() {
  static const Point b = [] {
    Nat inv5;
    if (!mod_inverse(Int(Nat(5)), FieldP(), &inv5)) throw std::logic_error("ed25519: 5 has no inverse");
    const Bytes32 enc = ToLe32(fmul(Nat(4), inv5));  // y = 4/5, x even
    Point p;
    if (!Decode(enc.data(), &p)) throw std::logic_error("ed25519: the base point does not decode");
    return p;
  }();
  return b;
}

bool IsOnCurve(const Point& P) {
  const Nat& p = FieldP();
  if (!(P.x < p) || !(P.y < p)) return false;
  const Nat xx = fmul(P.x, P.x), yy = fmul(P.y, P.y);
  return fsub(yy, xx) == fadd(Nat(1), fmul(CurveD(), fmul(xx, yy)));
}

Nat ScAdd(const Nat& a, const Nat& b) { return (a + b) % OrderL(); }
Nat ScMul(const Nat& a, const Nat& b) { return (a * b) % OrderL(); }
Nat ScNeg(const Nat& a) {
  const Nat r = a % OrderL();
  return r.is_zero() ? r : OrderL() - r;
}
bool ScInv(const Nat& a, Nat* out) {
  const Nat r = a % OrderL();
  if (r.is_zero()) return false;
  return mod_inverse(Int(r), OrderL(), out);
}
Nat FromLe(const uint8_t* le, size_t n) {
  std::vector<uint8_t> be(le, le + n);
  std::reverse(be.begin(), be.end());
  return Nat::from_bytes_be(be.data(), be.size());
}
Nat ScReduce(const uint8_t* le, size_t n) { return FromLe(le, n) % OrderL(); }
Bytes32 ToLe32(const Nat& v) {
  if (v.bit_len() > 256) throw std::invalid_argument("ed25519: value wider than 256 bits");
  uint32_t w[8];
  v.to_words(w, 8);
  Bytes32 out;
  for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
  return out;
}

Bytes32 Encode(const Point& P) {
  Bytes32 out = ToLe32(P.y);
  if (P.x.is_odd()) out[31] |= 0x80;
  return out;
}

bool Decode(const uint8_t enc[32], Point* out) {
  uint8_t yb[32];
  std::copy(enc, enc + 32, yb);
  const bool sign = (yb[31] & 0x80) != 0;
  yb[31] &= 0x7F;
  const Nat y = FromLe(yb, 32);
  if (!(y < FieldP())) return false;
  // x^2 = u / v, u = y^2 - 1, v = d y^2 + 1; the candidate root u v^3 (u v^7)^((p - 5) / 8)
  const Nat yy = fmul(y, y), u = fsub(yy, Nat(1)), v = fadd(fmul(CurveD(), yy), Nat(1));
  const Nat v3 = fmul(fmul(v, v), v), v7 = fmul(fmul(v3, v3), v);
  Nat x = fmul(fmul(u, v3), fpow(fmul(u, v7), (FieldP() - Nat(5)) >> 3));
  const Nat vxx = fmul(v, fmul(x, x));
  if (vxx != u) {
    if (vxx != fsub(Nat(0), u)) return false;  // u / v is not a square
    x = fmul(x, SqrtM1());
  }
  if (x.is_zero() && sign) return false;
  if (x.is_odd() != sign) x = FieldP() - x;
  out->x = x;
  out->y = y;
  return true;
}

std::array<uint8_t, 64> Sha512(const std::vector<std::pair<const uint8_t*, size_t>>& parts) {
  size_t n = 0;
  for (const auto& p : parts) n += p.second;
  std::vector<uint8_t> buf;
  buf.reserve(n);
  for (const auto& p : parts) buf.insert(buf.end(), p.first, p.first + p.second);
  std::array<uint8_t, 64> out;
  if (!SHA512(buf.data(), buf.size(), out.data())) throw std::runtime_error("SHA512");
  return out;
}

Nat Hram(const uint8_t R[32], const uint8_t A[32], const uint8_t* msg, size_t msg_len) {
  const auto h = Sha512({{R, 32}, {A, 32}, {msg, msg_len}});
  return ScReduce(h.data(), 64);
}

}  // namespace mpcx::host::ed
