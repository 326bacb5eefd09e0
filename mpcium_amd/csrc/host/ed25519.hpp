// ed25519.hpp -- the host side of Ed25519 as mpcium's EdDSA sessions use it
// (tss-lib v2 up:eddsa/signing over decred's edwards/v2; mpcium checks every
// result with edwards.Verify, /root/reference/pkg/mpc/eddsa_signing_session.go):
// scalars mod the group order L, the on-curve check of crypto.NewECPoint, the
// RFC 8032 point encoding (ecPointToEncodedBytes) and its section 5.1.3
// decoding, and SHA-512 through libcrypto. Host only: nothing here touches a
// device (the point sums are eddsa.cpp's, on libmpcx's k_ed_msm), so every
// function runs and is tested without a GPU.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "bignum.hpp"

namespace mpcx::host::ed {

using Bytes32 = std::array<uint8_t, 32>;

const Nat& FieldP();  // p = 2^255 - 19
const Nat& OrderL();  // L = 2^252 + 27742317777372353535851937790883648493
const Nat& CurveD();  // d = -121665 / 121666 mod p

// An affine point of -x^2 + y^2 = 1 + d x^2 y^2; the identity is (0, 1).
struct Point {
  Nat x, y{1};
};
const Point& BasePoint();  // B of RFC 8032

// crypto.NewECPoint's check: x, y < p and on the curve
bool IsOnCurve(const Point& P);

// scalars mod L
Nat ScAdd(const Nat& a, const Nat& b);
Nat ScMul(const Nat& a, const Nat& b);
Nat ScNeg(const Nat& a);                // L - (a mod L), 0 for 0
bool ScInv(const Nat& a, Nat* out);     // false for a = 0 mod L
Nat ScReduce(const uint8_t* le, size_t n);  // a little-endian value of n bytes (64 for a SHA-512 digest) mod L
Nat FromLe(const uint8_t* le, size_t n);
Bytes32 ToLe32(const Nat& v);  // requires v < 2^256

// ecPointToEncodedBytes: y little-endian with the sign (low bit) of x in bit 255
Bytes32 Encode(const Point& P);
// RFC 8032 5.1.3: false for y >= p, for a y with no x on the curve, and for
// x = 0 with the sign bit set
bool Decode(const uint8_t enc[32], Point* out);

// SHA-512 of the concatenation of the parts
std::array<uint8_t, 64> Sha512(const std::vector<std::pair<const uint8_t*, size_t>>& parts);
// SHA-512(R || A || M) mod L
Nat Hram(const uint8_t R[32], const uint8_t A[32], const uint8_t* msg, size_t msg_len);

}  // namespace mpcx::host::ed
