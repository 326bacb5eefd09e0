/*
 * mpcx_host.h -- C surface of libmpcx_host.so, the C++ mirror of the
 * reference's modexp-calling interfaces (tss-lib v2.0.2, pinned at
 * /root/reference/go.mod:10; Go/tss-lib are absent from this image, so the
 * host side that would be Go is C++ here). Every exponentiation goes through
 * libmpcx.so (include/mpcx.h). Integers: little-endian 32-bit words with a
 * separate sign byte array where Go accepts negative *big.Int values.
 * Return codes are the MPCX_* codes of mpcx.h; mpcxh_last_error() has text.
 *
 * Reference interface each entry point mirrors:
 *   mpcxh_modint_exp_batch       up:common/int.go (*modInt).Exp -> Go (*Int).Exp
 *   mpcxh_paillier_*_batch       up:crypto/paillier/paillier.go
 *                                (EncryptAndReturnRandomness, HomoMult,
 *                                 HomoAdd, Decrypt; per-op error codes
 *                                 1 = ErrMessageTooLong, 2 = ErrMessageMalFormed)
 *   mpcxh_safe_primes            up:common/safe_prime.go GetRandomSafePrimesConcurrent
 *   mpcxh_safe_prime_batch       up:common/safe_prime.go runGenPrimeRoutine (one stream batch, sharded)
 *   mpcxh_generate_preparams     up:ecdsa/keygen/prepare.go GeneratePreParams,
 *                                called at /root/reference/pkg/mpc/node.go:69
 *   mpcxh_dln_*, mpcxh_mod_*,    up:crypto/dlnproof, up:crypto/modproof,
 *   mpcxh_fac_*_batch            up:crypto/facproof (keygen / reshare proofs)
 *   mpcxh_mta_*_batch            up:crypto/mta/{share_protocol,range_proof,proofs}.go
 *                                (AliceInit, BobMid[WC], AliceEnd[WC], the
 *                                 range / Bob proofs and their Verify)
 *   mpcxh_vss_create_batch       up:crypto/vss/feldman_vss.go Create
 *   mpcxh_vss_verify_batch       up:crypto/vss/feldman_vss.go (*Share).Verify
 *   mpcxh_vss_public_shares_batch  up:ecdsa/keygen/round_3.go, up:ecdsa/resharing/round_4_new_step_2.go
 *                                (Vc = sum of the parties' Vs, BigXj = sum_k id_j^k Vc_k)
 *   mpcxh_vss_reconstruct_batch  up:crypto/vss/feldman_vss.go (Shares).ReConstruct
 *   mpcxh_ed25519_decode_batch   RFC 8032 5.1.3 (decred edwards/v2 point decoding)
 *   mpcxh_ed25519_hram_batch     SHA-512(R || A || M) mod L (up:eddsa/signing/round_3.go)
 *   mpcxh_eddsa_verify_batch     decred edwards/v2 Verify, called at
 *                                /root/reference/pkg/mpc/eddsa_signing_session.go
 *   mpcxh_eddsa_sign_batch       up:eddsa/signing round_1.go .. finalize.go
 *   mpcxh_ed25519_admit_batch    up:crypto/ecpoint.go NewECPoint, EightInvEight
 *   mpcxh_edvss_*_batch          up:crypto/vss/feldman_vss.go over Edwards
 *   mpcxh_eddsa_keygen_batch     up:eddsa/keygen round_1.go .. round_3.go, called through
 *                                /root/reference/pkg/mpc/eddsa_keygen_session.go
 *   mpcxh_eddsa_reshare_batch    up:eddsa/resharing, called through
 *                                /root/reference/pkg/mpc/eddsa_resharing_session.go
 *   mpcxh_paillier_prove_batch,  up:crypto/paillier/paillier.go (*PrivateKey).Proof,
 *   mpcxh_paillier_proof_verify_batch  (*Proof).Verify (keygen rounds 3 and 4)
 *   mpcxh_ecdsa_keygen_batch     up:ecdsa/keygen round_1.go .. round_4.go, called through
 *                                /root/reference/pkg/mpc/ecdsa_keygen_session.go
 *   mpcxh_ecdsa_sign_batch       up:ecdsa/signing prepare.go .. finalize.go on stored keys,
 *                                /root/reference/pkg/mpc/ecdsa_signing_session.go
 */
#ifndef MPCX_HOST_H_
#define MPCX_HOST_H_

#include <stddef.h>
#include <stdint.h>

#include "mpcx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* io.Reader stand-in: fill buf[0..n) with random bytes (io.ReadFull). */
typedef void (*mpcxh_rand_fn)(void* ctx, uint8_t* buf, size_t n);

/* One session's randomness source: tss-lib draws every MtA / proof random
 * value from the party's io.Reader inside party.UpdateFromBytes
 * (/root/reference/pkg/mpc/session.go:199). fn != NULL: fn(ctx, ...) is that
 * reader (a cgo export wrapping the Go io.Reader); it is
 * called from libmpcx_host's worker threads, never concurrently for one
 * session, but concurrently across sessions (a reader shared by several
 * sessions must be thread-safe, as crypto/rand.Reader is). fn == NULL: the
 * build's CounterDRBG stream seeded with `seed` (tests, benchmarks). */
typedef struct {
  mpcxh_rand_fn fn;
  void* ctx;
  uint64_t seed;
} mpcxh_reader_t;

#define MPCXH_PREPARAM_FIELDS 12

const char* mpcxh_last_error(void);
/* Bind one more GPU (mpcx_init) / GPUs 0..n_gpus-1 (mpcx_init_devices, n_gpus
 * <= 0: all visible). Every batch below spreads over the bound GPUs. */
int mpcxh_init(int device);
int mpcxh_init_devices(int n_gpus);

/* z_i = x_i^y_i mod m with Go semantics; ok[i] = 0 where Go returns nil
 * (y < 0 and x not invertible). y_shared != 0: one y for every x. m odd,
 * 1 <= m < 2^4096. */
int mpcxh_modint_exp_batch(const uint32_t* m, uint32_t mw, uint32_t count,
                           const uint32_t* xs, uint32_t xw, const uint8_t* x_neg,
                           const uint32_t* ys, uint32_t yw, const uint8_t* y_neg, int y_shared,
                           uint32_t* out, uint32_t ow, uint8_t* ok);

int mpcxh_paillier_encrypt_batch(const uint32_t* N, uint32_t nw, uint32_t count,
                                 const uint32_t* m, uint32_t mw, const uint8_t* m_neg,
                                 const uint32_t* r, uint32_t rw,
                                 uint32_t* c, uint32_t cw, uint8_t* err);
int mpcxh_paillier_homomult_batch(const uint32_t* N, uint32_t nw, uint32_t count,
                                  const uint32_t* m, uint32_t mw, const uint8_t* m_neg,
                                  const uint32_t* c1, uint32_t c1w, const uint8_t* c1_neg,
                                  uint32_t* out, uint32_t ow, uint8_t* err);
int mpcxh_paillier_homoadd_batch(const uint32_t* N, uint32_t nw, uint32_t count,
                                 const uint32_t* c1, uint32_t c1w, const uint8_t* c1_neg,
                                 const uint32_t* c2, uint32_t c2w, const uint8_t* c2_neg,
                                 uint32_t* out, uint32_t ow, uint8_t* err);
int mpcxh_paillier_decrypt_batch(const uint32_t* N, uint32_t nw, const uint32_t* lambda, uint32_t lw,
                                 const uint32_t* P, uint32_t pw, const uint32_t* Q, uint32_t qw,
                                 uint32_t count, const uint32_t* c, uint32_t cw, const uint8_t* c_neg,
                                 uint32_t* m, uint32_t mw, uint8_t* err);

/* First `num` safe primes p = 2q+1 of bit_len bits in candidate-stream order.
 * Random source: rand_fn(rand_ctx, ...) if non-NULL (read on the host), else
 * the CounterDRBG seeded with `seed` (drawn on the GPU). p_out/q_out: num x
 * words. index_out: stream positions. stats_out[6]: candidates, sieved out,
 * GPU Fermat tests, GPU Miller-Rabin rounds, usec, GPU strong Lucas tests. */
int mpcxh_safe_primes(int bit_len, int num, uint64_t seed, mpcxh_rand_fn rand_fn, void* rand_ctx,
                      uint32_t* p_out, uint32_t* q_out, uint32_t words, uint64_t* index_out,
                      uint64_t* stats_out);

/* One batch of the same search for sharding across GPUs (up:common/safe_prime.go
 * runGenPrimeRoutine, one batch of its candidate stream): candidates
 * [batch_no*batch, (batch_no+1)*batch) of the CounterDRBG(seed) stream
 * (batch 0 = default 196608). Writes up to max_out accepted primes in stream
 * order and their count to *n_found. Rank g of G takes batch_no = g (mod G);
 * the first `num` indices over all ranks equal mpcxh_safe_primes' output. */
int mpcxh_safe_prime_batch(int bit_len, uint64_t seed, uint64_t batch_no, uint32_t batch, uint32_t max_out,
                           uint32_t* p_out, uint32_t* q_out, uint32_t words, uint64_t* index_out,
                           uint32_t* n_found, uint64_t* stats_out);

/* LocalPreParams as 12 fields x 64 words: N, LambdaN, PhiN, P, Q (Paillier),
 * NTildei, H1i, H2i, Alpha, Beta, P, Q (Germain primes of N~). One stream:
 * the Paillier search, then N~'s, then f and alpha; each search consumes the
 * stream up to its last accepted candidate, as tss-lib at concurrency 1.
 * stats_out[6] as mpcxh_safe_primes. */
int mpcxh_generate_preparams(uint64_t seed, mpcxh_rand_fn rand_fn, void* rand_ctx,
                             uint32_t* out, uint64_t* stats_out);

/* ---------------------------------------------------------------- MtA
 * Batched mirror of tss-lib v2.0.2's MtA / MtAwc (up:crypto/mta/share_protocol.go,
 * range_proof.go, proofs.go), the Paillier work of GG18 signing that mpcium's
 * signing sessions (/root/reference/pkg/mpc/ecdsa_signing_session.go:134-147)
 * run through party.UpdateFromBytes (/root/reference/pkg/mpc/session.go:199).
 * One call = a batch of independent sessions sharing key material. Every
 * integer is `w` little-endian 32-bit words (w >= 128: N^2 fits); proofs are
 * count x fields x w words:
 *   RangeProofAlice (6 fields): Z, U, W, S, S1, S2
 *   ProofBob[WC]   (12 fields): Z, ZPrm, T, V, W, S, S1, S2, T1, T2, U.x, U.y
 *                               (U = 0, 0 for the plain ProofBob)
 * Points (B, the MtAwc public value) are count x 16 words: x (8), y (8).
 * Session ids are count x session_len bytes. readers[i]: session i's
 * io.Reader. err[i]: 0 ok, 1 ErrMessageTooLong, 2
 * ErrMessageMalFormed, 3 proof verification failed. */
typedef struct {
  const uint32_t* N;       /* Paillier N */
  const uint32_t* LambdaN; /* private-key fields: NULL for a peer's public key */
  const uint32_t* P;
  const uint32_t* Q;
} mpcxh_paillier_t;

typedef struct {
  const uint32_t* NTilde;
  const uint32_t* h1;
  const uint32_t* h2;
  const uint32_t* P; /* safe-prime factors of NTilde when the caller owns it, else NULL */
  const uint32_t* Q;
} mpcxh_dln_t;

#define MPCXH_RANGE_PROOF_FIELDS 6
#define MPCXH_PROOF_BOB_FIELDS 12

/* mta.AliceInit(ec, pkA, a, NTildeB, h1B, h2B, rand) -> cA, RangeProofAlice */
int mpcxh_mta_alice_init_batch(uint32_t w, const mpcxh_paillier_t* pkA, const mpcxh_dln_t* dlnB, uint32_t count,
                               const uint32_t* a, const mpcxh_reader_t* readers, uint32_t* cA, uint32_t* pf,
                               uint8_t* err);
/* (*RangeProofAlice).Verify(ec, pk, NTilde, h1, h2, c) */
int mpcxh_mta_verify_range_alice_batch(uint32_t w, const mpcxh_paillier_t* pk, const mpcxh_dln_t* dln,
                                       uint32_t count, const uint32_t* c, const uint32_t* pf, uint8_t* ok);
/* mta.BobMid (B == NULL) / BobMidWC(Session, ec, pkA, pf, b, cA, NTildeA, h1A, h2A,
 * NTildeB, h1B, h2B[, B], rand) -> beta, cB, betaPrm, ProofBob[WC] */
int mpcxh_mta_bob_mid_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const mpcxh_paillier_t* pkA,
                            const mpcxh_dln_t* dlnA, const mpcxh_dln_t* dlnB, uint32_t count, const uint32_t* pfA,
                            const uint32_t* b, const uint32_t* cA, const uint32_t* B,
                            const mpcxh_reader_t* readers, uint32_t* beta, uint32_t* cB, uint32_t* betaPrm,
                            uint32_t* pfB, uint8_t* err);
/* (*ProofBob).Verify / (*ProofBobWC).Verify(Session, ec, pk, NTilde, h1, h2, c1, c2[, X]) */
int mpcxh_mta_verify_bob_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const mpcxh_paillier_t* pk,
                               const mpcxh_dln_t* dln, uint32_t count, const uint32_t* c1, const uint32_t* c2,
                               const uint32_t* pfB, const uint32_t* X, uint8_t* ok);
/* mta.AliceEnd (B == NULL) / AliceEndWC(Session, ec, pkA, pf, h1A, h2A, cA, cB, NTildeA[, B], sk) -> alpha */
int mpcxh_mta_alice_end_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const mpcxh_paillier_t* skA,
                              const mpcxh_dln_t* dlnA, uint32_t count, const uint32_t* pfB, const uint32_t* cA,
                              const uint32_t* cB, const uint32_t* B, uint32_t* alpha, uint8_t* err);

/* Signing round 2 runs BobMid and BobMidWC on every peer's round-1 message
 * (up:ecdsa/signing/round_2.go): both halves of each session in one call,
 * RangeProofAlice.Verify once for both. b / readers / beta / cB / betaPrm /
 * pfB / err: the BobMid half; bwc, Bwc, readers_wc, *_wc: the BobMidWC half.
 * With distinct readers the two halves run concurrently (readers[i] and
 * readers_wc[i] may then be called at the same time); when readers[i] and
 * readers_wc[i] are the same callback (same fn and ctx) for any session, the
 * halves run one after the other, BobMid first. Every output equals the two
 * separate calls' (BobMid, then BobMidWC). */
int mpcxh_mta_bob_mid_pair_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len,
                                 const mpcxh_paillier_t* pkA, const mpcxh_dln_t* dlnA, const mpcxh_dln_t* dlnB,
                                 uint32_t count, const uint32_t* pfA, const uint32_t* cA, const uint32_t* b,
                                 const mpcxh_reader_t* readers, const uint32_t* bwc, const uint32_t* Bwc,
                                 const mpcxh_reader_t* readers_wc, uint32_t* beta, uint32_t* cB, uint32_t* betaPrm,
                                 uint32_t* pfB, uint8_t* err, uint32_t* beta_wc, uint32_t* cB_wc,
                                 uint32_t* betaPrm_wc, uint32_t* pfB_wc, uint8_t* err_wc);
/* Signing round 3's AliceEnd and AliceEndWC per peer (up:ecdsa/signing/round_3.go)
 * in one call: each half's ProofBob[WC] verification and Decrypt batch, the two
 * halves as concurrent tasks (no reader is involved). */
int mpcxh_mta_alice_end_pair_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len,
                                   const mpcxh_paillier_t* skA, const mpcxh_dln_t* dlnA, uint32_t count,
                                   const uint32_t* cA, const uint32_t* pfB, const uint32_t* cB,
                                   const uint32_t* pfB_wc, const uint32_t* cB_wc, const uint32_t* Bwc,
                                   uint32_t* alpha, uint8_t* err, uint32_t* mu, uint8_t* err_wc);

/* ---------------------------------------------------------------- keygen proofs
 * Batched mirror of tss-lib v2.0.2's DLN (up:crypto/dlnproof, 128 iterations),
 * Paillier-Blum modulus (up:crypto/modproof, 80 iterations) and no-small-factor
 * (up:crypto/facproof) proofs: keygen round 1-3 and reshare
 * (/root/reference/pkg/mpc/ecdsa_keygen_session.go:85-92,
 * /root/reference/pkg/mpc/ecdsa_resharing_session.go:132-143). A batch holds
 * `count` proofs over the same public parameters; integers are `w` words
 * (w >= 160: FacProof's v and sigma reach ~4.9 kbit), readers[i] is proof i's
 * io.Reader, sessions are count x session_len bytes.
 *   DLN proof: alpha (count x 128 x w), t (count x 128 x w)
 *   Mod proof: W (count x w), X (count x 80 x w), A, B (count x w), Z (count x 80 x w)
 *   Fac proof: count x 11 x w fields P, Q, A, B, T, Sigma, Z1, Z2, W1, W2, |V|
 *              and v_neg[count] (sign of V) */
#define MPCXH_PROOF_WORDS 160
#define MPCXH_DLN_ITERATIONS 128
#define MPCXH_MOD_ITERATIONS 80
#define MPCXH_FAC_FIELDS 11
int mpcxh_dln_prove_batch(uint32_t w, const uint32_t* h1, const uint32_t* h2, const uint32_t* x, const uint32_t* p,
                          const uint32_t* q, const uint32_t* N, uint32_t count, const mpcxh_reader_t* readers,
                          uint32_t* alpha, uint32_t* t);
int mpcxh_dln_verify_batch(uint32_t w, const uint32_t* h1, const uint32_t* h2, const uint32_t* N, uint32_t count,
                           const uint32_t* alpha, const uint32_t* t, uint8_t* ok);
int mpcxh_mod_prove_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const uint32_t* N,
                          const uint32_t* P, const uint32_t* Q, uint32_t count, const mpcxh_reader_t* readers,
                          uint32_t* W, uint32_t* X, uint32_t* A, uint32_t* B, uint32_t* Z);
int mpcxh_mod_verify_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const uint32_t* N,
                           uint32_t count, const uint32_t* W, const uint32_t* X, const uint32_t* A, const uint32_t* B,
                           const uint32_t* Z, uint8_t* ok);
int mpcxh_fac_prove_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const uint32_t* N0,
                          const uint32_t* NCap, const uint32_t* s, const uint32_t* t, const uint32_t* N0p,
                          const uint32_t* N0q, uint32_t count, const mpcxh_reader_t* readers, uint32_t* pf,
                          uint8_t* v_neg);
int mpcxh_fac_verify_batch(uint32_t w, const uint8_t* sessions, uint32_t session_len, const uint32_t* N0,
                           const uint32_t* NCap, const uint32_t* s, const uint32_t* t, uint32_t count,
                           const uint32_t* pf, const uint8_t* v_neg, uint8_t* ok);
/* The Paillier key proof of keygen rounds 3 and 4 (up:crypto/paillier/paillier.go
 * (*PrivateKey).Proof / (*Proof).Verify, 13 iterations; restated as recalled:
 * upstream, verify -- csrc/host/proofs.hpp has GenerateXs): `count` proofs under
 * one key N = P Q, proof i bound to k[i] (w words: the prover's party id) and
 * the ECDSA public key pub[i] (16 words x|y). y receives / holds count x 13 x w
 * words. The 13 x count exponentiations are one GPU launch step (the prover's
 * by CRT over P and Q). ok[i] = 0 when a prime below 1000 divides N or some
 * y_k^N mod N differs from GenerateXs' x_k. retries (or NULL) receives each
 * proof's final GenerateXs retry counter. */
#define MPCXH_PAILLIER_PROOF_ITERATIONS 13
int mpcxh_paillier_prove_batch(uint32_t w, const uint32_t* N, const uint32_t* P, const uint32_t* Q, uint32_t count,
                               const uint32_t* k /* count x w */, const uint32_t* pub /* count x 16 */,
                               uint32_t* y /* count x 13 x w */, uint32_t* retries /* count */);
int mpcxh_paillier_proof_verify_batch(uint32_t w, const uint32_t* N, uint32_t count, const uint32_t* k,
                                      const uint32_t* pub, const uint32_t* y, uint8_t* ok);

/* ---------------------------------------------------------------- Feldman VSS
 * Batched mirror of tss-lib v2.0.2's up:crypto/vss/feldman_vss.go at any
 * threshold t with t + 1 <= 16 (csrc/host/vss.hpp; restated as recalled:
 * upstream, verify), for keygen rounds 2-3 and resharing rounds 4-5
 * (/root/reference/pkg/mpc/ecdsa_keygen_session.go:84,
 * /root/reference/pkg/mpc/ecdsa_resharing_session.go). The point sums run on the
 * GPU (mpcx_ec_msm_batch), so every call but the reconstruction needs a bound
 * device. Ids are id_words (1..16) little-endian words each -- mpcium's party
 * keys are SetBytes(nodeID + ":" + label), ~360 bits
 * (/root/reference/pkg/mpc/node.go:43) -- and are used mod q, the group order.
 * Scalars are 8 words, points 16 words (x, y; all-zero = infinity). A call
 * takes 1..16 ids; an id that is 0 mod q or two ids equal mod q (CheckIndexes)
 * and every limit above are MPCX_EINVAL.
 *
 * vss.Create for `count` secrets over the same n_ids ids (threshold < n_ids):
 * a_0 = secret, a_1..a_t = GetRandomPositiveInt(readers[i], q) in that order;
 * vs[i][k] = a_k G, shares[i][j] = sum_k a_k id_j^k mod q. */
int mpcxh_vss_create_batch(uint32_t threshold, uint32_t n_ids, const uint32_t* ids, uint32_t id_words,
                           uint32_t count, const uint32_t* secrets /* count x 8 */, const mpcxh_reader_t* readers,
                           uint32_t* vs /* count x (t+1) x 16 */, uint32_t* shares /* count x n_ids x 8 */);
/* (*Share).Verify for `count` (Vs, id, share) items: ok[i] = share_i G ==
 * sum_k id_i^k V_ik. ok[i] = 0 without failing the call when n_vs != t + 1, a
 * V_ik is infinity or not on the curve (crypto.NewECPoint refuses it), or id_i
 * is 0 mod q. */
int mpcxh_vss_verify_batch(uint32_t threshold, uint32_t count, uint32_t n_vs, const uint32_t* vs /* count x n_vs x 16 */,
                           const uint32_t* ids /* count x id_words */, uint32_t id_words,
                           const uint32_t* shares /* count x 8 */, uint8_t* ok);
/* Keygen round 3 / resharing round 4-5's public shares for `count` sessions of
 * the same n_parties ids: vc[s][k] = sum_i vs[s][i][k] (vc[s][0] is the
 * wallet's public key), xs[s][j] = sum_k id_j^k vc[s][k] (BigXj). */
int mpcxh_vss_public_shares_batch(uint32_t threshold, uint32_t n_parties, const uint32_t* ids, uint32_t id_words,
                                  uint32_t count, const uint32_t* vs /* count x n_parties x (t+1) x 16 */,
                                  uint32_t* vc /* count x (t+1) x 16 */, uint32_t* xs /* count x n_parties x 16 */);
/* (Shares).ReConstruct for `count` items of n_shares (id, share) pairs each
 * (ids: count x n_shares x id_words, shares: count x n_shares x 8): Lagrange
 * interpolation at 0, on the host (no device needed). ok[i] = 0 and secret 0 on
 * an id that is 0 mod q or two ids equal mod q. */
int mpcxh_vss_reconstruct_batch(uint32_t count, uint32_t n_shares, const uint32_t* ids, uint32_t id_words,
                                const uint32_t* shares, uint32_t* secrets /* count x 8 */, uint8_t* ok);

/* ---------------------------------------------------------------- EdDSA (Ed25519)
 * The other protocol mpcium runs for every wallet: threshold EdDSA over Ed25519
 * (tss-lib v2 up:eddsa/signing, /root/reference/pkg/mpc/eddsa_signing_session.go),
 * every result checked with decred's edwards.Verify (csrc/host/ed25519.hpp,
 * csrc/host/eddsa.hpp). Points are 16 words (affine x, y; the identity is
 * (0, 1)), scalars 8 words, encodings 32 bytes (y little-endian, the sign of x
 * in bit 255). Messages of a batch are variable-length byte strings given as
 * count + 1 offsets into one buffer: item i is msgs[msg_off[i] .. msg_off[i+1]).
 * A message is taken as given: mpcium signs tx.Bytes(), a big.Int's bytes,
 * which drop leading zero bytes (mpcium_amd.eddsa.tx_message does the same).
 *
 * The first two entries are host-only (no device needed).
 * RFC 8032 5.1.3 decoding of `count` encodings: ok[i] = 0 and xy[i] zero for
 * y >= p, for a y with no x on the curve, and for x = 0 with the sign bit set. */
int mpcxh_ed25519_decode_batch(uint32_t count, const uint8_t* enc /* count x 32 */, uint32_t* xy /* count x 16 */,
                               uint8_t* ok);
/* h[i] = SHA-512(R_i || A_i || M_i) mod L (the challenge of RFC 8032 and of
 * up:eddsa/signing round 3). */
int mpcxh_ed25519_hram_batch(uint32_t count, const uint8_t* R /* count x 32 */, const uint8_t* A /* count x 32 */,
                             const uint8_t* msgs, const uint64_t* msg_off /* count + 1 */, uint32_t* h /* count x 8 */);
/* What edwards.Verify decides for `count` (public key, message, signature)
 * items: ok[i] = 1 iff the key is on the curve, s < L (RFC 8032 and OpenSSL;
 * decred's behaviour for s >= L: upstream, verify) and enc(s B - h A) equals
 * the signature's first 32 bytes byte for byte. One GPU batch
 * (mpcx_ed_msm_batch: a = s, the point A with scalar L - h). */
int mpcxh_eddsa_verify_batch(uint32_t count, const uint32_t* pk /* count x 16 */, const uint8_t* msgs,
                             const uint64_t* msg_off /* count + 1 */, const uint8_t* sigs /* count x 64 */,
                             uint8_t* ok);
/* up:eddsa/signing rounds 1-3 and finalize for `count` wallets of n_signers
 * (2..16) signers each, every signer replayed in process (csrc/host/eddsa.hpp
 * gives the steps; draw order and hash inputs: upstream, verify). Per wallet:
 * the signers' ids (id_words 1..16 words each, used mod L; zero or equal ids
 * are MPCX_EINVAL), their Shamir shares, the public key, the message, the
 * session bytes of the Schnorr proofs (session_len each; signer i uses
 * session || big.Int(i).Bytes()) and one reader per signer. Every point
 * equation of a step is one mpcx_ed_msm_batch over all wallets and signers.
 * status[w] = 0 with sigs[w] = enc(R) || LE32(s), or the round that aborted the
 * wallet (3: a decommitment or Schnorr proof failed; 4: the final
 * verification) with sigs[w] zero; the other wallets are unaffected.
 * trace_flags (or NULL) marks wallets to trace; trace receives, per flagged
 * wallet in order, n_signers x 64 words -- r_i (8), R_i (16), the commitment
 * (8), the proof's alpha (16) and t (8), s_i (8) -- then the 8-word
 * SHA512_256i of the round transcript (eddsa.hpp). Test hooks: tamper_kind 1
 * shifts signer 0's Schnorr response in wallet tamper_wallet, 2 swaps the
 * coordinates of its decommitment; -1 / 0 for none. gpu_s (or NULL) receives
 * the wall time spent inside the GPU batches. */
int mpcxh_eddsa_sign_batch(uint32_t count, uint32_t n_signers, const uint32_t* ids /* count x n_signers x id_words */,
                           uint32_t id_words, const uint32_t* shares /* count x n_signers x 8 */,
                           const uint32_t* pk /* count x 16 */, const uint8_t* msgs,
                           const uint64_t* msg_off /* count + 1 */, const uint8_t* sessions /* count x session_len */,
                           uint32_t session_len, const mpcxh_reader_t* readers /* count x n_signers */,
                           const uint8_t* trace_flags, int64_t tamper_wallet, int tamper_kind,
                           uint8_t* sigs /* count x 64 */, uint8_t* status /* count */, uint32_t* trace,
                           double* gpu_s);

/* ---------------------------------------------------------------- EdDSA keygen and resharing
 * The other two EdDSA sessions mpcium runs for every wallet
 * (/root/reference/pkg/mpc/eddsa_keygen_session.go, eddsa_resharing_session.go
 * over tss-lib v2 up:eddsa/keygen and up:eddsa/resharing): Feldman VSS over
 * Ed25519 (csrc/host/edvss.hpp, the mirror of the secp256k1 entries above with
 * scalars mod L and mpcx_ed_msm_batch for the sums; the identity is (0, 1),
 * there is no all-zero point), the admission of received points, and the two
 * protocols with every party replayed in process (csrc/host/eddsa_keygen.hpp
 * gives the steps; restated as recalled: upstream, verify). Every entry but the
 * reconstruction needs a bound device.
 *
 * What a receiver does to a commitment point before using it: crypto.NewECPoint's
 * check, then (clear == 1) EightInvEight. mpcx_ed_admit_batch (k_ed_admit) with
 * its statuses; a rejected item's output is all zero. clear > 1 is MPCX_EINVAL. */
int mpcxh_ed25519_admit_batch(uint32_t count, uint32_t clear, const uint32_t* points /* count x 16 */,
                              uint32_t* out /* count x 16 */, uint8_t* status /* count */);
/* vss.Create over Ed25519: a_0 = secret mod L, a_1..a_t =
 * GetRandomPositiveInt(readers[i], L); vs[i][k] = a_k B, shares[i][j] =
 * sum_k a_k id_j^k mod L. Limits and errors as mpcxh_vss_create_batch, mod L. */
int mpcxh_edvss_create_batch(uint32_t threshold, uint32_t n_ids, const uint32_t* ids, uint32_t id_words,
                             uint32_t count, const uint32_t* secrets /* count x 8 */, const mpcxh_reader_t* readers,
                             uint32_t* vs /* count x (t+1) x 16 */, uint32_t* shares /* count x n_ids x 8 */);
/* (*Share).Verify: ok[i] = (L - share_i) B + sum_k id_i^k V_ik is the identity.
 * ok[i] = 0 without failing the call when n_vs != t + 1, a V_ik has a coordinate
 * >= p or is not on the curve, or id_i is 0 mod L. */
int mpcxh_edvss_verify_batch(uint32_t threshold, uint32_t count, uint32_t n_vs,
                             const uint32_t* vs /* count x n_vs x 16 */, const uint32_t* ids /* count x id_words */,
                             uint32_t id_words, const uint32_t* shares /* count x 8 */, uint8_t* ok);
/* vc[s][k] = sum_i vs[s][i][k] (vc[s][0] is the public key), xs[s][j] =
 * sum_k id_j^k vc[s][k]. A point that is not on the curve is MPCX_EINVAL. */
int mpcxh_edvss_public_shares_batch(uint32_t threshold, uint32_t n_parties, const uint32_t* ids, uint32_t id_words,
                                    uint32_t count, const uint32_t* vs /* count x n_parties x (t+1) x 16 */,
                                    uint32_t* vc /* count x (t+1) x 16 */, uint32_t* xs /* count x n_parties x 16 */);
/* (Shares).ReConstruct mod L, on the host (no device needed); as
 * mpcxh_vss_reconstruct_batch. */
int mpcxh_edvss_reconstruct_batch(uint32_t count, uint32_t n_shares, const uint32_t* ids, uint32_t id_words,
                                  const uint32_t* shares, uint32_t* secrets /* count x 8 */, uint8_t* ok);

/* words per party of a traced keygen session: u_i (8), the commitment C_i (8),
 * the proof's t (8) and alpha (16), V_i0..V_it as committed (16 each), the
 * shares s_i0..s_i,n-1 as sent (8 each) */
#define MPCXH_EDDSA_KEYGEN_TRACE_WORDS(t, n) (40u + 16u * ((t) + 1u) + 8u * (n))
/* up:eddsa/keygen rounds 1-3 for `count` sessions of n_parties (2..16) parties
 * at threshold t (1 <= t < n_parties) over the same ids (id_words 1..16 words
 * each, used mod L; zero or equal ids are MPCX_EINVAL): session bytes
 * (session_len each; party i proves under session || big.Int(i).Bytes()) and
 * one reader per party. status[s] = 0 with pk[s], x[s][j] (party j's share)
 * and X[s][j] = x_j B, or 3 (round 3) with culprit[s] the dealer whose
 * decommitment, points, Schnorr proof or shares failed and the outputs zero;
 * culprit is 255 otherwise. The other sessions are unaffected. trace_flags (or
 * NULL) marks sessions to trace; trace receives, per flagged session in order,
 * n_parties x MPCXH_EDDSA_KEYGEN_TRACE_WORDS(t, n_parties) words. Test hooks on
 * dealer 0 of session tamper_session (-1 / 0 for none): 1 shifts its Schnorr
 * response, 2 swaps two coordinates of its decommitment, 3 shifts the share
 * s_01, 4 adds the point (sqrt(-1), 0) of order four to V_01 before committing
 * (admission clears it: the session succeeds with the untampered result), 5
 * commits to an off-curve V_01. gpu_s (or NULL) receives the wall time inside the GPU
 * batches. */
int mpcxh_eddsa_keygen_batch(uint32_t count, uint32_t threshold, uint32_t n_parties,
                             const uint32_t* ids /* n_parties x id_words */, uint32_t id_words,
                             const uint8_t* sessions /* count x session_len */, uint32_t session_len,
                             const mpcxh_reader_t* readers /* count x n_parties */, const uint8_t* trace_flags,
                             int64_t tamper_session, int tamper_kind, uint8_t* status /* count */,
                             uint8_t* culprit /* count */, uint32_t* pk /* count x 16 */,
                             uint32_t* x /* count x n_parties x 8 */, uint32_t* X /* count x n_parties x 16 */,
                             uint32_t* trace, double* gpu_s);
/* up:eddsa/resharing for `count` wallets: the n_old old parties of old_ids (at
 * least the old threshold + 1 of them), their shares and the wallet's public
 * key, one reader per old party, to the n_new parties of new_ids at
 * new_threshold (1 <= new_threshold < n_new <= 16). status[s] = 0 with
 * pk_out[s] == pk[s], the new shares x[s][j] and X[s][j], or 4 with the
 * outputs zero: culprit[s] is the old party whose decommitment, points or
 * shares failed, or 255 when the dealt constant terms do not sum to pk[s]. */
int mpcxh_eddsa_reshare_batch(uint32_t count, uint32_t n_old, const uint32_t* old_ids /* n_old x old_id_words */,
                              uint32_t old_id_words, const uint32_t* shares /* count x n_old x 8 */,
                              const uint32_t* pk /* count x 16 */, const mpcxh_reader_t* readers /* count x n_old */,
                              uint32_t new_threshold, uint32_t n_new, const uint32_t* new_ids /* n_new x new_id_words */,
                              uint32_t new_id_words, uint8_t* status /* count */, uint8_t* culprit /* count */,
                              uint32_t* pk_out /* count x 16 */, uint32_t* x /* count x n_new x 8 */,
                              uint32_t* X /* count x n_new x 16 */, double* gpu_s);

/* Config-4 driver: one GG18 signature for each of `wallets` wallets, signed by
 * the first `signers` of `n_nodes` nodes (keys: Paillier private keys + own
 * DLN params with factors, width w). Plays every signer through all of tss-lib
 * v2's signing rounds (csrc/host/signing.hpp): rounds 1-3 MtA / MtAwc of
 * up:ecdsa/signing on the GPU, checking alpha + beta = k gamma and mu + nu = k w
 * (mod q) for every session; the round-1 commitments, round-4 Schnorr proofs,
 * round 5-9 commitments, Schnorr / ZKV proofs and their checks; then s
 * (low-s) and ecdsa.Verify of every signature by every signer, twice (tss-lib's
 * finalize and mpcium's session: /root/reference/pkg/mpc/ecdsa_signing_session.go:162).
 * stats_out[MPCXH_SIGNING_STATS]: round1_s, round2_s, round3_s, total_s,
 * wallets, sessions, errors, relation_failures, engine_busy_s (time inside
 * libmpcx calls), finalize_s (rounds 4-9 + finalize), signatures, verified,
 * alg_macs (Go-equivalent algorithmic work of the exponentiations sent to the
 * GPU), aborted (wallets whose transcript failed a check).
 * trace_wallets > 0: trace_out receives, for the wallets floor(t * wallets /
 * trace_wallets), t = 0 .. trace_wallets-1 (spread over every wallet pipeline),
 * per ordered pair (i-major) and wallet 40 words (alpha, beta, mu, nu as 8
 * words each, SHA512_256i over the session's cA, RangeProofAlice, cB,
 * ProofBob, cB', ProofBobWC fields), then per wallet 25 words (r, s, recid,
 * SHA512_256i of the GG18 round 1/4-9 transcript). tamper_wallet >= 0 (test
 * hook): corrupt signer 0's round-4 Schnorr proof (tamper_kind 1), round-6
 * ZKV proof (2) or round-7 decommitment (3) in that wallet, which must abort. */
#define MPCXH_SIGNING_STATS 14
int mpcxh_bench_signing(uint32_t w, const mpcxh_paillier_t* sks, const mpcxh_dln_t* dlns, uint32_t n_nodes,
                        uint32_t signers, uint32_t wallets, uint64_t seed, double* stats_out, uint32_t trace_wallets,
                        uint32_t* trace_out, int64_t tamper_wallet, int tamper_kind);

/* Config-5 driver: the proof work of `sessions` keygen / reshare sessions of
 * n_parties nodes (csrc/host/keygenload.hpp): every party proves DLN x2,
 * Paillier-Blum Mod, and a Fac proof to each peer; every party verifies
 * every peer's proofs. Integers are w words wide (w >= 64). Sessions stream in
 * waves of wave_sessions (0: 1024), two waves in flight, every proof chain of a
 * wave (each party's proofs and their verification by every peer) at once:
 * host memory is bounded by the waves, not by `sessions`.
 * stats_out[MPCXH_KEYGEN_STATS]: prove_s, verify_s, total_s, sessions, parties,
 * proofs, verifications, failures, engine_busy_s, alg_macs, waves,
 * wave_sessions, max_wave_s.
 * trace_out (NULL: none): per wave, one traced session of
 * 1 + n(n+2)*8 + 1 words: its index, per party the 8-word SHA512_256i digests of
 * its DLN (h1, h2, alpha), DLN (h2, h1, beta), Mod proof and its Fac proof to
 * each peer (ascending), then the count of its verifications that passed
 * (keygenload.hpp TraceSessionWords). */
#define MPCXH_KEYGEN_STATS 13
typedef struct {
  mpcxh_paillier_t paillier;  /* the party's own Paillier private key */
  const uint32_t* NTilde;
  const uint32_t* h1;
  const uint32_t* h2;
  const uint32_t* alpha;      /* h2 = h1^alpha mod N~ */
  const uint32_t* beta;       /* alpha^-1 mod pq */
  const uint32_t* p;          /* N~ = (2p+1)(2q+1) */
  const uint32_t* q;
} mpcxh_party_t;
int mpcxh_bench_keygen_proofs(uint32_t w, const mpcxh_party_t* parties, uint32_t n_parties, uint32_t sessions,
                              uint64_t seed, uint32_t wave_sessions, double* stats_out, uint32_t* trace_out);
/* Config 5 with resharing as mpcium runs it (two resharing sessions per node
 * per wallet: old party and new party, /root/reference/pkg/eventconsumer/
 * event_consumer.go:407-416): reshare_mix = 1 makes every odd wave a resharing
 * wave -- the new committee's proof work (as keygen) plus the old committee's
 * VSS of its Lagrange-weighted share with new threshold 2 and the new
 * committee's decommitment, share and public-key checks (keygenload.hpp);
 * 0: keygen waves only (= mpcxh_bench_keygen_proofs).
 * stats_out[MPCXH_KEYGEN_RESHARE_STATS]: the MPCXH_KEYGEN_STATS values, then
 * keygen_sessions, reshare_sessions, keygen_wave_s, reshare_wave_s (summed
 * wave wall times per kind), vss_checks, vss_failures.
 * trace_out: per wave the keygen trace words, then n*8 + 9 VSS words (per old
 * party the 8-word digest of its commitment, points and shares; the digest of
 * the new shares; the count of VSS checks that passed; zero on keygen waves).
 * tamper_session >= 0 (test hook; -1: none): in that resharing session old party
 * 0 sends new party 1 a share off by one, so exactly one VSS check fails. */
#define MPCXH_KEYGEN_RESHARE_STATS 19
int mpcxh_bench_keygen_reshare(uint32_t w, const mpcxh_party_t* parties, uint32_t n_parties, uint32_t sessions,
                               uint64_t seed, uint32_t wave_sessions, int reshare_mix, int64_t tamper_session,
                               double* stats_out, uint32_t* trace_out);

/* ---------------------------------------------------------------- ECDSA keygen
 * words per party of a traced keygen session: u_i (8), the commitment C_i (8),
 * V_i0..V_it (16 each), the shares s_i0..s_i,n-1 as sent (8 each), then 8-word
 * SHA512_256i digests: its DLN proof (h1, h2, alpha), its DLN proof (h2, h1,
 * beta), its Mod proof, its Fac proof to party 0..n-1 (zero at its own index) --
 * the digests of mpcxh_bench_keygen_proofs' trace -- and its Paillier proof
 * (y_0..y_12; zero when the session did not reach it) */
#define MPCXH_ECDSA_KEYGEN_TRACE_WORDS(t, n) (16u + 16u * ((t) + 1u) + 8u * (n) + 8u * (4u + (n)))
/* up:ecdsa/keygen rounds 1-4 (csrc/host/ecdsa_keygen.hpp; restated as recalled:
 * upstream, verify) for `count` sessions over one committee of n_parties
 * (2..16) nodes at threshold t (1 <= t < n_parties), every party replayed in
 * process: parties[i] is node i's LocalPreParams (w >= 64 words per integer),
 * ids its party id (id_words 1..16 words, used mod q; zero or equal ids are
 * MPCX_EINVAL). Round 2's checks of the committee (N_j and N~_j of 2048 bits,
 * h1_j != h2_j, no N~, h1 or h2 used twice) are made once and fail the call
 * with MPCX_EINVAL. Per session: session bytes (session_len each; party i
 * proves under session || big.Int(i).Bytes()) and one reader per party.
 * status[s] = 0 with pub[s] (ECDSAPub), x[s][j] (party j's Xi) and X[s][j]
 * (BigXj), or the round that aborted it -- 2 (a DLN proof), 3 (the
 * decommitment, its points, the Mod proof, a Fac proof or a share), 4 (the
 * Paillier proof) -- with culprit[s] the lowest party whose message failed and
 * the outputs zero; culprit is 255 otherwise. The other sessions are
 * unaffected. Every proof kind of a party is one batch over the sessions, and
 * every point equation of a step one GPU batch over the sessions, dealers and
 * receivers. trace_flags / trace as mpcxh_eddsa_keygen_batch, n_parties x
 * MPCXH_ECDSA_KEYGEN_TRACE_WORDS(t, n_parties) words per flagged session. Test
 * hooks on dealer 0 of session tamper_session (-1 / 0 for none): 1 shifts a
 * response of its first DLN proof (round 2), 2 swaps two coordinates of its
 * decommitment (round 3), 3 shifts the share s_01 (round 3), 4 shifts y_0 of
 * its Paillier proof (round 4). flags: 0, or
 * MPCXH_ECDSA_KEYGEN_SERIAL_LAUNCHES to issue every launch of the call after
 * the one before instead of running the parties' batches side by side: the
 * number of kernel launches then depends on the inputs alone (concurrent
 * launches are merged by the coalescer as they happen to meet), at the price
 * of the overlap. gpu_s (or NULL) receives the wall time inside the GPU batch
 * calls. */
#define MPCXH_ECDSA_KEYGEN_SERIAL_LAUNCHES 1u
int mpcxh_ecdsa_keygen_batch(uint32_t w, const mpcxh_party_t* parties, uint32_t n_parties, uint32_t threshold,
                             const uint32_t* ids /* n_parties x id_words */, uint32_t id_words, uint32_t count,
                             const uint8_t* sessions /* count x session_len */, uint32_t session_len,
                             const mpcxh_reader_t* readers /* count x n_parties */, const uint8_t* trace_flags,
                             int64_t tamper_session, int tamper_kind, uint32_t flags, uint8_t* status /* count */,
                             uint8_t* culprit /* count */, uint32_t* pub /* count x 16 */,
                             uint32_t* x /* count x n_parties x 8 */, uint32_t* X /* count x n_parties x 16 */,
                             uint32_t* trace, double* gpu_s);
/* GG18 signing on stored wallets: mpcxh_bench_signing's rounds (the same code)
 * on the caller's key shares, messages and session ids. Every wallet is signed
 * by the same `signers` (2..n_nodes) nodes, sks[i] / dlns[i] the keys of signer
 * i. Per wallet: the signers' party ids (id_words 1..16 words each, used mod q),
 * their Shamir shares x_i and BigX_i = x_i G, ECDSAPub, the message as an
 * integer < q (8 words) and 32 session bytes. w_i = lambda_i x_i with lambda_i
 * the Lagrange weight at 0 over the wallet's signer ids, W_i = lambda_i BigX_i
 * (one GPU point batch over all wallets and signers), X = ECDSAPub. The
 * ephemeral randomness is the driver's: CounterDRBG(mix(seed, wallet, 0xFFFF,
 * 0)) draws k_i then gamma_i per signer; the pair and GG18 readers are
 * mpcxh_bench_signing's. status[wi] = 0 with r, s (8 words each, low-s) and
 * recid, or no signature (zeros): 1 an MtA proof or decryption was refused, 2
 * a round 5-9 check failed, 3 the signature failed ecdsa.Verify under
 * ECDSAPub; the other wallets are unaffected. Malformed input (ids zero or
 * equal mod q, msg >= q, a point off the curve) is MPCX_EINVAL. stats_out (or
 * NULL) and trace_wallets / trace_out as mpcxh_bench_signing. */
int mpcxh_ecdsa_sign_batch(uint32_t w, const mpcxh_paillier_t* sks, const mpcxh_dln_t* dlns, uint32_t n_nodes,
                           uint32_t signers, uint32_t wallets, const uint32_t* ids /* wallets x signers x id_words */,
                           uint32_t id_words, const uint32_t* x /* wallets x signers x 8 */,
                           const uint32_t* BigX /* wallets x signers x 16 */, const uint32_t* pub /* wallets x 16 */,
                           const uint32_t* msgs /* wallets x 8 */, const uint8_t* sessions /* wallets x 32 */,
                           uint64_t seed, uint8_t* status, uint32_t* r, uint32_t* s, uint32_t* recid,
                           double* stats_out, uint32_t trace_wallets, uint32_t* trace_out);

/* Host-side helpers of the MtA path, exported as test hooks (no GPU needed):
 * common.SHA512_256i / SHA512_256i_TAGGED (tag == NULL: untagged) over count
 * integers of w words -> 32-byte digest; secp256k1 k*G and k*P (k: w words,
 * points 16 words x|y, all-zero = infinity); the first `count` draws of
 * common.GetRandomPositiveInt(rand, lessThan) (relprime != 0:
 * GetRandomPositiveRelativelyPrimeInt) from the CounterDRBG `seed`. */
int mpcxh_sha512_256i(const uint8_t* tag, size_t tag_len, uint32_t count, const uint32_t* ints, uint32_t w,
                      uint8_t* digest32);
int mpcxh_secp_scalar_base_mult(const uint32_t* k, uint32_t w, uint32_t* out16);
int mpcxh_secp_scalar_mult(const uint32_t* p16, const uint32_t* k, uint32_t w, uint32_t* out16);
/* u1*G + u2*P (the ecdsa.Verify combination) */
int mpcxh_secp_lincomb(const uint32_t* u1, const uint32_t* p16, const uint32_t* u2, uint32_t w, uint32_t* out16);
int mpcxh_random_draws(uint64_t seed, const uint32_t* less_than, uint32_t w, int relprime, uint32_t count,
                       uint32_t* out);

/* Go (*Int).ProbablyPrime(reps) for count odd or even n of `words` words
 * (go:src/math/big/prime.go: small-prime exits, Miller-Rabin with base 2 and
 * `reps` further bases drawn as Go draws them -- math/rand seeded with n's low
 * word, nat.random below n - 3, plus 2 -- and the extra strong Lucas test with
 * Baillie-OEIS parameter P, both on the GPU for n of up to 2048 bits). The same
 * tests as Go; only their order differs (base 2 first). ok[i] = 1: probably prime. */
int mpcxh_probably_prime_batch(uint32_t count, const uint32_t* n, uint32_t words, int reps, uint8_t* ok);
/* ok[i] = gcd(x[i], m[i]) == 1 for odd m[i] (math/big GCD(nil, nil, x, m).Cmp(one)
 * == 0, the coprimality test behind common.GetRandomPositiveRelativelyPrimeInt
 * and the proof verifiers' gcd checks); host-side, count operands of `words`
 * words each. MPCX_EINVAL for an even modulus. */
int mpcxh_coprime_batch(uint32_t count, const uint32_t* x, const uint32_t* m, uint32_t words, uint8_t* ok);

/* Host-time profile (environment MPCX_HOST_PROFILE=1 at process start, else
 * empty): "label: seconds (calls)" lines summed over threads, largest first,
 * written NUL-terminated into buf (truncated to cap); reset != 0 clears it. */
int mpcxh_profile_report(char* buf, size_t cap, int reset);

/* Host worker pool size: *threads = the threads parallel loops use now
 * (MPCX_HOST_THREADS, else min(usable CPUs, 16 per bound GPU)); *usable = the
 * CPUs this process may run on (affinity mask capped by the cgroup CPU quota). */
int mpcxh_host_threads(int* threads, int* usable);
/* The engine's page-locked staging pool (no GPU needed): bytes held (in use +
 * cached), peak bytes in use, and the pageable fallbacks taken when pinning
 * failed (count, bytes; each is also logged to stderr). Any pointer may be NULL. */
int mpcxh_pinned_pool_stats(uint64_t* held_bytes, uint64_t* peak_in_use_bytes, uint64_t* fallbacks,
                            uint64_t* fallback_bytes);
/* Pool self-test (no GPU): `tasks` threads each run a parallel loop of `outer`
 * indices, each index a nested parallel loop of `inner` indices adding
 * (task+1)(o+1)(i+1); *sum = the total. */
int mpcxh_pool_selftest(uint32_t tasks, uint32_t outer, uint32_t inner, uint64_t* sum);

/* Host bignum arithmetic (test hook, no GPU): op 0: a * b, 1: a / b, 2: a mod b,
 * 3: a^-1 mod b (Go ModInverse; MPCX_EINVAL when none), 4: gcd(a, b). Little-endian
 * words; *out_words = the result's normalized length (<= nout). */
int mpcxh_nat_arith(int op, const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb, uint32_t* out,
                    uint32_t nout, uint32_t* out_words);

/* tss-lib candidate q from raw stream bytes (masking + delta walk; test hook). */
int mpcxh_candidate_from_bytes(const uint8_t* bytes, size_t n, int q_bit_len, uint32_t* q_out, uint32_t words);

/* n bytes of the CounterDRBG stream for `seed` (test hook). */
int mpcxh_drbg_read(uint64_t seed, uint8_t* out, size_t n);

/* Go math/rand (test hooks): count Int63() values of rand.New(rand.NewSource(seed)),
 * and the `reps` Miller-Rabin bases big.Int.ProbablyPrime(reps) draws for the odd
 * n (w words, n > 3), in Go's order, w words each (go:src/math/big/prime.go). */
int mpcxh_go_rand_int63(int64_t seed, uint32_t count, int64_t* out);
int mpcxh_go_mr_bases(const uint32_t* n, uint32_t w, uint32_t reps, uint32_t* out);

#ifdef __cplusplus
}
#endif

#endif /* MPCX_HOST_H_ */
