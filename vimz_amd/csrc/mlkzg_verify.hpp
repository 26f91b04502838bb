// The multilinear KZG opening's transcript, proof layout and verifier (vimz_mlkzg_verify), host only over pairing.hpp and decider_verify.hpp.  No HIP
// in this file: tests/native/mlkzg_check.cpp runs it under the host sanitizers.  The prover (mlkzg.hip) draws its challenges through the same Rounds.
//
// A proof for ℓ variables is 20ℓ + 16 canonical little-endian u64 words: C_1 .. C_(ℓ−1) (x, y; the identity as zeros), E_r[0..ℓ), E_(−r)[0..ℓ), E_(r²)[0..ℓ),
// W_r, W_(−r), W_(r²).  Everything that crosses this file's interface is canonical; inside, elements are Montgomery.
#pragma once
#include "decider_verify.hpp"
#include "keccak.hpp"
#include "mlkzg_stage.hpp"

namespace vz {
namespace mlk {

using dv::G1A;
using dv::G2A;
using dv::Fq;

enum { ML_MALFORMED = 1, ML_OFF_CURVE = 2, ML_FOLD = 4, ML_PAIRING = 8 };      // VIMZ_MLKZG_* (include/vimz_hip.h)

inline size_t proof_words(uint32_t logn) { return 20 * (size_t)logn + 16; }
// where the parts of a proof start, in words
inline size_t at_ck(uint32_t) { return 0; }
inline size_t at_evals(uint32_t logn) { return 8 * ((size_t)logn - 1); }
inline size_t at_w(uint32_t logn) { return at_evals(logn) + 12 * (size_t)logn; }

// proof_io.hpp's Transcript — a SHA3-256 chain, state' = H(state ‖ tag[8] ‖ len ‖ data), a challenge the low 128 bits of state' = H(state ‖ 'c') — restated over
// keccak.hpp alone, so that a program without HIP can include it
struct Chain {
  uint8_t st[32];
  struct Sponge {
    uint64_t s[25]; int pos = 0;
    Sponge() { for (auto& x : s) x = 0; }
    void update(const void* data, size_t n) {
      const uint8_t* p = (const uint8_t*)data;
      for (size_t i = 0; i < n; i++) { s[pos >> 3] ^= (uint64_t)p[i] << (8 * (pos & 7)); if (++pos == 136) { keccak_f1600(s); pos = 0; } }
    }
    void finish(uint8_t out[32]) { s[pos >> 3] ^= (uint64_t)0x06 << (8 * (pos & 7)); s[16] ^= 0x8000000000000000ULL; keccak_f1600(s); memcpy(out, s, 32); }
  };
  explicit Chain(const char* label) { memset(st, 0, 32); absorb_bytes("init", label, strlen(label)); }
  void absorb_bytes(const char* tag, const void* data, size_t n) {
    Sponge h; h.update(st, 32);
    uint8_t t[8] = {0}; for (int i = 0; i < 8 && tag[i]; i++) t[i] = (uint8_t)tag[i];
    h.update(t, 8);
    const uint64_t len = n; h.update(&len, 8);
    if (n) h.update(data, n);
    h.finish(st);
  }
  void absorb_words(const char* tag, const uint64_t* w, size_t nwords) { absorb_bytes(tag, w, 8 * nwords); }
  Fr challenge() {      // 128 bits, Montgomery
    Sponge h; h.update(st, 32); const uint8_t c = 'c'; h.update(&c, 1); h.finish(st);
    Fr x = Fr::zero(); memcpy(x.v, st, 16);
    return Fr::to_mont(x);
  }
};

// the three rounds of the opening: what is absorbed before r, before q and before d (all canonical words)
struct Rounds {
  Chain t{"vimz-mlkzg-v1"};
  Fr round_r(uint32_t logn, const uint64_t comm[8], const uint64_t* point, const uint64_t eval[4], const uint64_t* ck) {
    const uint64_t l = logn;
    t.absorb_words("logn", &l, 1); t.absorb_words("C", comm, 8); t.absorb_words("x", point, 4 * (size_t)logn); t.absorb_words("y", eval, 4);
    t.absorb_words("Ck", ck, 8 * ((size_t)logn - 1));
    return t.challenge();
  }
  Fr round_q(uint32_t logn, const uint64_t* evals) { t.absorb_words("E", evals, 12 * (size_t)logn); return t.challenge(); }
  Fr round_d(const uint64_t* w) { t.absorb_words("W", w, 24); return t.challenge(); }
};

inline bool get_fr(const uint64_t* src, Fr* out) { Fr c; memcpy(c.v, src, 32); if (!c.is_reduced()) return false; *out = Fr::to_mont(c); return true; }
inline void put_fr(uint64_t* dst, const Fr& mont) { const Fr c = Fr::from_mont(mont); memcpy(dst, c.v, 32); }
inline G1A g1_generator() { G1A g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
inline Fq fq_hex(const char* h) {
  Fq c = Fq::zero(); int bit = 0;
  for (size_t i = strlen(h); i-- > 0; bit += 4) { const char ch = h[i]; const uint32_t d = ch <= '9' ? ch - '0' : ch - 'a' + 10; c.v[bit >> 5] |= d << (bit & 31); }
  return Fq::to_mont(c);
}
inline G2A g2_generator() {      // EIP-197's
  G2A g;
  g.x.c0 = fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g.x.c1 = fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g.y.c0 = fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g.y.c1 = fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
  return g;
}
// a + k·b with k a Montgomery element
inline G1A g1_lin_fr(const G1A& a, const Fr& k, const G1A& b) { uint64_t w[4]; put_fr(w, k); return dv::g1_lin(a, w, b); }

// a proof and its statement as parsed: the range checks alone
struct Parsed {
  uint32_t logn = 0;
  G2A vk; G1A C; std::vector<G1A> ck;            // ck[k − 1] = C_k
  std::vector<Fr> x, E[3]; Fr y; G1A W[3];
};
// false: the verdict is ML_MALFORMED (wrong word count, ℓ out of range, an element not below r, a coordinate not below q)
inline bool parse(const uint64_t vk_g2[16], const uint64_t comm[8], uint32_t logn, const uint64_t* point, const uint64_t eval[4], const uint64_t* proof, size_t n_words, Parsed* P) {
  if (logn == 0 || logn > (uint32_t)ML_MAX_LOGN || n_words != proof_words(logn)) return false;
  P->logn = logn;
  if (!dv::get_g2(vk_g2, &P->vk) || !dv::get_g1(comm, &P->C) || !get_fr(eval, &P->y)) return false;
  P->x.resize(logn); P->ck.resize(logn - 1);
  for (uint32_t k = 0; k < logn; k++) if (!get_fr(point + 4 * k, &P->x[k])) return false;
  for (uint32_t k = 0; k + 1 < logn; k++) if (!dv::get_g1(proof + at_ck(logn) + 8 * k, &P->ck[k])) return false;
  for (int u = 0; u < 3; u++) {
    P->E[u].resize(logn);
    for (uint32_t k = 0; k < logn; k++) if (!get_fr(proof + at_evals(logn) + 4 * ((size_t)u * logn + k), &P->E[u][k])) return false;
    if (!dv::get_g1(proof + at_w(logn) + 8 * u, &P->W[u])) return false;
  }
  return true;
}

// the verdict word: 0 accepted, else ONE of ML_* — each stage runs only if the earlier ones found nothing
inline uint32_t verify(const uint64_t vk_g2[16], const uint64_t comm[8], uint32_t logn, const uint64_t* point, const uint64_t eval[4], const uint64_t* proof, size_t n_words) {
  Parsed P;
  if (!pairing::consts().ok || !parse(vk_g2, comm, logn, point, eval, proof, n_words, &P)) return ML_MALFORMED;
  if (!pairing::g1_on_curve(P.C) || !pairing::g2_on_curve(P.vk) || !pairing::g2_in_subgroup(P.vk)) return ML_OFF_CURVE;
  for (const G1A& p : P.ck) if (!pairing::g1_on_curve(p)) return ML_OFF_CURVE;
  for (const G1A& p : P.W) if (!pairing::g1_on_curve(p)) return ML_OFF_CURVE;
  Rounds R;
  const Fr r = R.round_r(logn, comm, point, eval, proof + at_ck(logn));
  const Fr q = R.round_q(logn, proof + at_evals(logn));
  const Fr d = R.round_d(proof + at_w(logn));
  if (r.is_zero()) return ML_FOLD;
  // 2r·next_k = r(1 − x_k)(E_r[k] + E_(−r)[k]) + x_k(E_r[k] − E_(−r)[k])
  const Fr two_r = Fr::dbl(r);
  for (uint32_t k = 0; k < logn; k++) {
    const Fr next = k + 1 < logn ? P.E[2][k + 1] : P.y;
    const Fr sum = Fr::add(P.E[0][k], P.E[1][k]), dif = Fr::sub(P.E[0][k], P.E[1][k]);
    const Fr rhs = Fr::add(Fr::mul(Fr::mul(r, Fr::sub(Fr::one(), P.x[k])), sum), Fr::mul(P.x[k], dif));
    if (!Fr::mul(two_r, next).eq(rhs)) return ML_FOLD;
  }
  // C_B = Σ q^k·C_k by Horner over the points;  b_u = Σ q^k·E_u[k]
  G1A cb = logn > 1 ? P.ck[logn - 2] : P.C;
  for (uint32_t k = logn - 1; k-- > 0;) cb = g1_lin_fr(k ? P.ck[k - 1] : P.C, q, cb);
  const Fr u[3] = {r, Fr::neg(r), Fr::sqr(r)};
  const Fr dj[3] = {Fr::one(), d, Fr::sqr(d)};
  Fr bsum = Fr::zero();
  for (int j = 0; j < 3; j++) {
    Fr b = Fr::zero();
    for (uint32_t k = logn; k-- > 0;) b = Fr::add(Fr::mul(b, q), P.E[j][k]);
    bsum = Fr::add(bsum, Fr::mul(dj[j], b));
  }
  // L = (1 + d + d²)·C_B − (Σ d^j·b_j)·G + Σ d^j·u_j·W_j,   Rr = W_0 + d·(W_1 + d·W_2);   e(L, G2) = e(Rr, [tau]G2)
  G1A id; id.x = id.y = Fq::zero();
  G1A L = g1_lin_fr(id, Fr::add(Fr::add(dj[0], dj[1]), dj[2]), cb);
  L = g1_lin_fr(L, Fr::neg(bsum), g1_generator());
  for (int j = 0; j < 3; j++) L = g1_lin_fr(L, Fr::mul(dj[j], u[j]), P.W[j]);
  const G1A Rr = g1_lin_fr(P.W[0], d, g1_lin_fr(P.W[1], d, P.W[2]));
  if (!pairing::product_is_one({{L, g2_generator()}, {dv::g1_negate(Rr), P.vk}})) return ML_PAIRING;
  return 0;
}

}  // namespace mlk
}  // namespace vz
