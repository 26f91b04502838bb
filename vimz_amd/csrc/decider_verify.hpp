// The decider's verifier on the host: what contracts/*Verifier.sol::verifyNovaProof does with the 25 calldata words (ContrastVerifier.sol:685-783) over pairing.hpp.
// Shared by vimz_decider_verify / vimz_decider_verify_key (groth16.hip), which judge one proof, and vimz_decider_verify_batch (decider_batch.hpp / .hip), which
// judges many under one key: both read a proof through parse_proof, so their early returns are the same code.  No HIP in this file:
// tests/native/decider_batch_check.cpp runs it under the host sanitizers.
#pragma once
#include <cstring>
#include <vector>
#include "g16_point_stage.hpp"

namespace vz {
namespace dv {

typedef Fp<BnFr> Fr;
typedef Fp<BnFq> Fq;
using pairing::Fq2;
typedef Affine<Fq> G1A;
typedef Affine<Fq2> G2A;
typedef XYZZ<Fq> G1X;

struct VerifierKey {
  Fr pp_hash; uint32_t len_z = 0;
  G1A alpha; G2A beta, gamma, delta; std::vector<G1A> ic;
  G1A kzg_g1; G2A kzg_g2, kzg_vk;
};
enum { DV_STEPS = 1, DV_KZG_W = 2, DV_KZG_E = 4, DV_GROTH16 = 8, DV_MALFORMED = 16 };
constexpr int LIMBS = 5, LIMB_BITS = 55;      // LimbsDecomposition of contracts/*Verifier.sol (:632-640): aug/decider.hpp's DEC_LIMBS, DEC_LIMB_BITS
inline uint32_t n_public(uint32_t len_z) { return 2 + 2 * len_z + 4 * LIMBS + 4 + 2 * LIMBS; }      // aug::decider_n_public

inline bool get_fq(const uint64_t* src, Fq* out) { Fq c; memcpy(c.v, src, 32); if (!c.is_reduced()) return false; *out = Fq::to_mont(c); return true; }
inline bool get_g1(const uint64_t* src, G1A* p) { return get_fq(src, &p->x) && get_fq(src + 4, &p->y); }
inline bool get_g2(const uint64_t* src, G2A* p) { return get_fq(src, &p->x.c0) && get_fq(src + 4, &p->x.c1) && get_fq(src + 8, &p->y.c0) && get_fq(src + 12, &p->y.c1); }
inline Fr fr_u64(uint64_t v) { Fr c = Fr::zero(); c.v[0] = (uint32_t)v; c.v[1] = (uint32_t)(v >> 32); return Fr::to_mont(c); }
inline G1A g1_negate(const G1A& p) { G1A r = p; if (!aff_is_identity(p)) r.y = Fq::neg(p.y); return r; }
inline G1A g1_lin(const G1A& a, const uint64_t* k256, const G1A& b) {      // a + k·b, k: any 256 bits
  G1X acc = pt_scalar_mul_bits(b, (const uint32_t*)k256, 256);
  add_mixed(acc, a);
  return to_affine(acc);
}
// the 5 limbs of 55 bits of each coordinate of p, little end first, as public inputs
inline void push_limbs(std::vector<Fr>& pub, const Fq& coord) {
  const Fq c = Fq::from_mont(coord);
  uint64_t w[5] = {0, 0, 0, 0, 0}; memcpy(w, c.v, 32);
  for (int k = 0; k < LIMBS; k++) {
    const int bit = LIMB_BITS * k, q = bit >> 6, s = bit & 63;
    uint64_t l = w[q] >> s;
    if (s + LIMB_BITS > 64 && q + 1 < 5) l |= w[q + 1] << (64 - s);
    pub.push_back(fr_u64(l & ((1ull << LIMB_BITS) - 1)));
  }
}

// key blob (vimz_decider_vk): pp_hash, len_z, alpha (G1), beta, gamma, delta (G2: x.c0, x.c1, y.c0, y.c1), n_ic, IC points, KZG G_1 (G1), G_2, VK (G2)
inline bool parse_key(const uint64_t* w, size_t n, VerifierKey* K) {
  using namespace vz::pairing;
  size_t pos = 0;
  auto need = [&](size_t k) { return pos + k <= n; };
  if (!need(5)) return false;
  { Fr c; memcpy(c.v, w, 32); if (!c.is_reduced()) return false; K->pp_hash = Fr::to_mont(c); } pos += 4;
  K->len_z = (uint32_t)w[pos++];
  if (!need(8 + 48 + 1) || !get_g1(w + pos, &K->alpha)) return false; pos += 8;
  for (G2A* p : {&K->beta, &K->gamma, &K->delta}) { if (!get_g2(w + pos, p)) return false; pos += 16; }
  const uint64_t n_ic = w[pos++];
  if (n_ic != 1 + (uint64_t)n_public(K->len_z) || !need(8 * n_ic + 8 + 32)) return false;
  K->ic.resize(n_ic);
  for (auto& p : K->ic) { if (!get_g1(w + pos, &p)) return false; pos += 8; }
  if (!get_g1(w + pos, &K->kzg_g1)) return false; pos += 8;
  if (!get_g2(w + pos, &K->kzg_g2) || !get_g2(w + pos + 16, &K->kzg_vk)) return false; pos += 32;
  if (pos != n) return false;
  if (!g1_on_curve(K->alpha) || !g1_on_curve(K->kzg_g1)) return false;
  for (auto& p : K->ic) if (!g1_on_curve(p)) return false;
  for (const G2A* p : {&K->beta, &K->gamma, &K->delta, &K->kzg_g2, &K->kzg_vk}) if (!g2_on_curve(*p) || !g2_in_subgroup(*p)) return false;
  return true;
}

// One proof as its words give it: the eight G1 points U_i.cmW, U_i.cmE, u_i.cmW, cmT, A, C, proof_W, proof_E, B, and the public inputs up to z_i
// (pp_hash, steps, z_0, z_i) — the folded commitments' limbs, the four KZG scalars and cmT's limbs follow once cmW and cmE are known (finish_public).
struct Proof {
  uint32_t res = 0;      // DV_STEPS so far; the verdict when parse_proof returns false
  G1A P[8]; G2A B;
  std::vector<Fr> pub;
};
enum { P_UW = 0, P_UE = 1, P_LW = 2, P_T = 3, P_A = 4, P_C = 5, P_PIW = 6, P_PIE = 7 };
inline bool points_on_curve(const Proof& p) {
  for (int k = 0; k < 8; k++) if (!pairing::g1_on_curve(p.P[k])) return false;
  return pairing::g2_on_curve(p.B) && pairing::g2_in_subgroup(p.B);
}
// The parsing and early-return part of the verifier.  w: the 25 calldata words as 4 little-endian limbs each.  false: out->res is the verdict, nothing else is
// to be evaluated — malformed words (a coordinate not below q, a point off its curve, a B that r does not kill) give DV_MALFORMED, a public element not below r
// gives DV_GROTH16 without the KZG bits; steps < 2 sets DV_STEPS and the checks go on.  true: the checks go on over *out.
// judge_points = false leaves "on its curve" and "killed by r" to the caller's own stage (the batch's per-point kernel), which must give DV_MALFORMED in their
// place — except for a proof with a public element out of range, whose points are then judged here: malformed words come before that verdict.
inline bool parse_proof(const VerifierKey& K, uint64_t steps, const uint64_t* z0, const uint64_t* zi, const uint64_t* w, bool judge_points, Proof* out) {
  out->res = 0; out->pub.clear();
  if (!pairing::consts().ok) { out->res = DV_MALFORMED; return false; }
  if (steps < 2) out->res |= DV_STEPS;                                              // :697
  static const int at[8] = {0, 2, 4, 6, 9, 15, 21, 23};
  for (int k = 0; k < 8; k++) if (!get_g1(w + 4 * at[k], &out->P[k])) { out->res |= DV_MALFORMED; return false; }
  G2A& B = out->B;      // calldata: x imaginary, x real, y imaginary, y real
  if (!get_fq(w + 4 * 11, &B.x.c1) || !get_fq(w + 4 * 12, &B.x.c0) || !get_fq(w + 4 * 13, &B.y.c1) || !get_fq(w + 4 * 14, &B.y.c0)) { out->res |= DV_MALFORMED; return false; }
  if (judge_points && !points_on_curve(*out)) { out->res |= DV_MALFORMED; return false; }
  bool canon = true;
  auto push_canon = [&](const uint64_t* c) { Fr x; memcpy(x.v, c, 32); if (!x.is_reduced()) { canon = false; return; } out->pub.push_back(Fr::to_mont(x)); };      // checkField
  out->pub.push_back(K.pp_hash); out->pub.push_back(fr_u64(steps));
  for (uint32_t k = 0; k < K.len_z && canon; k++) push_canon(z0 + 4 * k);
  for (uint32_t k = 0; k < K.len_z && canon; k++) push_canon(zi + 4 * k);
  for (int k = 17; k <= 20 && canon; k++) { Fr x; memcpy(x.v, w + 4 * k, 32); canon = x.is_reduced(); }
  if (!canon) { out->res |= (!judge_points && !points_on_curve(*out)) ? DV_MALFORMED : DV_GROTH16; return false; }
  if (n_public(K.len_z) + 1 != K.ic.size()) { out->res |= DV_MALFORMED; return false; }
  return true;
}
// the rest of the public inputs, once the folded commitments are known (:716-722, :739-745, :758-772)
inline void finish_public(Proof& p, const uint64_t* w, const G1A& cmW, const G1A& cmE) {
  push_limbs(p.pub, cmW.x); push_limbs(p.pub, cmW.y); push_limbs(p.pub, cmE.x); push_limbs(p.pub, cmE.y);
  for (int k = 17; k <= 20; k++) { Fr x; memcpy(x.v, w + 4 * k, 32); p.pub.push_back(Fr::to_mont(x)); }
  push_limbs(p.pub, p.P[P_T].x); push_limbs(p.pub, p.P[P_T].y);
}

// KZG10Verifier.check (:167-189): e(pi, VK) · e(x·(−pi) − c + y·G_1, G_2) == 1
inline bool kzg_check(const VerifierKey& K, const G1A& c, const G1A& pi, const uint64_t* x, const uint64_t* y) {
  G1X acc = pt_scalar_mul_bits(g1_negate(pi), (const uint32_t*)x, 256);
  add_mixed(acc, g1_negate(c));
  { const G1X t = pt_scalar_mul_bits(K.kzg_g1, (const uint32_t*)y, 256); add_full(acc, t); }
  return pairing::product_is_one({{pi, K.kzg_vk}, {to_affine(acc), K.kzg_g2}});
}
// Returns a bit set of DV_* (0 = accepted)
inline uint32_t verify_words(const VerifierKey& K, uint64_t steps, const uint64_t* z0, const uint64_t* zi, const uint64_t* w) {
  Proof p;
  if (!parse_proof(K, steps, z0, zi, w, true, &p)) return p.res;
  uint32_t res = p.res;
  const uint64_t* r = w + 4 * 8;
  const G1A cmW = g1_lin(p.P[P_UW], r, p.P[P_LW]), cmE = g1_lin(p.P[P_UE], r, p.P[P_T]);      // :712-713, :735-736
  finish_public(p, w, cmW, cmE);
  if (!kzg_check(K, cmW, p.P[P_PIW], w + 4 * 17, w + 4 * 19)) res |= DV_KZG_W;             // :725-730
  if (!kzg_check(K, cmE, p.P[P_PIE], w + 4 * 18, w + 4 * 20)) res |= DV_KZG_E;             // :748-753
  // Groth16 (:386-620): vk_x = IC_0 + Σ pub_k·IC_{k+1};  e(−A, B)·e(alpha, beta)·e(vk_x, gamma)·e(C, delta) == 1
  G1X vkx = G1X::identity();
  add_mixed(vkx, K.ic[0]);
  for (size_t k = 0; k < p.pub.size(); k++) {
    if (p.pub[k].is_zero() || aff_is_identity(K.ic[k + 1])) continue;
    const Fr c = Fr::from_mont(p.pub[k]);
    const G1X t = pt_scalar_mul_bits(K.ic[k + 1], c.v, 256);
    add_full(vkx, t);
  }
  if (!pairing::product_is_one({{g1_negate(p.P[P_A]), p.B}, {K.alpha, K.beta}, {to_affine(vkx), K.gamma}, {p.P[P_C], K.delta}})) res |= DV_GROTH16;
  return res;
}

}  // namespace dv
}  // namespace vz
