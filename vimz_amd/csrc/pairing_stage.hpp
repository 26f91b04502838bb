// What ONE thread of the batched decider verifier's two kernels does (decider_batch.hip: k_g1_lincomb, k_miller), as host-and-device functions of the thread's
// index: the kernels call them with their thread index, the host path of vimz_decider_verify_batch (ctx == NULL) and tests/native/decider_batch_check.cpp loop
// them over every index on the CPU.  No HIP in this file beyond VZ_HD.
//
// The Miller loop here is NOT pairing.hpp::miller_loop: that one takes affine steps with one Fq2 inversion each (about 380 of its 520 base-field products a
// step), fine for a handful of pairings.  Here T runs in homogeneous projective coordinates (X : Y : Z) on the twist y² = x³ + b', b' = 3/ξ, with no inversion,
// and a step's line has three non-zero Fq2 coefficients, at 1, w and w³ (c0.c0, c1.c0, c1.c1 of pairing.hpp's Fq12), multiplied into f by a sparse product:
//     doubling   B = Y², C = Z², E = 3b'·C, F = 3E, H = 2YZ, J = X²:     line (H·yP, −3J·xP, B − E);   T <- (2XY·(B − F), (B + F)² − 12E², 4B·H)
//     addition   θ = Y − yQ·Z, λ = X − xQ·Z:                            line (λ·yP, −θ·xP, θ·xQ − λ·yQ)
//                C = θ², D = λ², E = λD, F = ZC, G = XD, H = E + F − 2G:  T <- (λH, θ(G − H) − E·Y, Z·E)
// (Costello, Lange, Naehrig: "Faster pairing computations on curves with high-degree twists", PKC 2010; the doubling scaled by 4 so that no halving is needed.)
// These lines are pairing.hpp's affine lines times 2YZ and times λ: factors in Fq2, which the final exponentiation removes.  So a Miller value of this file differs
// from miller_loop's word for word and has the same pairing; its word-for-word reference is tests/_miller_ref.py, which restates these formulas.
// The steps have no special cases: for Q of order r (every caller has checked r·Q = O point by point) T meets neither O nor ±Q inside the loop, and for any other
// input the arithmetic is total — no inversion, no branch on a value — so a thread cannot fault or spin on bad data; it computes a value that means nothing.
#pragma once
#include "g16_point_stage.hpp"

namespace vz {
namespace pairing {

constexpr uint64_t ATE_LOW = 11347224129447541672ull;      // 6t + 2 = 2^64 + this: the 64 bits below the leading one
constexpr int ATE_LOW_BITS = 64;

struct G2Proj { Fq2 X, Y, Z; };
struct Line { Fq2 l0, l1, l3; };      // l0 + l1·w + l3·w³

VZ_HD Fq2 fq2_triple(const Fq2& a) { return Fq2::add(Fq2::dbl(a), a); }

// On the device the products in Fq2 are CALLS, their operands and result in registers: inlined, the loop body is some three hundred Montgomery products — a kernel of
// several hundred thousand instructions that takes the compiler half an hour and spills eleven thousand registers.  On the host they inline as ever.
#if defined(__HIP_DEVICE_COMPILE__)
#define VZ_STAGE_CALL __attribute__((noinline))
#else
#define VZ_STAGE_CALL
#endif
VZ_HD VZ_STAGE_CALL Fq2 m2(Fq2 a, Fq2 b) { return Fq2::mul(a, b); }
VZ_HD VZ_STAGE_CALL Fq2 s2(Fq2 a) { return Fq2::sqr(a); }
VZ_HD VZ_STAGE_CALL Fq2 k2(Fq2 a, Fq k) { return Fq2::scale(a, k); }

// Fq6::mul's schoolbook with v³ = ξ over m2
VZ_HD Fq6 fq6_mul(const Fq6& a, const Fq6& b) {
  const Fq2 a0b0 = m2(a.c0, b.c0), a1b1 = m2(a.c1, b.c1), a2b2 = m2(a.c2, b.c2);
  const Fq2 t12 = Fq2::sub(Fq2::sub(m2(Fq2::add(a.c1, a.c2), Fq2::add(b.c1, b.c2)), a1b1), a2b2);
  const Fq2 t01 = Fq2::sub(Fq2::sub(m2(Fq2::add(a.c0, a.c1), Fq2::add(b.c0, b.c1)), a0b0), a1b1);
  const Fq2 t02 = Fq2::sub(Fq2::sub(m2(Fq2::add(a.c0, a.c2), Fq2::add(b.c0, b.c2)), a0b0), a2b2);
  Fq6 r; r.c0 = Fq2::add(a0b0, Fq2::mul_xi(t12)); r.c1 = Fq2::add(t01, Fq2::mul_xi(a2b2)); r.c2 = Fq2::add(t02, a1b1); return r;
}
// f·(l0 + l1 w + l3 w³): with f = a + b w, A = (l0, 0, 0), B = (l1, l3, 0) the product is (aA + v·bB) + ((a + b)(A + B) − aA − bB) w: 15 products in Fq2
VZ_HD Fq6 fq6_mul_by_01(const Fq6& b, const Fq2& m0, const Fq2& m1) {      // (b0 + b1 v + b2 v²)(m0 + m1 v)
  const Fq2 b0m0 = m2(b.c0, m0), b1m1 = m2(b.c1, m1);
  Fq6 r;
  r.c0 = Fq2::add(b0m0, Fq2::mul_xi(m2(b.c2, m1)));
  r.c1 = Fq2::sub(Fq2::sub(m2(Fq2::add(b.c0, b.c1), Fq2::add(m0, m1)), b0m0), b1m1);
  r.c2 = Fq2::add(m2(b.c2, m0), b1m1);
  return r;
}
VZ_HD void fq12_mul_by_line(Fq12& f, const Line& l) {
  Fq6 aA; aA.c0 = m2(f.c0.c0, l.l0); aA.c1 = m2(f.c0.c1, l.l0); aA.c2 = m2(f.c0.c2, l.l0);
  const Fq6 bB = fq6_mul_by_01(f.c1, l.l1, l.l3);
  const Fq6 s = fq6_mul_by_01(Fq6::add(f.c0, f.c1), Fq2::add(l.l0, l.l1), l.l3);
  f.c1 = Fq6::sub(Fq6::sub(s, aA), bB);
  f.c0 = Fq6::add(aA, Fq6::mul_v(bB));
}
// f²: (a + b w)² = (a + b)(a + v b) − ab − v·ab + 2ab·w: two products in Fq6 where Fq12::mul takes three
VZ_HD void fq12_square(Fq12& f) {
  const Fq6 ab = fq6_mul(f.c0, f.c1);
  const Fq6 t = fq6_mul(Fq6::add(f.c0, f.c1), Fq6::add(f.c0, Fq6::mul_v(f.c1)));
  f.c0 = Fq6::sub(Fq6::sub(t, ab), Fq6::mul_v(ab));
  f.c1 = Fq6::add(ab, ab);
}

VZ_HD void miller_double(Fq12& f, G2Proj& T, const G1PAff& P, const Fq2& twist_b) {
  const Fq2 B = s2(T.Y), C = s2(T.Z), J = s2(T.X);
  const Fq2 E = fq2_triple(m2(twist_b, C)), F = fq2_triple(E), H = Fq2::dbl(m2(T.Y, T.Z));
  Line l; l.l0 = k2(H, P.y); l.l1 = Fq2::neg(k2(fq2_triple(J), P.x)); l.l3 = Fq2::sub(B, E);
  fq12_mul_by_line(f, l);
  const Fq2 EE = s2(E), EE4 = Fq2::dbl(Fq2::dbl(EE));
  G2Proj n;
  n.X = m2(Fq2::dbl(m2(T.X, T.Y)), Fq2::sub(B, F));
  n.Y = Fq2::sub(s2(Fq2::add(B, F)), fq2_triple(EE4));
  n.Z = Fq2::dbl(Fq2::dbl(m2(B, H)));
  T = n;
}
VZ_HD void miller_add(Fq12& f, G2Proj& T, const G2PAff& Q, const G1PAff& P) {
  const Fq2 theta = Fq2::sub(T.Y, m2(Q.y, T.Z)), lam = Fq2::sub(T.X, m2(Q.x, T.Z));
  Line l; l.l0 = k2(lam, P.y); l.l1 = Fq2::neg(k2(theta, P.x)); l.l3 = Fq2::sub(m2(theta, Q.x), m2(lam, Q.y));
  fq12_mul_by_line(f, l);
  const Fq2 C = s2(theta), D = s2(lam), E = m2(lam, D), F = m2(T.Z, C), G = m2(T.X, D);
  const Fq2 H = Fq2::sub(Fq2::add(E, F), Fq2::dbl(G));
  G2Proj n;
  n.X = m2(lam, H);
  n.Y = Fq2::sub(m2(theta, Fq2::sub(G, H)), m2(E, T.Y));
  n.Z = m2(T.Z, E);
  T = n;
}

// out[index] = the Miller value of (P[index], Q[index]) over 6t + 2 with the two Frobenius steps; one when either point is the identity (0, 0).  twist_b, g12,
// g13: consts()'s 3/ξ, ξ^((q−1)/3), ξ^((q−1)/2), computed on the host.  The trip count is the constant ATE_LOW_BITS; the thread writes its own 96 words alone.
VZ_HD void miller_thread(size_t index, const G1PAff* P, const G2PAff* Q, const Fq2& twist_b, const Fq2& g12, const Fq2& g13, Fq12* out) {
  const G1PAff p = P[index];
  const G2PAff q = Q[index];
  Fq12 f = Fq12::one();
  if (!aff_is_identity(p) && !aff_is_identity(q)) {
    G2Proj T; T.X = q.x; T.Y = q.y; T.Z = Fq2::one();
#pragma unroll 1
    for (int i = ATE_LOW_BITS - 1; i >= 0; i--) {
      fq12_square(f);
      miller_double(f, T, p, twist_b);
      if ((ATE_LOW >> i) & 1ull) miller_add(f, T, q, p);
    }
    G2PAff q1; q1.x = m2(Fq2::conj(q.x), g12); q1.y = m2(Fq2::conj(q.y), g13);                       // pi(Q)
    miller_add(f, T, q1, p);
    G2PAff q2; q2.x = m2(Fq2::conj(q1.x), g12); q2.y = Fq2::neg(m2(Fq2::conj(q1.y), g13));          // −pi²(Q)
    miller_add(f, T, q2, p);
  }
  out[index] = f;
}

// out[index] = a[index] + k[index]·b[index], affine with reduced coordinates and the identity as (0, 0): pt_scalar_mul_bits over exactly bits[index] <= 256 bits of
// the 8 words k[8·index ..] (the host knows each row's bit length), then one mixed addition, which skips an identity a, doubles when a = k·b and cancels when
// a = −k·b; an identity b, or k = 0, leaves a.  The thread writes its own slot alone.
VZ_HD void g1_lincomb_thread(size_t index, const G1PAff* a, const uint32_t* k, const uint32_t* bits, const G1PAff* b, G1PAff* out) {
  uint32_t s[8];
  for (int i = 0; i < 8; i++) s[i] = k[8 * index + i];
  XYZZ<Fq> acc = pt_scalar_mul_bits(b[index], s, (int)bits[index]);
  const G1PAff p = a[index];
  add_mixed(acc, p);
  out[index] = to_affine(acc);
}

}  // namespace pairing
}  // namespace vz
