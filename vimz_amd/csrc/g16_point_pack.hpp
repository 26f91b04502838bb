// Packed curve points (vimz_points_pack / _unpack, vimz_decider_key_pack / _unpack): x and one bit of y, y recovered as a square root of x³ + b
// when the point is read — half the bytes, and a point that unpacks is on its curve by construction.  What ONE thread of g16_point_pack.hip's kernels does
// (k_points_pack, k_points_unpack), as host-and-device functions of the thread's index, and the HOST side of a packed key: where its points lie.  The kernels call
// the functions with their thread index, tests/native/point_pack_check.cpp loops them over every index on the CPU under the host sanitizers.  No HIP in this file
// beyond VZ_HD.
//
// The encoding (this project's own; canonical: ONE encoding per point).  G1: the 4 little-endian 64-bit words of x as an integer below q (254 bits, so the two top
// bits of word 3 are free); bit 63 of word 3 is INF, bit 62 SIGN = 1 iff the canonical y is greater than (q − 1)/2; the identity is INF alone.  G2: x.c0 (4 words), then
// x.c1 (4 words) with the flags in the top bits of word 7 — the top two bits of word 3 must be 0; SIGN = 1 iff y is the larger of (y, −y): y.c1 > (q − 1)/2 when
// y.c1 != 0, y.c0 > (q − 1)/2 otherwise.  The unpacked side is the library's affine layout in either form (canonical or Montgomery words, the identity as zeros);
// the packed side is always canonical.  y = 0 is on neither curve (both group orders are odd), so −y != y wherever a root exists.
// Membership of G2's subgroup of order r is NOT judged here: a point that unpacks is on the twist, no more.
#pragma once
#include "../../include/vimz_hip.h"
#include "g16_key_contrib.hpp"

namespace vz {

constexpr uint32_t PK_COORD = VIMZ_PACK_COORD, PK_FLAGS = VIMZ_PACK_FLAGS, PK_OFF_CURVE = VIMZ_PACK_OFF_CURVE;      // a point's findings
constexpr uint32_t PK_INF = 0x80000000u, PK_SIGN = 0x40000000u, PK_TOP = PK_INF | PK_SIGN;      // in the last 32-bit word of a packed point

static_assert((BnFq::MOD.w[0] & 3u) == 3u, "the square roots below are those of a prime 3 mod 4");
constexpr U256 ct_quarter_up(const U256& q) {      // (q + 1)/4
  U256 t{}; uint64_t c = 1;
  for (int i = 0; i < 8; i++) { const uint64_t s = (uint64_t)q.w[i] + c; t.w[i] = (uint32_t)s; c = s >> 32; }
  U256 r{};
  for (int i = 0; i < 8; i++) r.w[i] = (t.w[i] >> 2) | (i < 7 ? t.w[i + 1] << 30 : 0u);
  return r;
}
constexpr U256 ct_half_up(const U256& q) {         // (q + 1)/2 = 1/2 mod q
  U256 r{}; uint64_t c = 1;
  for (int i = 0; i < 8; i++) { const uint64_t s = (uint64_t)((q.w[i] >> 1) | (i < 7 ? q.w[i + 1] << 31 : 0u)) + c; r.w[i] = (uint32_t)s; c = s >> 32; }
  return r;
}
constexpr int PK_SQRT_BITS = ct_bits(ct_quarter_up(BnFq::MOD));      // 252

namespace pack {
typedef Fp<BnFq> Fq;
using pairing::Fq2;

// a^((q+1)/4), Montgomery in and out: square and multiply over the exponent's PK_SQRT_BITS bits — a constant, so the lanes of a wave walk it together
VZ_HD Fq fq_pow_quarter(const Fq& a) {
  constexpr U256 E = ct_quarter_up(BnFq::MOD);
  uint32_t e[8];
  for (int i = 0; i < 8; i++) e[i] = E.w[i];
  Fq acc = Fq::one();
#pragma unroll 1
  for (int i = PK_SQRT_BITS - 1; i >= 0; i--) {
    acc = Fq::sqr(acc);
    if ((e[i >> 5] >> (i & 31)) & 1u) acc = Fq::mul(acc, a);
  }
  return acc;
}

// canonical c > (q − 1)/2
VZ_HD bool fq_is_larger(const Fq& c) {
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint32_t h = (BnFq::MOD.w[i] >> 1) | (i < 7 ? BnFq::MOD.w[i + 1] << 31 : 0u);      // (q − 1)/2 = q >> 1
    const uint64_t d = (uint64_t)h - c.v[i] - br; br = (d >> 32) & 1;
  }
  return br != 0;
}
VZ_HD bool fq_is_larger(const Fq2& c) { return c.c1.is_zero() ? fq_is_larger(c.c0) : fq_is_larger(c.c1); }

// *root = a square root of a (Montgomery) and true, or false: t = a^((q+1)/4) squares to a or to −a
VZ_HD bool fq_sqrt(const Fq& a, Fq* root) {
  const Fq t = fq_pow_quarter(a);
  *root = t;
  return Fq::sqr(t).eq(a);
}

// The same over Fq2 = Fq[i]/(i² + 1).  For a = a0 + a1·i with a1 != 0: s = (a0² + a1²)^((q+1)/4), d = (a0 + s)/2, t = d^((q+1)/4), w = a1/(2t); the root is (t, w) if
// t² = d, else (w, t) — t² = −d then, and the other candidate (a0 − s)/2 equals w²: no second exponentiation, and the trip count does not depend on the value.
// For a1 = 0: t = a0^((q+1)/4), the root is (t, 0) if t² = a0, else (0, t).  a is a square iff the root squared is a — that one comparison decides (a norm that is
// no square, or t = 0 whose inverse is taken as 0, leaves a root that fails it).  Three exponentiations with the inversion.
VZ_HD bool fq2_sqrt(const Fq2& a, Fq2* root) {
  Fq2 r;
  if (a.c1.is_zero()) {
    const Fq t = fq_pow_quarter(a.c0);
    if (Fq::sqr(t).eq(a.c0)) { r.c0 = t; r.c1 = Fq::zero(); } else { r.c0 = Fq::zero(); r.c1 = t; }
  } else {
    const Fq s = fq_pow_quarter(Fq::add(Fq::sqr(a.c0), Fq::sqr(a.c1)));
    constexpr U256 H = ct_half_up(BnFq::MOD);
    Fq half;
    for (int i = 0; i < 8; i++) half.v[i] = H.w[i];
    half = Fq::to_mont(half);                                                         // 1/2
    const Fq d = Fq::mul(Fq::add(a.c0, s), half);
    const Fq t = fq_pow_quarter(d);
    const Fq w = Fq::mul(a.c1, Fq::pow_pm2(Fq::dbl(t)));
    if (Fq::sqr(t).eq(d)) { r.c0 = t; r.c1 = w; } else { r.c0 = w; r.c1 = t; }
  }
  *root = r;
  return Fq2::sqr(r).eq(a);
}
VZ_HD bool fq_sqrt(const Fq2& a, Fq2* root) { return fq2_sqrt(a, root); }

}  // namespace pack

// packed[index] and flags[index] from points[index], whose words are canonical, or Montgomery when `mont`.  b: the curve's constant in Montgomery form.  A coordinate
// not below q (y included): PK_COORD; y² != x³ + b: PK_OFF_CURVE; zeros: the identity, INF alone.  A point with a finding leaves zeros in its slot.  The thread reads
// its own point and writes its own two slots alone.
template <class F>
VZ_HD void pt_pack(size_t index, const Affine<F>* points, bool mont, const F& b, uint32_t* packed, uint32_t* flags) {
  using pack::Fq;
  constexpr int NC = sizeof(F) / sizeof(Fq), PW = 8 * NC;      // coordinates of Fq in an element of F; 32-bit words of a packed point
  Affine<F> p = points[index];
  Fq* c = (Fq*)&p;                                             // x's coordinates, then y's (every loop below is unrolled: the indices are constants)
  bool below = true, zero = true;
#pragma unroll
  for (int k = 0; k < 2 * NC; k++) { below = below && c[k].is_reduced(); zero = zero && c[k].is_zero(); }
  uint32_t f = 0, top = 0;
  if (!below) f = PK_COORD;
  else if (zero) top = PK_INF;
  else {
    if (!mont) {
#pragma unroll
      for (int k = 0; k < 2 * NC; k++) c[k] = Fq::to_mont(c[k]);
    }
    if (!F::sqr(p.y).eq(F::add(F::mul(F::sqr(p.x), p.x), b))) f = PK_OFF_CURVE;
    else {
#pragma unroll
      for (int k = 0; k < 2 * NC; k++) c[k] = Fq::from_mont(c[k]);
      if (pack::fq_is_larger(p.y)) top = PK_SIGN;
    }
  }
  const bool keep = !f && !(top & PK_INF);                     // x is written; zeros otherwise
  flags[index] = f;
#pragma unroll
  for (int k = 0; k < NC; k++) {
#pragma unroll
    for (int i = 0; i < 8; i++) packed[(size_t)PW * index + 8 * k + i] = (keep ? c[k].v[i] : 0u) | (8 * k + i == PW - 1 ? top : 0u);
  }
}

// points[index] and flags[index] from packed[index]; the point's words canonical, or Montgomery when `mont`.  INF together with any other bit, or a stray top bit in
// a G2 word 3: PK_FLAGS; a coordinate not below q (the flag bits apart): PK_COORD; x³ + b no square: PK_OFF_CURVE.  After the root, y is negated when its sign
// disagrees with SIGN.  A point with a finding leaves zeros in its slot.  The thread reads its own packed point and writes its own two slots alone.
template <class F>
VZ_HD void pt_unpack(size_t index, const uint32_t* packed, const F& b, bool mont, Affine<F>* points, uint32_t* flags) {
  using pack::Fq;
  constexpr int NC = sizeof(F) / sizeof(Fq), PW = 8 * NC;
  Affine<F> p;
  Fq* c = (Fq*)&p;                                             // x's coordinates, then y's (every loop below is unrolled: the indices are constants)
  uint32_t f = 0, any = 0;
#pragma unroll
  for (int k = 0; k < NC; k++) {
#pragma unroll
    for (int i = 0; i < 8; i++) c[k].v[i] = packed[(size_t)PW * index + 8 * k + i];
    c[NC + k] = Fq::zero();
  }
  const uint32_t top = c[NC - 1].v[7] & PK_TOP;
  c[NC - 1].v[7] &= ~PK_TOP;
  if (NC == 2) { if (c[0].v[7] & PK_TOP) f |= PK_FLAGS; c[0].v[7] &= ~PK_TOP; }
  bool below = true;
#pragma unroll
  for (int k = 0; k < NC; k++) { below = below && c[k].is_reduced(); any |= c[k].is_zero() ? 0u : 1u; }
  if (top & PK_INF) { if (any || (top & PK_SIGN)) f |= PK_FLAGS; }
  else {
    if (!below) f |= PK_COORD;
    if (!f) {
      const F xc = p.x;                                        // the canonical words
#pragma unroll
      for (int k = 0; k < NC; k++) c[k] = Fq::to_mont(c[k]);
      F y;
      if (!pack::fq_sqrt(F::add(F::mul(F::sqr(p.x), p.x), b), &y)) f = PK_OFF_CURVE;
      else {
        F yc = y;
        Fq* cy = (Fq*)&yc;
#pragma unroll
        for (int k = 0; k < NC; k++) cy[k] = Fq::from_mont(cy[k]);
        if (pack::fq_is_larger(yc) != (bool)(top & PK_SIGN)) { y = F::neg(y); yc = F::neg(yc); }      // (−y canonical is the negation of the canonical y)
        p.y = mont ? y : yc;
        if (!mont) p.x = xc;
      }
    }
  }
  flags[index] = f;
  if (f || (top & PK_INF)) {
#pragma unroll
    for (int k = 0; k < 2 * NC; k++) c[k] = Fq::zero();
  }
  points[index] = p;
}

// ---- the packed key at rest: the host side ----
namespace keyc {

constexpr uint64_t PACKED_KEY_MAGIC = 0x314b504b36314756ull;      // "VG16KPK1"
// A packed key: the magic, words 1..10 of the key verbatim (m, n_pub, n_c, n, len_z, mode, pp_hash), then every point of the key in the key's own order, packed:
// the KZG [tau]G2, alpha1, beta1, delta1, beta2, gamma2, delta2, IC, a, b1, l, h, b2.  The fixed points, then ONE run of G1 (IC‖a‖b1‖l‖h) and ONE run of G2 (b2).
constexpr size_t KEY_KZG = 11, KEY_ALPHA1 = 27, KEY_BETA2 = 51;                     // words of the key's fixed points (KEY_IC: the first run)
constexpr size_t PKEY_KZG = 11, PKEY_ALPHA1 = 19, PKEY_BETA2 = 31, PKEY_IC = 55;    // ... and of the packed key's
// the two runs of a key of either kind, in words of the key and of the packed key
struct KeyRuns { size_t n_g1 = 0, n_g2 = 0, off_g1 = 0, off_g2 = 0, words = 0, poff_g1 = 0, poff_g2 = 0, pwords = 0; };
inline void key_runs(uint64_t m, uint64_t n_pub, uint64_t n, KeyRuns* R) {
  R->n_g1 = (size_t)((n_pub + 1) + 2 * m + (m - n_pub - 1) + (n - 1)); R->n_g2 = (size_t)m;
  R->off_g1 = KEY_IC; R->off_g2 = KEY_IC + 8 * R->n_g1; R->words = R->off_g2 + 16 * R->n_g2;
  R->poff_g1 = PKEY_IC; R->poff_g2 = PKEY_IC + 4 * R->n_g1; R->pwords = R->poff_g2 + 8 * R->n_g2;
}
// NULL: fine; otherwise what is wrong.  As key_layout: every size is read from the blob's own header and checked against its length before anything is indexed.
inline const char* packed_key_layout(const void* blob, size_t len, KeyRuns* R) {
  if (!blob || (len & 7) || len / 8 < PKEY_IC) return "not a packed decider key";
  uint64_t w[7]; memcpy(w, blob, sizeof(w));
  const uint64_t m = w[1], n_pub = w[2], n = w[4];
  if (w[0] != PACKED_KEY_MAGIC || w[6] > 1) return "not a packed decider key";
  if (m >= ((uint64_t)1 << 31) || n >= ((uint64_t)1 << 31) || !n || n_pub >= m) return "not a packed decider key";
  key_runs(m, n_pub, n, R);                                                        // (below 2^38: no overflow)
  if (R->pwords != len / 8) return "wrong length";
  return nullptr;
}
// the same for a key as vimz_decider_key_save writes it (key_layout's checks)
inline const char* plain_key_runs(const void* blob, size_t len, KeyRuns* R) {
  KeyLayout L;
  if (const char* why = key_layout(blob, len, &L)) return why;
  uint64_t w[5]; memcpy(w, blob, sizeof(w));
  key_runs(w[1], w[2], w[4], R);
  return R->words == L.words ? nullptr : "wrong length";
}

}  // namespace keyc
}  // namespace vz
