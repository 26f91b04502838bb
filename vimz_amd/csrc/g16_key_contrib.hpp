// Further delta contributions to a saved decider key (vimz_decider_key_contribute / _verify_contributions) — the HOST side: where the points
// of a key blob lie, and the record a contributor leaves.  Phase 2 of a Groth16 ceremony (what snarkjs calls `zkey contribute` / `zkey verify`) on this project's
// own key layout; the record is this project's own format too, NOT a section of snarkjs's `.zkey` container.  No HIP in this file: tests/native/key_contrib_check.cpp
// runs it under the host sanitizers.
//
// A contribution with delta' turns a key of delta into the key of delta·delta': delta1, delta2 <- delta'·(delta1, delta2), every point of the l and h queries <-
// (1/delta')·point, every other byte as it was.  The record (RECORD_WORDS little-endian u64 words, points canonical): magic "VG16CTR1", delta1 after (8), delta2 after
// (16), T (8), z (4), a Schnorr proof of knowledge of delta' over the base delta1_before:  T = k·delta1_before,  c = SHA3-256(tag ‖ the key's seven header words and
// pp_hash ‖ delta1_before ‖ delta1_after ‖ delta2_after ‖ T) read as groth16.hip's fr_from_hash reads a digest (the top byte cleared),  z = k + c·delta' mod r;  the
// check is z·delta1_before = T + c·delta1_after.  delta1_before is the previous record's delta1, or the origin key's: that chains the records.
#pragma once
#include <cstring>
#include "g16_point_stage.hpp"
#include "aug/augmented.hpp"

namespace vz {
namespace keyc {

typedef Fp<BnFr> Fr;
typedef Fp<BnFq> Fq;
using pairing::Fq2;
typedef Affine<Fq> G1A;
typedef Affine<Fq2> G2A;

constexpr uint64_t KEY_MAGIC = 0x3259454b36314756ull;         // "VG16KEY2": the key at rest (groth16.hip: vimz_decider_key_save)
constexpr uint64_t RECORD_MAGIC = 0x3152544336314756ull;      // "VG16CTR1"
constexpr size_t RECORD_WORDS = 37, REC_DELTA1 = 1, REC_DELTA2 = 9, REC_T = 25, REC_Z = 33;
// words of a key blob: the seven header words and pp_hash, the KZG key (16), alpha1, beta1, delta1 (8 each), beta2, gamma2, delta2 (16 each), then IC
constexpr size_t KEY_HEAD_WORDS = 11, KEY_DELTA1 = 43, KEY_DELTA2 = 83, KEY_IC = 99;
static const char RECORD_TAG[] = "vimz-decider-key-contribution";

// where the l and h queries lie in a blob: side by side, n_lh = (m − n_pub − 1) + (n − 1) points of 8 words from word off_lh
struct KeyLayout { size_t words = 0, off_lh = 0, n_lh = 0; };
// NULL: fine; otherwise what is wrong.  Every size is read from the blob's own header and checked against its length before anything is indexed.
inline const char* key_layout(const void* blob, size_t len, KeyLayout* L) {
  if (!blob || (len & 7) || len / 8 < KEY_IC) return "not a decider key";
  uint64_t w[7]; memcpy(w, blob, sizeof(w));
  const uint64_t m = w[1], n_pub = w[2], n = w[4];
  if (w[0] != KEY_MAGIC || w[6] > 1) return "not a decider key";
  if (m >= ((uint64_t)1 << 31) || n >= ((uint64_t)1 << 31) || !n || n_pub >= m) return "not a decider key";
  const uint64_t n_l = m - n_pub - 1, n_h = n - 1;
  const uint64_t words = KEY_IC + 8 * (n_pub + 1) + 8 * (2 * m + n_l + n_h) + 16 * m;      // (below 2^38: no overflow)
  if (words != len / 8) return "wrong length";
  L->words = (size_t)words; L->off_lh = (size_t)(KEY_IC + 8 * (n_pub + 1) + 16 * m); L->n_lh = (size_t)(n_l + n_h);
  return nullptr;
}

inline bool get_fq(const uint64_t* src, Fq* out) { Fq c; memcpy(c.v, src, 32); if (!c.is_reduced()) return false; *out = Fq::to_mont(c); return true; }
inline void put_fq(uint64_t* dst, const Fq& mont) { const Fq c = Fq::from_mont(mont); memcpy(dst, c.v, 32); }
inline bool get_g1(const uint64_t* src, G1A* p) { return get_fq(src, &p->x) && get_fq(src + 4, &p->y); }
inline bool get_g2(const uint64_t* src, G2A* p) { return get_fq(src, &p->x.c0) && get_fq(src + 4, &p->x.c1) && get_fq(src + 8, &p->y.c0) && get_fq(src + 12, &p->y.c1); }
inline void put_g1(uint64_t* dst, const G1A& p) { put_fq(dst, p.x); put_fq(dst + 4, p.y); }
inline void put_g2(uint64_t* dst, const G2A& p) { put_fq(dst, p.x.c0); put_fq(dst + 4, p.x.c1); put_fq(dst + 8, p.y.c0); put_fq(dst + 12, p.y.c1); }
inline bool same_point(const G1A& p, const G1A& q) { return p.x.eq(q.x) && p.y.eq(q.y); }

// the challenge of a record, as canonical words below r: head = the key's first KEY_HEAD_WORDS words, delta1_before 8 canonical words
inline Fr record_challenge(const uint64_t* head, const uint64_t* delta1_before, const uint64_t* record) {
  aug::Sha3 h;
  h.update(RECORD_TAG, sizeof(RECORD_TAG) - 1); h.update(head, 8 * KEY_HEAD_WORDS); h.update(delta1_before, 64);
  h.update(record + REC_DELTA1, 8 * (REC_Z - REC_DELTA1));      // delta1 after, delta2 after, T
  uint8_t d[32]; h.finish(d); d[31] = 0;
  Fr c; memcpy(c.v, d, 32);
  return c;
}

// The contributor's side: delta1, delta2 (Montgomery coordinates) become delta'·delta1, delta'·delta2, and `record` is filled.  delta, k: Montgomery, delta non-zero;
// both are the caller's secrets and the caller wipes them — the one intermediate that determines delta' (c·delta') is wiped here.
inline void make_record(const uint64_t* head, G1A* delta1, G2A* delta2, const Fr& delta, const Fr& k, uint64_t* record) {
  uint64_t before[8]; put_g1(before, *delta1);
  Fr dc = Fr::from_mont(delta), kc = Fr::from_mont(k);
  const G1A T = to_affine(pt_scalar_mul(*delta1, kc.v));
  *delta1 = to_affine(pt_scalar_mul(*delta1, dc.v)); *delta2 = to_affine(pt_scalar_mul(*delta2, dc.v));
  record[0] = RECORD_MAGIC;
  put_g1(record + REC_DELTA1, *delta1); put_g2(record + REC_DELTA2, *delta2); put_g1(record + REC_T, T);
  Fr cd = Fr::mul(Fr::to_mont(record_challenge(head, before, record)), delta);
  const Fr z = Fr::from_mont(Fr::add(cd, k));
  memcpy(record + REC_Z, z.v, 32);
  explicit_bzero(&cd, sizeof(cd)); explicit_bzero(&dc, sizeof(dc)); explicit_bzero(&kc, sizeof(kc));
}

// the verifier's side of the proof of knowledge: z·delta1_before = T + c·delta1_after (points already range- and curve-checked; a z not below r fails)
inline bool record_knowledge(const uint64_t* head, const uint64_t* delta1_before_words, const G1A& delta1_before, const G1A& delta1_after, const G1A& T, const uint64_t* record) {
  Fr z; memcpy(z.v, record + REC_Z, 32);
  if (!z.is_reduced()) return false;
  const Fr c = record_challenge(head, delta1_before_words, record);
  XYZZ<Fq> rhs = pt_scalar_mul(delta1_after, c.v);
  add_mixed(rhs, T);
  return same_point(to_affine(pt_scalar_mul(delta1_before, z.v)), to_affine(rhs));
}

}  // namespace keyc
}  // namespace vz
