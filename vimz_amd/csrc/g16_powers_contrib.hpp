// A contribution to a powers-of-tau string (vimz_powers_contribute / vimz_powers_verify_contributions) — the HOST side: the record a
// contributor leaves and its three proofs of knowledge.  Phase 1 of a ceremony (what snarkjs calls `powersoftau contribute` / `powersoftau verify`) on the arrays
// iden3.read_ptau hands over; the record is this project's own format, NOT snarkjs's transcript.  No HIP in this file: tests/native/powers_contrib_check.cpp runs it
// under the host sanitizers.
//
// A contribution with (tau', alpha', beta') turns the string of (tau, alpha, beta) into the string of (tau·tau', alpha·alpha', beta·beta'): tau_g1[k], tau_g2[k] <-
// tau'^k·(..), alpha_g1[k] <- alpha'·tau'^k·alpha_g1[k], beta_g1[k] <- beta'·tau'^k·beta_g1[k], beta_g2 <- beta'·beta_g2.  The record (RECORD_WORDS little-endian
// u64 words, points canonical): magic "VPOTCTR1"; A_tau, A_alpha, A_beta — tau_g1[1], alpha_g1[0], beta_g1[0] AFTER the contribution (8 words each); T_tau, T_alpha,
// T_beta (8 each); z_tau, z_alpha, z_beta (4 each).  Each secret s' of index i in (tau', alpha', beta') gets a Schnorr proof over the base B_s, the same point BEFORE
// the contribution:  T_s = k_s·B_s,  c_s = SHA3-256(tag ‖ i as a 64-bit word ‖ B_tau ‖ B_alpha ‖ B_beta ‖ A_tau ‖ A_alpha ‖ A_beta ‖ T_s) read as groth16.hip's
// fr_from_hash reads a digest (the top byte cleared),  z_s = k_s + c_s·s' mod r;  the check is z_s·B_s = T_s + c_s·A_s.  B of record j is A of record j − 1, or the
// origin's three points: that chains the records.
#pragma once
#include "g16_key_contrib.hpp"

namespace vz {
namespace powc {

using keyc::Fq; using keyc::Fr; using keyc::G1A; using keyc::G2A;
using keyc::get_g1; using keyc::put_g1; using keyc::same_point;

constexpr uint64_t RECORD_MAGIC = 0x31525443544f5056ull;      // "VPOTCTR1"
constexpr size_t RECORD_WORDS = 61, REC_A = 1, REC_T = 25, REC_Z = 49;
static const char RECORD_TAG[] = "vimz-powers-of-tau-contribution";

// NULL: `len` bytes are *n whole records, each with the magic; otherwise what is wrong, *n then the first bad record.  Nothing past len is read.
inline const char* powers_records_layout(const void* records, size_t len, size_t* n) {
  *n = 0;
  if (len % (8 * RECORD_WORDS) || (len && !records)) return "records are 488 bytes each";
  for (size_t j = 0; j < len / (8 * RECORD_WORDS); j++) {
    uint64_t magic; memcpy(&magic, (const uint8_t*)records + 8 * RECORD_WORDS * j, 8);
    if (magic != RECORD_MAGIC) { *n = j; return "not a contribution record"; }
  }
  *n = len / (8 * RECORD_WORDS);
  return nullptr;
}

// the challenge of secret `which` (0 tau', 1 alpha', 2 beta') of a record, as canonical words below r; before: B_tau, B_alpha, B_beta as 24 canonical words
inline Fr powers_record_challenge(unsigned which, const uint64_t* before, const uint64_t* record) {
  aug::Sha3 h;
  const uint64_t index = which;
  h.update(RECORD_TAG, sizeof(RECORD_TAG) - 1); h.update(&index, 8); h.update(before, 8 * 24);
  h.update(record + REC_A, 8 * 24); h.update(record + REC_T + 8 * which, 64);
  uint8_t d[32]; h.finish(d); d[31] = 0;
  Fr c; memcpy(c.v, d, 32);
  return c;
}

// The contributor's side: before[s] (Montgomery coordinates) is B_s; `record` is filled with A_s = s'·B_s, T_s = k_s·B_s and z_s.  secrets, nonces: Montgomery,
// the secrets non-zero; they are the caller's and the caller wipes them — the intermediates that determine them are wiped here.
inline void make_powers_record(const G1A before[3], const Fr secrets[3], const Fr nonces[3], uint64_t* record) {
  uint64_t b[24];
  for (int s = 0; s < 3; s++) put_g1(b + 8 * s, before[s]);
  record[0] = RECORD_MAGIC;
  Fr canon[2];
  for (int s = 0; s < 3; s++) {
    canon[0] = Fr::from_mont(secrets[s]); canon[1] = Fr::from_mont(nonces[s]);
    put_g1(record + REC_A + 8 * s, to_affine(pt_scalar_mul(before[s], canon[0].v)));
    put_g1(record + REC_T + 8 * s, to_affine(pt_scalar_mul(before[s], canon[1].v)));
  }
  for (unsigned s = 0; s < 3; s++) {      // (every A is part of every challenge: after the loop above)
    canon[0] = Fr::mul(Fr::to_mont(powers_record_challenge(s, b, record)), secrets[s]);
    const Fr z = Fr::from_mont(Fr::add(canon[0], nonces[s]));
    memcpy(record + REC_Z + 4 * s, z.v, 32);
  }
  explicit_bzero(canon, sizeof(canon));
}

// The verifier's side: bit s of the result is set where the proof of secret s FAILS — z_s·B_s = T_s + c_s·A_s (points already range- and curve-checked; a z not
// below r fails).  before_words: B's 24 canonical words, before / after / T the same points in Montgomery coordinates.
inline unsigned powers_record_knowledge(const uint64_t* before_words, const G1A before[3], const G1A after[3], const G1A T[3], const uint64_t* record) {
  unsigned failed = 0;
  for (unsigned s = 0; s < 3; s++) {
    Fr z; memcpy(z.v, record + REC_Z + 4 * s, 32);
    if (!z.is_reduced()) { failed |= 1u << s; continue; }
    const Fr c = powers_record_challenge(s, before_words, record);
    XYZZ<Fq> rhs = pt_scalar_mul(after[s], c.v);
    add_mixed(rhs, T[s]);
    if (!same_point(to_affine(pt_scalar_mul(before[s], z.v)), to_affine(rhs))) failed |= 1u << s;
  }
  return failed;
}

}  // namespace powc
}  // namespace vz
