// Framing of the two compressed Nova + CycleFold proofs (spartan.hip: vimz_cf_compress, vimz_cf_merged_compress) as a verifier meets them: an
// untrusted sequence of 8-byte words.  Host only, no GPU or field code: header, exact sizes, the records' framing and every bound that later
// indexing relies on.  The elements themselves (below their modulus, points on their curves) are checked where they are read (proof_io.hpp's
// Reader).  tests/native/cf_compressed_parse_check.cpp runs these functions over truncated and garbled blobs under AddressSanitizer + UBSan.
//
// One chain:   {magic, steps, len_z, s_main, t_main, s_cf, t_cf, 0} ‖ z_0 ‖ z_n ‖ U_n (W, E, u, x0, x1) ‖ u_n (W, x0, x1) ‖ cfU_n (W, E, u, x[0..7))
//              ‖ argument(U_n) ‖ argument(u_n, no E opening) ‖ argument(cfU_n)                      — every element four words, a point eight
// Merged:      {magic, words of records} ‖ records (vimz_cf_merged_records' layout) ‖ argument(main accumulator) ‖ argument(CycleFold accumulator)
#pragma once
#include <cstddef>
#include <cstdint>

namespace cfz {

constexpr uint64_t CHAIN_MAGIC = 0x314e534643565aull;        // "ZVCFSN1"
constexpr uint64_t MERGED_MAGIC = 0x31474d4346565aull;       // "ZVFCMG1"
constexpr uint64_t RECORDS_MAGIC = 0x32474d46435a56ull;      // "VZCFMG2": the records' own header (cyclefold_merge.hip)
constexpr uint64_t MAX_SEGMENTS = 4096;
constexpr size_t CF_PUBLIC = 7;                               // public elements of a CycleFold instance
constexpr size_t CHAIN_INSTANCE_WORDS = 4 * (7 + 4 + 5 + CF_PUBLIC);

struct Shapes { uint64_t len_z, n_w1, n_c1, n_w2, n_c2; uint32_t s1, t1, s2, t2; };      // main (F + F') and CycleFold: wires, constraints, log2 of the padded sizes

// words of one argument over a shape padded to 2^s rows and 2^t columns: the two sum-checks with their claims and evalW, the W opening, the E opening
inline size_t arg_words(size_t s, size_t t, bool e) { return 4 * (3 * s + 4 + 2 * t + 1) + 4 * (4 * t + 1) + (e ? 4 * (4 * s + 1) : 0); }

inline size_t chain_words(const Shapes& sh) {
  return 8 + 8 * (size_t)sh.len_z + CHAIN_INSTANCE_WORDS + arg_words(sh.s1, sh.t1, true) + arg_words(sh.s1, sh.t1, false) + arg_words(sh.s2, sh.t2, true);
}
struct ChainFrame { uint64_t steps = 0; size_t z0_at = 0, zn_at = 0, inst_at = 0, args_at = 0; };
// false: malformed (another kind of blob, another circuit's, a wrong length)
inline bool parse_chain(const uint64_t* w, size_t n, const Shapes& sh, ChainFrame* f) {
  if (!w || n < 8 || n != chain_words(sh)) return false;
  if (w[0] != CHAIN_MAGIC || w[2] != sh.len_z || w[3] != sh.s1 || w[4] != sh.t1 || w[5] != sh.s2 || w[6] != sh.t2 || w[7] != 0) return false;
  f->steps = w[1];
  f->z0_at = 8; f->zn_at = 8 + 4 * (size_t)sh.len_z; f->inst_at = 8 + 8 * (size_t)sh.len_z; f->args_at = f->inst_at + CHAIN_INSTANCE_WORDS;
  return true;
}

inline size_t segment_words(const Shapes& sh) { return 1 + 4 * (2 * (size_t)sh.len_z + 7 + 4 + 5 + CF_PUBLIC + 6); }
inline size_t records_words(const Shapes& sh, size_t segments, size_t runs) { return 8 + runs + segments * segment_words(sh) + (runs - 1) * 16; }
struct MergedFrame { size_t rec_at = 0, rec_words = 0, segments = 0, runs = 0, runs_at = 0, segs_at = 0, junctions_at = 0, args_at = 0; };
// the records alone (w[0 .. n) must be exactly them): header against the verifier's shapes, counts, the runs' first segments strictly increasing from 0
inline bool parse_records(const uint64_t* w, size_t n, const Shapes& sh, MergedFrame* f) {
  if (!w || n < 8) return false;
  const uint64_t S = w[1], R = w[7];
  if (w[0] != RECORDS_MAGIC || w[2] != sh.len_z || w[3] != sh.n_w1 || w[4] != sh.n_c1 || w[5] != sh.n_w2 || w[6] != sh.n_c2) return false;
  if (S == 0 || S > MAX_SEGMENTS || R == 0 || R > S) return false;
  if (n != records_words(sh, (size_t)S, (size_t)R)) return false;
  f->segments = (size_t)S; f->runs = (size_t)R;
  f->runs_at = 8; f->segs_at = 8 + (size_t)R; f->junctions_at = f->segs_at + (size_t)S * segment_words(sh);
  uint64_t prev = 0;
  for (size_t k = 0; k < (size_t)R; k++) {
    const uint64_t r0 = w[f->runs_at + k];
    if (r0 >= S || (k == 0 ? r0 != 0 : r0 <= prev)) return false;
    prev = r0;
  }
  return true;
}
inline bool parse_merged(const uint64_t* w, size_t n, const Shapes& sh, MergedFrame* f) {
  if (!w || n < 2 || w[0] != MERGED_MAGIC) return false;
  const uint64_t rw = w[1];
  const size_t args = arg_words(sh.s1, sh.t1, true) + arg_words(sh.s2, sh.t2, true);
  if (n < 2 + args || rw != n - 2 - args) return false;
  if (!parse_records(w + 2, (size_t)rw, sh, f)) return false;
  f->rec_at = 2; f->rec_words = (size_t)rw; f->runs_at += 2; f->segs_at += 2; f->junctions_at += 2; f->args_at = 2 + (size_t)rw;
  return true;
}

}  // namespace cfz
