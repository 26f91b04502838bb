// What ONE thread of the multilinear KZG opening's kernels does (mlkzg.hip: k_mle_fold, k_poly_eval3, k_eval3_sum, k_batch_levels, k_div_carry, k_div_scan, k_div_chunk;
// DESIGN.md §5e), as host-and-device functions of the thread's index over BN254 Fr in Montgomery form: the kernels call them with their thread index,
// tests/native/mlkzg_check.cpp loops them over every index on the CPU.  No HIP in this file beyond VZ_HD.
//
// The levels P_0 .. P_ℓ of the fold lie side by side in ONE buffer: level k has n0 >> k elements and starts at level_offset(n0, k).  A polynomial is its
// coefficient vector, lowest degree first.  A chunk is ML_CHUNK consecutive coefficients, a block ML_BLOCK consecutive chunks; chunk t starts at ML_CHUNK·t, an even
// index.  Every function writes the slots of its own index alone and every loop bound is an argument.
#pragma once
#include <stddef.h>
#include "fp.hpp"

namespace vz {
namespace mlk {

typedef Fp<BnFr> Fr;

constexpr unsigned ML_BLOCK = 256;     // threads of a block of every kernel here, and the chunks one block of the division's carries spans
constexpr unsigned ML_CHUNK = 8;       // coefficients of one thread of the evaluation and of the division (even: a chunk's even and odd coefficients keep their parity)
constexpr int ML_MAX_LOGN = 26;        // 2^26 elements: 2 GiB of levels, 6 GiB of quotients
static_assert(ML_CHUNK % 2 == 0 && (ML_BLOCK & (ML_BLOCK - 1)) == 0, "the even/odd split and the block's tree");

VZ_HD size_t level_offset(size_t n0, unsigned k) { size_t o = 0; for (unsigned i = 0; i < k; i++) o += n0 >> i; return o; }
VZ_HD size_t n_chunks(size_t len) { return (len + ML_CHUNK - 1) / ML_CHUNK; }
VZ_HD size_t n_blocks(size_t len) { return (n_chunks(len) + ML_BLOCK - 1) / ML_BLOCK; }

// base^e over exactly `bits` bits of e, from the top: the trip count comes from the host
VZ_HD Fr pow_bits(const Fr& base, size_t e, int bits) {
  Fr acc = Fr::one();
  for (int b = bits - 1; b >= 0; b--) {
    acc = Fr::sqr(acc);
    if ((e >> b) & 1u) acc = Fr::mul(acc, base);
  }
  return acc;
}

// ---- k_mle_fold: output j of one level, out[j] = in[2j] + x·(in[2j+1] − in[2j]) ------------------------------------------------------------------------------------
VZ_HD void fold_one(size_t j, const Fr* in, const Fr& x, Fr* out) {
  const Fr a = in[2 * j], b = in[2 * j + 1];
  out[j] = Fr::add(a, Fr::mul(x, Fr::sub(b, a)));
}

// ---- k_poly_eval3: chunk t of a polynomial of `len` coefficients at r, −r and r² in ONE walk --------------------------------------------------------------------------
// With w = r²:  P(±r) = Pe(w) ± r·Po(w) over the even and the odd coefficients, and P(r²) = P(w).  The chunk's three Horner sums in w — even part, odd part, all —
// are scaled to their place: the chunk starts at ML_CHUNK·t, so its even and odd parts carry w^(ML_CHUNK/2 · t) = wh^t and the whole w^(ML_CHUNK·t) = (wh^t)².
// out[0] + r·out[1] summed over the chunks is P(r), out[0] − r·out[1] is P(−r), out[2] is P(r²).  bits >= bitlen(t).  A chunk past the end gives zeros.
VZ_HD void eval3_chunk(size_t t, const Fr* a, size_t len, const Fr& w, const Fr& wh, int bits, Fr out[3]) {
  const size_t lo = (size_t)ML_CHUNK * t, hi = lo + ML_CHUNK < len ? lo + ML_CHUNK : len;
  Fr e = Fr::zero(), o = Fr::zero(), f = Fr::zero();
  for (size_t i = hi; i > lo; i--) {
    const Fr c = a[i - 1];
    f = Fr::add(Fr::mul(f, w), c);
    if ((i - 1 - lo) & 1u) o = Fr::add(Fr::mul(o, w), c); else e = Fr::add(Fr::mul(e, w), c);
  }
  if (lo >= len) { out[0] = out[1] = out[2] = Fr::zero(); return; }
  const Fr s = pow_bits(wh, t, bits);
  out[0] = Fr::mul(e, s); out[1] = Fr::mul(o, s); out[2] = Fr::mul(f, Fr::sqr(s));
}
// k_eval3_sum: the three sums over a level's block partials (3 elements a block), then E_r, E_{−r}, E_{r²}
VZ_HD void eval3_finish(const Fr* partials, size_t nblocks, const Fr& r, Fr out[3]) {
  Fr e = Fr::zero(), o = Fr::zero(), f = Fr::zero();
  for (size_t b = 0; b < nblocks; b++) { e = Fr::add(e, partials[3 * b]); o = Fr::add(o, partials[3 * b + 1]); f = Fr::add(f, partials[3 * b + 2]); }
  const Fr ro = Fr::mul(r, o);
  out[0] = Fr::add(e, ro); out[1] = Fr::sub(e, ro); out[2] = f;
}

// ---- k_batch_levels: B[j] = Σ_{k < nlevels, j < n0 >> k} q^k·P_k[j], Horner in q from the highest level that still has a slot j ----------------------------------
VZ_HD void batch_one(size_t j, const Fr* levels, size_t n0, unsigned nlevels, const Fr& q, Fr* out) {
  Fr acc = Fr::zero();
  size_t off = level_offset(n0, nlevels);
  for (unsigned k = nlevels; k-- > 0;) {
    off -= n0 >> k;
    if (j < (n0 >> k)) acc = Fr::add(Fr::mul(acc, q), levels[off + j]);
  }
  out[j] = acc;
}

// ---- the division by (X − u): s_i = b_i + u·s_(i+1) walking down from s_len = 0; the quotient is q_(i−1) = s_i for i >= 1 and s_0 the remainder b(u) -----------------
// 1. k_div_carry: chunk t's carry-out with a zero carry-in, z_t = Σ_{i in chunk} b_i·u^(i − ML_CHUNK·t).  Then s_(ML_CHUNK·t) = z_t + u^ML_CHUNK · s_(ML_CHUNK·(t+1)).
VZ_HD void div_carry(size_t t, const Fr* b, size_t len, const Fr& u, Fr* z) {
  const size_t lo = (size_t)ML_CHUNK * t, hi = lo + ML_CHUNK < len ? lo + ML_CHUNK : len;
  Fr acc = Fr::zero();
  for (size_t i = hi; i > lo; i--) acc = Fr::add(Fr::mul(acc, u), b[i - 1]);
  z[t] = acc;
}
// 2. k_div_scan, one workgroup: (a) block `blk`'s carry-out with a zero carry-in over its chunks' z, the same recurrence with uc = u^ML_CHUNK;
VZ_HD void div_block_carry(size_t blk, const Fr* z, size_t nchunks, const Fr& uc, Fr* zb) {
  const size_t lo = (size_t)ML_BLOCK * blk, hi = lo + ML_BLOCK < nchunks ? lo + ML_BLOCK : nchunks;
  Fr acc = Fr::zero();
  for (size_t t = hi; t > lo; t--) acc = Fr::add(Fr::mul(acc, uc), z[t - 1]);
  zb[blk] = acc;
}
//    (b) ONE thread: the carry into every block, walking the blocks down with ubc = uc^ML_BLOCK;
VZ_HD void div_block_scan(const Fr* zb, size_t nblocks, const Fr& ubc, Fr* ib) {
  Fr acc = Fr::zero();
  for (size_t b = nblocks; b > 0; b--) { ib[b - 1] = acc; acc = Fr::add(Fr::mul(acc, ubc), zb[b - 1]); }
}
//    (c) block `blk` again with its carry-in: the carry into each of its chunks.
VZ_HD void div_chunk_carries(size_t blk, const Fr* z, size_t nchunks, const Fr& uc, const Fr* ib, Fr* cin) {
  const size_t lo = (size_t)ML_BLOCK * blk, hi = lo + ML_BLOCK < nchunks ? lo + ML_BLOCK : nchunks;
  Fr acc = ib[blk];
  for (size_t t = hi; t > lo; t--) { cin[t - 1] = acc; acc = Fr::add(Fr::mul(acc, uc), z[t - 1]); }
}
// 3. k_div_chunk: chunk t again with its carry-in: quot[i − 1] = s_i for the chunk's i >= 1 (len − 1 coefficients in all), and chunk 0 writes *rem = s_0
VZ_HD void div_chunk(size_t t, const Fr* b, size_t len, const Fr& u, const Fr* cin, Fr* quot, Fr* rem) {
  const size_t lo = (size_t)ML_CHUNK * t, hi = lo + ML_CHUNK < len ? lo + ML_CHUNK : len;
  Fr acc = cin[t];
  for (size_t i = hi; i > lo; i--) {
    acc = Fr::add(Fr::mul(acc, u), b[i - 1]);
    if (i - 1) quot[i - 2] = acc; else *rem = acc;
  }
}

}  // namespace mlk
}  // namespace vz
