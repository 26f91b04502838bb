// What ONE thread of the point transform does (g16_powers.hip: k_pt_twiddles, k_pt_bitrev, k_pt_stage), as host-and-device functions of the thread's index:
// the kernels call them with their thread index, tests/native/pt_stage_check.cpp loops them over every index on the CPU — the algorithm is checked there
// before a launch is.  No HIP in this file beyond VZ_HD.
//
// The transform out_j = Σ_k w^(jk)·P_k over n = 2^logn points of a group of order r is radix 2, decimation in time: the bit reversal, then logn stages of n/2
// butterflies (half = 1, 2, .., n/2).  Butterfly `index` of a stage works on the slots lo = 2·half·(index / half) + index % half and lo + half alone, so a stage
// in place is race-free with one thread per butterfly, and the stages are sequenced by whoever launches them.
#pragma once
#include "g16_colsum_plan.hpp"
#include "pairing.hpp"

namespace vz {

constexpr unsigned PT_BLOCK = 64;      // threads of a block of k_scale_points and of the transform's kernels: one wave
constexpr int PT_SCALAR_BITS = 254;    // r < 2^254

// k·p by double-and-add from the top bit over the XYZZ accumulator with the affine p as the addend; k: 8 canonical words below r
template <class F>
VZ_HD XYZZ<F> pt_scalar_mul(const Affine<F>& p, const uint32_t* k) {
  XYZZ<F> acc = XYZZ<F>::identity();
#pragma unroll 1
  for (int b = PT_SCALAR_BITS - 1; b >= 0; b--) {
    acc = dbl(acc);                                     // (the identity until the scalar's top bit: a compare and a branch)
    if ((k[b >> 5] >> (b & 31)) & 1u) add_mixed(acc, p);
  }
  return acc;
}

// entry `index` of the twiddle table, w^index as canonical words (the scalars pt_scalar_mul walks), for index < n/2 = 2^bits; w in Montgomery form.  Square and
// multiply over the index's `bits` bits: the trip count comes from the host.
VZ_HD void pt_twiddle(size_t index, int bits, const Fp<BnFr>& w, uint32_t* twiddles) {
  typedef Fp<BnFr> Fr;
  Fr acc = Fr::one();
  for (int b = bits - 1; b >= 0; b--) {
    acc = Fr::sqr(acc);
    if ((index >> b) & 1u) acc = Fr::mul(acc, w);
  }
  acc = Fr::from_mont(acc);
  for (int i = 0; i < 8; i++) twiddles[8 * index + i] = acc.v[i];
}

// the bit reversal as a swap done once per pair: the thread of the lower index moves both
template <class F>
VZ_HD void pt_bitrev_swap(size_t index, int logn, Affine<F>* points) {
  size_t r = 0;
  for (int b = 0; b < logn; b++) r = (r << 1) | ((index >> b) & 1u);
  if (index >= r) return;
  uint32_t *a = (uint32_t*)(points + index), *b = (uint32_t*)(points + r);      // word by word: no copy of a point on the stack
  for (size_t i = 0; i < sizeof(Affine<F>) / 4; i++) { const uint32_t t = a[i]; a[i] = b[i]; b[i] = t; }
}

// butterfly `index` (< n/2) of the stage of that `half`: (u, v) -> (u + t, u − t), t = w·v, w = twiddles[(index % half)·(n/2 / half)].  The twiddle one,
// the identity on either side, u = t (a doubling) and u = −t (a cancellation) take no path of their own: add_mixed and dbl handle them.
template <class F>
VZ_HD void pt_butterfly(size_t index, size_t half, size_t n_half, Affine<F>* points, const uint32_t* twiddles) {
  const size_t j = index % half, lo = 2 * half * (index / half) + j, hi = lo + half;
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = twiddles[8 * (j * (n_half / half)) + i];
  XYZZ<F> sum = pt_scalar_mul(points[hi], w);           // t
  XYZZ<F> dif = sum; dif.Y = F::neg(sum.Y);             // −t
  const Affine<F> u = points[lo];                       // (read after the multiplication: it need not live through it)
  add_mixed(sum, u);
  add_mixed(dif, u);
  points[lo] = to_affine(sum);
  points[hi] = to_affine(dif);
}

// ---- the column sums and the h query of the set-up (k_col_runs, k_point_diff): what ONE thread does, looped on the CPU by tests/native/colsum_plan_check.cpp ----

// k·p over exactly `bits` bits of k (the host's plan knows bitlen(k)): the top bit's doubling of the identity is a compare and a branch
template <class F>
VZ_HD XYZZ<F> pt_scalar_mul_bits(const Affine<F>& p, const uint32_t* k, int bits) {
  XYZZ<F> acc = XYZZ<F>::identity();
#pragma unroll 1
  for (int b = bits - 1; b >= 0; b--) {
    acc = dbl(acc);
    if ((k[b >> 5] >> (b & 31)) & 1u) add_mixed(acc, p);
  }
  return acc;
}

// run `index` of a level of g16_colsum_plan.hpp's plan: S = Σ ±src[..] over the run's entries (level 0: `entries` names point and sign; above: entries is NULL and
// src the previous level's partials), then |c|·S when |c| is not one, written as a canonical affine point to the run's own slot — of `partials`, or of `out`.
// add_mixed skips an identity, doubles equal points and restarts after opposite ones.  Every bound (len, bits) is the plan's; nothing another thread writes is read.
template <class F>
VZ_HD void colsum_run(size_t index, const ColsumRun* runs, const uint32_t* entries, const uint32_t* mags, const Affine<F>* src, Affine<F>* partials, Affine<F>* out) {
  const ColsumRun r = runs[index];
  XYZZ<F> acc = XYZZ<F>::identity();
#pragma unroll 1
  for (uint32_t k = 0; k < r.len; k++) {
    Affine<F> p;
    if (entries) {
      const uint32_t e = entries[r.off + k];
      p = src[e >> 1];
      if ((e & 1u) && !aff_is_identity(p)) p.y = F::neg(p.y);
    } else p = src[r.off + k];
    add_mixed(acc, p);
  }
  Affine<F> a = to_affine(acc);
  if (r.bits > 1) a = to_affine(pt_scalar_mul_bits(a, mags + 8 * (size_t)r.mag, (int)r.bits));
  if (r.dst & COLSUM_FINAL) out[r.dst & ~COLSUM_FINAL] = a; else partials[r.dst] = a;
}

// out[j] = P[j + n] − P[j] for j < n − 1: the points [(tau^n − 1)·tau^j]G of the h query before 1/delta
template <class F>
VZ_HD void pt_diff(size_t j, size_t n, const Affine<F>* points, Affine<F>* out) {
  Affine<F> m = points[j];
  if (!aff_is_identity(m)) m.y = F::neg(m.y);
  XYZZ<F> acc = from_affine(points[j + n]);
  add_mixed(acc, m);
  out[j] = to_affine(acc);
}

// ---- judging a powers-of-tau string (g16_powers_verify.hip: k_powers_flags, k_powers_rlc): what ONE thread does, looped on the CPU by tests/native/pt_verify_check.cpp ----

// what a point of a string can be flagged with — the values of VIMZ_POWERS_* (include/vimz_hip.h); a coordinate not below q is the host's finding (bit 1)
constexpr uint32_t PV_OFF_CURVE = 2, PV_IDENTITY = 4, PV_SUBGROUP = 8;
constexpr unsigned RLC_CHUNK = 8;      // consecutive pairs of one thread of k_powers_rlc: they share the 128 doublings.  A wave runs an addition for every (bit, pair) some
                                       // lane has set — nearly all —, so a point costs 128 addition slots + 128 / RLC_CHUNK doublings: 144 at 8 against 132 at 32, and a thread's
                                       // serial chain is 128·(1 + RLC_CHUNK) operations.  At 32 a string of 2^18 left three quarters of the SIMDs empty and the chain set the time
                                       // (profiles/powers_verify.txt); at 8 its 2^19 / 8 chunks are one wave a SIMD.
constexpr int RLC_BITS = 128;          // bits of a rho

// flags[index] = what is wrong with points[index], 0: nothing.  b: the curve's constant in the coordinates' form (y² = x³ + b).  order: the 8 canonical words of r
// for a curve with a cofactor (the twist), and the point must then be killed by r — for a point of the subgroup the last addition is (r − 1)Q + Q, add_mixed's
// cancellation: that branch is the accept path; NULL for G1 (cofactor one: on the curve is in the group).  An identity is flagged (a power of a non-zero tau never
// is one) and not looked at further, nor is a point off its curve: r times it would be arithmetic on another curve.  Only the flag is written.
template <class F>
VZ_HD void pt_flags(size_t index, const Affine<F>* points, const F& b, const uint32_t* order, uint32_t* flags) {
  const Affine<F> p = points[index];
  uint32_t f = 0;
  if (aff_is_identity(p)) f = PV_IDENTITY;
  else if (!F::sqr(p.y).eq(F::add(F::mul(F::sqr(p.x), p.x), b))) f = PV_OFF_CURVE;
  else if (order && !pt_scalar_mul(p, order).is_identity()) f = PV_SUBGROUP;
  flags[index] = f;
}

// chunk `index` of a random linear combination over pairs of neighbours: out[index] = Σ rho_i · points[i + shift] over the pairs i of the chunk,
// RLC_CHUNK·index <= i < min(RLC_CHUNK·(index + 1), n_pairs); rho_i = the 4 words rho[4i ..].  shift = 0 gives the chunks of S = Σ rho_i·P_i, shift = 1 those of
// S' = Σ rho_i·P_(i+1): a string of ONE tau has S' = tau·S whatever the rho.  The 128 bit positions are walked once from the top: double, then add every point of the
// chunk whose rho has the bit — one doubling serves the whole chunk.  A zero rho adds nothing, a partial last chunk is shorter; add_mixed handles the identity,
// equal and opposite points.  Reads points[.. n_pairs − 1 + shift] and writes its own slot alone.
template <class F>
VZ_HD void pt_rlc_chunk(size_t index, const Affine<F>* points, size_t n_pairs, const uint32_t* rho, unsigned shift, Affine<F>* out) {
  const size_t lo = (size_t)RLC_CHUNK * index, hi = lo + RLC_CHUNK < n_pairs ? lo + RLC_CHUNK : n_pairs;
  XYZZ<F> acc = XYZZ<F>::identity();
#pragma unroll 1
  for (int b = RLC_BITS - 1; b >= 0; b--) {
    acc = dbl(acc);
#pragma unroll 1
    for (size_t i = lo; i < hi; i++)
      if ((rho[4 * i + (b >> 5)] >> (b & 31)) & 1u) add_mixed(acc, points[i + shift]);
  }
  out[index] = to_affine(acc);
}

// the plan (g16_colsum_plan.hpp) that sums the n_chunks chunk sums into ONE point: a single column that takes every chunk with coefficient one, through colsum_run
inline bool rlc_sum_plan(size_t n_chunks, ColsumPlan* plan) {
  if (!n_chunks || n_chunks >= ((size_t)1 << 31)) return false;
  std::vector<ColsumUnit> units(n_chunks);
  for (size_t t = 0; t < n_chunks; t++) units[t] = {(uint32_t)t, 0u};
  return colsum_plan(nullptr, 0, units.data(), units.size(), nullptr, 0, BnFr::MOD.w, 1u, (uint32_t)n_chunks, plan, nullptr);
}

// ---- the same-ratio check of two keys' l‖h arrays (g16_key_contrib.hip: k_ratio_rlc): what ONE thread does, looped on the CPU by tests/native/key_contrib_check.cpp ----

// chunk `index` of row `row` of ONE launch over two arrays of n points under ONE vector of rho: row 0 sums the chunk of `before`, row 1 that of `after`, as
// pt_rlc_chunk sums it with shift 0 — out[row·n_chunks + index] = Σ rho_i·P_i over RLC_CHUNK·index <= i < min(RLC_CHUNK·(index + 1), n).  The two rows share
// nothing but what they read: a thread writes its own slot alone.
template <class F>
VZ_HD void pt_ratio_chunk(size_t index, unsigned row, const Affine<F>* before, const Affine<F>* after, size_t n, size_t n_chunks, const uint32_t* rho, Affine<F>* out) {
  pt_rlc_chunk(index, row ? after : before, n, rho, 0u, out + (size_t)row * n_chunks);
}

// the plan of TWO columns over the 2·n_chunks chunk sums k_ratio_rlc leaves: column 0 takes the first n_chunks (S), column 1 the rest (S')
inline bool ratio_sum_plan(size_t n_chunks, ColsumPlan* plan) {
  if (!n_chunks || n_chunks >= ((size_t)1 << 30)) return false;
  std::vector<ColsumUnit> units(2 * n_chunks);
  for (size_t t = 0; t < n_chunks; t++) { units[t] = {(uint32_t)t, 0u}; units[n_chunks + t] = {(uint32_t)(n_chunks + t), 1u}; }
  return colsum_plan(nullptr, 0, units.data(), units.size(), nullptr, 0, BnFr::MOD.w, 2u, (uint32_t)(2 * n_chunks), plan, nullptr);
}

// ---- a contribution to a powers-of-tau string (g16_powers_contrib.hip: k_power_vec, k_scale_points_by): what ONE thread does, looped on the CPU by tests/native/powers_contrib_check.cpp ----

// entry `index` of the power vector, w^index as 8 MONTGOMERY words (pt_scale_by multiplies it by c before it walks it), for index < count <= 2^bits; w in Montgomery
// form.  Square and multiply over exactly `bits` bits, as pt_twiddle: the trip count comes from the host (bitlen(count − 1), 0 for count = 1).
VZ_HD void pt_power(size_t index, int bits, const Fp<BnFr>& w, uint32_t* out) {
  typedef Fp<BnFr> Fr;
  Fr acc = Fr::one();
  for (int b = bits - 1; b >= 0; b--) {
    acc = Fr::sqr(acc);
    if ((index >> b) & 1u) acc = Fr::mul(acc, w);
  }
  for (int i = 0; i < 8; i++) out[8 * index + i] = acc.v[i];
}

// out[index] = (c·pw[index])·in[index]: the scalar is ONE product in Fr (c and pw in Montgomery form) brought to canonical words, then pt_scalar_mul's walk and one
// inversion.  out may be in: the point is read before it is written and the thread touches its own slot alone.  The identity stays the identity (add_mixed skips
// it), and a zero scalar gives it.
template <class F>
VZ_HD void pt_scale_by(size_t index, const Affine<F>* in, const uint32_t* pw, const Fp<BnFr>& c, Affine<F>* out) {
  typedef Fp<BnFr> Fr;
  Fr s;
  for (int i = 0; i < 8; i++) s.v[i] = pw[8 * index + i];
  s = Fr::from_mont(Fr::mul(c, s));
  const Affine<F> p = in[index];
  out[index] = to_affine(pt_scalar_mul(p, s.v));
}

}  // namespace vz
