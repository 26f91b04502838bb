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

}  // namespace vz
