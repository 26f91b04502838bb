// What ONE thread of the point transform does (g16_powers.hip: k_pt_twiddles, k_pt_bitrev, k_pt_stage), as host-and-device functions of the thread's index:
// the kernels call them with their thread index, tests/native/pt_stage_check.cpp loops them over every index on the CPU — the algorithm is checked there
// before a launch is.  No HIP in this file beyond VZ_HD.
//
// The transform out_j = Σ_k w^(jk)·P_k over n = 2^logn points of a group of order r is radix 2, decimation in time: the bit reversal, then logn stages of n/2
// butterflies (half = 1, 2, .., n/2).  Butterfly `index` of a stage works on the slots lo = 2·half·(index / half) + index % half and lo + half alone, so a stage
// in place is race-free with one thread per butterfly, and the stages are sequenced by whoever launches them.
#pragma once
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

}  // namespace vz
