// What ONE thread of the origin check's scalar kernels does (g16_key_origin.hip: k_spmv3_dict, k_origin_vec), as host-and-device functions of the thread's
// index: the kernels call them with their thread index, tests/native/key_origin_check.cpp loops them over every index on the CPU under the host sanitizers.
// No HIP in this file beyond VZ_HD.
//
// Vectors are arrays of 8 x 32-bit words an element over BN254 Fr, in Montgomery form unless said otherwise.  The matrices are a circuit builder's CSR as it is:
// row_ptr (n_c + 1 offsets), col (a wire number below m), coef (an index into dict).  The host checks those bounds before anything is launched
// (g16_key_origin.hip: csr_is_sound): no function here looks at a bound again.
#pragma once
#include <cstddef>
#include <cstdint>
#include "fp.hpp"

namespace vz {

typedef Fp<BnFr> KoFr;
constexpr unsigned KO_BLOCK = 256;      // threads of a block of both kernels
// k_origin_vec's modes
enum : uint32_t { KO_EXPAND = 0, KO_UNITS = 1, KO_H_SCALARS = 2, KO_ADD = 3 };

VZ_HD KoFr ko_load(const uint32_t* v, size_t i) { KoFr x; for (int k = 0; k < 8; k++) x.v[k] = v[8 * i + k]; return x; }
VZ_HD void ko_store(uint32_t* v, size_t i, const KoFr& x) { for (int k = 0; k < 8; k++) v[8 * i + k] = x.v[k]; }

// out[row] = Σ_k dict[coef[k]]·v[col[k]] over the row's entries, row_ptr[row] <= k < row_ptr[row + 1]; zero for an empty row and for the padding rows
// n_c <= row < n (the caller's guard is row < n).  One thread owns the row from its first term to its store: a column named twice is two terms, nothing is shared,
// and the trip count is the host's row_ptr.  (Why a row is not split over a wave: the header comment of g16_key_origin.hip and profiles/key_origin.txt.)
VZ_HD void spmv_dict_row(size_t row, uint32_t n_c, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* coef, const uint32_t* dict, const uint32_t* v, uint32_t* out) {
  KoFr acc = KoFr::zero();
  if (row < n_c) {
    const uint32_t lo = row_ptr[row], hi = row_ptr[row + 1];
#pragma unroll 1
    for (uint32_t k = lo; k < hi; k++) acc = KoFr::add(acc, KoFr::mul(ko_load(dict, coef[k]), ko_load(v, col[k])));
  }
  ko_store(out, row, acc);
}

// out[i] = rho_i·scale for lo <= i < hi, zero elsewhere (i < the vector's length: the caller's guard): the 128 bits at rho[4i ..] as an element of Fr, masked to
// the public wires or to the private ones.  scale_r2 = scale·R² (the Montgomery form of scale's Montgomery form), so that ONE multiplication both converts and scales
// — the 1/n of the inverse transforms rides here, everything downstream being linear.
VZ_HD void ko_expand(size_t i, size_t lo, size_t hi, const uint32_t* rho, const KoFr& scale_r2, uint32_t* out) {
  KoFr x = KoFr::zero();
  if (i >= lo && i < hi) {
    for (int k = 0; k < 4; k++) x.v[k] = rho[4 * i + k];
    x = KoFr::mul(x, scale_r2);
  }
  ko_store(out, i, x);
}

// the unit rows of the constant and the public inputs, which belong to A: u[n_c + i] += v[i] for i <= n_pub (the caller's guard; n_c + n_pub + 1 <= n)
VZ_HD void ko_unit(size_t i, uint32_t n_c, const uint32_t* v, uint32_t* u) { ko_store(u, (size_t)n_c + i, KoFr::add(ko_load(u, (size_t)n_c + i), ko_load(v, i))); }

// the scalars of the h equation over the string's 2n − 1 powers: Σ_j rho'_j·(tau^(j+n) − tau^j) = Σ_k s_k·tau^k with s_k = −rho'_k for k < n − 1, + rho'_(k−n) for
// k >= n (s_(n−1) = 0), mod r.  rho': n − 1 scalars of 128 bits; k < 2n − 1 is the caller's guard; r2 = R² (KoFr::r2()).
VZ_HD void ko_h_scalar(size_t k, size_t n, const uint32_t* rho, const KoFr& r2, uint32_t* out) {
  KoFr x = KoFr::zero();
  if (k + 1 < n || k >= n) {
    const size_t j = k >= n ? k - n : k;
    for (int w = 0; w < 4; w++) x.v[w] = rho[4 * j + w];
    x = KoFr::mul(x, r2);
    if (k < n) x = KoFr::neg(x);
  }
  ko_store(out, k, x);
}

VZ_HD void ko_add(size_t i, const uint32_t* a, const uint32_t* b, uint32_t* out) { ko_store(out, i, KoFr::add(ko_load(a, i), ko_load(b, i))); }

}  // namespace vz
