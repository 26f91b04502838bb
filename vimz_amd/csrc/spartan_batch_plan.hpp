// The GPU-free pieces of the batched compressed-proof verifier (spartan_batch.hpp): the constants, the half-table layout and the per-thread body of
// k_half_tables, the index map and the mask of k_svec_accum, the unrolled coefficients of an opening's group equation, and the chunk plan.  No HIP in this file:
// tests/native/spartan_batch_check.cpp runs every function here against the definitions under the host sanitizers.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>
#include "fp.hpp"

namespace vz {
namespace sb {

constexpr uint32_t GROUP = 4;          // proofs one k_mat_eval pass serves, openings one k_svec_accum pass serves
constexpr uint32_t SPLIT_H = 10;       // a table over k variables is the product of a half-table over the low min(k, H) index bits and one over the rest
constexpr uint32_t MAX_VARS = 24;      // variables a point may have (shapes are capped at 2^21)
constexpr size_t DEFAULT_CHUNK = 32;   // (a refused chunk without bisection: 32 single verifications)
constexpr size_t DEFAULT_LEAF = 1;     // a refused subset of one member goes to the single verifier: a subset equation costs a small fraction of one (profiles/batch_bisect.txt)

// two points of nv[0], nv[1] variables -> four tables: element offsets of (point 0 low, point 0 high, point 1 low, point 1 high), and their total
struct HalfLayout { uint32_t hl[2], off[4], elems; };
inline HalfLayout half_layout(uint32_t nv0, uint32_t nv1) {
  HalfLayout L{};
  L.hl[0] = std::min(SPLIT_H, nv0); L.hl[1] = std::min(SPLIT_H, nv1);
  L.off[0] = 0; L.off[1] = 1u << L.hl[0]; L.off[2] = L.off[1] + (1u << (nv0 - L.hl[0])); L.off[3] = L.off[2] + (1u << L.hl[1]);
  L.elems = L.off[3] + (1u << (nv1 - L.hl[1]));
  return L;
}

// Entry `local` of one half-table of a point of nv variables (var(q), q = 0 the TOP bit of the full index): bit p of a full index selects variable nv − 1 − p; the
// low table covers bits [0, hl), the high one bits [hl, nv).  kind 1: eq(point, ·) — a set bit takes v, a clear one 1 − v;  kind 0: the monomials of an opening's
// s-vector — a set bit takes x, a clear one 1.
template <class F, class Var>
VZ_HD F half_entry(Var var, uint32_t nv, uint32_t hl, bool high, uint32_t kind, uint32_t local) {
  const uint32_t bits = high ? nv - hl : hl, top = high ? nv - 1 - hl : nv - 1;      // `top`: the variable of this table's bit 0
  F acc = F::one();
  for (uint32_t q = 0; q < bits; q++) {
    const F v = var(top - q);
    const bool bit = (local >> q) & 1u;
    acc = F::mul(acc, bit ? v : (kind ? F::sub(F::one(), v) : F::one()));
  }
  return acc;
}

// the index of an opening's vectors whose key point is ck[j]: load_bases(shifted) puts ck[n − 1] at index 0 and ck[i − 1] at index i (n a power of two)
VZ_HD size_t svec_index(size_t j, size_t n, bool shifted) { return shifted ? ((j + 1) & (n - 1)) : j; }
// k_mask_public's rule; n_w = 0: an E opening, nothing is masked
VZ_HD bool svec_masked(size_t i, uint32_t n_pub, uint32_t n_w) { return n_w != 0 && (i == 0 || i + n_pub >= n_w); }

// ipa_verify's P <- R + x·P + x²·L from P_0 = comm + claim·r0·U, unrolled:  c[0] on comm = Π x;  c[1 + 2j] on R_j = Π_{i>j} x_i;  c[2 + 2j] on L_j = x_j²·Π_{i>j} x_i;
// *g0 on U = (Π x)·claim·r0
template <class F>
void ipa_unroll(const std::vector<F>& xs, const F& claim, const F& r0, std::vector<F>& c, F* g0) {
  const size_t rounds = xs.size();
  c.assign(2 * rounds + 1, F::zero());
  F run = F::one();
  for (size_t j = rounds; j-- > 0;) {
    c[1 + 2 * j] = run;
    c[2 + 2 * j] = F::mul(run, F::sqr(xs[j]));
    run = F::mul(run, xs[j]);
  }
  c[0] = run;
  *g0 = F::mul(run, F::mul(claim, r0));
}

// the pending proofs cut into chunks: [first, last) pairs in order; chunk = 0 is the default
inline std::vector<std::pair<size_t, size_t>> chunk_plan(size_t n_pending, size_t chunk) {
  if (!chunk) chunk = DEFAULT_CHUNK;
  std::vector<std::pair<size_t, size_t>> out;
  for (size_t c0 = 0; c0 < n_pending; c0 += chunk) out.emplace_back(c0, std::min(n_pending, c0 + chunk));
  return out;
}

}  // namespace sb
}  // namespace vz
