// Group-side kernels of a Groth16 set-up from a powers-of-tau string: what such a set-up does to POINTS where the trapdoor set-up
// (groth16.hip) works on scalars and ends in fixed-base multiplications: the same-scalar multiplication that applies 1/delta to the l and h queries, the
// transform over points that turns the string's [tau^k]G into the Lagrange basis [L_j(tau)]G, the column sums Σ c·L_r of the matrices over that basis (the a, b
// and K queries) — each for G1 and for G2 — and the differences [tau^(j+n) − tau^j]G1 of the h query.  Shared by vimz_decider_setup_from_powers (groth16.hip),
// vimz_powers_lagrange and the test hooks (g16_powers.hip).  In every kernel a thread owns its outputs, no kernel waits on another workgroup, the stream orders the
// launches and every loop bound comes from the host; what a thread does is a host-and-device function of its index (g16_point_stage.hpp), looped on the CPU by
// tests/native/pt_stage_check.cpp and colsum_plan_check.cpp.
#pragma once
#include "cyclefold_internal.hpp"
#include "g16_point_stage.hpp"

typedef Affine<vz::pairing::Fq2> G2PowAff;      // a point of BN254 G2 on the device: x.c0, x.c1, y.c0, y.c1 in 8 x 32 Montgomery words each, the identity as zeros

// Queues on `s`: out[i] = k · in[i] for n affine points of BN254 G1 (device, standard Montgomery coordinates, the identity as (0, 0)) and ONE scalar k below r
// given as 8 canonical words on the device — the caller wipes that copy once the stream has passed it.  out may be in.  Output coordinates are canonical.
hipError_t g16_scale_points(hipStream_t s, const G1Aff* in, size_t n, const uint32_t* k_canon, G1Aff* out);
// ... and for points of G2
hipError_t g16_scale_points(hipStream_t s, const G2PowAff* in, size_t n, const uint32_t* k_canon, G2PowAff* out);

// a primitive 2^k-th root of unity of Fr, k <= 28, in Montgomery form (groth16.hip: the domain of the decider's NTTs uses the same one)
Fe fr_root_of_unity(int k);

// words of the table g16_point_transform fills: the n/2 twiddles and 1/n, 8 canonical words each
inline size_t g16_point_transform_words(int logn) { return 8 * (((size_t)1 << logn) / 2 + 1); }

// Queues on `s`, IN PLACE on n = 2^logn affine points (device, Montgomery coordinates, the identity as zeros), 1 <= logn <= 26:
//     points[j] = Σ_k w^(jk)·points[k],   w = fr_root_of_unity(logn), or its inverse when `inverse`;   times 1/n when `scaled`
// in natural order on both sides.  Radix 2: the table's launch, the bit reversal's, one launch per stage (each thread reads and writes its own two slots;
// the stream sequences the stages: no kernel waits on another workgroup), and k_scale_points when scaled: logn + 2 or + 3 launches, no host work beyond them,
// no allocation, no synchronisation.  `twiddles`: g16_point_transform_words(logn) words on the device, filled here (public values: no wiping).
hipError_t g16_point_transform(hipStream_t s, G1Aff* points, int logn, bool inverse, bool scaled, uint32_t* twiddles);
hipError_t g16_point_transform(hipStream_t s, G2PowAff* points, int logn, bool inverse, bool scaled, uint32_t* twiddles);

// A plan of column sums (g16_colsum_plan.hpp) on the device, with room for the partials of points of `point_bytes` each: made and freed by the caller, read by
// any number of g16_column_sums calls one after another on one stream.
struct ColsumDevice {
  uint32_t n_cols = 0, n_points = 0;
  uint32_t *entries = nullptr, *mags = nullptr;
  vz::ColsumRun* runs = nullptr;                  // the levels' runs one after another
  struct Level { size_t first; uint32_t n_runs, n_partials; };
  std::vector<Level> levels;
  void* partials[2] = {nullptr, nullptr};         // level k writes partials[k & 1] and reads the other
  size_t point_bytes = 0;
};
// blocking copies (the plan's vectors are pageable); any failure frees what was allocated
hipError_t g16_colsum_upload(const vz::ColsumPlan& plan, size_t point_bytes, ColsumDevice* dev);
void g16_colsum_free(ColsumDevice& dev);
// Queues on `s`: out[j] = Σ_{entries of column j} c·points[row] for the plan's n_cols columns, canonical affine with the identity as zeros (the form
// bases_from_device takes); points: at least plan.n_points affine points (Montgomery coordinates).  A memset of `out`, then one k_col_runs launch per level, one
// thread per run; `dev` must have been uploaded for this point size.  out must not overlap points.
hipError_t g16_column_sums(hipStream_t s, const ColsumDevice& dev, const G1Aff* points, G1Aff* out);
hipError_t g16_column_sums(hipStream_t s, const ColsumDevice& dev, const G2PowAff* points, G2PowAff* out);
// Queues on `s`: out[j] = dinv·(tau_g1[j + n] − tau_g1[j]) for j < n − 1 — the h query [(tau^n − 1)·tau^j / delta]G1 from the string's 2n − 1 powers: k_point_diff,
// then k_scale_points in place.  dinv_canon: 8 canonical words on the device, wiped by the caller.  out: n − 1 points, not overlapping tau_g1.
hipError_t g16_h_query(hipStream_t s, const G1Aff* tau_g1, size_t n, const uint32_t* dinv_canon, G1Aff* out);

// ---- judging a string before a set-up trusts it (g16_powers_verify.hip: vimz_powers_verify) ------------------------------------------------------------------
// the generators in Montgomery coordinates, and the OS's randomness (groth16.hip: what a proof's blinders are drawn from)
G1Aff g16_g1_generator();
G2PowAff g16_g2_generator();
bool g16_os_random(void* buf, size_t n);
// Queues on `s`: flags[i] = 0, or what is wrong with points[i] (g16_point_stage.hpp: pt_flags — the identity, off its curve, and for G2 not killed by r), one
// thread per point, each writing its own 4 bytes.  order_canon: the 8 canonical words of r on the device (read for G2 alone).
hipError_t g16_powers_flags(hipStream_t s, const G1Aff* points, size_t n, const uint32_t* order_canon, uint32_t* flags);
hipError_t g16_powers_flags(hipStream_t s, const G2PowAff* points, size_t n, const uint32_t* order_canon, uint32_t* flags);
// the chunk sums a combination over n_pairs pairs leaves for the reduction
inline size_t g16_powers_rlc_chunks(size_t n_pairs) { return (n_pairs + vz::RLC_CHUNK - 1) / vz::RLC_CHUNK; }
// Queues on `s`: out[0] = S = Σ rho_i·points[i], out[1] = S' = Σ rho_i·points[i + 1] over i < n_pairs (so n_pairs + 1 points are read), rho_i the 128 bits at
// rho[4i ..] on the device: two launches of k_powers_rlc (shift 0 and 1; thread t sums the chunk t into chunks[t], g16_point_stage.hpp: pt_rlc_chunk), each followed
// by g16_column_sums over `sum`, the plan of ONE column that takes every chunk with coefficient one (g16_point_stage.hpp: rlc_sum_plan, uploaded for this point size).
// chunks: g16_powers_rlc_chunks(n_pairs) points.  out: affine as g16_column_sums leaves it (reduced Montgomery coordinates), the identity as zeros.
hipError_t g16_powers_rlc(hipStream_t s, const G1Aff* points, size_t n_pairs, const uint32_t* rho, const ColsumDevice& sum, G1Aff* chunks, G1Aff* out);
hipError_t g16_powers_rlc(hipStream_t s, const G2PowAff* points, size_t n_pairs, const uint32_t* rho, const ColsumDevice& sum, G2PowAff* chunks, G2PowAff* out);
#ifdef VIMZ_TESTING
// ONE pass of the above without its reduction — chunks[t] = the sum of chunk t with that shift (0 or 1) —: what the two-launch form of the same-ratio check of two
// keys is measured with (g16_key_contrib.hip, profiles/key_contrib.txt); in the testing library alone
hipError_t g16_powers_rlc_pass(hipStream_t s, const G1Aff* points, size_t n_pairs, const uint32_t* rho, unsigned shift, G1Aff* chunks);
#endif

// ---- further delta contributions to a saved key (g16_key_contrib.hip: vimz_decider_key_verify_contributions) ------------------------------------------------
// Queues on `s`: out[0] = S = Σ rho_i·before[i], out[1] = S' = Σ rho_i·after[i] over i < n, rho_i the 128 bits at rho[4i ..] on the device: ONE launch of k_ratio_rlc over
// a grid of (chunks, 2) — blockIdx.y = 0 sums `before`, 1 `after`; thread t of a row sums its chunk into chunks[row·n_chunks + t] (g16_point_stage.hpp:
// pt_ratio_chunk) —, then g16_column_sums over `sum`, the plan of TWO columns of ratio_sum_plan uploaded for G1.  chunks: 2·g16_powers_rlc_chunks(n) points.  out: as
// g16_column_sums leaves it (reduced Montgomery coordinates, the identity as zeros).
hipError_t g16_ratio_rlc(hipStream_t s, const G1Aff* before, const G1Aff* after, size_t n, const uint32_t* rho, const ColsumDevice& sum, G1Aff* chunks, G1Aff* out);

// ---- a contribution to a powers-of-tau string (g16_powers_contrib.hip: vimz_powers_contribute) ------------------------------------------------------------------
// Queues on `s`: pw[8i ..] = w^i for i < count as 8 Montgomery words (k_power_vec, one thread per power, g16_point_stage.hpp: pt_power over bitlen(count − 1) bits).
// w: Montgomery, a kernel argument.  When w is a secret so is the vector: the caller overwrites it before freeing it.  count <= 2^31.
hipError_t g16_power_vec(hipStream_t s, uint32_t* pw, size_t count, const Fe& w);
// Queues on `s`: out[i] = (c·pw[i])·in[i] for n affine points (device, Montgomery coordinates, the identity as zeros) and the power vector above (n entries or more):
// k_scale_points_by, one thread per point (pt_scale_by), a DIFFERENT scalar at every point.  c: Montgomery, a kernel argument.  out may be in; output coordinates are
// canonical.
hipError_t g16_scale_points_by(hipStream_t s, const G1Aff* in, size_t n, const uint32_t* pw, const Fe& c, G1Aff* out);
hipError_t g16_scale_points_by(hipStream_t s, const G2PowAff* in, size_t n, const uint32_t* pw, const Fe& c, G2PowAff* out);
