// Group-side kernels of a Groth16 set-up from a powers-of-tau string: what such a set-up does to POINTS where the trapdoor set-up
// (groth16.hip) works on scalars and ends in fixed-base multiplications.  Built so far: the same-scalar multiplication that applies 1/delta to the l and
// h queries, and the transform over points that turns the string's [tau^k]G into the Lagrange basis [L_j(tau)]G — both for G1 and for G2.  Shared by the
// set-up to come, vimz_powers_lagrange and the test hooks (g16_powers.hip).
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
