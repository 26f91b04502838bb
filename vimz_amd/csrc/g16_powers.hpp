// Group-side kernels of a Groth16 set-up from a powers-of-tau string: what such a set-up does to POINTS where the trapdoor set-up
// (groth16.hip) works on scalars and ends in fixed-base multiplications.  Built so far: the same-scalar multiplication that applies 1/delta to the l and
// h queries.  Shared by the set-up to come and the test hook (g16_powers.hip).
#pragma once
#include "cyclefold_internal.hpp"

// Queues on `s`: out[i] = k · in[i] for n affine points of BN254 G1 (device, standard Montgomery coordinates, the identity as (0, 0)) and ONE scalar k below r
// given as 8 canonical words on the device — the caller wipes that copy once the stream has passed it.  out may be in.  Output coordinates are canonical.
hipError_t g16_scale_points(hipStream_t s, const G1Aff* in, size_t n, const uint32_t* k_canon, G1Aff* out);
