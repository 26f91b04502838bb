// The chains of the full decider's check 5 (aug/decider_cf.hpp: every scalar of the running CycleFold witness and error vector walks 127 windows of
// its generator's table by affine additions from H) on the device: k_cf_open_chains, one thread per scalar, both openings in one launch.
// What the host computes in cf_open_chains_host, word for word.  Shared by the decider (groth16.hip) and the test hook (decider_chains.hip).
#pragma once
#include "cyclefold_internal.hpp"
#include "aug/decider_cf.hpp"

// the opening key's window table [k][j][d] = (d + 1)·4^j·G_k and H, resident on the device (64 B per entry: 43 MB at 1 313 generators)
struct CfChainsKey {
  Affine<Fe>* table = nullptr;
  Affine<Fe> H;
  uint32_t n = 0;      // generators
};
constexpr size_t CF_CHAIN_WORDS = (size_t)aug::CFO_WINDOWS * 4 * 8;      // words of one scalar's wires

// upload on `s` and wait for it (the table is pageable host memory); cf_chains_key_free releases it
hipError_t cf_chains_key_upload(hipStream_t s, const aug::CfOpeningKey& key, CfChainsKey& out);
void cf_chains_key_free(CfChainsKey& k);
// Queues on `s`: bad = 0, then the kernel over sW[0 .. nW) and sE[0 .. nE) (Montgomery Fq, 8 words each, device; scalar k of either uses generator k).
//   wires: (nW + nE)·127·4 elements, W's chains first, [k][j][4] = (b0·b1, slope, x, y);  ends: nW + nE points;  bad: one word, 1 when an addition met
//   two points with the same x.  All canonical Montgomery Fr.  hipErrorInvalidValue: a vector is longer than the key.
hipError_t cf_chains_launch(hipStream_t s, const CfChainsKey& key, const uint32_t* sW, uint32_t nW, const uint32_t* sE, uint32_t nE, uint32_t* wires,
                            uint32_t* ends, uint32_t* bad);
