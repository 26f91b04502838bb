// The merged Nova + CycleFold proof object (cyclefold_merge.hip: protocol comment there) as the TUs that read it see it: cyclefold_merge.hip
// itself and spartan.hip, which compresses it (vimz_cf_merged_compress).
#pragma once
#include "cyclefold_internal.hpp"

struct CfSegRec { uint64_t n = 0; std::vector<Fe> zs, ze; CfMainRelaxed U; G1Aff UW, UE; CfMainFresh u; G1Aff uW; CfRelaxed cfU; G1Aff T1, T2; G2Aff Tc; };
struct CfAcc { uint8_t h[32] = {}; uint64_t n = 0; std::vector<Fe> zs, ze; G1Aff cW, cE; Fe u, x0, x1; G2Aff qW, qE; Fq qu; Fq qx[CF_IO]; };
struct CfJunction { G1Aff Tp; G2Aff Tq; };
struct vimz_cf_merged {
  vimz_cf* vk = nullptr;                  // shapes, keys, context: must outlive this object
  std::vector<CfSegRec> segs;
  // RUNS: segs[run_start[k] .. run_start[k+1]) were folded in row order by vimz_cf_merge on one GPU (one run per GPU of a sharded proof);
  // run k > 0 was folded into the runs before it as a whole (vimz_cf_merge_merged: two relaxed accumulators), junction k-1 holds that fold's
  // two cross-term commitments
  std::vector<uint32_t> run_start{0};
  std::vector<CfJunction> junctions;
  CfAcc acc;
  uint32_t* dev = nullptr;                // one allocation
  uint32_t *Zp = nullptr, *Ep = nullptr, *AZp = nullptr, *BZp = nullptr, *CZp = nullptr, *Tp = nullptr;
  uint32_t *Zq = nullptr, *Eq = nullptr, *AZq = nullptr, *BZq = nullptr, *CZq = nullptr, *Tq = nullptr;
  bool broken = false;
  double seconds[4] = {};                 // GPU cross terms + commitments, folds, host, total
};

namespace vz {
// the records of m as vimz_cf_merged_records writes them (canonical little-endian words)
std::vector<uint64_t> cf_merged_records_words(const vimz_cf_merged* m);
// The records of an untrusted source, already framed (cf_compressed_parse.hpp): every element range-checked, every point checked to be on its
// curve.  false: malformed.
bool cf_merged_read_records(const vimz_cf* vk, const uint64_t* w, size_t nwords, std::vector<CfSegRec>& segs, std::vector<uint32_t>& run_start, std::vector<CfJunction>& junctions);
// The statement side of the verifier (what vimz_cf_merged_verify runs): every segment's hash checks, adjacency, the folds of the instances, the runs
// folded left to right.  flags: bit 0 / 1 a segment's main / CycleFold hash, bit 2 not adjacent or empty.  false: nothing could be evaluated.
bool cf_merged_replay(const vimz_cf* vk, const std::vector<CfSegRec>& segs, const std::vector<uint32_t>& run_start, const std::vector<CfJunction>& junctions, CfAcc& out, uint32_t* flags);
}
