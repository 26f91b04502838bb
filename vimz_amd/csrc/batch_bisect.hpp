// The bisection of a refused batch chunk, shared by the two batch verifiers (decider_batch.hpp, spartan_batch.hpp).  No HIP in this file:
// tests/native/batch_bisect_check.cpp runs it under the host sanitizers against tests/_batch_bisect_ref.py.
//
// A chunk's equation is the sum of its members' equations under the members' own random multipliers, per SIDE (one side for the decider; the two curves of a
// compressed proof).  When the chunk [0, c) is refused on the sides `sides`, the same equation is asked again of subsets, every member under the multipliers it had:
//   * a refused subset of at most `leaf` members goes to the single verifier (a chunk with c <= leaf at once, with no evaluation);
//   * a larger refused subset [lo, hi) is split into L = [lo, lo + ceil((hi − lo)/2)) and R, the rest.  L is asked on the sides its parent refused and on no
//     other (a side that held for the parent is the guarantee an accepted chunk gives, for every member of it: it is never asked again).  If L holds on all of them its members are
//     accepted and R is refused BY IMPLICATION, with the parent's sides and without an evaluation; if L is refused on any, R is asked as well and may be accepted.
// The implication only ever refuses.  Every member therefore ends in exactly one of two places: in a subset that an evaluation accepted — the guarantee an accepted
// chunk gives, a failing member surviving with probability about 2^-128 — or before the single verifier.  results[i] stays the single verifier's word.
//
// The order is level-synchronous over ALL roots: every L of a level in one call of `holds`, then the R subsets that need it in a second call, so that a verifier can
// form a level's sums in one device pass and judge them side by side.
//
// BOUND: a root of c > leaf members costs at most 2·(c − 1) subsets asked (a subset of more than `leaf` members has two children, each asked at most once, and
// the tree over c members has at most c − 1 such subsets); a root with c <= leaf costs none.  One bad member among c = 2^k at leaf 1 costs between k and 2k.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace vz {
namespace bb {

struct Subset { size_t lo, hi; uint32_t sides; };      // members [lo, hi); the sides asked (a request) or refused (a node)

// what a refused chunk cost.  Indices as the entries' stats[4].
enum { ST_REFUSED = 0, ST_EQUATIONS, ST_SINGLES, ST_ACCEPTED, ST_N };
struct Outcome {
  std::vector<Subset> singles;      // the subsets left to the single verifier, with the sides they were refused on, in the order they were met
  uint64_t subsets = 0;             // subsets asked (the bound above counts these)
  uint64_t equations = 0;           // Σ over the subsets asked of the number of sides asked: the side equations evaluated
  uint64_t accepted = 0;            // members of subsets an evaluation accepted
  uint64_t single_members = 0;
};

inline uint32_t popcount32(uint32_t x) { uint32_t n = 0; for (; x; x &= x - 1) n++; return n; }

// holds(ask, held): held[k] <- the sides of ask[k].sides on which the equation over [ask[k].lo, ask[k].hi) holds; false ends the plan (a device error).
typedef std::function<bool(const std::vector<Subset>& ask, std::vector<uint32_t>& held)> HoldsFn;

// roots: disjoint refused subsets (whole chunks), every one with sides != 0.  trace (optional): every subset asked, in order.
inline bool bisect(const std::vector<Subset>& roots, size_t leaf, const HoldsFn& holds, Outcome* out, std::vector<Subset>* trace = nullptr) {
  if (leaf < 1) leaf = 1;
  std::vector<Subset> frontier(roots), work, ask, next;
  std::vector<uint32_t> held_l, held_r;
  auto run = [&](std::vector<uint32_t>& held) {
    held.assign(ask.size(), 0);
    if (ask.empty()) return true;
    for (const Subset& a : ask) { out->subsets++; out->equations += popcount32(a.sides); if (trace) trace->push_back(a); }
    if (!holds(ask, held)) return false;
    for (size_t k = 0; k < ask.size(); k++) held[k] &= ask[k].sides;
    return true;
  };
  while (!frontier.empty()) {
    work.clear();
    for (const Subset& nd : frontier) {
      if (nd.hi - nd.lo <= leaf) { out->singles.push_back(nd); out->single_members += nd.hi - nd.lo; }
      else work.push_back(nd);
    }
    auto mid = [](const Subset& nd) { return nd.lo + (nd.hi - nd.lo + 1) / 2; };
    ask.clear();
    for (const Subset& nd : work) ask.push_back({nd.lo, mid(nd), nd.sides});
    if (!run(held_l)) return false;
    ask.clear();
    for (size_t k = 0; k < work.size(); k++) if (work[k].sides & ~held_l[k]) ask.push_back({mid(work[k]), work[k].hi, work[k].sides});
    if (!run(held_r)) return false;
    next.clear();
    size_t r = 0;
    for (size_t k = 0; k < work.size(); k++) {
      const Subset& nd = work[k];
      const size_t m = mid(nd);
      const uint32_t left = nd.sides & ~held_l[k];
      if (!left) { out->accepted += m - nd.lo; next.push_back({m, nd.hi, nd.sides}); continue; }      // R: refused by implication, never accepted by it
      next.push_back({nd.lo, m, left});
      const uint32_t right = nd.sides & ~held_r[r++];
      if (!right) out->accepted += nd.hi - m; else next.push_back({m, nd.hi, right});
    }
    frontier.swap(next);
  }
  return true;
}

}  // namespace bb
}  // namespace vz
