// The bisection planner of the batch verifiers (vimz_amd/csrc/batch_bisect.hpp) on the CPU, built with g++ -fsanitize=address,undefined and run directly
// (tests/test_batch_bisect_native_host.py).  For c = 1…9 members, leaf 1…4, the chunks of c, 4 and 2, three ways of giving a bad member its failing sides and
// EVERY bad subset, the planner runs with a callback that knows the bad set, and one line a case goes out:
//     c leaf chunk pattern badset | asked lo-hi:sides … | singles lo-hi:sides … | refused equations singles accepted subsets
// which the test compares with tests/_batch_bisect_ref.py.  The last line is "done cases=N".
#include <cstdio>
#include "batch_bisect.hpp"

using namespace vz::bb;

static uint32_t side_of(int pattern, size_t i) { return pattern == 0 ? 1u : pattern == 1 ? 1u + (uint32_t)(i & 1) : (uint32_t)(i % 3) + 1u; }

int main() {
  size_t cases = 0;
  for (size_t c = 1; c <= 9; c++)
    for (size_t leaf = 1; leaf <= 4; leaf++)
      for (size_t chunk : {(size_t)0, (size_t)4, (size_t)2})
        for (int pattern = 0; pattern < 3; pattern++)
          for (uint32_t badset = 0; badset < (1u << c); badset++) {
            std::vector<uint32_t> bad(c, 0);      // (heap blocks of exact size: an index past a range is a report)
            for (size_t i = 0; i < c; i++) if ((badset >> i) & 1) bad[i] = side_of(pattern, i);
            auto fails = [&](size_t lo, size_t hi) { uint32_t m = 0; for (size_t i = lo; i < hi; i++) m |= bad.at(i); return m; };
            std::vector<Subset> roots;
            const size_t step = chunk ? chunk : c;
            for (size_t lo = 0; lo < c; lo += step) { const size_t hi = lo + step < c ? lo + step : c; if (fails(lo, hi)) roots.push_back({lo, hi, fails(lo, hi)}); }
            Outcome out;
            std::vector<Subset> trace;
            const bool ok = bisect(roots, leaf, [&](const std::vector<Subset>& ask, std::vector<uint32_t>& held) {
              if (held.size() != ask.size()) return false;
              for (size_t k = 0; k < ask.size(); k++) {
                if (ask[k].lo >= ask[k].hi || ask[k].hi > c || !ask[k].sides) return false;
                held[k] = ~fails(ask[k].lo, ask[k].hi);      // (every side, asked or not: the planner keeps what it asked)
              }
              return true;
            }, &out, &trace);
            if (!ok) { printf("planner failed at c=%zu leaf=%zu chunk=%zu pattern=%d badset=%u\n", c, leaf, chunk, pattern, badset); return 1; }
            printf("%zu %zu %zu %d %u |", c, leaf, chunk, pattern, badset);
            for (const Subset& s : trace) printf(" %zu-%zu:%u", s.lo, s.hi, s.sides);
            printf(" |");
            for (const Subset& s : out.singles) printf(" %zu-%zu:%u", s.lo, s.hi, s.sides);
            printf(" | %zu %llu %llu %llu %llu\n", roots.size(), (unsigned long long)out.equations, (unsigned long long)out.single_members, (unsigned long long)out.accepted,
                   (unsigned long long)out.subsets);
            cases++;
          }
  printf("done cases=%zu\n", cases);
  return 0;
}
