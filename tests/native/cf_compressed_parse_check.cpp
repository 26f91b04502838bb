// tests/test_cf_compressed_parse_host.py builds this with -fsanitize=address,undefined and runs it.  It loops the framing of the two compressed
// Nova + CycleFold proofs (vimz_amd/csrc/cf_compressed_parse.hpp — what vimz_cf_verify_compressed and vimz_cf_verify_merged_compressed run before they read
// an element) over structurally valid blobs of both kinds: every truncation length and every single-word garbling of the header and of the records'
// framing.  Each input sits in a heap block of exactly its size, so a read past its end is a sanitizer report; after a clean parse every range the frame
// describes is read.  Output: one line per loop, "<name> inputs=<n> clean=<n> malformed=<n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cf_compressed_parse.hpp"

namespace {

uint64_t g_sink = 0;
uint64_t sum(const uint64_t* w, size_t lo, size_t hi) { uint64_t s = 0; for (size_t i = lo; i < hi; i++) s += w[i]; return s; }

struct Tally { size_t inputs = 0, clean = 0, malformed = 0; };

// the blob in a heap block of exactly n words (n = 0: a block of one byte, never read)
struct Exact {
  std::unique_ptr<uint64_t[]> p; size_t n;
  Exact(const std::vector<uint64_t>& v, size_t len) : p(new uint64_t[len ? len : 1]), n(len) { if (len) memcpy(p.get(), v.data(), 8 * len); }
};

bool run_chain(const uint64_t* w, size_t n, const cfz::Shapes& sh) {
  cfz::ChainFrame f;
  if (!cfz::parse_chain(w, n, sh, &f)) return false;
  if (!(f.z0_at <= f.zn_at && f.zn_at <= f.inst_at && f.inst_at <= f.args_at && f.args_at <= n)) abort();
  g_sink += sum(w, f.z0_at, f.zn_at) + sum(w, f.zn_at, f.inst_at) + sum(w, f.inst_at, f.args_at) + sum(w, f.args_at, n) + f.steps;
  return true;
}
bool run_merged(const uint64_t* w, size_t n, const cfz::Shapes& sh) {
  cfz::MergedFrame f;
  if (!cfz::parse_merged(w, n, sh, &f)) return false;
  const size_t seg = cfz::segment_words(sh);
  if (!(f.rec_at == 2 && f.runs_at + f.runs == f.segs_at && f.segs_at + f.segments * seg == f.junctions_at && f.junctions_at + 16 * (f.runs - 1) == f.args_at &&
        f.rec_at + f.rec_words == f.args_at && f.args_at <= n && f.runs >= 1 && f.runs <= f.segments)) abort();
  for (size_t k = 0; k < f.runs; k++) if (w[f.runs_at + k] >= f.segments) abort();
  g_sink += sum(w, f.runs_at, f.segs_at) + sum(w, f.segs_at, f.junctions_at) + sum(w, f.junctions_at, f.args_at) + sum(w, f.args_at, n);
  return true;
}

template <class Run>
void tally(Tally& t, Run run, const std::vector<uint64_t>& v, size_t len, const cfz::Shapes& sh) {
  Exact e(v, len);
  t.inputs++;
  if (run(e.p.get(), e.n, sh)) t.clean++; else t.malformed++;
}

template <class Run>
void loops(const char* kind, Run run, const std::vector<uint64_t>& good, const std::vector<size_t>& framing, const cfz::Shapes& sh) {
  Tally whole, trunc, longer, garbled, other_shape;
  tally(whole, run, good, good.size(), sh);
  for (size_t len = 0; len < good.size(); len++) tally(trunc, run, good, len, sh);
  for (size_t extra = 1; extra <= 40; extra++) { std::vector<uint64_t> v(good); v.resize(good.size() + extra, 5); tally(longer, run, v, v.size(), sh); }
  for (size_t at : framing) {
    const uint64_t x = good[at];
    const uint64_t values[] = {0, 1, 2, x + 1, x - 1, x ^ 1, x << 1, x << 32, ~x, ~(uint64_t)0, (uint64_t)1 << 63, good.size(), good.size() - 2, (uint64_t)good.size() << 3, 4096, 4097};
    for (uint64_t val : values) {
      if (val == x) continue;
      std::vector<uint64_t> v(good); v[at] = val;
      tally(garbled, run, v, v.size(), sh);
      for (size_t cut : {(size_t)1, (size_t)8, v.size() / 2}) tally(garbled, run, v, v.size() - cut, sh);      // ... and truncated as well
    }
  }
  {   // a verifier for another circuit
    cfz::Shapes o = sh; o.len_z++; tally(other_shape, run, good, good.size(), o);
    o = sh; o.t1++; tally(other_shape, run, good, good.size(), o);
    o = sh; o.s2++; tally(other_shape, run, good, good.size(), o);
    o = sh; o.n_w1 = 17; o.t1 = 5; o.n_c2++; tally(other_shape, run, good, good.size(), o);
  }
  const Tally* ts[] = {&whole, &trunc, &longer, &garbled, &other_shape};
  const char* names[] = {"whole", "truncated", "longer", "garbled", "other_shape"};
  for (int k = 0; k < 5; k++) printf("%s/%s inputs=%zu clean=%zu malformed=%zu\n", kind, names[k], ts[k]->inputs, ts[k]->clean, ts[k]->malformed);
}

}  // namespace

int main() {
  cfz::Shapes sh{};
  sh.len_z = 2; sh.n_w1 = 13; sh.n_c1 = 7; sh.n_w2 = 9; sh.n_c2 = 3; sh.s1 = 3; sh.t1 = 4; sh.s2 = 2; sh.t2 = 4;
  uint64_t ctr = 0x9e3779b97f4a7c15ull;
  auto next = [&] { ctr = ctr * 6364136223846793005ull + 1442695040888963407ull; return ctr >> 3; };
  {   // one chain
    std::vector<uint64_t> good = {cfz::CHAIN_MAGIC, 10, sh.len_z, sh.s1, sh.t1, sh.s2, sh.t2, 0};
    while (good.size() < cfz::chain_words(sh)) good.push_back(next());
    loops("chain", run_chain, good, {0, 1, 2, 3, 4, 5, 6, 7}, sh);
  }
  for (int runs = 1; runs <= 2; runs++) {   // merged: three segments in one run, then in two
    const size_t S = 3;
    std::vector<uint64_t> good = {cfz::MERGED_MAGIC, cfz::records_words(sh, S, runs), cfz::RECORDS_MAGIC, S, sh.len_z, sh.n_w1, sh.n_c1, sh.n_w2, sh.n_c2, (uint64_t)runs, 0};
    if (runs == 2) good.push_back(2);
    const size_t total = 2 + cfz::records_words(sh, S, runs) + cfz::arg_words(sh.s1, sh.t1, true) + cfz::arg_words(sh.s2, sh.t2, true);
    std::vector<size_t> framing;
    for (size_t i = 0; i < good.size(); i++) framing.push_back(i);
    for (size_t j = 0; j < S; j++) framing.push_back(good.size() + j * cfz::segment_words(sh));      // every segment's step count (no framing role: stays clean)
    while (good.size() < total) good.push_back(next());
    loops(runs == 1 ? "merged1" : "merged2", run_merged, good, framing, sh);
  }
  // the two kinds are not each other's
  {
    std::vector<uint64_t> c = {cfz::CHAIN_MAGIC, 10, sh.len_z, sh.s1, sh.t1, sh.s2, sh.t2, 0};
    while (c.size() < cfz::chain_words(sh)) c.push_back(next());
    Tally t; tally(t, run_merged, c, c.size(), sh);
    c[0] = cfz::MERGED_MAGIC; tally(t, run_chain, c, c.size(), sh);
    printf("cross/kinds inputs=%zu clean=%zu malformed=%zu\n", t.inputs, t.clean, t.malformed);
  }
  printf("done sink=%llu\n", (unsigned long long)(g_sink & 0xff));
  return 0;
}
