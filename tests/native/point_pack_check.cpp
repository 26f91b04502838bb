// Packed curve points (vimz_amd/csrc/g16_point_pack.hpp) on the CPU: the functions k_points_pack and k_points_unpack call with their thread index (pt_pack, pt_unpack,
// and through them fq_sqrt and fq2_sqrt) looped over every thread, and the host's parser of a packed key, with the canonical Fp fields.  Reads lines from the file
// named on the command line:
//     PACK LABEL GROUP MONT N HEX      N unpacked points of G1 (GROUP 1, 64 bytes each) or G2 (2, 128 bytes) as they lie in memory — canonical words, or Montgomery
//                                      words with MONT = 1 — from a heap block of exactly that size into heap blocks of exactly N packed points and N flag words:
//                                      every thread of the grid (blocks of PT_BLOCK) under the kernel's guard, all three blocks checked after EVERY thread — only that
//                                      thread's output slot and flag may have changed, the input never.  Prints LABEL, then FLAG:SLOT per point (the slot's bytes as hex).
//     UNPACK LABEL GROUP MONT N HEX    the other way: N packed points (32 / 64 bytes each) into N points in that form.
//     PARSE LABEL HEX                  packed_key_layout over exactly those bytes (a heap block of that very size): prints LABEL ok n_g1 n_g2 words pwords, or
//                                      LABEL err MESSAGE.
// Nothing else is judged here: tests/test_point_pack_host.py compares.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "g16_point_pack.hpp"

using namespace vz;
using namespace vz::keyc;

static std::vector<uint8_t> bytes_of(const std::string& hex) {
  std::vector<uint8_t> b;
  if (hex != "-") for (size_t i = 0; i + 1 < hex.size(); i += 2) b.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
  return b;
}

// heap blocks of exactly the size the threads may touch: the sanitizer sees a read or write past them
struct Block {
  uint8_t* p; size_t n;
  explicit Block(size_t bytes) : p((uint8_t*)malloc(bytes ? bytes : 1)), n(bytes) { memset(p, 0xa5, bytes); }
  ~Block() { free(p); }
  Block(const Block&) = delete;
};

// after thread t (own = it ran under the guard) only slot t of `now` (slots of `size` bytes) may differ from `seen`, and must; `seen` is brought up to date
static bool only_own_slot(const std::string& label, const Block& now, std::vector<uint8_t>& seen, size_t size, size_t t, bool own) {
  for (size_t k = 0; k < now.n / size; k++) {
    const bool same = !memcmp(now.p + size * k, seen.data() + size * k, size);
    if (!(own && k == t) && !same) { fprintf(stderr, "%s: thread %zu wrote slot %zu\n", label.c_str(), t, k); return false; }
    if (own && k == t && same) { fprintf(stderr, "%s: thread %zu left its own slot\n", label.c_str(), t); return false; }      // (0xa5.. is no output: a flag is below 8, a slot's top byte has a free bit pattern)
  }
  if (own && t < now.n / size) memcpy(seen.data() + size * t, now.p + size * t, size);
  return true;
}

template <class F>
static int run(const std::string& label, bool packing, bool mont, size_t n, const std::vector<uint8_t>& data) {
  const size_t pt = 2 * sizeof(F), pk = sizeof(F), in_size = packing ? pt : pk, out_size = packing ? pk : pt;
  if (data.size() != in_size * n) { fprintf(stderr, "%s: %zu bytes for %zu points\n", label.c_str(), data.size(), n); return 2; }
  F b;
  if (sizeof(F) == sizeof(pack::Fq)) { const pack::Fq b1 = pairing::fq_u64(3); memcpy((void*)&b, &b1, sizeof(b1)); }
  else { const pack::Fq2 b2 = pairing::consts().twist_b; memcpy((void*)&b, &b2, sizeof(F)); }
  Block in(in_size * n), out(out_size * n), flags(4 * n);
  memcpy(in.p, data.data(), data.size());
  std::vector<uint8_t> seen_in(in.p, in.p + in.n), seen_out(out.p, out.p + out.n), seen_flags(flags.p, flags.p + flags.n);
  const size_t blocks = (n + PT_BLOCK - 1) / PT_BLOCK;
  for (size_t t = 0; t < blocks * PT_BLOCK; t++) {
    if (t < n) {      // (the kernel's guard)
      if (packing) pt_pack(t, (const Affine<F>*)in.p, mont, b, (uint32_t*)out.p, (uint32_t*)flags.p);
      else pt_unpack(t, (const uint32_t*)in.p, b, mont, (Affine<F>*)out.p, (uint32_t*)flags.p);
    }
    if (!only_own_slot(label, out, seen_out, out_size, t, t < n) || !only_own_slot(label + " (flags)", flags, seen_flags, 4, t, t < n) ||
        !only_own_slot(label + " (input)", in, seen_in, in_size, t, false)) return 1;
  }
  fputs(label.c_str(), stdout);
  for (size_t i = 0; i < n; i++) {
    uint32_t f; memcpy(&f, flags.p + 4 * i, 4);
    printf(" %u:", f);
    for (size_t k = 0; k < out_size; k++) printf("%02x", out.p[out_size * i + k]);
  }
  putchar('\n');
  return 0;
}

static void parse(const std::string& label, const std::string& hex) {
  const std::vector<uint8_t> b = bytes_of(hex);
  uint8_t* exact = (uint8_t*)malloc(b.size() ? b.size() : 1);
  if (!b.empty()) memcpy(exact, b.data(), b.size());
  KeyRuns R;
  const char* why = packed_key_layout(exact, b.size(), &R);
  if (why) printf("%s err %s\n", label.c_str(), why); else printf("%s ok %zu %zu %zu %zu\n", label.c_str(), R.n_g1, R.n_g2, R.words, R.pwords);
  free(exact);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: point_pack_check CASES.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  if (!vz::pairing::consts().ok) { fprintf(stderr, "pairing constants\n"); return 1; }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what, label, hex;
    if (!(ls >> what)) continue;
    if (!(ls >> label)) { fprintf(stderr, "a line without a label\n"); return 2; }
    int rc = 0;
    if (what == "PACK" || what == "UNPACK") {
      int group = 0, mont = 0; size_t n = 0;
      if (!(ls >> group >> mont >> n >> hex) || (group != 1 && group != 2) || !n || n > 4096) { fprintf(stderr, "bad %s\n", what.c_str()); return 2; }
      rc = group == 1 ? run<pack::Fq>(label, what == "PACK", mont != 0, n, bytes_of(hex)) : run<pack::Fq2>(label, what == "PACK", mont != 0, n, bytes_of(hex));
    }
    else if (what == "PARSE") { if (!(ls >> hex)) { fprintf(stderr, "bad PARSE\n"); return 2; } parse(label, hex); }
    else { fprintf(stderr, "bad line: %s\n", what.c_str()); return 2; }
    if (rc) return rc;
  }
  return 0;
}
