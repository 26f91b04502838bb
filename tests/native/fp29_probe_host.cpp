// Host run of the probe of the lazily reduced field (vimz_amd/csrc/fp29_probe.hpp): the very function the testing library's kernel calls, compiled
// with g++.  usage: fp29_probe_host IN OUT.  IN is a sequence of blocks [field, op, n : uint32][a, b, c, d : n x 9 uint32 each]; OUT receives the
// n x 9 result words of every block in order.  tests/_fp29_ref.py writes IN and checks OUT against Python integers.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fp29_probe.hpp"
using namespace vz;

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
  uint32_t hdr[3]; size_t blocks = 0, total = 0;
  while (fread(hdr, 4, 3, in) == 3) {
    const size_t n = hdr[2], W = FP29_PROBE_WORDS;
    std::vector<uint32_t> v(4 * n * W), o(n * W);
    if (fread(v.data(), 4, v.size(), in) != v.size()) { fprintf(stderr, "short block %zu\n", blocks); return 2; }
    const int op = (int)hdr[1];
    int rc = fp29_probe_field((int)hdr[0], [&](auto p) {
      typedef decltype(p) P; int bad = 0;
      for (size_t i = 0; i < n; i++) bad |= fp29_probe<P>(op, &v[i * W], &v[(n + i) * W], &v[(2 * n + i) * W], &v[(3 * n + i) * W], &o[i * W]);
      return bad;
    });
    if (rc) { fprintf(stderr, "block %zu: unknown field %u or operation %u\n", blocks, hdr[0], hdr[1]); return 3; }
    if (fwrite(o.data(), 4, o.size(), out) != o.size()) return 2;
    blocks++; total += n;
  }
  fclose(in); if (fclose(out)) return 2;
  printf("fp29 probe: %zu blocks, %zu operations\n", blocks, total);
  return 0;
}
