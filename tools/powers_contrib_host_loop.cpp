// The yardstick tools/powers_contrib_bench.py puts beside the GPU's contribution: the same per-point work (g16_point_stage.hpp: pt_power, then pt_scale_by with a
// different 254-bit scalar at every point) looped on HOST threads over N points of G1 — multiples of the generator, which cost what any point costs.
//     powers_contrib_host_loop N THREADS REPS   prints REPS lines "seconds" (the scaling alone; the power vector is made before the clock starts)
// No HIP: g++ -O3 -mbmi2 -madx -std=c++17 -pthread -I vimz_amd/csrc.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include "g16_powers_contrib.hpp"

using namespace vz;
using namespace vz::powc;

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: powers_contrib_host_loop N THREADS REPS\n"); return 2; }
  const size_t n = strtoull(argv[1], nullptr, 10);
  const unsigned threads = (unsigned)atoi(argv[2]);
  const int reps = atoi(argv[3]);
  if (!n || n > (1u << 24) || !threads || threads > 256 || reps < 1) { fprintf(stderr, "bad argument\n"); return 2; }
  Fr w = Fr::zero(), c = Fr::zero();
  for (int i = 0; i < 8; i++) { w.v[i] = 0x9e3779b9u * (i + 1); c.v[i] = 0x85ebca6bu * (i + 3); }
  w.v[7] &= 0x0fffffffu; c.v[7] &= 0x0fffffffu;      // below r, above 2^250 in all likelihood: a full walk
  w = Fr::to_mont(w); c = Fr::to_mont(c);
  G1A g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one());
  std::vector<G1A> pts(n), out(n);
  std::vector<uint32_t> pw(8 * n);
  int bits = 0; for (size_t v = n - 1; v; v >>= 1) bits++;
  auto run = [&](auto&& body) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++) th.emplace_back([&, t] { for (size_t i = n * t / threads; i < n * (t + 1) / threads; i++) body(i); });
    for (auto& x : th) x.join();
  };
  run([&](size_t i) { pt_power(i, bits, w, pw.data()); });
  run([&](size_t i) { uint32_t k[8] = {(uint32_t)i + 2, 0, 0, 0, 0, 0, 0, 0}; pts[i] = to_affine(pt_scalar_mul(g, k)); });
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    run([&](size_t i) { pt_scale_by(i, (const G1A*)pts.data(), (const uint32_t*)pw.data(), c, out.data()); });
    printf("%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  uint32_t sink = 0;
  for (const G1A& p : out) sink ^= p.x.v[0];
  fprintf(stderr, "checksum %08x\n", sink);
  return 0;
}
