// The yardstick tools/point_pack_bench.py puts beside the GPU's packing and unpacking: the same per-thread functions (g16_point_pack.hpp: pt_pack, pt_unpack — one
// exponentiation a G1 point unpacked, three a G2 point) looped on HOST threads over N points — small multiples of the generator, which cost what any point costs.
//     point_pack_host_loop GROUP N THREADS REPS   prints REPS lines "pack_seconds unpack_seconds"
// No HIP: g++ -O3 -mbmi2 -madx -std=c++17 -pthread -I vimz_amd/csrc.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#include "g16_point_pack.hpp"

using namespace vz;
using vz::pack::Fq;
using vz::pairing::Fq2;

static Fq fq_dec(const char* hex) {      // canonical words of a hex integer, then Montgomery
  Fq c = Fq::zero();
  int bit = 0;
  for (const char* e = hex + strlen(hex); e-- > hex; bit += 4) { const uint32_t d = *e <= '9' ? *e - '0' : *e - 'a' + 10; c.v[bit >> 5] |= d << (bit & 31); }
  return Fq::to_mont(c);
}
static void generator(Affine<Fq>* g, Fq* b) { g->x = Fq::one(); g->y = Fq::dbl(Fq::one()); *b = pairing::fq_u64(3); }
static void generator(Affine<Fq2>* g, Fq2* b) {      // the generator of G2 every BN254 library uses (EIP-197)
  g->x.c0 = fq_dec("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g->x.c1 = fq_dec("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g->y.c0 = fq_dec("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g->y.c1 = fq_dec("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
  *b = pairing::consts().twist_b;
}

template <class F>
static int loop(size_t n, unsigned threads, int reps) {
  Affine<F> g; F b;
  generator(&g, &b);
  std::vector<Affine<F>> pts(n), back(n);
  std::vector<uint32_t> packed(n * sizeof(F) / 4), flags(n);
  auto run = [&](auto&& body) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++) th.emplace_back([&, t] { for (size_t i = n * t / threads; i < n * (t + 1) / threads; i++) body(i); });
    for (auto& x : th) x.join();
  };
  run([&](size_t i) { uint32_t k[8] = {(uint32_t)i + 2, 0, 0, 0, 0, 0, 0, 0}; pts[i] = to_affine(pt_scalar_mul(g, k)); });      // (Montgomery words)
  for (int r = 0; r < reps; r++) {
    auto t0 = std::chrono::steady_clock::now();
    run([&](size_t i) { pt_pack(i, (const Affine<F>*)pts.data(), true, b, packed.data(), flags.data()); });
    const double t_pack = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    t0 = std::chrono::steady_clock::now();
    run([&](size_t i) { pt_unpack(i, (const uint32_t*)packed.data(), b, true, back.data(), flags.data()); });
    printf("%.6f %.6f\n", t_pack, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  size_t wrong = 0;
  for (size_t i = 0; i < n; i++) wrong += flags[i] != 0 || memcmp((const void*)&pts[i], (const void*)&back[i], sizeof(Affine<F>)) != 0;
  if (wrong) { fprintf(stderr, "%zu points did not come back\n", wrong); return 1; }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: point_pack_host_loop GROUP N THREADS REPS\n"); return 2; }
  const int group = atoi(argv[1]);
  const size_t n = strtoull(argv[2], nullptr, 10);
  const unsigned threads = (unsigned)atoi(argv[3]);
  const int reps = atoi(argv[4]);
  if ((group != 1 && group != 2) || !n || n > (1u << 24) || !threads || threads > 256 || reps < 1) { fprintf(stderr, "bad argument\n"); return 2; }
  if (!pairing::consts().ok) { fprintf(stderr, "pairing constants\n"); return 1; }
  return group == 1 ? loop<Fq>(n, threads, reps) : loop<Fq2>(n, threads, reps);
}
