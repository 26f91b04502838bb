// k_cf_open_chains: the commitment-opening chains of the full decider's check 5 on the GPU (decider_chains.hpp; the circuit: aug/decider_cf.hpp).
//
// 2 619 scalars at the real size (1 306 of the running CycleFold witness, 1 313 of its error vector), each a chain of 127 DEPENDENT affine additions
// acc += table[k][j][digit_j] with a slope that needs an inversion: nothing to share between the windows of one scalar, nothing but the table's
// generator index between scalars.  One thread per scalar, the inversion by Fermat in the thread (384 dependent products per window), workgroups of one
// wave so that the chains spread over as many SIMDs as there are waves (41 at the real size): what decides the time is the latency of ONE chain of
// ~55 000 dependent products, and that is shortest with a SIMD to itself (fp29.hpp's header).  Values are kept in the 8 x 32 Montgomery form the circuit's
// wires are in, so every word written is canonical as it stands.
#include "decider_chains.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

typedef Fp<BnFr> Fr;      // Grumpkin's coordinates, the decider circuit's field
typedef Fp<BnFq> FqS;     // Grumpkin's scalars: the CycleFold circuit's field

__device__ __forceinline__ void put_fr(uint32_t* __restrict__ dst, const Fr& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) dst[i] = a.v[i];
}

__global__ void __launch_bounds__(64) k_cf_open_chains(const Affine<Fr>* __restrict__ table, const Affine<Fr> H, const uint32_t* __restrict__ sW, uint32_t nW,
                                                       const uint32_t* __restrict__ sE, uint32_t nE, uint32_t* __restrict__ wires, uint32_t* __restrict__ ends,
                                                       uint32_t* __restrict__ bad) {
  const uint32_t t = blockIdx.x * 64u + threadIdx.x;
  if (t >= nW + nE) return;
  const uint32_t k = t < nW ? t : t - nW;      // the scalar's place in its vector = its generator
  const uint32_t* sp = t < nW ? sW + 8 * (size_t)k : sE + 8 * (size_t)k;
  FqS m;
#pragma unroll
  for (int i = 0; i < 8; i++) m.v[i] = sp[i];
  const FqS s = FqS::from_mont(m);             // canonical: its bits are the circuit's bit wires
  const Affine<Fr>* tk = table + (size_t)k * aug::CFO_WINDOWS * 4;
  uint32_t* o = wires + (size_t)t * CF_CHAIN_WORDS;
  const Fr one = Fr::one(), zero = Fr::zero();
  Affine<Fr> acc = H;
  bool same_x = false;
#pragma unroll 1
  for (int j = 0; j < aug::CFO_WINDOWS; j++) {
    const uint32_t d = (s.v[j >> 4] >> (2 * (j & 15))) & 3u;      // bit(2j) + 2·bit(2j + 1): both in word j / 16
    const Affine<Fr> q = tk[4 * j + d];
    const Fr den = Fr::sub(q.x, acc.x);
    same_x = same_x || den.is_zero();
    const Fr lam = Fr::mul(Fr::sub(q.y, acc.y), Fr::pow_pm2(den));
    Affine<Fr> r;
    r.x = Fr::sub(Fr::sub(Fr::sqr(lam), acc.x), q.x);
    r.y = Fr::sub(Fr::mul(lam, Fr::sub(acc.x, r.x)), acc.y);
    put_fr(o + 32 * j, d == 3u ? one : zero); put_fr(o + 32 * j + 8, lam); put_fr(o + 32 * j + 16, r.x); put_fr(o + 32 * j + 24, r.y);
    acc = r;
  }
  put_fr(ends + 16 * (size_t)t, acc.x); put_fr(ends + 16 * (size_t)t + 8, acc.y);
  if (same_x) *bad = 1u;      // (a plain store: whoever writes, writes 1)
}

}  // namespace

hipError_t cf_chains_key_upload(hipStream_t s, const aug::CfOpeningKey& key, CfChainsKey& out) {
  const size_t bytes = sizeof(Affine<Fe>) * key.table.size();
  if (!key.n || key.table.size() != (size_t)key.n * aug::CFO_WINDOWS * 4) return hipErrorInvalidValue;
  hipError_t e = hipMalloc((void**)&out.table, bytes);
  if (e != hipSuccess) { out.table = nullptr; return e; }
  out.H = key.H; out.n = key.n;
  e = hipMemcpyAsync(out.table, key.table.data(), bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) cf_chains_key_free(out);
  return e;
}
void cf_chains_key_free(CfChainsKey& k) {
  if (k.table) hipFree(k.table);
  k.table = nullptr; k.n = 0;
}
hipError_t cf_chains_launch(hipStream_t s, const CfChainsKey& key, const uint32_t* sW, uint32_t nW, const uint32_t* sE, uint32_t nE, uint32_t* wires,
                            uint32_t* ends, uint32_t* bad) {
  if (!key.table || nW > key.n || nE > key.n || !(nW + nE)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(bad, 0, 4, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cf_open_chains, dim3((nW + nE + 63) / 64), dim3(64), 0, s, (const Affine<Fr>*)key.table, key.H, sW, nW, sE, nE, wires, ends, bad);
  return hipGetLastError();
}

#ifdef VIMZ_TESTING
extern "C" int vimz_test_decider_chains(vimz_ctx* ctx, int where, const uint64_t* gens_xy, size_t n_gens, const uint64_t* scalars, size_t cnt, uint64_t* wires_out,
                                        uint64_t* ends_out, uint64_t h_out[8], int* bad_out) {
  if ((where != 0 && where != 1) || (where == 1 && !ctx) || !gens_xy || !scalars || !wires_out || !ends_out || !h_out || !bad_out)
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_decider_chains: bad argument");
  if (!cnt || cnt > n_gens || n_gens > (1u << 16)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_decider_chains: needs 0 < cnt <= n_gens <= 2^16");
  std::vector<Affine<Fe>> gens(n_gens);
  for (size_t k = 0; k < n_gens; k++) {
    Fe x, y; memcpy(x.v, gens_xy + 8 * k, 32); memcpy(y.v, gens_xy + 8 * k + 4, 32);
    if (!x.is_reduced() || !y.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_decider_chains: a coordinate is not below the modulus");
    gens[k].x = Fe::to_mont(x); gens[k].y = Fe::to_mont(y);
  }
  std::vector<Fq> sc(cnt);      // Montgomery, as Zrun holds them
  std::vector<aug::U256w> vals(cnt);
  for (size_t k = 0; k < cnt; k++) {
    Fq c; memcpy(c.v, scalars + 4 * k, 32);
    if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_decider_chains: a scalar is not below the modulus");
    sc[k] = Fq::to_mont(c); memcpy(vals[k].w, scalars + 4 * k, 32);
  }
  aug::CfOpeningKey key;
  key.build(gens.data(), (uint32_t)n_gens);
  { const Fe c = Fe::from_mont(key.H.x); memcpy(h_out, c.v, 32); } { const Fe c = Fe::from_mont(key.H.y); memcpy(h_out + 4, c.v, 32); }
  std::vector<Fe> wires(cnt * (size_t)aug::CFO_WINDOWS * 4);
  std::vector<Affine<Fe>> ends(cnt);
  uint32_t bad = 0;
  if (where == 0) {
    bad = aug::cf_open_chains_host(key, vals.data(), (uint32_t)cnt, wires.data(), ends.data()) ? 0 : 1;
  } else {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CfChainsKey dk;
    uint32_t* dev = nullptr;      // scalars, wires, end points, the flag
    struct Free { CfChainsKey* k; uint32_t** d; ~Free() { cf_chains_key_free(*k); if (*d) hipFree(*d); } } fr{&dk, &dev};
    P_TRY(cf_chains_key_upload(s, key, dk));
    // Both openings in one grid, as the prover launches them: the scalars once as the witness's vector and once as the error vector's (scalar k of either uses
    // generator k), so a wave that straddles the two vectors is covered too.  The second opening must repeat the first word for word.
    const size_t w_sc = 8 * cnt, w_wi = CF_CHAIN_WORDS * cnt, w_en = 16 * cnt;
    P_TRY(hipMalloc((void**)&dev, 4 * (w_sc + 2 * w_wi + 2 * w_en + 1)));
    uint32_t *d_sc = dev, *d_wi = d_sc + w_sc, *d_en = d_wi + 2 * w_wi, *d_bad = d_en + 2 * w_en;
    P_TRY(hipMemcpyAsync(d_sc, sc.data(), 4 * w_sc, hipMemcpyHostToDevice, s));
    P_TRY(cf_chains_launch(s, dk, d_sc, (uint32_t)cnt, d_sc, (uint32_t)cnt, d_wi, d_en, d_bad));
    std::vector<Fe> wires2(wires.size()); std::vector<Affine<Fe>> ends2(cnt);
    P_TRY(hipMemcpyAsync(wires.data(), d_wi, 4 * w_wi, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(wires2.data(), d_wi + w_wi, 4 * w_wi, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(ends.data(), d_en, 4 * w_en, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(ends2.data(), d_en + w_en, 4 * w_en, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
    if (!bad && (memcmp(wires.data(), wires2.data(), 4 * w_wi) || memcmp(ends.data(), ends2.data(), 4 * w_en)))
      return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_decider_chains: the two openings of one launch differ");
  }
  *bad_out = (int)bad;
  for (size_t i = 0; i < wires.size(); i++) { const Fe c = Fe::from_mont(wires[i]); memcpy(wires_out + 4 * i, c.v, 32); }
  for (size_t k = 0; k < cnt; k++) { const Fe x = Fe::from_mont(ends[k].x), y = Fe::from_mont(ends[k].y); memcpy(ends_out + 8 * k, x.v, 32); memcpy(ends_out + 8 * k + 4, y.v, 32); }
  return VIMZ_OK;
}
#endif
