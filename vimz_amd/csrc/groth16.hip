// vimz_decider_*: the decider of the Nova + CycleFold path — the Groth16 proof the reference's Sonobe backend makes of its final fold before
// the proof goes on chain (`DeciderEth<.., Groth16<Bn254>, ..>`, vimz/src/sonobe_backend/decider.rs:13-21; `Decider::preprocess` / `prove`,
// mod.rs:72-78; eight of the 25 calldata words, solidity.rs:13-27, contracts/*Verifier.sol:785-810).  Groth16 over BN254 is a published
// protocol (Groth, EUROCRYPT 2016; verification equation as the EVM's pairing precompile evaluates it); the circuit it proves here is ours
// (aug/decider.hpp), as is the deterministic TEST setup — the toxic waste is derived from a caller's seed, where Sonobe draws its keys from
// `StdRng::from_seed([41; 32])` (mod.rs:54) inside crates that are not vendored: proofs are checked by the oracle-side pairing
// (tests/_pairing.py), not by the reference's contracts.  Parity unpinned, like every layer above the step relation.
//
// On the GPU: the radix-2 NTTs over BN254 Fr that turn (A·z, B·z, C·z) into the quotient polynomial h, the three G1 multi-scalar
// multiplications of a proof over the key's queries (the Pippenger of msm.hpp), the G2 one (per-point double-and-add over Fq2 and a host sum:
// one MSM of ~10^6 points per proof, not a hot loop), and the fixed-base multiplications that make the keys.  On the host: the circuit
// (synthesis, witness, its sparse products — 10^6 rows of a few terms), the QAP evaluation at the trapdoor, the final point arithmetic.
#include <sys/random.h>
#include <functional>
#include <map>
#include <thread>
#include "cyclefold_internal.hpp"
#include "decider_view.hpp"
#include "aug/decider.hpp"
#include "decider_chains.hpp"
#include "g16_powers.hpp"
#include "g16_key_contrib.hpp"
#include "g16_key_origin.hpp"
#include "decider_verify.hpp"
#include "vecops_api.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

// check 5's chains of the full decider: on the device unless VIMZ_DECIDER_CHAINS=host (profiles/decider_chains.txt: the measurement the default follows)
constexpr bool DECIDER_CHAINS_GPU_DEFAULT = true;

// Secrets are wiped when they go out of scope: the trapdoor, everything derived from it that still determines it (powers of tau, the
// Lagrange basis at tau, the query scalars), a proof's blinders.
void wipe(void* p, size_t n) { explicit_bzero(p, n); }
template <class T> void wipe(std::vector<T>& v) { if (!v.empty()) explicit_bzero(v.data(), v.size() * sizeof(T)); }

// ---- Fq2 = Fq[u] / (u² + 1): coordinates of G2 (the twist y² = x³ + 3/(9 + u)) — pairing.hpp ------------------------------------------------
using vz::pairing::Fq2;
typedef Affine<Fq2> G2PAff;      // a point of BN254 G2
typedef XYZZ<Fq2> G2P;

Fq fq_from_dec_limbs(const uint64_t w[4]) { Fq c; memcpy(c.v, w, 32); return Fq::to_mont(c); }
G2PAff g2_generator() {
  // (10857046999023057135944570762232829481370756359578518086990519993285655852781 + 11559732032986387107991004021392285783925812861821192530917403151452391805634 u,
  //   8495653923123431417604973247489272438418190587263600148770280649306958101930 +  4082367875863433681332203403145435568316851327593401208105741076214120093531 u)
  static const uint64_t x0[4] = {0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull};
  static const uint64_t x1[4] = {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull};
  static const uint64_t y0[4] = {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull};
  static const uint64_t y1[4] = {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull};
  G2PAff g; g.x.c0 = fq_from_dec_limbs(x0); g.x.c1 = fq_from_dec_limbs(x1); g.y.c0 = fq_from_dec_limbs(y0); g.y.c1 = fq_from_dec_limbs(y1);
  return g;
}
G1Aff g1_generator() { G1Aff g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
using vz::pairing::g2_on_curve;

// ---- host helpers over Fr -----------------------------------------------------------------------------------------------------------------
Fe fr_pow(Fe base, const uint32_t e[8]) {
  Fe acc = Fe::one();
  for (int i = 255; i >= 0; i--) { acc = Fe::sqr(acc); if ((e[i >> 5] >> (i & 31)) & 1u) acc = Fe::mul(acc, base); }
  return acc;
}
Fe fr_pow_u64(Fe base, uint64_t e) { uint32_t w[8] = {(uint32_t)e, (uint32_t)(e >> 32), 0, 0, 0, 0, 0, 0}; return fr_pow(base, w); }
Fe fr_from_hash(const void* seed, size_t n, const char* tag) {      // an element of Fr from SHA3-256(seed ‖ tag): 248 bits, never zero in practice
  Sha3 h; h.update(seed, n); h.update(tag, strlen(tag));
  uint8_t d[32]; h.finish(d); d[31] = 0;
  Fe c; memcpy(c.v, d, 32);
  return Fe::to_mont(c);
}
}  // namespace
// a primitive 2^k-th root of unity of Fr: 5 generates the multiplicative group, r - 1 = 2^28 · odd  (g16_powers.hpp: the transform over points uses it too)
Fe fr_root_of_unity(int k) {
  uint32_t e[8]; uint64_t br = 1;
  for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)BnFr::MOD.w[i] - br; e[i] = (uint32_t)d; br = (d >> 32) & 1; }      // r - 1
  for (int s = 0; s < k; s++) { for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? e[i + 1] << 31 : 0u); }                 // >> k (exact: k <= 28)
  return fr_pow(cb::f_from_u64<Fe>(5), e);
}
namespace {

// ---- kernels --------------------------------------------------------------------------------------------------------------------------------
// out[i] = s_i · G for a fixed base G: T[w][d] = d · 2^(4w) · G (64 windows of 16 multiples) turns a multiplication into at most 64 mixed additions
template <class F>
__global__ void __launch_bounds__(128) k_fixed_mul(const uint32_t* __restrict__ scalars /* canonical words */, size_t n, const Affine<F>* __restrict__ table, Affine<F>* __restrict__ out) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t s[8];
  for (int k = 0; k < 8; k++) s[k] = scalars[8 * i + k];
  XYZZ<F> acc = XYZZ<F>::identity();
  for (int w = 0; w < 64; w++) {
    const uint32_t d = (s[w >> 3] >> (4 * (w & 7))) & 15u;
    if (d) { const Affine<F> q = table[16 * w + d]; add_mixed(acc, q); }
  }
  out[i] = to_affine(acc);
}
// The G2 multi-scalar multiplication of a proof, Σ z_i·[b_i]_2 over the wires whose query point is not the identity, BIT PLANE BY BIT PLANE:
//     Σ_i s_i·P_i = Σ_j 2^j·S_j,   S_j = Σ_{i: bit j of s_i} P_i
// — no doublings on the device (a per-point double-and-add spends two thirds of its additions on them and ran 2.0 s for the full decider's 0.7 M
// full-size scalars: a quarter of the threads held all the work), no sorting: plane j is a filtered sum.  A wave walks 64 consecutive scalars at a time,
// queues the indices whose bit j is set in LDS (ballot + prefix count: the compaction of msm.hpp's k_ones_dense) and adds 64 queued bases at a time, one per
// lane.  blockIdx.y = the plane; partial[plane][thread]; k_g2_plane_tree folds a plane's partials; the host adds the 254 plane sums by Horner.
constexpr uint32_t G2_PLANE_THREADS = 2048, G2_PLANES = 254;
__global__ void __launch_bounds__(256) k_g2_canon(const uint32_t* __restrict__ scalars_mont, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_fe(out, i, Fr::from_mont(load_fe<Fr>(scalars_mont, idx[i])));
}
__global__ void __launch_bounds__(256) k_g2_planes(const Affine<Fq2>* __restrict__ bases, const uint32_t* __restrict__ canon, uint32_t n, XYZZ<Fq2>* __restrict__ partial) {
  __shared__ uint32_t queue[4][128];
  const uint32_t plane = blockIdx.y, word = plane >> 5, bit = plane & 31u;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t wave = t >> 6, nwaves = G2_PLANE_THREADS / 64;
  volatile uint32_t* q = queue[wv];
  XYZZ<Fq2> acc = XYZZ<Fq2>::identity();
  uint32_t cnt = 0;                                     // (wave-uniform)
  for (uint32_t base = wave * 64; base < n; base += nwaves * 64) {
    const uint32_t i = base + lane;
    const bool on = i < n && ((canon[8 * (size_t)i + word] >> bit) & 1u);
    const uint64_t m = __ballot(on);
    if (on) q[cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
    cnt += (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
    if (cnt >= 64) {
      cnt -= 64;
      const uint32_t ix = q[cnt + lane];
      __builtin_amdgcn_wave_barrier();
      const Affine<Fq2> pt = bases[ix];
      add_mixed(acc, pt);
    }
  }
  if (lane < cnt) { const Affine<Fq2> pt = bases[q[lane]]; add_mixed(acc, pt); }
  partial[(size_t)plane * G2_PLANE_THREADS + t] = acc;
}
__global__ void __launch_bounds__(128) k_g2_plane_tree(const XYZZ<Fq2>* __restrict__ partial, XYZZ<Fq2>* __restrict__ out) {
  __shared__ XYZZ<Fq2> sh[128];
  const uint32_t plane = blockIdx.x, t = threadIdx.x;
  XYZZ<Fq2> acc = XYZZ<Fq2>::identity();
  for (uint32_t k = t; k < G2_PLANE_THREADS; k += 128) add_full(acc, partial[(size_t)plane * G2_PLANE_THREADS + k]);
  sh[t] = acc;
  __syncthreads();
  for (uint32_t h = 64; h >= 1; h >>= 1) {
    if (t < h) { XYZZ<Fq2> a = sh[t]; add_full(a, sh[t + h]); sh[t] = a; }
    __syncthreads();
  }
  if (t == 0) out[plane] = sh[0];
}
// tw[k] = base^k
__global__ void k_pow_table(uint32_t* __restrict__ out, size_t n, Fr base) {
  const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (k >= n) return;
  Fr acc = Fr::one(), b = base;
  for (size_t e = k; e; e >>= 1) { if (e & 1) acc = Fr::mul(acc, b); b = Fr::sqr(b); }
  store_fe(out, k, acc);
}
__global__ void k_bitrev(uint32_t* __restrict__ a, uint32_t n, int logn) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = __brev(i) >> (32 - logn);
  if (i < j) { const Fr x = load_fe<Fr>(a, i), y = load_fe<Fr>(a, j); store_fe(a, i, y); store_fe(a, j, x); }
}
// one radix-2 stage (decimation in time over bit-reversed input): butterflies of span `half`, twiddle ω^(j · n / (2 half))
__global__ void k_ntt_stage(uint32_t* __restrict__ a, uint32_t n, uint32_t half, const uint32_t* __restrict__ tw) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n / 2) return;
  const uint32_t j = t & (half - 1), i0 = ((t - j) << 1) + j, i1 = i0 + half;
  const Fr w = load_fe<Fr>(tw, (size_t)j * (n / (2 * half)));
  const Fr u = load_fe<Fr>(a, i0), v = Fr::mul(load_fe<Fr>(a, i1), w);
  store_fe(a, i0, Fr::add(u, v)); store_fe(a, i1, Fr::sub(u, v));
}
// a[i] *= s · g^i   (coset shift and its inverse; the 1/n of an inverse transform rides in s)
__global__ void k_scale_pow(uint32_t* __restrict__ a, uint32_t n, Fr s, Fr g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr acc = s, b = g;
  for (uint32_t e = i; e; e >>= 1) { if (e & 1) acc = Fr::mul(acc, b); b = Fr::sqr(b); }
  store_fe(a, i, Fr::mul(load_fe<Fr>(a, i), acc));
}
// a[i] = (a[i]·b[i] − c[i]) · zinv
__global__ void k_quotient(uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c, uint32_t n, Fr zinv) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_fe(a, i, Fr::mul(Fr::sub(Fr::mul(load_fe<Fr>(a, i), load_fe<Fr>(b, i)), load_fe<Fr>(c, i)), zinv));
}

// ---- the key --------------------------------------------------------------------------------------------------------------------------------
struct G16Key {
  uint32_t m = 0, n_pub = 0, n_c = 0, n = 0; int logn = 0;      // wires, public inputs (without the constant), constraints, domain
  Fe omega, omega_inv, n_inv, coset, coset_inv, zinv;           // domain constants (coset generator 5: Z(5·ω^i) = 5^n − 1)
  uint32_t *tw = nullptr, *tw_inv = nullptr;                    // ω^k, ω^-k for k < n/2
  vimz_bases *a_q = nullptr, *b1_q = nullptr, *l_q = nullptr, *h_q = nullptr;      // G1 queries (a, b: m points; l: private wires; h: n − 1)
  G2PAff* b2_q = nullptr; uint32_t* b2_idx = nullptr; uint32_t n_b2 = 0;      // G2 query: the n_b2 wires whose point is not the identity (device: points, wire numbers)
  G1Aff alpha1, beta1, delta1; G2PAff beta2, gamma2, delta2;
  std::vector<G1Aff> ic;                                        // n_pub + 1 points
};
void free_key_raw(G16Key& K) {      // (not vimz_bases_free: it takes the context's lock, which callers on an error path hold)
  for (vimz_bases** b : {&K.a_q, &K.b1_q, &K.l_q, &K.h_q}) if (*b) {
    if ((*b)->d) hipFree((*b)->d);
    if ((*b)->tables) hipFree((*b)->tables);
    for (auto& t : (*b)->small) { if (t.rows) hipFree(t.rows); if (t.mult) hipFree(t.mult); }
    delete *b; *b = nullptr;
  }
  if (K.b2_q) hipFree(K.b2_q); K.b2_q = nullptr;
  if (K.b2_idx) hipFree(K.b2_idx); K.b2_idx = nullptr;
  if (K.tw) hipFree(K.tw); if (K.tw_inv) hipFree(K.tw_inv); K.tw = K.tw_inv = nullptr;
}
}  // namespace

struct vimz_decider {
  vimz_cf* vk = nullptr; vimz_ctx* ctx = nullptr;
  aug::DeciderCircuit circ;
  G16Key key;
  G2PAff kzg_vk;                         // [tau]G2 of the SRS the prover's ck_main is made of (identity: not given — KZG checks are refused)
  double setup_s[4] = {0, 0, 0, 0};      // circuit synthesis, QAP evaluation at the trapdoor (host), key points (GPU), total
  // Full decider only (a light one allocates none of it): check 5's chains on the device — the opening key's window table, the kernel's outputs, their
  // pinned copies on the host, a stream of its own (the kernel runs beside the prover's final fold) and the two events that time it.  mu: one prove at a time uses them,
  // from before its final fold until its witness is done; taken BEFORE the context's lock, never while holding it.
  struct Chains {
    CfChainsKey key;
    uint32_t nW = 0, nE = 0;
    uint32_t* dev = nullptr;             // wires of W's and E's chains, their end points, the flag
    uint32_t* host = nullptr;            // the same, pinned
    hipStream_t stream = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::mutex mu;
    size_t wire_words() const { return CF_CHAIN_WORDS * ((size_t)nW + nE); }
    size_t words() const { return wire_words() + 16 * ((size_t)nW + nE) + 1; }
  } chains;
  void free_chains() {
    cf_chains_key_free(chains.key);
    if (chains.dev) hipFree(chains.dev); if (chains.host) hipHostFree(chains.host);
    if (chains.ev0) hipEventDestroy(chains.ev0); if (chains.ev1) hipEventDestroy(chains.ev1);
    if (chains.stream) hipStreamDestroy(chains.stream);
    chains.dev = chains.host = nullptr; chains.ev0 = chains.ev1 = nullptr; chains.stream = nullptr;
  }
  ~vimz_decider() { if (ctx) { hipSetDevice(ctx->device); free_key_raw(key); free_chains(); } }      // (error paths of the setup end here too; vimz_decider_free)
};

namespace {

template <class F> std::vector<Affine<F>> fixed_table(const Affine<F>& g) {      // T[w][d] = d · 2^(4w) · g on the host
  std::vector<Affine<F>> T(64 * 16);
  XYZZ<F> base = from_affine(g);
  for (int w = 0; w < 64; w++) {
    const Affine<F> b = to_affine(base);
    XYZZ<F> acc = XYZZ<F>::identity();
    T[16 * w].x = F::zero(); T[16 * w].y = F::zero();
    for (int d = 1; d < 16; d++) { add_mixed(acc, b); T[16 * w + d] = to_affine(acc); }
    for (int k = 0; k < 4; k++) base = dbl(base);
  }
  return T;
}
template <class F> XYZZ<F> host_mul_fr(const Affine<F>& p, const Fe& k_mont) {
  const Fe c = Fe::from_mont(k_mont);
  XYZZ<F> acc = XYZZ<F>::identity();
  for (int i = 255; i >= 0; i--) { acc = dbl(acc); if ((c.v[i >> 5] >> (i & 31)) & 1u) add_mixed(acc, p); }
  return acc;
}

// scalars (Montgomery, host) -> s_i · G as device affine points (standard Montgomery coordinates)
template <class F>
hipError_t fixed_base_batch(hipStream_t s, const std::vector<Fe>& sc, const Affine<F>* d_table, Affine<F>** d_out) {
  const size_t n = sc.size();
  std::vector<uint32_t> canon(8 * std::max<size_t>(n, 1));
  for (size_t i = 0; i < n; i++) { const Fe c = Fe::from_mont(sc[i]); memcpy(&canon[8 * i], c.v, 32); }
  uint32_t* d_sc = nullptr;
  hipError_t e = hipMalloc((void**)&d_sc, 32 * std::max<size_t>(n, 1)); if (e != hipSuccess) return e;
  e = hipMalloc((void**)d_out, sizeof(Affine<F>) * std::max<size_t>(n, 1)); if (e != hipSuccess) { hipFree(d_sc); return e; }
  e = hipMemcpyAsync(d_sc, canon.data(), 32 * n, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n) hipLaunchKernelGGL(k_fixed_mul<F>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, d_sc, n, d_table, *d_out);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(d_sc);
  wipe(canon);
  return e;
}
// device std-form G1 points -> a commitment key in the MSM's resident form
int bases_from_device(vimz_ctx* ctx, const G1Aff* d_pts, size_t n, vimz_bases** out, int canonical = 0) {
  vimz_bases* b = new vimz_bases(); b->curve = VIMZ_CURVE_BN254_G1; b->n = n; b->d = nullptr;
  if (n) {
    hipError_t e = hipMalloc(&b->d, 4 * (size_t)AFFINE_WORDS * n);
    if (e != hipSuccess) { delete b; return vz_fail(ctx, VIMZ_ERR_HIP, "decider: hipMalloc(query)", e); }
    launch_points_to_internal<Fq>(ctx->stream, (const uint32_t*)d_pts, canonical, b->d, n);
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { hipFree(b->d); delete b; return vz_fail(ctx, VIMZ_ERR_HIP, "decider: query conversion", e); }
  }
  *out = b;
  return VIMZ_OK;
}

hipError_t ntt(hipStream_t s, uint32_t* d, const G16Key& K, bool inverse) {
  hipLaunchKernelGGL(k_bitrev, dim3((K.n + 255) / 256), dim3(256), 0, s, d, K.n, K.logn);
  for (uint32_t half = 1; half < K.n; half <<= 1)
    hipLaunchKernelGGL(k_ntt_stage, dim3((K.n / 2 + 255) / 256), dim3(256), 0, s, d, K.n, half, (const uint32_t*)(inverse ? K.tw_inv : K.tw));
  return hipGetLastError();
}
// ---- the domain H of n = 2^logn points: its constants (host), then its twiddle tables (device; the caller holds the context's lock) ------------------
// false: Fr has no primitive root of unity of that order (logn beyond 26 is refused: the kernels index with 32 bits)
bool domain_constants(G16Key& K, int logn) {
  if (logn < 0 || logn > 26) return false;
  K.logn = logn; K.n = 1u << logn;
  K.omega = fr_root_of_unity(K.logn); K.omega_inv = Fe::pow_pm2(K.omega);
  K.n_inv = Fe::pow_pm2(cb::f_from_u64<Fe>(K.n));
  K.coset = cb::f_from_u64<Fe>(5); K.coset_inv = Fe::pow_pm2(K.coset);
  K.zinv = Fe::pow_pm2(Fe::sub(fr_pow_u64(K.coset, K.n), Fe::one()));
  const Fe chk = fr_pow_u64(K.omega, K.n / 2);
  return K.n == 1 || Fe::add(chk, Fe::one()).is_zero();
}
int domain_tables(vimz_ctx* ctx, hipStream_t s, G16Key& K) {
  P_TRY(hipMalloc((void**)&K.tw, 32 * (size_t)std::max<uint32_t>(K.n / 2, 1))); P_TRY(hipMalloc((void**)&K.tw_inv, 32 * (size_t)std::max<uint32_t>(K.n / 2, 1)));
  Fr w, wi; memcpy(w.v, K.omega.v, 32); memcpy(wi.v, K.omega_inv.v, 32);
  hipLaunchKernelGGL(k_pow_table, dim3((K.n / 2 + 255) / 256), dim3(256), 0, s, K.tw, (size_t)K.n / 2, w);
  hipLaunchKernelGGL(k_pow_table, dim3((K.n / 2 + 255) / 256), dim3(256), 0, s, K.tw_inv, (size_t)K.n / 2, wi);
  P_TRY(hipGetLastError()); P_TRY(hipStreamSynchronize(s));
  return VIMZ_OK;
}
Fr as_fr(const Fe& x) { Fr r; memcpy(r.v, x.v, 32); return r; }
// evaluations over H -> evaluations over the coset 5·H, in place
hipError_t coset_extend(hipStream_t s, uint32_t* d, const G16Key& K) {
  hipError_t e = ntt(s, d, K, true); if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scale_pow, dim3((K.n + 255) / 256), dim3(256), 0, s, d, K.n, as_fr(K.n_inv), as_fr(K.coset));
  return ntt(s, d, K, false);
}
// h = (a·b − c) / Z on the coset 5·H: dv[0..2] = (A·z, B·z, C·z) over H; dv[0] leaves as the n coefficients of h, dv[1] and dv[2] are spent.  Not synchronized.
hipError_t quotient(hipStream_t s, uint32_t* const dv[3], const G16Key& K) {
  const unsigned gb = (K.n + 255) / 256;
  for (int q = 0; q < 3; q++) { const hipError_t e = coset_extend(s, dv[q], K); if (e != hipSuccess) return e; }
  hipLaunchKernelGGL(k_quotient, dim3(gb), dim3(256), 0, s, dv[0], (const uint32_t*)dv[1], (const uint32_t*)dv[2], K.n, as_fr(K.zinv));
  const hipError_t e = ntt(s, dv[0], K, true); if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_scale_pow, dim3(gb), dim3(256), 0, s, dv[0], K.n, as_fr(K.n_inv), as_fr(K.coset_inv));
  return hipGetLastError();
}
// Σ_i z[idx_i]·P_i over n G2 points, bit plane by bit plane (k_g2_planes): bases, wires (Montgomery) and wire numbers on the device; canon = 8 n words of
// device scratch for the canonical scalars; the 254 plane sums are added on the host by Horner
int g2_msm(vimz_ctx* ctx, hipStream_t s, const G2PAff* bases, const uint32_t* wires, const uint32_t* idx, uint32_t n, uint32_t* canon, G2P* out) {
  G2P sum = G2P::identity();
  if (n) {
    G2P* dpart = nullptr;
    P_TRY(hipMalloc((void**)&dpart, sizeof(G2P) * ((size_t)G2_PLANES * G2_PLANE_THREADS + G2_PLANES)));
    struct FreePart { G2P* p; ~FreePart() { hipFree(p); } } fp{dpart};
    G2P* dsum = dpart + (size_t)G2_PLANES * G2_PLANE_THREADS;
    hipLaunchKernelGGL(k_g2_canon, dim3((n + 255) / 256), dim3(256), 0, s, wires, idx, n, canon);
    hipLaunchKernelGGL(k_g2_planes, dim3(G2_PLANE_THREADS / 256, G2_PLANES), dim3(256), 0, s, bases, (const uint32_t*)canon, n, dpart);
    hipLaunchKernelGGL(k_g2_plane_tree, dim3(G2_PLANES), dim3(128), 0, s, (const G2P*)dpart, dsum);
    P_TRY(hipGetLastError());
    std::vector<G2P> planes(G2_PLANES);
    P_TRY(hipMemcpyAsync(planes.data(), dsum, sizeof(G2P) * G2_PLANES, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
    for (int j = (int)G2_PLANES - 1; j >= 0; j--) { sum = dbl(sum); add_full(sum, planes[j]); }
  }
  *out = sum;
  return VIMZ_OK;
}

// (A,B,C)·z of a builder's CSR on the host threads
template <class FF>
void host_spmv3(const cb::BuilderT<FF>& b, const std::vector<FF>& z, std::vector<FF>* out /* [3] of n_c */) {
  typedef FF Fe;
  const uint32_t nc = b.n_constraints();
  const cb::Csr* Ms[3] = {&b.A, &b.B, &b.C};
  for (int m = 0; m < 3; m++) out[m].assign(nc, Fe::zero());
  const unsigned T = std::max(1u, std::min(16u, usable_cpus()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; t++) th.emplace_back([&, t] {
    const uint32_t lo = (uint32_t)((uint64_t)nc * t / T), hi = (uint32_t)((uint64_t)nc * (t + 1) / T);
    for (int m = 0; m < 3; m++) for (uint32_t r = lo; r < hi; r++) {
      Fe acc = Fe::zero();
      for (uint32_t k = Ms[m]->row_ptr[r]; k < Ms[m]->row_ptr[r + 1]; k++) acc = Fe::add(acc, Fe::mul(b.dict[Ms[m]->coef[k]], z[Ms[m]->col[k]]));
      out[m][r] = acc;
    }
  });
  for (auto& x : th) x.join();
}

}  // namespace


namespace {

// ---- randomness: the toxic waste of a locally run setup and a proof's blinding scalars come from the OS -------------------------------------------
bool os_random(void* buf, size_t n) {
  uint8_t* p = (uint8_t*)buf;
  while (n) { const ssize_t k = getrandom(p, n, 0); if (k <= 0) return false; p += k; n -= (size_t)k; }
  return true;
}
struct Trapdoor { Fe tau, alpha, beta, gamma, delta; ~Trapdoor() { wipe(this, sizeof(*this)); } };
// a uniform non-zero element of Fr by rejection (254-bit draws below the modulus: accepted with probability 0.76)
bool fr_random(Fe* out) {
  for (;;) {
    uint8_t raw[32];
    if (!os_random(raw, sizeof(raw))) return false;
    raw[31] &= 0x3f;
    Fe c; memcpy(c.v, raw, 32);
    wipe(raw, sizeof(raw));
    if (!c.is_reduced() || c.is_zero()) continue;
    *out = Fe::to_mont(c);
    wipe(&c, sizeof(c));
    return true;
  }
}
bool trapdoor_random(Trapdoor& t) {
  Fe* dst[5] = {&t.tau, &t.alpha, &t.beta, &t.gamma, &t.delta};
  for (int k = 0; k < 5; k++) if (!fr_random(dst[k])) return false;
  return true;
}
Trapdoor trapdoor_seeded(const uint8_t* seed, size_t n) {
  Trapdoor t;
  t.tau = fr_from_hash(seed, n, "vimz-decider-tau"); t.alpha = fr_from_hash(seed, n, "vimz-decider-alpha"); t.beta = fr_from_hash(seed, n, "vimz-decider-beta");
  t.gamma = fr_from_hash(seed, n, "vimz-decider-gamma"); t.delta = fr_from_hash(seed, n, "vimz-decider-delta");
  return t;
}
void put_fq(uint64_t* dst, const Fq& mont) { const Fq c = Fq::from_mont(mont); memcpy(dst, c.v, 32); }
bool get_fq(const uint64_t* src, Fq* out) { Fq c; memcpy(c.v, src, 32); if (!c.is_reduced()) return false; *out = Fq::to_mont(c); return true; }
void put_g2(uint64_t* dst, const G2PAff& p) { put_fq(dst, p.x.c0); put_fq(dst + 4, p.x.c1); put_fq(dst + 8, p.y.c0); put_fq(dst + 12, p.y.c1); }
bool get_g2(const uint64_t* src, G2PAff* p) { return get_fq(src, &p->x.c0) && get_fq(src + 4, &p->x.c1) && get_fq(src + 8, &p->y.c0) && get_fq(src + 12, &p->y.c1); }
bool get_g1(const uint64_t* src, G1Aff* p) { return get_fq(src, &p->x) && get_fq(src + 4, &p->y); }
U256w u256_of(const uint64_t* w) { U256w r; memcpy(r.w, w, 32); return r; }

// KZG::setup: srs[i] = [tau^i]G1 for i < n (resident MSM form), vk = [tau]G2
int kzg_setup_impl(vimz_ctx* ctx, const Fe& tau, size_t n, vimz_bases** srs_out, uint64_t vk_g2_out[16]) {
  std::vector<Fe> pw(n);
  struct Wipe { std::vector<Fe>& v; ~Wipe() { wipe(v); } } wp{pw};
  { Fe t = Fe::one(); for (size_t i = 0; i < n; i++) { pw[i] = t; t = Fe::mul(t, tau); } }
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  const std::vector<G1Aff> T1 = fixed_table<Fq>(g1_generator());
  G1Aff* dT1 = nullptr;
  P_TRY(hipMalloc((void**)&dT1, sizeof(G1Aff) * T1.size()));
  struct Tab { G1Aff* a; ~Tab() { hipFree(a); } } tab{dT1};
  P_TRY(hipMemcpy(dT1, T1.data(), sizeof(G1Aff) * T1.size(), hipMemcpyHostToDevice));
  G1Aff* pts = nullptr;
  hipError_t e = fixed_base_batch<Fq>(ctx->stream, pw, dT1, &pts);
  if (e != hipSuccess) { if (pts) hipFree(pts); return vz_fail(ctx, VIMZ_ERR_HIP, "vimz_kzg_setup: powers of tau", e); }
  const int rc = bases_from_device(ctx, pts, n, srs_out);
  hipFree(pts);
  if (rc) return rc;
  put_g2(vk_g2_out, to_affine(host_mul_fr<Fq2>(g2_generator(), tau)));
  return VIMZ_OK;
}

// the decider circuit for this prover's shapes: light (checks 1-4) or full (also the CycleFold instance's commitments and relation: the first
// generators of the prover's CycleFold commitment key become constants of the circuit)
int decider_circuit_build(vimz_cf* v, bool light, vimz_decider& dec) {
  vimz_ctx* ctx = v->ctx;
  aug::DeciderCircuit& circ = dec.circ;
  const cb::BuilderT<Fe>& main = v->circ->build->b;
  std::vector<G2Aff> gens;
  if (!light) {
    const cb::BuilderT<Fq>& cfb = v->cf.b;
    const size_t need = std::max<size_t>(cfb.n_wires - 1 - aug::CF_IO, cfb.n_constraints());
    if (!v->ck2 || v->ck2->n < need) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: the CycleFold commitment key is shorter than the vectors it commits to");
    gens.resize(need);
    // (a stream of its own and NOT the context's lock: the key is immutable, and the prover whose context this is may be in the middle of a fold that holds the
    //  lock for seconds — the set-up's host part is meant to run under that fold: tools/e2e.py)
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t ts = nullptr;
    P_TRY(hipStreamCreateWithFlags(&ts, hipStreamNonBlocking));
    uint32_t* tmp = nullptr;
    struct FreeTmp { uint32_t** q; hipStream_t* s; ~FreeTmp() { if (*q) hipFree(*q); hipStreamDestroy(*s); } } ft{&tmp, &ts};
    P_TRY(hipMalloc((void**)&tmp, 64 * need));
    launch_points_from_internal<Fe>(ts, v->ck2->d, 0, tmp, need);
    P_TRY(hipGetLastError());
    P_TRY(hipMemcpyAsync(gens.data(), tmp, 64 * need, hipMemcpyDeviceToHost, ts));
    P_TRY(hipStreamSynchronize(ts));
  }
  try {
    if (light) circ.finish(main, v->c1->len_z);
    else circ.finish(main, v->c1->len_z, &v->cf.b, gens.data(), (uint32_t)gens.size());
  } catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  if (!light) {      // check 5's chains on the device: the window table once (43 MB at 1 313 generators), on the stream the chains will run on — not the context's, as above
    vimz_decider::Chains& ch = dec.chains;
    ch.nW = v->cf.b.n_wires - 1 - aug::CF_IO; ch.nE = v->cf.b.n_constraints();
    P_TRY(hipStreamCreateWithFlags(&ch.stream, hipStreamNonBlocking));
    P_TRY(hipEventCreate(&ch.ev0)); P_TRY(hipEventCreate(&ch.ev1));
    P_TRY(cf_chains_key_upload(ch.stream, circ.okey, ch.key));
    P_TRY(hipMalloc((void**)&ch.dev, 4 * ch.words()));
    P_TRY(hipHostMalloc((void**)&ch.host, 4 * ch.words()));
  }
  return VIMZ_OK;
}
// [tau]G2 given with a prover whose main key is not the SRS it belongs to makes every later KZG check fail far from its cause:
// e(srs[1], G2) == e(G1, [tau]G2) once, at set-up / load.  (srs[0] = G1 for an SRS made by vimz_kzg_setup; any other key fails here.)
int kzg_vk_matches_srs(vimz_cf* v, const G2PAff& vk, const char* who) {
  vimz_ctx* ctx = v->ctx;
  G1Aff p01[2];
  if (!v->ck1 || v->ck1->n < 2) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: the main commitment key is too short to be an SRS");
  {      // (a stream of its own, not the context's lock: see decider_circuit_build)
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t ts = nullptr;
    P_TRY(hipStreamCreateWithFlags(&ts, hipStreamNonBlocking));
    uint32_t* tmp = nullptr;
    struct FreeTmp { uint32_t** q; hipStream_t* s; ~FreeTmp() { if (*q) hipFree(*q); hipStreamDestroy(*s); } } ft{&tmp, &ts};
    P_TRY(hipMalloc((void**)&tmp, 128));
    launch_points_from_internal<Fq>(ts, v->ck1->d, 0, tmp, 2);
    P_TRY(hipGetLastError());
    P_TRY(hipMemcpyAsync(p01, tmp, 128, hipMemcpyDeviceToHost, ts));
    P_TRY(hipStreamSynchronize(ts));
  }
  const G1Aff g1 = g1_generator();
  G1Aff ng = g1; ng.y = Fq::neg(g1.y);
  if (!vz::pairing::consts().ok) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: pairing constants");
  if (!p01[0].x.eq(g1.x) || !p01[0].y.eq(g1.y) || !vz::pairing::g1_on_curve(p01[1]) || !vz::pairing::product_is_one({{p01[1], g2_generator()}, {ng, vk}})) {
    std::string m = std::string(who) + ": the KZG verifying key is not [tau]G2 of the SRS the prover commits with";
    return vz_fail(ctx, VIMZ_ERR_INVALID, m.c_str());
  }
  return VIMZ_OK;
}

}  // namespace
// What every set-up begins with: the KZG verifying key (optional) checked against the prover's SRS, the decider circuit for the prover's shapes, the key's sizes
// and the constants of the domain  (declared in g16_key_origin.hpp: the origin check of a key starts from the same circuit)
int decider_setup_head(vimz_cf* v, const uint64_t kzg_vk_g2[16], bool light, vimz_decider& d) {
  vimz_ctx* ctx = v->ctx;
  d.vk = v; d.ctx = ctx;
  d.kzg_vk.x = d.kzg_vk.y = Fq2::zero();
  if (kzg_vk_g2) {
    if (!get_g2(kzg_vk_g2, &d.kzg_vk) || !vz::pairing::g2_on_curve(d.kzg_vk) || !vz::pairing::g2_in_subgroup(d.kzg_vk))
      return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_setup: the KZG verifying key is not a point of G2");
    const int rcv = kzg_vk_matches_srs(v, d.kzg_vk, "vimz_decider_setup");
    if (rcv) return rcv;
  }
  { const int rcb = decider_circuit_build(v, light, d); if (rcb) return rcb; }
  G16Key& K = d.key;
  const cb::BuilderT<Fe>& b = d.circ.b;
  K.m = b.n_wires; K.n_pub = d.circ.n_public; K.n_c = b.n_constraints();
  K.n = 1; K.logn = 0;
  while (K.n < K.n_c + K.n_pub + 1) { K.n <<= 1; K.logn++; }
  if (K.logn > 26) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: circuit too large for the domain");
  if (!domain_constants(K, K.logn)) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: root of unity");
  return VIMZ_OK;
}
namespace {

int decider_setup_impl(vimz_cf* v, const uint64_t kzg_vk_g2[16], const Trapdoor& td, bool light, vimz_decider** out, double seconds[4]) {
  vimz_ctx* ctx = v->ctx;
  const double t_all = now_s();
  std::unique_ptr<vimz_decider> d(new vimz_decider());
  { const int rch = decider_setup_head(v, kzg_vk_g2, light, *d); if (rch) return rch; }
  const double t_syn = now_s();
  G16Key& K = d->key;
  const cb::BuilderT<Fe>& b = d->circ.b;
  const Fe tau = td.tau, alpha = td.alpha, beta = td.beta, gamma = td.gamma, delta = td.delta;
  const Fe gamma_inv = Fe::pow_pm2(gamma), delta_inv = Fe::pow_pm2(delta);
  // Lagrange basis at tau: L_j(tau) = Z(tau)/n · ω^j / (tau − ω^j)   (batch inversion)
  const Fe z_tau = Fe::sub(fr_pow_u64(tau, K.n), Fe::one());
  if (z_tau.is_zero()) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: tau lies in the domain");
  std::vector<Fe> L(K.n), den(K.n);
  std::vector<Fe> uvw[3];
  std::vector<Fe> lq, icq, hq;
  struct WipeAll { std::vector<Fe>*v[8]; ~WipeAll() { for (auto* x : v) wipe(*x); } } wa{{&L, &den, &uvw[0], &uvw[1], &uvw[2], &lq, &icq, &hq}};
  // (all of this on the host's threads, in chunks: 4 M elements at the full decider's size — 0.8 s on one thread per phase)
  const unsigned TH = std::max(1u, std::min(16u, usable_cpus()));
  auto parallel = [&](uint64_t n, const std::function<void(uint64_t, uint64_t)>& f) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < TH; t++) { const uint64_t lo = n * t / TH, hi = n * (t + 1) / TH; if (lo < hi) th.emplace_back([&f, lo, hi] { f(lo, hi); }); }
    for (auto& x : th) x.join();
  };
  { const Fe c = Fe::mul(z_tau, K.n_inv);
    parallel(K.n, [&](uint64_t lo, uint64_t hi) {      // ω^j, tau − ω^j, one batched inversion per chunk
      Fe w = fr_pow_u64(K.omega, lo);
      for (uint64_t j = lo; j < hi; j++) { den[j] = Fe::sub(tau, w); L[j] = w; w = Fe::mul(w, K.omega); }
      std::vector<Fe> pre(hi - lo); Fe run = Fe::one();
      for (uint64_t j = lo; j < hi; j++) { pre[j - lo] = run; run = Fe::mul(run, den[j]); }
      Fe inv = Fe::pow_pm2(run);
      for (uint64_t j = hi; j-- > lo;) { const Fe dj = den[j]; den[j] = Fe::mul(inv, pre[j - lo]); inv = Fe::mul(inv, dj); }
      for (uint64_t j = lo; j < hi; j++) L[j] = Fe::mul(Fe::mul(L[j], den[j]), c);
      wipe(pre);
    }); }
  // u_i = A_i(tau), v_i = B_i(tau), w_i = C_i(tau); the constant and the public inputs get a row of their own (a = z_i, b = c = 0).
  // Every thread walks all the non-zeros and accumulates the wires of ITS range: no shared accumulator, no per-thread copy of three 130 MB vectors
  for (int q = 0; q < 3; q++) uvw[q].assign(K.m, Fe::zero());
  { const cb::Csr* Ms[3] = {&b.A, &b.B, &b.C};
    parallel(K.m, [&](uint64_t wlo, uint64_t whi) {
      for (int q = 0; q < 3; q++) {
        const cb::Csr& M = *Ms[q];
        for (uint32_t r = 0; r < K.n_c; r++) for (uint32_t k = M.row_ptr[r]; k < M.row_ptr[r + 1]; k++) {
          const uint32_t col = M.col[k];
          if (col < wlo || col >= whi) continue;
          Fe& dst = uvw[q][col]; dst = Fe::add(dst, Fe::mul(b.dict[M.coef[k]], L[r]));
        }
      }
    });
    for (uint32_t i = 0; i <= K.n_pub; i++) uvw[0][i] = Fe::add(uvw[0][i], L[K.n_c + i]); }
  lq.assign(K.m - K.n_pub - 1, Fe::zero()); icq.assign(K.n_pub + 1, Fe::zero()); hq.assign(K.n - 1, Fe::zero());
  parallel(K.m, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      const Fe k = Fe::add(Fe::add(Fe::mul(beta, uvw[0][i]), Fe::mul(alpha, uvw[1][i])), uvw[2][i]);
      if (i <= K.n_pub) icq[i] = Fe::mul(k, gamma_inv); else lq[i - K.n_pub - 1] = Fe::mul(k, delta_inv);
    }
  });
  { const Fe t0 = Fe::mul(z_tau, delta_inv);
    parallel(K.n - 1, [&](uint64_t lo, uint64_t hi) { Fe t = Fe::mul(t0, fr_pow_u64(tau, lo)); for (uint64_t j = lo; j < hi; j++) { hq[j] = t; t = Fe::mul(t, tau); } }); }
  const double t_qap = now_s();
  // key points on the GPU (any failure below: ~vimz_decider releases what was built)
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const G1Aff g1 = g1_generator(); const G2PAff g2 = g2_generator();
  if (!g2_on_curve(g2)) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: G2 generator constant");
  const std::vector<G1Aff> T1 = fixed_table<Fq>(g1); const std::vector<G2PAff> T2 = fixed_table<Fq2>(g2);
  struct Tables { G1Aff* a = nullptr; G2PAff* b = nullptr; ~Tables() { if (a) hipFree(a); if (b) hipFree(b); } } tables;
  P_TRY(hipMalloc((void**)&tables.a, sizeof(G1Aff) * T1.size())); P_TRY(hipMalloc((void**)&tables.b, sizeof(G2PAff) * T2.size()));
  P_TRY(hipMemcpy(tables.a, T1.data(), sizeof(G1Aff) * T1.size(), hipMemcpyHostToDevice)); P_TRY(hipMemcpy(tables.b, T2.data(), sizeof(G2PAff) * T2.size(), hipMemcpyHostToDevice));
  auto g1_query = [&](const std::vector<Fe>& sc, vimz_bases** outb) -> int {
    G1Aff* pts = nullptr;
    hipError_t e = fixed_base_batch<Fq>(s, sc, tables.a, &pts);
    if (e != hipSuccess) { if (pts) hipFree(pts); return vz_fail(ctx, VIMZ_ERR_HIP, "decider: key points", e); }
    const int rc = bases_from_device(ctx, pts, sc.size(), outb);
    hipFree(pts);
    return rc;
  };
  int rc;
  if ((rc = g1_query(uvw[0], &K.a_q)) || (rc = g1_query(uvw[1], &K.b1_q)) || (rc = g1_query(lq, &K.l_q)) || (rc = g1_query(hq, &K.h_q))) return rc;
  { // the G2 query holds only the wires that occur in B (the others' points are the identity)
    std::vector<uint32_t> ix; std::vector<Fe> sc;
    for (uint32_t i = 0; i < K.m; i++) if (!uvw[1][i].is_zero()) { ix.push_back(i); sc.push_back(uvw[1][i]); }
    K.n_b2 = (uint32_t)ix.size();
    hipError_t e = fixed_base_batch<Fq2>(s, sc, tables.b, &K.b2_q);
    wipe(sc);
    if (e != hipSuccess) return vz_fail(ctx, VIMZ_ERR_HIP, "decider: G2 key points", e);
    P_TRY(hipMalloc((void**)&K.b2_idx, 4 * std::max<size_t>(ix.size(), 1)));
    P_TRY(hipMemcpy(K.b2_idx, ix.data(), 4 * ix.size(), hipMemcpyHostToDevice)); }
  if ((rc = domain_tables(ctx, s, K))) return rc;
  // the few points of the verifying key, on the host
  K.alpha1 = to_affine(host_mul_fr<Fq>(g1, alpha)); K.beta1 = to_affine(host_mul_fr<Fq>(g1, beta)); K.delta1 = to_affine(host_mul_fr<Fq>(g1, delta));
  K.beta2 = to_affine(host_mul_fr<Fq2>(g2, beta)); K.gamma2 = to_affine(host_mul_fr<Fq2>(g2, gamma)); K.delta2 = to_affine(host_mul_fr<Fq2>(g2, delta));
  K.ic.resize(K.n_pub + 1);
  for (uint32_t i = 0; i <= K.n_pub; i++) K.ic[i] = to_affine(host_mul_fr<Fq>(g1, icq[i]));
  const double t_end = now_s();
  d->setup_s[0] = t_syn - t_all; d->setup_s[1] = t_qap - t_syn; d->setup_s[2] = t_end - t_qap; d->setup_s[3] = t_end - t_all;
  if (seconds) memcpy(seconds, d->setup_s, sizeof(d->setup_s));
  *out = d.release();
  return VIMZ_OK;
}

// ---- the set-up from a powers-of-tau string: the key by GROUP operations on the string's points — tau, alpha and beta are never in this
// process, gamma = 1, and delta is the only secret drawn here.  tests/_g16_powers_ref.derive_key states the derivation on scalars. ------------------------------
struct PowersString { const uint64_t* tau_g1; size_t n_tau_g1; const uint64_t *tau_g2, *alpha_g1, *beta_g1; size_t n_pow; const uint64_t* beta_g2; int form; };

void host_parallel(uint64_t n, const std::function<void(uint64_t, uint64_t)>& f) {
  const unsigned TH = std::max(1u, std::min(16u, usable_cpus()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < TH; t++) { const uint64_t lo = n * t / TH, hi = n * (t + 1) / TH; if (lo < hi) th.emplace_back([&f, lo, hi] { f(lo, hi); }); }
  for (auto& x : th) x.join();
}
bool string_point_on_curve(const G1Aff& p) { return vz::pairing::g1_on_curve(p); }
bool string_point_on_curve(const G2PAff& p) { return vz::pairing::g2_on_curve(p); }
}  // namespace
// n points of a string as words (form = VIMZ_FORM_*) -> Montgomery coordinates.  0: fine; 1: a coordinate is not below q; 2: a point is not on its curve
// (declared in g16_key_origin.hpp, instantiated below for both groups)
template <class A>
int string_points_in(const uint64_t* words, size_t n, int form, A* out) {
  const size_t per = sizeof(A) / sizeof(Fq);
  std::atomic<int> bad{0};
  host_parallel(n, [&](uint64_t lo, uint64_t hi) {
    for (uint64_t i = lo; i < hi; i++) {
      Fq* c = (Fq*)(out + i);
      for (size_t k = 0; k < per; k++) {
        Fq x; memcpy(x.v, words + 4 * (per * i + k), 32);
        if (!x.is_reduced()) { bad.store(1); return; }
        c[k] = form == VIMZ_FORM_MONTGOMERY ? x : Fq::to_mont(x);
      }
      if (!string_point_on_curve(out[i])) { int z = 0; bad.compare_exchange_strong(z, 2); return; }
    }
  });
  return bad.load();
}
template int string_points_in<G1Aff>(const uint64_t*, size_t, int, G1Aff*);
template int string_points_in<G2PowAff>(const uint64_t*, size_t, int, G2PowAff*);
namespace {

// delta_given: the test hook's; NULL: drawn from the OS.  seconds (optional) = {synthesis, checks + upload, transforms, column sums, l/h scaling + key tables, total}
int decider_setup_powers_impl(vimz_cf* v, bool light, const PowersString& S, const Fe* delta_given, vimz_decider** out, double seconds[6]) {
  vimz_ctx* ctx = v->ctx;
  auto bad = [&](const char* m) { return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string("vimz_decider_setup_from_powers: ") + m).c_str()); };
  const double t_all = now_s();
  std::unique_ptr<vimz_decider> d(new vimz_decider());
  { const int rch = decider_setup_head(v, nullptr, light, *d); if (rch) return rch; }
  const double t_syn = now_s();
  G16Key& K = d->key;
  const cb::BuilderT<Fe>& b = d->circ.b;
  const size_t n = K.n, m = K.m, n_l = m - K.n_pub - 1;
  if (K.logn < 1) return bad("the circuit's domain is a single point");
  if (S.n_pow < n || S.n_tau_g1 < 2 * n - 1) return bad("the string is shorter than the circuit's domain: n powers are needed, and 2n - 1 of tau in G1");
  // the string's points: beta·tau^k, alpha·tau^k and tau^k side by side (the K query sums over all three), the 2n − 1 powers for h, and G2's
  std::vector<G1Aff> lag(3 * n), tau(2 * n - 1); std::vector<G2PAff> tau2(n); G2PAff beta2;
  { const struct { const uint64_t* w; size_t n; G1Aff* dst; } g1s[3] = {{S.beta_g1, n, lag.data()}, {S.alpha_g1, n, lag.data() + n}, {S.tau_g1, 2 * n - 1, tau.data()}};
    int rc = 0;
    for (const auto& a : g1s) if (!rc) rc = string_points_in<G1Aff>(a.w, a.n, S.form, a.dst);
    if (!rc) rc = string_points_in<G2PAff>(S.tau_g2, n, S.form, tau2.data());
    if (!rc) rc = string_points_in<G2PAff>(S.beta_g2, 1, S.form, &beta2);
    if (rc) return bad(rc == 1 ? "a coordinate is not below the modulus" : "a point is not on its curve"); }
  memcpy(lag.data() + 2 * n, tau.data(), sizeof(G1Aff) * n);
  const G1Aff g1 = g1_generator(); const G2PAff g2 = g2_generator();
  G1Aff ng = g1; ng.y = Fq::neg(g1.y);
  auto same2 = [](const G2PAff& p, const G2PAff& q) { return p.x.c0.eq(q.x.c0) && p.x.c1.eq(q.x.c1) && p.y.c0.eq(q.y.c0) && p.y.c1.eq(q.y.c1); };
  if (!vz::pairing::consts().ok) return bad("pairing constants");
  if (!tau[0].x.eq(g1.x) || !tau[0].y.eq(g1.y)) return bad("tau_g1[0] is not the generator of G1");
  if (!same2(tau2[0], g2)) return bad("tau_g2[0] is not the generator of G2");
  if (aff_is_identity(tau[1]) || aff_is_identity(lag[0]) || aff_is_identity(lag[n]) || aff_is_identity(tau2[1]) || aff_is_identity(beta2)) return bad("tau, alpha or beta is zero: a point of the string is the identity");
  if (!vz::pairing::g2_in_subgroup(beta2)) return bad("beta_g2 is not in the subgroup");
  if (!vz::pairing::g2_in_subgroup(tau2[1])) return bad("tau_g2[1] is not in the subgroup");
  if (!vz::pairing::product_is_one({{tau[1], g2}, {ng, tau2[1]}})) return bad("tau_g1[1] and tau_g2[1] are not of one tau");
  if (!vz::pairing::product_is_one({{lag[0], g2}, {ng, beta2}})) return bad("beta_g1[0] and beta_g2 are not of one beta");
  d->kzg_vk = tau2[1];
  { const int rcv = kzg_vk_matches_srs(v, d->kzg_vk, "vimz_decider_setup_from_powers"); if (rcv) return rcv; }
  // delta: this party's only secret
  struct Secret { Fe delta, dinv_canon; ~Secret() { wipe(this, sizeof(*this)); } } sec;
  if (delta_given) sec.delta = *delta_given; else if (!fr_random(&sec.delta)) return bad("no randomness from the OS");
  if (sec.delta.is_zero()) return bad("delta is zero");
  sec.dinv_canon = Fe::from_mont(Fe::pow_pm2(sec.delta));

  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  struct Dev {
    G1Aff *lag = nullptr, *tau = nullptr, *a = nullptr, *b1 = nullptr, *k = nullptr, *h = nullptr; G2PAff *l2 = nullptr, *b2 = nullptr; uint32_t *tw = nullptr, *dinv = nullptr;
    ColsumDevice plan;
    void drop(void* p) { if (p) hipFree(p); }
    ~Dev() { if (dinv) { hipMemset(dinv, 0, 32); }      // (an error path between 1/delta's upload and its wipe ends here: the device copy never outlives the call unwiped)
             for (void* p : {(void*)lag, (void*)tau, (void*)a, (void*)b1, (void*)k, (void*)h, (void*)l2, (void*)b2, (void*)tw, (void*)dinv}) drop(p); g16_colsum_free(plan); }
  } D;
  P_TRY(hipMalloc((void**)&D.lag, sizeof(G1Aff) * 3 * n)); P_TRY(hipMalloc((void**)&D.tau, sizeof(G1Aff) * (2 * n - 1))); P_TRY(hipMalloc((void**)&D.l2, sizeof(G2PAff) * n));
  P_TRY(hipMalloc((void**)&D.tw, 4 * g16_point_transform_words(K.logn)));
  P_TRY(hipMemcpy(D.lag, lag.data(), sizeof(G1Aff) * 3 * n, hipMemcpyHostToDevice)); P_TRY(hipMemcpy(D.tau, tau.data(), sizeof(G1Aff) * (2 * n - 1), hipMemcpyHostToDevice));
  P_TRY(hipMemcpy(D.l2, tau2.data(), sizeof(G2PAff) * n, hipMemcpyHostToDevice));
  const double t_up = now_s();
  // the four Lagrange bases: beta·L, alpha·L, L in G1, L in G2 (one table of twiddles serves all: the stream orders them)
  for (int q = 0; q < 3; q++) P_TRY(g16_point_transform(s, D.lag + q * n, K.logn, true, true, D.tw));
  P_TRY(g16_point_transform(s, D.l2, K.logn, true, true, D.tw));
  // ... under which the host plans the column sums
  std::vector<uint32_t> dict(8 * b.dict.size());
  for (size_t i = 0; i < b.dict.size(); i++) { const Fe c = Fe::from_mont(b.dict[i]); memcpy(&dict[8 * i], c.v, 32); }
  const cb::Csr* Ms[3] = {&b.A, &b.B, &b.C};
  for (const cb::Csr* M : Ms) if (M->row_ptr.size() != (size_t)K.n_c + 1) return bad("a matrix does not have one row a constraint");
  std::vector<ColsumUnit> units(K.n_pub + 1);
  for (uint32_t i = 0; i <= K.n_pub; i++) units[i] = {K.n_c + i, i};
  auto part = [&](int q, uint32_t base) { return ColsumPart{Ms[q]->row_ptr.data(), Ms[q]->col.data(), Ms[q]->coef.data(), K.n_c, base}; };
  ColsumPlan plan_a, plan_b, plan_k; std::string err;
  { const ColsumPart pa = part(0, 0), pb = part(1, 0), pk[3] = {part(0, 0), part(1, (uint32_t)n), part(2, (uint32_t)(2 * n))};
    if (!colsum_plan(&pa, 1, units.data(), units.size(), dict.data(), b.dict.size(), BnFr::MOD.w, K.m, (uint32_t)n, &plan_a, &err) ||
        !colsum_plan(&pb, 1, nullptr, 0, dict.data(), b.dict.size(), BnFr::MOD.w, K.m, (uint32_t)n, &plan_b, &err) ||
        !colsum_plan(pk, 3, units.data(), units.size(), dict.data(), b.dict.size(), BnFr::MOD.w, K.m, (uint32_t)(3 * n), &plan_k, &err)) return bad(err.c_str()); }
  P_TRY(hipStreamSynchronize(s));
  const double t_tr = now_s();
  // VIMZ_DECIDER_POWERS_STATS (read per call): the plans' shapes and the set-up's device memory on stderr, for profiles/decider_powers.txt
  const bool stats = getenv("VIMZ_DECIDER_POWERS_STATS") != nullptr;
  size_t free_start = 0, free_min = 0, mem_total = 0;
  auto sample = [&] { size_t f = 0; if (stats && hipMemGetInfo(&f, &mem_total) == hipSuccess) { if (!free_start) free_start = free_min = f; free_min = std::min(free_min, f); } };
  sample();
  if (stats) for (const auto& pl : {std::make_pair("a", &plan_a), std::make_pair("b", &plan_b), std::make_pair("K", &plan_k)}) {
    fprintf(stderr, "decider from powers: plan %s: %zu entries, %zu magnitudes, runs per level", pl.first, pl.second->entries.size(), pl.second->mags.size() / 8);
    for (const ColsumLevel& lv : pl.second->levels) fprintf(stderr, " %zu", lv.runs.size());
    fprintf(stderr, "; most level-0 runs of a column %u; level-0 runs by bitlen(|c|):", pl.second->max_col_runs);
    std::map<uint32_t, size_t> hist;
    for (const ColsumRun& r : pl.second->levels[0].runs) hist[r.bits]++;
    for (const auto& h : hist) fprintf(stderr, " %u:%zu", h.first, h.second);
    fputc('\n', stderr);
  }
  // the queries: a = colsum(A, L) + units, b = colsum(B, L) in both groups, K = colsum(A, beta·L) + colsum(B, alpha·L) + colsum(C, L) + units over beta·L
  auto sums = [&](const ColsumPlan& plan, auto* points, auto** dst) -> int {
    typedef typename std::remove_pointer<typename std::remove_pointer<decltype(dst)>::type>::type A;
    P_TRY(g16_colsum_upload(plan, sizeof(A), &D.plan));
    P_TRY(hipMalloc((void**)dst, sizeof(A) * m));
    P_TRY(g16_column_sums(s, D.plan, (const A*)points, *dst));
    sample();
    P_TRY(hipStreamSynchronize(s));
    g16_colsum_free(D.plan);
    return VIMZ_OK;
  };
  int rc;
  if ((rc = sums(plan_k, D.lag, &D.k)) || (rc = sums(plan_a, D.lag + 2 * n, &D.a)) || (rc = sums(plan_b, D.lag + 2 * n, &D.b1)) || (rc = sums(plan_b, D.l2, &D.b2))) return rc;
  const double t_cs = now_s();
  // l = K[n_pub + 1 ..]/delta in place, h = (tau^(j+n) − tau^j)/delta; ic = K[.. n_pub] (gamma = 1)
  P_TRY(hipMalloc((void**)&D.dinv, 32)); P_TRY(hipMalloc((void**)&D.h, sizeof(G1Aff) * std::max<size_t>(n - 1, 1)));
  P_TRY(hipMemcpy(D.dinv, sec.dinv_canon.v, 32, hipMemcpyHostToDevice));
  P_TRY(g16_scale_points(s, D.k + K.n_pub + 1, n_l, D.dinv, D.k + K.n_pub + 1));
  P_TRY(g16_h_query(s, D.tau, n, D.dinv, D.h));
  sample();
  P_TRY(hipMemsetAsync(D.dinv, 0, 32, s));
  K.ic.resize(K.n_pub + 1);
  P_TRY(hipMemcpyAsync(K.ic.data(), D.k, sizeof(G1Aff) * (K.n_pub + 1), hipMemcpyDeviceToHost, s));
  std::vector<G2PAff> b2(m);
  P_TRY(hipMemcpyAsync(b2.data(), D.b2, sizeof(G2PAff) * m, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  // the bases and the full G2 query go before the key's tables come
  for (void** p : {(void**)&D.lag, (void**)&D.tau, (void**)&D.l2, (void**)&D.b2, (void**)&D.tw, (void**)&D.dinv}) { hipFree(*p); *p = nullptr; }
  const struct { G1Aff** pts; size_t off, n; vimz_bases** q; } qs[4] = {{&D.a, 0, m, &K.a_q}, {&D.b1, 0, m, &K.b1_q}, {&D.k, (size_t)K.n_pub + 1, n_l, &K.l_q}, {&D.h, 0, n - 1, &K.h_q}};
  for (const auto& q : qs) {
    if ((rc = bases_from_device(ctx, *q.pts + q.off, q.n, q.q))) return rc;
    hipFree(*q.pts); *q.pts = nullptr;
  }
  { // the G2 query holds only the wires whose point is not the identity
    std::vector<uint32_t> ix; std::vector<G2PAff> pts;
    for (uint32_t i = 0; i < K.m; i++) if (!aff_is_identity(b2[i])) { ix.push_back(i); pts.push_back(b2[i]); }
    K.n_b2 = (uint32_t)ix.size();
    P_TRY(hipMalloc((void**)&K.b2_q, sizeof(G2PAff) * std::max<size_t>(ix.size(), 1))); P_TRY(hipMalloc((void**)&K.b2_idx, 4 * std::max<size_t>(ix.size(), 1)));
    P_TRY(hipMemcpy(K.b2_q, pts.data(), sizeof(G2PAff) * pts.size(), hipMemcpyHostToDevice)); P_TRY(hipMemcpy(K.b2_idx, ix.data(), 4 * ix.size(), hipMemcpyHostToDevice)); }
  if ((rc = domain_tables(ctx, s, K))) return rc;
  sample();
  if (stats) fprintf(stderr, "decider from powers: device memory of the set-up at its peak %.1f MB above what was in use before the column sums (the four bases, the string's tau_g1 and the twiddles: %.1f MB), %.1f MB of %.1f MB free at the lowest\n",
                     (free_start - free_min) / 1048576.0, (sizeof(G1Aff) * (5 * n - 1) + sizeof(G2PAff) * n + 4 * g16_point_transform_words(K.logn)) / 1048576.0, free_min / 1048576.0, mem_total / 1048576.0);
  K.alpha1 = lag[n]; K.beta1 = lag[0]; K.beta2 = beta2; K.gamma2 = g2;
  K.delta1 = to_affine(host_mul_fr<Fq>(g1, sec.delta)); K.delta2 = to_affine(host_mul_fr<Fq2>(g2, sec.delta));
  const double t_end = now_s();
  d->setup_s[0] = t_syn - t_all; d->setup_s[1] = t_up - t_syn; d->setup_s[2] = t_end - t_up; d->setup_s[3] = t_end - t_all;
  if (seconds) { seconds[0] = t_syn - t_all; seconds[1] = t_up - t_syn; seconds[2] = t_tr - t_up; seconds[3] = t_cs - t_tr; seconds[4] = t_end - t_cs; seconds[5] = t_end - t_all; }
  *out = d.release();
  return VIMZ_OK;
}

// ---- the verifier: what contracts/*Verifier.sol::verifyNovaProof does with the 25 words (ContrastVerifier.sol:685-783) ---------------------------------
// (decider_verify.hpp: the verifier itself, shared with vimz_decider_verify_batch)
using vz::dv::VerifierKey; using vz::dv::verify_words; using vz::dv::parse_key; using vz::dv::g1_negate;
static_assert(vz::dv::LIMBS == aug::DEC_LIMBS && vz::dv::LIMB_BITS == aug::DEC_LIMB_BITS, "the verifier's limbs are the circuit's");
VerifierKey key_of(const vimz_decider* d) {
  VerifierKey K; const G16Key& G = d->key;
  K.pp_hash = d->vk->c1->digest; K.len_z = d->circ.len_z;
  K.alpha = G.alpha1; K.beta = G.beta2; K.gamma = G.gamma2; K.delta = G.delta2; K.ic = G.ic;
  K.kzg_g1 = g1_generator(); K.kzg_g2 = g2_generator(); K.kzg_vk = d->kzg_vk;
  return K;
}

}  // namespace

// what judging a string (g16_powers_verify.hip) shares with the set-up: the generators and the OS's randomness the blinders are drawn from
G1Aff g16_g1_generator() { return g1_generator(); }
G2PowAff g16_g2_generator() { return g2_generator(); }
bool g16_os_random(void* buf, size_t n) { return os_random(buf, n); }

// what the origin check of a key (g16_key_origin.hip) shares with the set-ups and the prover: the circuit a set-up head leaves, the domain's inverse transform over
// scalars, the MSM's resident form of a device array of points, and the bit-plane MSM over G2
vimz_decider* g16_decider_new() { return new vimz_decider(); }
void g16_decider_delete(vimz_decider* d) { delete d; }
void g16_decider_circuit(const vimz_decider& d, G16CircuitView* out) {
  const cb::BuilderT<Fe>& b = d.circ.b;
  const cb::Csr* Ms[3] = {&b.A, &b.B, &b.C};
  for (int q = 0; q < 3; q++) { out->row_ptr[q] = Ms[q]->row_ptr.data(); out->n_row_ptr[q] = Ms[q]->row_ptr.size(); out->col[q] = Ms[q]->col.data(); out->coef[q] = Ms[q]->coef.data(); out->nnz[q] = Ms[q]->col.size(); }
  static_assert(sizeof(Fe) == 32, "a dictionary entry is 8 words");
  out->dict = (const uint32_t*)b.dict.data(); out->n_dict = b.dict.size();
  out->m = d.key.m; out->n_pub = d.key.n_pub; out->n_c = d.key.n_c; out->logn = d.key.logn;
  out->len_z = d.circ.len_z; out->mode = d.circ.full ? 0 : 1; out->whole_header = true;
  const Fe c = Fe::from_mont(d.vk->c1->digest); memcpy(out->pp_hash, c.v, 32);
}
// host_spmv3 over the decider's matrices with a vector of ones, timed: what k_spmv3_dict's time is recorded beside (profiles/key_origin.txt; VIMZ_KEY_ORIGIN_STATS)
double g16_decider_host_spmv3_seconds(const vimz_decider& d) {
  const std::vector<Fe> z(d.circ.b.n_wires, Fe::one());
  std::vector<Fe> out[3];
  const double t0 = now_s();
  host_spmv3(d.circ.b, z, out);
  return now_s() - t0;
}
struct G16Domain { G16Key K; };
int g16_domain_new(vimz_ctx* ctx, hipStream_t s, int logn, G16Domain** out) {
  std::unique_ptr<G16Domain> D(new G16Domain());
  if (!domain_constants(D->K, logn)) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: root of unity");
  const int rc = domain_tables(ctx, s, D->K);
  if (rc) { free_key_raw(D->K); return rc; }
  *out = D.release();
  return VIMZ_OK;
}
void g16_domain_free(G16Domain* D) { if (D) { free_key_raw(D->K); delete D; } }
void g16_domain_n_inv(const G16Domain* D, uint32_t out[8]) { memcpy(out, D->K.n_inv.v, 32); }
hipError_t g16_domain_intt_unscaled(hipStream_t s, uint32_t* d, const G16Domain* D) { return ntt(s, d, D->K, true); }
int g16_bases_from_device(vimz_ctx* ctx, const G1Aff* d_pts, size_t n, vimz_bases** out) { return bases_from_device(ctx, d_pts, n, out); }
void g16_bases_free_raw(vimz_bases* b) { if (b) { if (b->d) hipFree(b->d); delete b; } }
int g16_g2_msm(vimz_ctx* ctx, hipStream_t s, const G2PowAff* bases, const uint32_t* wires, const uint32_t* idx, uint32_t n, uint32_t* canon, XYZZ<vz::pairing::Fq2>* out) {
  return g2_msm(ctx, s, bases, wires, idx, n, canon, out);
}

extern "C" {

void vimz_decider_free(vimz_decider* d) {
  if (!d) return;
  if (d->ctx) {
    std::unique_lock<std::mutex> g(d->ctx->mu);
    hipSetDevice(d->ctx->device);
    hipStreamSynchronize(d->ctx->stream);
    if (d->chains.stream) hipStreamSynchronize(d->chains.stream);
  }
  delete d;      // (~vimz_decider: the key's points and, for a full decider, the chains' table and buffers)
}

// KZG::setup (Sonobe's `KZG::setup(rng, n)` inside vimz/src/sonobe_backend/folding.rs:36-48 `prepare_folding`): tau from the OS, used and forgotten
int vimz_kzg_setup(vimz_ctx* ctx, size_t n, vimz_bases** srs_out, uint64_t vk_g2_out[16]) {
  if (!ctx || !srs_out || !vk_g2_out || !n) return VIMZ_ERR_INVALID;
  Trapdoor t;
  if (!trapdoor_random(t)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_kzg_setup: no randomness from the OS");
  return kzg_setup_impl(ctx, t.tau, n, srs_out, vk_g2_out);
}

// Decider::preprocess (vimz/src/sonobe_backend/mod.rs:72-75): the decider circuit for this prover's shapes and a Groth16 key pair.  The toxic
// waste is drawn from the OS's randomness, used and forgotten: a LOCALLY TRUSTED setup (whoever runs it could have kept it) — what the
// reference's own `StdRng::from_seed([41; 32])` (mod.rs:54) is, too; a deployment would import keys from a ceremony instead.
// kzg_vk_g2 (optional): [tau]G2 of the SRS the prover's ck_main is made of (vimz_kzg_setup) — needed by vimz_decider_verify and part of vimz_decider_vk.
// seconds (optional) = {circuit synthesis, QAP evaluation at the trapdoor, key points on the GPU, total}.
// light != 0: the shrunken circuit of the reference's opt-in `light-test` feature (vimz/Cargo.toml:56-59; checks 1-4 of aug/decider.hpp: the CycleFold
// instance is bound by its hash only); light == 0: the full decider, as `decider.rs:13-21` instantiates it (≈ 2.75 M constraints more: set-up in seconds).
int vimz_decider_setup(vimz_cf* v, const uint64_t kzg_vk_g2[16], int light, vimz_decider** out, double seconds[4]) {
  if (!v || !out) return VIMZ_ERR_INVALID;
  Trapdoor t;
  if (!trapdoor_random(t)) return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_decider_setup: no randomness from the OS");
  return decider_setup_impl(v, kzg_vk_g2, t, light != 0, out, seconds);
}
// The same from a powers-of-tau string (iden3.read_ptau's arrays; form = VIMZ_FORM_* of the coordinates): tau, alpha and beta are the string's and never in this
// process, gamma = 1, delta is drawn here from the OS and wiped.  The KZG verifying key is the string's tau_g2[1]: the prover's ck_main must be the SRS of the same
// string (hip.kzg_from_powers).  Refusals and what stays unjudged: include/vimz_hip.h.
int vimz_decider_setup_from_powers(vimz_cf* v, int light, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, size_t n_pow,
                                   const uint64_t beta_g2[16], int form, vimz_decider** out, double seconds[6]) {
  if (!v) return VIMZ_ERR_INVALID;
  if (!out || !tau_g1 || !tau_g2 || !alpha_g1 || !beta_g1 || !beta_g2) return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_decider_setup_from_powers: NULL argument");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_decider_setup_from_powers: form is VIMZ_FORM_*");
  return decider_setup_powers_impl(v, light != 0, PowersString{tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form}, nullptr, out, seconds);
}
// The domain a set-up of this prover's decider works over, without a set-up: the circuit is synthesised (host only) and dropped.  For a caller that judges the
// prefix of a string a set-up will read (vimz_powers_verify) before the set-up runs.
int vimz_decider_domain(vimz_cf* v, int light, uint64_t* domain) {
  if (!v) return VIMZ_ERR_INVALID;
  if (!domain) return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_decider_domain: NULL argument");
  std::unique_ptr<vimz_decider> d(new vimz_decider());
  { const int rch = decider_setup_head(v, nullptr, light != 0, *d); if (rch) return rch; }
  *domain = d->key.n;
  return VIMZ_OK;
}
#ifdef VIMZ_TESTING
// Host only, no GPU: the decider circuit (aug/decider.hpp) over the Nova + CycleFold recursion of the trivial step circuit with made-up commitments — the
// run of vimz_cf_selfcheck, with the running relaxed witness kept by folding on the host — then the decider's final fold, its witness, and the checks:
// result bit 0 a step's F' witness is bad, 1 the folded scalars differ from F''s, 2 the decider's witness generator flags the honest input, 3 its witness
// violates a row of the decider's R1CS, 4 the public inputs are not the contract's layout (pp_hash, i, z_0, z_i, 4 x 5 limbs, c_W, c_E, e_W, e_E, 2 x 5 limbs),
// 5 a wrong KZG evaluation / a wrong challenge / a changed cmT limb is NOT flagged, 6 a changed public input leaves every row satisfied.
// full != 0: the FULL decider (aug/decider_cf.hpp) — the CycleFold instances of every step are real here (witnesses of the CycleFold circuit for the step's
// two folds, committed under a made-up key G_k = (k + 1)·G, folded on the host into a running witness and error vector): 7 the host's running CycleFold
// instance differs from the one F' folds in-circuit, 8 a running CycleFold witness / error vector that violates its relation, or a commitment that does not
// open to it, is NOT flagged by the witness generator, 9 such a witness leaves every row of the decider satisfied.
// counts = {decider constraints, wires, public inputs, main constraints}.
int vimz_decider_selfcheck(int steps, int full, uint32_t* result, uint64_t counts[4]) {
  if (!result || steps < 2 || steps > 32) return VIMZ_ERR_INVALID;
  try {
    CfCircuit cf; cf.finish();
    cb::BuilderT<Fe> b;
    b.len_z = 1; b.n_priv = 0; b.n_wires = 3;
    b.enforce(cb::LCT<Fe>::constant(Fe::one()), cb::LCT<Fe>::wire(2), cb::LCT<Fe>::wire(1));
    b.n_linear = 1;
    CfMainCircuit c1(b); c1.use_worker = false; c1.finish(cf);
    const uint32_t nw = b.n_wires, nc = b.n_constraints();
    uint32_t res = 0;
    const G1Aff g1 = CycleSide<BnFq>::G(); const G2Aff g2 = CycleSide<BnFr>::G();
    auto fake1 = [&](uint64_t k) { const uint32_t w[2] = {(uint32_t)k, (uint32_t)(k >> 32)}; return to_affine(scalar_mul(g1, w, 64)); };
    auto fake2 = [&](uint64_t k) { const uint32_t w[2] = {(uint32_t)k, (uint32_t)(k >> 32)}; return to_affine(host_mul<Fe>(g2, w, 64)); };
    std::vector<Fe> z0 = {cb::f_from_u64<Fe>(7)};
    CfMainRelaxed U = CfMainRelaxed::zero(); G1Aff UW = g1_identity(), UE = g1_identity();
    CfMainFresh u = CfMainFresh::zero(); G1Aff uW = g1_identity();
    CfRelaxed cfU = CfRelaxed::zero();
    std::vector<Fe> Zrun(nw, Fe::zero()), Erun(nc, Fe::zero()), z_last;
    // full: the running CycleFold pair on the host, committed under G_k = (k + 1)·G (a made-up key: Σ v_k·G_k is one multiplication by Σ (k + 1)·v_k)
    const uint32_t cnw = cf.b.n_wires, cnc = cf.b.n_constraints(), cnW = cnw - 1 - aug::CF_IO;
    std::vector<Fq> cfZ(cnw, Fq::zero()), cfE(cnc, Fq::zero());
    G2Aff cf_cmW = g2_identity(), cf_cmE = g2_identity();
    auto cf_commit = [&](const Fq* v, size_t n) {
      Fq s = Fq::zero();
      for (size_t k = 0; k < n; k++) s = Fq::add(s, Fq::mul(v[k], cb::f_from_u64<Fq>(k + 1)));
      const Fq c = Fq::from_mont(s);
      return to_affine(host_mul<Fe>(g2, c.v, 256));
    };
    auto g2_fold = [&](const G2Aff& P, const uint32_t low[4], const G2Aff& Q) {
      const uint32_t k[5] = {low[0], low[1], low[2], low[3], 1u};
      G2 a = aff_is_identity(P) ? G2::identity() : from_affine(P);
      if (!aff_is_identity(Q)) { G2 t = host_mul<Fe>(Q, k, 129); add_full(a, t); }
      return to_affine(a);
    };
    // one CycleFold instance (r, P1, P2 -> P3 = P1 + r·P2): witness, commitments, and — once the caller has the challenge — the fold into the running pair
    struct CfInst { std::vector<Fq> z, T; G2Aff cmW, cmT; };
    auto cf_instance = [&](const uint32_t r_low[4], const G1Aff& P1, const G1Aff& P2, CfInst& o) {
      bool bad = false;
      cf.witness(r_low, P1, P2, o.z, &bad);
      if (bad) res |= 1;
      std::vector<Fq> p1[3], p2[3];
      host_spmv3(cf.b, cfZ, p1); host_spmv3(cf.b, o.z, p2);
      o.T.resize(cnc);
      for (uint32_t k = 0; k < cnc; k++) o.T[k] = Fq::sub(Fq::sub(Fq::add(Fq::mul(p1[0][k], p2[1][k]), Fq::mul(p2[0][k], p1[1][k])), Fq::mul(cfZ[0], p2[2][k])), p1[2][k]);
      o.cmW = cf_commit(o.z.data() + 1, cnW); o.cmT = cf_commit(o.T.data(), cnc);
    };
    auto cf_fold_in = [&](const CfInst& o, const uint32_t r_low[4]) {
      const Fq r = rho_element<Fq>(r_low);
      for (uint32_t k = 0; k < cnw; k++) cfZ[k] = Fq::add(cfZ[k], Fq::mul(r, o.z[k]));
      for (uint32_t k = 0; k < cnc; k++) cfE[k] = Fq::add(cfE[k], Fq::mul(r, o.T[k]));
      cf_cmW = g2_fold(cf_cmW, r_low, o.cmW); cf_cmE = g2_fold(cf_cmE, r_low, o.cmT);
    };
    // x1 += r·x2 over the main shape, with the cross term folded into E:  returns nothing, updates Zrun / Erun
    auto fold_in = [&](const std::vector<Fe>& z2, const Fe& r) {
      std::vector<Fe> p1[3], p2[3];
      host_spmv3(b, Zrun, p1); host_spmv3(b, z2, p2);
      const Fe u1 = Zrun[0];
      for (uint32_t k = 0; k < nc; k++) {
        const Fe T = Fe::sub(Fe::sub(Fe::add(Fe::mul(p1[0][k], p2[1][k]), Fe::mul(p2[0][k], p1[1][k])), Fe::mul(u1, p2[2][k])), p1[2][k]);      // u_2 = 1
        Erun[k] = Fe::add(Erun[k], Fe::mul(r, T));
      }
      for (uint32_t w = 0; w < nw; w++) Zrun[w] = Fe::add(Zrun[w], Fe::mul(r, z2[w]));
    };
    for (int i = 0; i < steps; i++) {
      CfMainIn in = CfMainIn::zero();
      in.digest = c1.digest; in.i = (uint64_t)i; in.z0 = z0; in.U = U; in.u = u; in.cfU = cfU;
      CfChallenges ch; ch.h_U = cf_hash_main(c1.digest, i, z0, z0.data(), U); ch.h_cf = cf_hash_cf(c1.digest, cfU);
      G1Aff Wn = g1_identity(), En = g1_identity();
      if (i > 0) {
        const G1Aff cT = i > 1 ? fake1(0x1000 + i) : g1_identity();
        in.T = nn_point(cT);
        cf_challenge_main(ch, u, in.T);
        Wn = g1_fold(UW, ch.r, uW); En = g1_fold(UE, ch.r, cT);
        in.Wn = nn_point(Wn); in.En = nn_point(En);
        if (full) {
          CfInst i1, i2;
          cf_instance(ch.r, UW, uW, i1);
          in.cf1W = i1.cmW; in.cf1T = i1.cmT;
          cf_challenge_cf1(ch, in.cf1W, in.Wn, in.cf1T);
          cf_fold_in(i1, ch.r1);
          cf_instance(ch.r, UE, cT, i2);
          in.cf2W = i2.cmW; in.cf2T = i2.cmT;
          cf_challenge_cf2(ch, in.cf2W, in.En, in.cf2T);
          cf_fold_in(i2, ch.r2);
        } else {
          in.cf1W = fake2(0x2000 + i); in.cf1T = i > 1 ? fake2(0x3000 + i) : g2_identity();
          in.cf2W = fake2(0x4000 + i); in.cf2T = fake2(0x5000 + i);
        }
        fold_in(z_last, rho_element<Fe>(ch.r));      // what this step's F' verifies: U_i = U_{i-1} (+) u_{i-1}
      }
      std::vector<Fe> augw; bool bad = false;
      CfMainOut o = c1.witness(in, z0.data(), z0.data(), augw, &bad);
      if (bad) res |= 1;
      if (full && i > 0) {      // the instance F' folded in-circuit is the one the host keeps
        const CfRelaxed& n = o.cfU_new;
        if (!n.W.x.eq(cf_cmW.x) || !n.W.y.eq(cf_cmW.y) || !n.E.x.eq(cf_cmE.x) || !n.E.y.eq(cf_cmE.y) || !cross_field<Fe>(cfZ[0]).eq(n.u)) res |= 128;
        for (int k = 0; k < aug::CF_IO; k++) if (memcmp(to_u256(cfZ[cnw - aug::CF_IO + k]).w, n.x[k].w, 32)) res |= 128;
      }
      std::vector<Fe> z = {Fe::one(), z0[0], z0[0]};
      z.insert(z.end(), augw.begin(), augw.end());
      if (i > 0 && (!o.U_new.u.eq(Zrun[0]) || !o.U_new.x0.eq(Zrun[nw - 2]) || !o.U_new.x1.eq(Zrun[nw - 1]))) res |= 2;
      U = o.U_new; UW = i > 0 ? Wn : g1_identity(); UE = i > 0 ? En : g1_identity(); cfU = o.cfU_new;
      uW = fake1(0x6000 + i); u.W = nn_point(uW); u.x0 = o.x0; u.x1 = o.x1;
      z_last = z;
    }
    // the decider's final fold U_{n+1} = U_n (+) u_n, on the host
    aug::DeciderIn in;
    in.digest = c1.digest; in.i = (uint64_t)steps; in.z0 = z0; in.zi = z0; in.U = U; in.u = u; in.cfU = cfU;
    const G1Aff cmT = fake1(0x7777);
    in.cmT = nn_point(cmT);
    uint32_t r_low[4]; aug::decider_challenge(u, in.cmT, r_low);
    fold_in(z_last, rho_element<Fe>(r_low));
    in.Wn = nn_point(g1_fold(UW, r_low, uW)); in.En = nn_point(g1_fold(UE, r_low, cmT));
    const Fe cW = aug::decider_kzg_challenge(in.digest, in.Wn), cE = aug::decider_kzg_challenge(in.digest, in.En);
    auto horner = [](const Fe* v, size_t n, const Fe& c) { Fe acc = Fe::zero(); for (size_t j = n; j-- > 0;) acc = Fe::add(Fe::mul(acc, c), v[j]); return acc; };
    in.eW = horner(Zrun.data() + 1, nw - 3, cW); in.eE = horner(Erun.data(), nc, cE);
    in.Wf = Zrun.data() + 1; in.Ef = Erun.data();
    aug::DeciderCircuit dc;
    if (full) {
      std::vector<G2Aff> gens(std::max(cnW, cnc));
      G2 acc = from_affine(g2);
      for (auto& p : gens) { p = to_affine(acc); add_mixed(acc, g2); }
      dc.finish(b, 1, &cf.b, gens.data(), (uint32_t)gens.size());
      in.full.W = cfZ.data() + 1; in.full.E = cfE.data();
    } else dc.finish(b, 1);
    if (counts) { counts[0] = dc.b.n_constraints(); counts[1] = dc.b.n_wires; counts[2] = dc.n_public; counts[3] = nc; }
    bool bad = false;
    std::vector<Fe> zd = dc.witness(b, in, &bad);
    if (bad) res |= 4;
    auto violated = [&](const std::vector<Fe>& zz) { std::vector<Fe> p[3]; host_spmv3(dc.b, zz, p); for (uint32_t k = 0; k < dc.b.n_constraints(); k++) if (!Fe::mul(p[0][k], p[1][k]).eq(p[2][k])) return true; return false; };
    if (violated(zd)) res |= 8;
    // the public inputs, in the contract's order
    { std::vector<Fe> want = {in.digest, cb::f_from_u64<Fe>((uint64_t)steps), z0[0], z0[0]};
      for (const U256w* c : {&in.Wn.x, &in.Wn.y, &in.En.x, &in.En.y}) { uint64_t l[aug::DEC_LIMBS]; aug::decider_limbs55(*c, l); for (int k = 0; k < aug::DEC_LIMBS; k++) want.push_back(cb::f_from_u64<Fe>(l[k])); }
      want.push_back(cW); want.push_back(cE); want.push_back(in.eW); want.push_back(in.eE);
      for (const U256w* c : {&in.cmT.x, &in.cmT.y}) { uint64_t l[aug::DEC_LIMBS]; aug::decider_limbs55(*c, l); for (int k = 0; k < aug::DEC_LIMBS; k++) want.push_back(cb::f_from_u64<Fe>(l[k])); }
      if (want.size() != dc.n_public || dc.n_public != aug::decider_n_public(1)) res |= 16;
      else for (size_t k = 0; k < want.size(); k++) if (!zd[1 + k].eq(want[k])) res |= 16; }
    // negatives: the witness generator flags a wrong evaluation and a cross-term commitment other than the one the challenge was derived from
    { aug::DeciderIn t = in; t.eW = Fe::add(t.eW, Fe::one()); bool b2 = false; dc.witness(b, t, &b2); if (!b2) res |= 32; }
    { aug::DeciderIn t = in; t.cmT = nn_point(fake1(0x7778)); bool b2 = false; dc.witness(b, t, &b2); if (!b2) res |= 32; }      // (another r: the folded scalars no longer match W')
    // ... and every public input matters to some row
    for (uint32_t k = 0; k < dc.n_public; k++) { std::vector<Fe> zz = zd; zz[1 + k] = Fe::add(zz[1 + k], Fe::one()); if (!violated(zz)) res |= 64; }
    if (full) {
      // negatives of checks 5 and 6: a changed witness element (the commitment no longer opens, a row no longer holds), a changed error element,
      // and a witness changed TOGETHER with its commitment (opens, but the relation fails: check 6 alone)
      auto flagged = [&](const std::vector<Fq>& Zc, const std::vector<Fq>& Ec) {
        aug::DeciderIn t = in; t.full.W = Zc.data() + 1; t.full.E = Ec.data();
        bool b2 = false; std::vector<Fe> zz = dc.witness(b, t, &b2);
        return std::make_pair(b2, violated(zz));
      };
      { std::vector<Fq> Zc = cfZ; Zc[5] = Fq::add(Zc[5], Fq::one()); auto f = flagged(Zc, cfE); if (!f.first) res |= 256; if (!f.second) res |= 512; }
      { std::vector<Fq> Ec = cfE; Ec[3] = Fq::add(Ec[3], Fq::one()); auto f = flagged(cfZ, Ec); if (!f.first) res |= 256; if (!f.second) res |= 512; }
      // (under G_k = (k + 1)·G, adding b + 1 to element a and taking a + 1 off element b leaves the commitment as it was: only the relation can object)
      { std::vector<Fq> Zc = cfZ; Zc[1 + 4] = Fq::add(Zc[1 + 4], cb::f_from_u64<Fq>(10)); Zc[1 + 9] = Fq::sub(Zc[1 + 9], cb::f_from_u64<Fq>(5));
        if (!(cf_commit(Zc.data() + 1, cnW).x.eq(cf_cmW.x))) res |= 256;
        auto f = flagged(Zc, cfE); if (!f.first) res |= 256; if (!f.second) res |= 512; }
    }
    *result = res;
    return VIMZ_OK;
  } catch (const std::exception& e) { return vz_fail(nullptr, VIMZ_ERR_INVALID, e.what()); }
}
// deterministic TEST setups: the trapdoor is derived from `seed` — anyone who knows the seed can forge.  Not in the product library.
int vimz_testing_kzg_setup_seeded(vimz_ctx* ctx, const uint8_t* seed, size_t seed_len, size_t n, vimz_bases** srs_out, uint64_t vk_g2_out[16]) {
  if (!ctx || !srs_out || !vk_g2_out || !n || (!seed && seed_len)) return VIMZ_ERR_INVALID;
  return kzg_setup_impl(ctx, fr_from_hash(seed, seed_len, "vimz-kzg-tau"), n, srs_out, vk_g2_out);
}
int vimz_testing_decider_setup_seeded(vimz_cf* v, const uint64_t kzg_vk_g2[16], int light, const uint8_t* seed, size_t seed_len, vimz_decider** out, double seconds[4]) {
  if (!v || !out || (!seed && seed_len)) return VIMZ_ERR_INVALID;
  return decider_setup_impl(v, kzg_vk_g2, trapdoor_seeded(seed, seed_len), light != 0, out, seconds);
}
// the trapdoor set-up with a GIVEN trapdoor (tau, alpha, beta, gamma, delta: 4 canonical words each, non-zero), and the set-up from a string with a given delta:
// what tests/test_gpu_decider_from_powers.py compares byte for byte
int vimz_testing_decider_setup_trapdoor(vimz_cf* v, const uint64_t kzg_vk_g2[16], int light, const uint64_t td[20], vimz_decider** out, double seconds[4]) {
  if (!v || !out || !td) return VIMZ_ERR_INVALID;
  Trapdoor t; Fe* dst[5] = {&t.tau, &t.alpha, &t.beta, &t.gamma, &t.delta};
  for (int k = 0; k < 5; k++) { Fe c; memcpy(c.v, td + 4 * k, 32); if (!c.is_reduced() || c.is_zero()) return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_testing_decider_setup_trapdoor: a scalar is zero or not below the modulus"); *dst[k] = Fe::to_mont(c); }
  return decider_setup_impl(v, kzg_vk_g2, t, light != 0, out, seconds);
}
int vimz_testing_decider_setup_from_powers_delta(vimz_cf* v, int light, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1,
                                                 size_t n_pow, const uint64_t beta_g2[16], int form, const uint64_t delta[4], vimz_decider** out, double seconds[6]) {
  if (!v) return VIMZ_ERR_INVALID;
  if (!out || !tau_g1 || !tau_g2 || !alpha_g1 || !beta_g1 || !beta_g2 || !delta || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY))
    return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_testing_decider_setup_from_powers_delta: bad argument");
  Fe c; memcpy(c.v, delta, 32);
  if (!c.is_reduced() || c.is_zero()) return vz_fail(v->ctx, VIMZ_ERR_INVALID, "vimz_testing_decider_setup_from_powers_delta: delta is zero or not below the modulus");
  const Fe dm = Fe::to_mont(c);
  return decider_setup_powers_impl(v, light != 0, PowersString{tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form}, &dm, out, seconds);
}
// ---- the decider's kernels on a caller's shapes (tests/test_gpu_g16_kernels.py): the functions the set-up and the prover call, over made-up inputs ----------
}  // extern "C"
namespace {
// n scalars of 4 words (form = VIMZ_FORM_*) -> Montgomery elements; false: one of them is not below r
bool g16_scalars_in(const uint64_t* src, size_t n, int form, std::vector<Fe>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; i++) { Fe c; memcpy(c.v, src + 4 * i, 32); if (!c.is_reduced()) return false; out[i] = form == VIMZ_FORM_CANONICAL ? Fe::to_mont(c) : c; }
  return true;
}
bool g16_form_ok(int form) { return form == VIMZ_FORM_CANONICAL || form == VIMZ_FORM_MONTGOMERY; }
// s_i·gen for the scalars of `sc` as the set-up makes its key points: fixed_table on the host, fixed_base_batch on the device
template <class F>
int g16_fixed_mul(vimz_ctx* ctx, const Affine<F>& gen, const std::vector<Fe>& sc, std::vector<Affine<F>>& pts) {
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  const std::vector<Affine<F>> T = fixed_table<F>(gen);
  Affine<F>*dT = nullptr, *d_out = nullptr;
  struct Free { Affine<F>**a, **b; ~Free() { if (*a) hipFree(*a); if (*b) hipFree(*b); } } fr{&dT, &d_out};
  P_TRY(hipMalloc((void**)&dT, sizeof(Affine<F>) * T.size()));
  P_TRY(hipMemcpy(dT, T.data(), sizeof(Affine<F>) * T.size(), hipMemcpyHostToDevice));
  const hipError_t e = fixed_base_batch<F>(ctx->stream, sc, dT, &d_out);
  if (e != hipSuccess) return vz_fail(ctx, VIMZ_ERR_HIP, "vimz_test_g16_fixed_mul", e);
  pts.resize(sc.size());
  P_TRY(hipMemcpy(pts.data(), d_out, sizeof(Affine<F>) * sc.size(), hipMemcpyDeviceToHost));
  return VIMZ_OK;
}
}  // namespace
extern "C" {
int vimz_test_g16_domain(vimz_ctx* ctx, int logn, int what, const uint64_t* a, const uint64_t* b, const uint64_t* c, int form, uint64_t* out) {
  if (!ctx || !a || !out || what < 0 || what > 3 || (what == 3 && (!b || !c)) || !g16_form_ok(form)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_domain: bad argument");
  if (logn < 1 || logn > 26) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_domain: logn outside 1..26");      // (0: an empty grid and a shift by 32)
  G16Key K;
  if (!domain_constants(K, logn)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_domain: root of unity");
  const size_t n = K.n;
  const int nv = what == 3 ? 3 : 1;
  const uint64_t* src[3] = {a, b, c};
  std::vector<Fe> in[3];
  for (int q = 0; q < nv; q++) if (!g16_scalars_in(src[q], n, form, in[q])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_domain: a scalar is not below the modulus");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  uint32_t* dv[3] = {nullptr, nullptr, nullptr};
  struct Free { G16Key* K; uint32_t** v; ~Free() { for (int q = 0; q < 3; q++) if (v[q]) hipFree(v[q]); free_key_raw(*K); } } fr{&K, dv};
  { const int rc = domain_tables(ctx, s, K); if (rc) return rc; }
  for (int q = 0; q < nv; q++) { P_TRY(hipMalloc((void**)&dv[q], 32 * n)); P_TRY(hipMemcpyAsync(dv[q], in[q].data(), 32 * n, hipMemcpyHostToDevice, s)); }
  P_TRY(what == 0 ? ntt(s, dv[0], K, false) : what == 1 ? ntt(s, dv[0], K, true) : what == 2 ? coset_extend(s, dv[0], K) : quotient(s, dv, K));
  P_TRY(hipMemcpyAsync(in[0].data(), dv[0], 32 * n, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++) { const Fe r = form == VIMZ_FORM_CANONICAL ? Fe::from_mont(in[0][i]) : in[0][i]; memcpy(out + 4 * i, r.v, 32); }
  return VIMZ_OK;
}
int vimz_test_g16_fixed_mul(vimz_ctx* ctx, int group, const uint64_t* scalars, size_t n, uint64_t* out_xy) {
  if (!ctx || !scalars || !out_xy || !n || n > (1u << 26) || (group != 1 && group != 2)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_fixed_mul: bad argument");
  std::vector<Fe> sc;
  if (!g16_scalars_in(scalars, n, VIMZ_FORM_CANONICAL, sc)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_fixed_mul: a scalar is not below the modulus");
  if (group == 1) {
    std::vector<G1Aff> pts;
    const int rc = g16_fixed_mul<Fq>(ctx, g1_generator(), sc, pts); if (rc) return rc;
    for (size_t i = 0; i < n; i++) { put_fq(out_xy + 8 * i, pts[i].x); put_fq(out_xy + 8 * i + 4, pts[i].y); }
  } else {
    std::vector<G2PAff> pts;
    const int rc = g16_fixed_mul<Fq2>(ctx, g2_generator(), sc, pts); if (rc) return rc;
    for (size_t i = 0; i < n; i++) put_g2(out_xy + 16 * i, pts[i]);
  }
  return VIMZ_OK;
}
int vimz_test_g16_g2_msm(vimz_ctx* ctx, const uint64_t* bases_xy, size_t n, const uint64_t* wires, size_t m, int form, const uint32_t* idx, uint64_t out_xy[16]) {
  if (!ctx || !bases_xy || !wires || !idx || !out_xy || !g16_form_ok(form)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_g2_msm: bad argument");
  if (!n || n > m || m > (1u << 26)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_g2_msm: needs 0 < n <= m <= 2^26");
  for (size_t i = 0; i < n; i++) if (idx[i] >= m) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_g2_msm: a wire number is not below m");
  std::vector<G2PAff> pts(n);
  for (size_t i = 0; i < n; i++) if (!get_g2(bases_xy + 16 * i, &pts[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_g2_msm: a coordinate is not below the modulus");
  std::vector<Fe> z;
  if (!g16_scalars_in(wires, m, form, z)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_g2_msm: a scalar is not below the modulus");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  void* dev[4] = {nullptr, nullptr, nullptr, nullptr};      // bases, wires, wire numbers, canonical scalars
  struct Free { void** v; ~Free() { for (int q = 0; q < 4; q++) if (v[q]) hipFree(v[q]); } } fr{dev};
  const size_t bytes[4] = {sizeof(G2PAff) * n, 32 * m, 4 * n, 32 * n};
  const void* src[3] = {pts.data(), z.data(), idx};
  for (int q = 0; q < 4; q++) P_TRY(hipMalloc(&dev[q], bytes[q]));
  for (int q = 0; q < 3; q++) P_TRY(hipMemcpyAsync(dev[q], src[q], bytes[q], hipMemcpyHostToDevice, s));
  G2P sum;
  { const int rc = g2_msm(ctx, s, (const G2PAff*)dev[0], (const uint32_t*)dev[1], (const uint32_t*)dev[2], (uint32_t)n, (uint32_t*)dev[3], &sum); if (rc) return rc; }
  put_g2(out_xy, to_affine(sum));
  return VIMZ_OK;
}
#endif

// info = {constraints, wires, public inputs, domain size, non-zeros of A, B, C, rows of checks 5 and 6 (0: the light decider)}
int vimz_decider_info(const vimz_decider* d, uint64_t info[8]) {
  if (!d || !info) return VIMZ_ERR_INVALID;
  const cb::BuilderT<Fe>& b = d->circ.b;
  info[0] = d->key.n_c; info[1] = d->key.m; info[2] = d->key.n_pub; info[3] = d->key.n; info[4] = b.A.col.size(); info[5] = b.B.col.size(); info[6] = b.C.col.size(); info[7] = d->circ.full ? d->key.n_c - d->circ.light_constraints : 0;
  return VIMZ_OK;
}

// The verifying key — everything a contract generated for this circuit would hold as constants (contracts/ContrastVerifier.sol:140-160 KZG G_1 / G_2 / VK,
// :238-… alpha…delta and IC_k, :703 the public-parameter hash) — as canonical little-endian words: pp_hash (4), len_z (1), alpha (G1: x, y), beta,
// gamma, delta (G2: x.c0, x.c1, y.c0, y.c1), the number of IC points, the IC points (G1), then KZG G_1 (G1), G_2, VK (G2; zeros when the decider was
// set up without one).  Returns the byte size (copies when buf is large enough).
int64_t vimz_decider_vk(const vimz_decider* d, void* buf, size_t cap) {
  if (!d) return VIMZ_ERR_INVALID;
  Writer w;
  const G16Key& K = d->key;
  w.fe(d->vk->c1->digest); w.word(d->circ.len_z);
  w.point(K.alpha1);
  auto g2w = [&](const G2PAff& p) { w.fe(p.x.c0); w.fe(p.x.c1); w.fe(p.y.c0); w.fe(p.y.c1); };
  for (const G2PAff* p : {&K.beta2, &K.gamma2, &K.delta2}) g2w(*p);
  w.word(K.ic.size());
  for (auto& p : K.ic) w.point(p);
  w.point(g1_generator()); g2w(g2_generator()); g2w(d->kzg_vk);
  const size_t bytes = 8 * w.w.size();
  if (buf && cap >= bytes) memcpy(buf, w.w.data(), bytes);
  return (int64_t)bytes;
}

// ---- the key at rest: vimz_decider_key_save / _load -------------------------------------------------------------------------------------------------------
// A Groth16 key pair for the decider circuit as bytes, so that a set-up is made ONCE per circuit and shape (0.4 s instead of 0.8 s per run at contrast HD) and —
// the point of ADVICE r4 — so that keys made ELSEWHERE (a ceremony's, converted to this layout) can be used: the library then never sees a trapdoor.
// Layout (little-endian u64 words; curve points canonical, G1 (x, y), G2 (x.c0, x.c1, y.c0, y.c1)): magic, m, n_pub, n_c, n, len_z, mode (0 full, 1 light), pp_hash (4), KZG [tau]G2 (16),
// alpha1, beta1, delta1 (8 each), beta2, gamma2, delta2 (16 each), IC (8 x (n_pub + 1)), then the queries a (8 m), b1 (8 m), l (8 (m - n_pub - 1)), h (8 (n - 1)), b2 (16 m).
// A loaded key is TRUSTED like any common reference string: its points are range- and curve-checked for the verifying part, the queries are taken as they are
// (a wrong query makes proofs that do not verify, nothing worse).
static const uint64_t G16_KEY_MAGIC = vz::keyc::KEY_MAGIC;          // "VG16KEY2" (g16_key_contrib.hpp reads the layout below from a blob's own header)
static const size_t G16_KEY_HEADER = 7;
int64_t vimz_decider_key_save(vimz_decider* d, void* buf, size_t cap) {
  if (!d) return VIMZ_ERR_INVALID;
  const G16Key& K = d->key; vimz_ctx* ctx = d->ctx;
  const size_t nq[4] = {K.m, K.m, (size_t)K.m - K.n_pub - 1, (size_t)K.n - 1};
  const size_t words = G16_KEY_HEADER + 4 + 16 + 24 + 48 + 8 * (size_t)(K.n_pub + 1) + 8 * (nq[0] + nq[1] + nq[2] + nq[3]) + 16 * (size_t)K.m;
  if (!buf || cap < 8 * words) return (int64_t)(8 * words);
  uint64_t* w = (uint64_t*)buf; size_t pos = 0;
  w[pos++] = G16_KEY_MAGIC; w[pos++] = K.m; w[pos++] = K.n_pub; w[pos++] = K.n_c; w[pos++] = K.n; w[pos++] = d->circ.len_z; w[pos++] = d->circ.full ? 0 : 1;
  { const Fe c = Fe::from_mont(d->vk->c1->digest); memcpy(w + pos, c.v, 32); pos += 4; }
  put_g2(w + pos, d->kzg_vk); pos += 16;
  for (const G1Aff* p : {&K.alpha1, &K.beta1, &K.delta1}) { put_fq(w + pos, p->x); put_fq(w + pos + 4, p->y); pos += 8; }
  for (const G2PAff* p : {&K.beta2, &K.gamma2, &K.delta2}) { put_g2(w + pos, *p); pos += 16; }
  for (auto& p : K.ic) { put_fq(w + pos, p.x); put_fq(w + pos + 4, p.y); pos += 8; }
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const vimz_bases* qs[4] = {K.a_q, K.b1_q, K.l_q, K.h_q};
  uint32_t* tmp = nullptr;
  P_TRY(hipMalloc((void**)&tmp, 64 * (size_t)std::max<size_t>(K.m, K.n)));
  struct FreeTmp { uint32_t* q; ~FreeTmp() { hipFree(q); } } ft{tmp};
  for (int q = 0; q < 4; q++) {
    if (nq[q]) {
      launch_points_from_internal<Fq>(s, qs[q]->d, 1, tmp, nq[q]);
      P_TRY(hipGetLastError());
      P_TRY(hipMemcpyAsync(w + pos, tmp, 64 * nq[q], hipMemcpyDeviceToHost, s));
      P_TRY(hipStreamSynchronize(s));
    }
    pos += 8 * nq[q];
  }
  { std::vector<G2PAff> b2c(K.n_b2); std::vector<uint32_t> ix(K.n_b2);
    P_TRY(hipMemcpyAsync(b2c.data(), K.b2_q, sizeof(G2PAff) * (size_t)K.n_b2, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(ix.data(), K.b2_idx, 4 * (size_t)K.n_b2, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
    memset(w + pos, 0, 128 * (size_t)K.m);      // (the identity: (0, 0))
    for (uint32_t k = 0; k < K.n_b2; k++) put_g2(w + pos + 16 * (size_t)ix[k], b2c[k]);
    pos += 16 * (size_t)K.m; }
  return pos == words ? (int64_t)(8 * words) : (int64_t)VIMZ_ERR_INVALID;
}
// prover: as for vimz_decider_setup (shapes, keys, context).  The key must be for exactly this prover's circuits (sizes and public-parameter hash are checked).
int vimz_decider_key_load(vimz_cf* v, const void* buf, size_t len, vimz_decider** out) {
  if (!v || !buf || !out || (len & 7)) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  const uint64_t* w = (const uint64_t*)buf; const size_t nwords = len / 8;
  if (nwords < G16_KEY_HEADER + 4 + 16 + 24 + 48 || w[0] != G16_KEY_MAGIC || w[6] > 1) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: not a decider key");
  std::unique_ptr<vimz_decider> d(new vimz_decider());
  d->vk = v; d->ctx = ctx;
  { const int rcb = decider_circuit_build(v, w[6] == 1, *d); if (rcb) return rcb; }
  G16Key& K = d->key;
  const cb::BuilderT<Fe>& b = d->circ.b;
  K.m = b.n_wires; K.n_pub = d->circ.n_public; K.n_c = b.n_constraints();
  K.n = 1; K.logn = 0;
  while (K.n < K.n_c + K.n_pub + 1) { K.n <<= 1; K.logn++; }
  size_t pos = 1;
  if (w[pos] != K.m || w[pos + 1] != K.n_pub || w[pos + 2] != K.n_c || w[pos + 3] != K.n || w[pos + 4] != d->circ.len_z)
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: the key is for a decider circuit of other sizes");
  pos += 6;
  { Fe c; memcpy(c.v, w + pos, 32); if (!c.is_reduced() || !Fe::to_mont(c).eq(v->c1->digest)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: the key is for other circuits (public-parameter hash)"); pos += 4; }
  const size_t nq[4] = {K.m, K.m, (size_t)K.m - K.n_pub - 1, (size_t)K.n - 1};
  const size_t words = G16_KEY_HEADER + 4 + 16 + 24 + 48 + 8 * (size_t)(K.n_pub + 1) + 8 * (nq[0] + nq[1] + nq[2] + nq[3]) + 16 * (size_t)K.m;
  if (nwords != words) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: wrong length");
  using vz::pairing::g1_on_curve; using vz::pairing::g2_in_subgroup;
  if (!get_g2(w + pos, &d->kzg_vk) || !g2_on_curve(d->kzg_vk) || !g2_in_subgroup(d->kzg_vk)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: KZG verifying key"); pos += 16;
  if (!aff_is_identity(d->kzg_vk)) { const int rcv = kzg_vk_matches_srs(v, d->kzg_vk, "vimz_decider_key_load"); if (rcv) return rcv; }
  for (G1Aff* p : {&K.alpha1, &K.beta1, &K.delta1}) { if (!get_g1(w + pos, p) || !g1_on_curve(*p)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: a G1 key point"); pos += 8; }
  for (G2PAff* p : {&K.beta2, &K.gamma2, &K.delta2}) { if (!get_g2(w + pos, p) || !g2_on_curve(*p) || !g2_in_subgroup(*p)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: a G2 key point"); pos += 16; }
  K.ic.resize(K.n_pub + 1);
  for (auto& p : K.ic) { if (!get_g1(w + pos, &p) || !g1_on_curve(p)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: an IC point"); pos += 8; }
  if (!domain_constants(K, K.logn)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: root of unity");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  uint32_t* tmp = nullptr;
  P_TRY(hipMalloc((void**)&tmp, 64 * (size_t)std::max<size_t>(K.m, K.n)));
  struct FreeTmp { uint32_t* q; ~FreeTmp() { hipFree(q); } } ft{tmp};
  vimz_bases** qs[4] = {&K.a_q, &K.b1_q, &K.l_q, &K.h_q};
  for (int q = 0; q < 4; q++) {
    if (nq[q]) { P_TRY(hipMemcpyAsync(tmp, w + pos, 64 * nq[q], hipMemcpyHostToDevice, s)); P_TRY(hipStreamSynchronize(s)); }
    const int rc = bases_from_device(ctx, (const G1Aff*)tmp, nq[q], qs[q], 1);
    if (rc) return rc;
    pos += 8 * nq[q];
  }
  { std::vector<G2PAff> b2; std::vector<uint32_t> ix;
    for (uint32_t i = 0; i < K.m; i++) {
      G2PAff pt;
      if (!get_g2(w + pos, &pt)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_load: a G2 query coordinate is not below the modulus");
      pos += 16;
      if (!aff_is_identity(pt)) { b2.push_back(pt); ix.push_back(i); }
    }
    K.n_b2 = (uint32_t)ix.size();
    P_TRY(hipMalloc((void**)&K.b2_q, sizeof(G2PAff) * std::max<size_t>(b2.size(), 1)));
    P_TRY(hipMemcpy(K.b2_q, b2.data(), sizeof(G2PAff) * b2.size(), hipMemcpyHostToDevice));
    P_TRY(hipMalloc((void**)&K.b2_idx, 4 * std::max<size_t>(ix.size(), 1)));
    P_TRY(hipMemcpy(K.b2_idx, ix.data(), 4 * ix.size(), hipMemcpyHostToDevice)); }
  { const int rc = domain_tables(ctx, s, K); if (rc) return rc; }
  *out = d.release();
  return VIMZ_OK;
}

// What vimz_decider_prove does up to the decider circuit's assignment: the final fold U_{i+1} = NIFS(U_i, u_i) and the KZG openings on the GPU, then the witness
// z of the decider circuit on the host.  chains_gpu (full decider): check 5's chains come from k_cf_open_chains instead of the host's loop.
}  // extern "C"
namespace {
struct DeciderWitness {
  std::vector<Fe> z;
  G1Aff cmT; uint32_t r_low[4]; uint64_t kzg_out[2][12];      // kzg_out: eval (4), proof (8)
  Fe cW, cE;
  double t_fold = 0, chains_gpu_s = 0;
};
// VIMZ_DECIDER_CHAINS = host | gpu, read per call (a debugging switch like the others); unset: the default
int decider_chains_mode(vimz_ctx* ctx, bool* gpu) {
  const char* e = getenv("VIMZ_DECIDER_CHAINS");
  if (!e || !*e) { *gpu = DECIDER_CHAINS_GPU_DEFAULT; return VIMZ_OK; }
  if (!strcmp(e, "gpu")) { *gpu = true; return VIMZ_OK; }
  if (!strcmp(e, "host")) { *gpu = false; return VIMZ_OK; }
  return vz_fail(ctx, VIMZ_ERR_INVALID, "VIMZ_DECIDER_CHAINS must be host or gpu");
}
// Check 5's chains while they are in flight on the decider's own stream: wait() where check 5 begins (CfFullIn::chains_wait), and whichever way decider_witness
// is left the stream is idle before the lock on the decider's buffers is given up — the kernel reads the IVC's vectors, the download writes the pinned block.
struct ChainsInFlight {
  vimz_decider::Chains* c = nullptr;      // set once work of this call may be queued
  bool waited = false; hipError_t err = hipSuccess; double seconds = 0;
  bool wait() {      // false: an addition met two points with the same x, or the device failed (err)
    waited = true;
    if ((err = hipEventSynchronize(c->ev1)) != hipSuccess) return false;
    float ms = 0; if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) seconds = 1e-3 * ms;
    return c->host[c->words() - 1] == 0;
  }
  static bool wait_cb(void* self) { return ((ChainsInFlight*)self)->wait(); }
  void drain() { if (c && !waited) { waited = true; err = hipStreamSynchronize(c->stream); } }
  ~ChainsInFlight() { drain(); }
};
int decider_witness(vimz_decider* d, vimz_cf* ivc, bool chains_gpu, DeciderWitness& out) {
  vimz_ctx* ctx = d->ctx; vimz_cf* v = d->vk;
  if (ivc->ctx != ctx || ivc->pri->n_wires != v->pri->n_wires || ivc->pri->n_c != v->pri->n_c || !ivc->c1->digest.eq(v->c1->digest) || ivc->ck1 != v->ck1)
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_prove: the IVC proof belongs to other shapes / keys than the decider was set up for");
  if (ivc->broken) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_prove: the IVC failed in the middle of a step");
  if (ivc->i == 0) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_prove: the IVC has no steps");
  if (d->circ.full && (ivc->ck2 != v->ck2 || ivc->sec.n_w != v->cf.b.n_wires || ivc->sec.n_c != v->cf.b.n_constraints()))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_prove: the IVC proof's CycleFold key / shape is not the one the full decider was set up for");
  chains_gpu = chains_gpu && d->circ.full;
  vimz_prover* p = ivc->pri;
  const size_t nw = p->n_wires, nc = p->n_c;
  std::vector<Fe> Wf(nw), Ef(nc);
  aug::DeciderIn in;
  G1Aff cWn, cEn;
  G1Aff& cmT = out.cmT; uint32_t* r_low = out.r_low; uint64_t (*kzg_out)[12] = out.kzg_out; Fe &cW = out.cW, &cE = out.cE;
  // the decider's chain buffers are this call's until it returns.  Lock order: the chains' lock, then the context's — never the other way round
  vimz_decider::Chains& chains = d->chains;
  std::unique_lock<std::mutex> chains_lock;
  if (chains_gpu) chains_lock = std::unique_lock<std::mutex>(chains.mu);
  ChainsInFlight flight;
  // (the final fold's vectors are released when this function returns, not where their block ends: hipFree waits for the whole device, the chains' kernel on its
  //  own stream included — presumably why the fold's span was 35 ms longer with the chains on the device in profiles/decider_chains.txt, which predates this)
  uint32_t* dev = nullptr;
  struct FreeDev { uint32_t** q; ~FreeDev() { if (*q) hipFree(*q); } } fd{&dev};
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (hipStream_t q : {ivc->s2, ivc->s3, ivc->s4}) if (q) P_TRY(hipStreamSynchronize(q));
    P_TRY(hipStreamSynchronize(s));
    if (chains_gpu) {
      // check 5's chains (full decider): the running CycleFold witness (wires 1 .. of Z) and error vector are final once the streams above are idle — both openings
      // in one launch on the decider's own stream, beside the final fold below; the values come home into pinned memory and are waited for where check 5 begins
      const SecDev& S = ivc->sec;
      uint32_t *d_wi = chains.dev, *d_en = d_wi + chains.wire_words(), *d_bad = chains.dev + chains.words() - 1;
      flight.c = &chains;
      P_TRY(hipEventRecord(chains.ev0, chains.stream));
      P_TRY(cf_chains_launch(chains.stream, chains.key, S.Zrun + 8, chains.nW, S.E, chains.nE, d_wi, d_en, d_bad));
      P_TRY(hipMemcpyAsync(chains.host, chains.dev, 4 * chains.words(), hipMemcpyDeviceToHost, chains.stream));
      P_TRY(hipEventRecord(chains.ev1, chains.stream));
    }
    P_TRY(hipMalloc((void**)&dev, 32 * (nw + 2 * nc)));
    uint32_t *Wd = dev, *Ed = dev + 8 * nw, *Td = Ed + 8 * nc;
    P_TRY(hipMemcpyAsync(Wd, p->Zrun, 32 * nw, hipMemcpyDeviceToDevice, s));
    P_TRY(hipMemcpyAsync(Ed, p->E, 32 * nc, hipMemcpyDeviceToDevice, s));
    // cross term of (U_i, W_i) and the last instance of F' (strict: u = 1), its commitment
    hipLaunchKernelGGL(k_cross_term<Fr>, dim3(stream_grid(nc)), dim3(256), 0, s, nc, p->AZ, p->BZ, p->CZ, ivc->u_run, ivc->azl, ivc->bzl, ivc->czl, Fe::one(), Td);
    P_TRY(hipGetLastError());
    uint64_t pt[8];
    int rc = vz_msm_device(ctx, p->ck, 0, Td, nc, 1, 0, pt, VIMZ_FORM_MONTGOMERY);
    if (rc) return rc;
    memcpy(cmT.x.v, pt, 32); memcpy(cmT.y.v, pt + 4, 32);
    // the challenge, as the decider circuit derives it
    aug::decider_challenge(ivc->u, nn_point(cmT), r_low);
    const Fe rho = cf_r_element_fr(r_low);
    Fold5 f; for (int k = 0; k < 5; k++) { f.x1[k] = nullptr; f.x2[k] = nullptr; f.n[k] = 0; }
    f.x1[0] = Wd; f.x2[0] = ivc->Zl; f.n[0] = nw;
    f.x1[1] = Ed; f.x2[1] = Td; f.n[1] = nc;
    hipLaunchKernelGGL(k_fold5<Fr>, dim3(1024), dim3(256), 0, s, f, rho);
    P_TRY(hipGetLastError());
    cWn = g1_fold(ivc->UW, r_low, ivc->uW); cEn = g1_fold(ivc->UE, r_low, cmT);
    in.digest = v->c1->digest;
    in.Wn = nn_point(cWn); in.En = nn_point(cEn); in.cmT = nn_point(cmT);
    cW = aug::decider_kzg_challenge(in.digest, in.Wn); cE = aug::decider_kzg_challenge(in.digest, in.En);
    uint64_t ch[4];
    { const Fe c = Fe::from_mont(cW); memcpy(ch, c.v, 32); }
    if ((rc = vz_kzg_open_device(ctx, p->ck, 0, VIMZ_FIELD_BN254_FR, Wd + 8, nw - 3, ch, VIMZ_FORM_CANONICAL, kzg_out[0], kzg_out[0] + 4))) return rc;
    { const Fe c = Fe::from_mont(cE); memcpy(ch, c.v, 32); }
    if ((rc = vz_kzg_open_device(ctx, p->ck, 0, VIMZ_FIELD_BN254_FR, Ed, nc, ch, VIMZ_FORM_CANONICAL, kzg_out[1], kzg_out[1] + 4))) return rc;
    P_TRY(hipMemcpyAsync(Wf.data(), Wd, 32 * nw, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(Ef.data(), Ed, 32 * nc, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
  }
  out.t_fold = now_s();
  in.i = ivc->i; in.z0 = ivc->z0; in.zi = p->z_cur;
  in.U = ivc->U; in.u = ivc->u; in.cfU = ivc->cfU;
  { Fe c; memcpy(c.v, kzg_out[0], 32); in.eW = Fe::to_mont(c); memcpy(c.v, kzg_out[1], 32); in.eE = Fe::to_mont(c); }
  in.Wf = Wf.data() + 1; in.Ef = Ef.data();
  std::vector<Fq> cfZ, cfE;
  if (d->circ.full) {      // checks 5 and 6: the running CycleFold pair's witness and error vector
    const SecDev& S = ivc->sec;
    cfZ.resize(S.n_w); cfE.resize(S.n_c);
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    P_TRY(hipMemcpyAsync(cfZ.data(), S.Zrun, 32 * (size_t)S.n_w, hipMemcpyDeviceToHost, ctx->stream));
    P_TRY(hipMemcpyAsync(cfE.data(), S.E, 32 * (size_t)S.n_c, hipMemcpyDeviceToHost, ctx->stream));
    P_TRY(hipStreamSynchronize(ctx->stream));
    in.full.W = cfZ.data() + 1; in.full.E = cfE.data();
  }
  if (chains_gpu) {
    const Fe* wires = (const Fe*)chains.host; const G2Aff* ends = (const G2Aff*)(chains.host + chains.wire_words());
    in.full.chW.wires = wires; in.full.chW.ends = ends;
    in.full.chE.wires = wires + (size_t)chains.nW * aug::CFO_WINDOWS * 4; in.full.chE.ends = ends + chains.nW;
    in.full.chains_wait = &ChainsInFlight::wait_cb; in.full.chains_wait_arg = &flight;
  }
  // (the main relation's rows are a third of the witness's time when evaluated one by one inside the circuit: their products come from the host's threads)
  std::vector<Fe> pre_abc[3];
  host_spmv3(v->circ->build->b, Wf, pre_abc);
  in.pre_az = pre_abc[0].data(); in.pre_bz = pre_abc[1].data(); in.pre_cz = pre_abc[2].data(); in.pre_z = Wf.data();
  std::vector<Fe>& z = out.z;
  bool bad = false;
  try { z = d->circ.witness(v->circ->build->b, in, &bad); } catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  flight.drain();      // (check 5 was never reached: its error, if any, is still this call's)
  out.chains_gpu_s = flight.seconds;
  if (flight.err != hipSuccess) return vz_fail(ctx, VIMZ_ERR_HIP, "vimz_decider_prove: the chains of check 5 on the device", flight.err);
  if (bad) return vz_fail(ctx, VIMZ_ERR_UNSAT, "vimz_decider_prove: the IVC proof does not satisfy the decider's statement (hashes, relaxed relations, CycleFold commitments or KZG evaluations)");
  return VIMZ_OK;
}
}  // namespace
extern "C" {

// Decider::prove (mod.rs:76-78) for the IVC proof `ivc` holds after i >= 1 steps (left unchanged): the final fold U_{i+1} = NIFS(U_i, u_i) on the GPU
// (cross term, its commitment, the challenge of aug/decider.hpp, the folded witness and error vector), the KZG openings of U_{i+1}'s two commitments at
// the challenges that follow from them, and the Groth16 proof of the decider circuit — ALL 25 calldata words (contracts/*Verifier.sol:785-810;
// vimz_amd/calldata.py names them), canonical, 4 little-endian limbs each.  public_out: the info[2] public inputs (canonical), as the contract
// assembles them from the words.  VIMZ_ERR_UNSAT when the IVC proof does not satisfy the decider's statement.
// seconds (optional) = {final fold + KZG openings (GPU), witness + sparse products (host), NTTs, MSMs, total, check 5's chains on the GPU}.
// The last one: kernel and download of k_cf_open_chains by the device's clock (they run beside the first two spans, not after them); 0 when the chains
// are made on the host — the light decider, or VIMZ_DECIDER_CHAINS=host (=gpu: on the device; read per call; unset: gpu).
int vimz_decider_prove(vimz_decider* d, vimz_cf* ivc, uint64_t* public_out, uint64_t words_out[100], double seconds[6]) {
  if (!d || !ivc || !public_out || !words_out) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = d->ctx;
  const G16Key& K = d->key;
  const double t_all = now_s();
  bool chains_gpu = false;
  { const int rcm = decider_chains_mode(ctx, &chains_gpu); if (rcm) return rcm; }
  DeciderWitness wit;
  { const int rcw = decider_witness(d, ivc, chains_gpu, wit); if (rcw) return rcw; }
  const std::vector<Fe>& z = wit.z;
  const G1Aff& cmT = wit.cmT; const uint32_t* r_low = wit.r_low; const uint64_t (*kzg_out)[12] = wit.kzg_out; const Fe &cW = wit.cW, &cE = wit.cE;
  const double t_fold = wit.t_fold;
  std::vector<Fe> abc[3];
  host_spmv3(d->circ.b, z, abc);
  for (int q = 0; q < 3; q++) abc[q].resize(K.n, Fe::zero());
  for (uint32_t i = 0; i <= K.n_pub; i++) abc[0][K.n_c + i] = z[i];
  const double t_wit = now_s();
  int rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // h = (a·b − c) / Z on the coset 5·H
  uint32_t* dv[3] = {nullptr, nullptr, nullptr}; uint32_t* dz = nullptr;
  struct Free { uint32_t** v; uint32_t** z; ~Free() { for (int q = 0; q < 3; q++) if (v[q]) hipFree(v[q]); if (*z) hipFree(*z); } } fr{dv, &dz};
  for (int q = 0; q < 3; q++) { P_TRY(hipMalloc((void**)&dv[q], 32 * (size_t)K.n)); P_TRY(hipMemcpyAsync(dv[q], abc[q].data(), 32 * (size_t)K.n, hipMemcpyHostToDevice, s)); }
  P_TRY(hipMalloc((void**)&dz, 32 * (size_t)K.m)); P_TRY(hipMemcpyAsync(dz, z.data(), 32 * (size_t)K.m, hipMemcpyHostToDevice, s));
  P_TRY(quotient(s, dv, K)); P_TRY(hipStreamSynchronize(s));
  const double t_ntt = now_s();
  // the multi-scalar multiplications
  uint64_t pt[8];
  // (the wires' MSMs take unit scalars out first: a third of the full decider's wires are bits)
  auto g1_msm = [&](const vimz_bases* q, const uint32_t* sc, size_t n, G1Aff* outp, int split_ones) -> int {
    if (!n) { outp->x = Fq::zero(); outp->y = Fq::zero(); return VIMZ_OK; }
    const int r2 = vz_msm_device(ctx, q, 0, sc, n, 1, 0, pt, VIMZ_FORM_MONTGOMERY, split_ones);
    if (!r2) { memcpy(outp->x.v, pt, 32); memcpy(outp->y.v, pt + 4, 32); }
    return r2;
  };
  G1Aff sa, sb1, sl, sh;
  const int so = d->circ.full ? 1 : 0;
  static const bool dbg_t = getenv("VIMZ_DEBUG_TIMING") != nullptr;
  double tm0 = now_s();
  auto lap = [&](const char* what) { if (dbg_t) { const double t = now_s(); fprintf(stderr, "[decider] %s %.1f ms\n", what, 1e3 * (t - tm0)); tm0 = t; } };
  if ((rc = g1_msm(K.a_q, dz, K.m, &sa, so))) return rc; lap("msm a");
  if ((rc = g1_msm(K.b1_q, dz, K.m, &sb1, so))) return rc; lap("msm b1");
  if ((rc = g1_msm(K.l_q, dz + 8 * (size_t)(K.n_pub + 1), K.m - K.n_pub - 1, &sl, so))) return rc; lap("msm l");
  if ((rc = g1_msm(K.h_q, dv[0], K.n - 1, &sh, 0))) return rc; lap("msm h");
  // the G2 one, bit plane by bit plane (k_g2_planes): dv[1] (the quotient's inputs are spent) holds the canonical scalars of the query's wires
  G2P sb2 = G2P::identity();
  if (K.n_b2) {
    if ((size_t)K.n_b2 > (size_t)K.n) return vz_fail(ctx, VIMZ_ERR_INVALID, "decider: the G2 query is longer than the domain");
    if ((rc = g2_msm(ctx, s, K.b2_q, dz, K.b2_idx, K.n_b2, dv[1], &sb2))) return rc;
  }
  lap("msm b2 (G2)");
  const double t_msm = now_s();
  // A = alpha + Σ z_i a_i + r·delta;  B = beta + Σ z_i b_i + s·delta;  C = Σ_priv z_i l_i + Σ h_j hq_j + s·A + r·B1 − r·s·delta;  r, s fresh from the OS (zero knowledge)
  Fe r, sr;
  struct WipeRs { Fe *a, *b; ~WipeRs() { wipe(a, sizeof(Fe)); wipe(b, sizeof(Fe)); } } wrs{&r, &sr};
  if (!fr_random(&r) || !fr_random(&sr)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_prove: no randomness from the OS");
  G1 A = from_affine(K.alpha1); add_mixed(A, sa); { G1 t = host_mul_fr<Fq>(K.delta1, r); add_full(A, t); }
  G1 B1 = from_affine(K.beta1); add_mixed(B1, sb1); { G1 t = host_mul_fr<Fq>(K.delta1, sr); add_full(B1, t); }
  G2P B2 = from_affine(K.beta2); add_full(B2, sb2); { G2P t = host_mul_fr<Fq2>(K.delta2, sr); add_full(B2, t); }
  const G1Aff Aa = to_affine(A), B1a = to_affine(B1);
  G1 C = from_affine(sl); add_mixed(C, sh);
  { G1 t = host_mul_fr<Fq>(Aa, sr); add_full(C, t); }
  { G1 t = host_mul_fr<Fq>(B1a, r); add_full(C, t); }
  { G1 t = host_mul_fr<Fq>(K.delta1, Fe::mul(r, sr)); if (!t.is_identity()) t.Y = Fq::neg(t.Y); add_full(C, t); }
  const G1Aff Ca = to_affine(C); const G2PAff Ba = to_affine(B2);
  // the 25 words
  uint64_t* w = words_out;
  memset(w, 0, 800);
  put_fq(w + 0, ivc->UW.x); put_fq(w + 4, ivc->UW.y); put_fq(w + 8, ivc->UE.x); put_fq(w + 12, ivc->UE.y);
  put_fq(w + 16, ivc->uW.x); put_fq(w + 20, ivc->uW.y); put_fq(w + 24, cmT.x); put_fq(w + 28, cmT.y);
  w[32] = (uint64_t)r_low[0] | ((uint64_t)r_low[1] << 32); w[33] = (uint64_t)r_low[2] | ((uint64_t)r_low[3] << 32); w[34] = 1;      // r = 2^128 + low
  put_fq(w + 36, Aa.x); put_fq(w + 40, Aa.y);
  put_fq(w + 44, Ba.x.c1); put_fq(w + 48, Ba.x.c0); put_fq(w + 52, Ba.y.c1); put_fq(w + 56, Ba.y.c0);      // imaginary parts first, as the EVM's precompile takes G2
  put_fq(w + 60, Ca.x); put_fq(w + 64, Ca.y);
  { const Fe c = Fe::from_mont(cW); memcpy(w + 68, c.v, 32); } { const Fe c = Fe::from_mont(cE); memcpy(w + 72, c.v, 32); }
  memcpy(w + 76, kzg_out[0], 32); memcpy(w + 80, kzg_out[1], 32);
  memcpy(w + 84, kzg_out[0] + 4, 64); memcpy(w + 92, kzg_out[1] + 4, 64);
  for (uint32_t i = 0; i < K.n_pub; i++) { const Fe c = Fe::from_mont(z[1 + i]); memcpy(public_out + 4 * i, c.v, 32); }
  if (seconds) { seconds[0] = t_fold - t_all; seconds[1] = t_wit - t_fold; seconds[2] = t_ntt - t_wit; seconds[3] = t_msm - t_ntt; seconds[4] = now_s() - t_all; seconds[5] = wit.chains_gpu_s; }
  return VIMZ_OK;
}

#ifdef VIMZ_TESTING
// The decider's full assignment z (canonical, 4 words per wire) as vimz_decider_prove builds it for the proof `ivc` holds, with check 5's chains from the host
// (chains_on_gpu = 0) or from the device.  Returns the byte size (copies when buf is large enough); negative: vimz_decider_prove's errors.
int64_t vimz_testing_decider_witness(vimz_decider* d, vimz_cf* ivc, int chains_on_gpu, void* buf, size_t cap) {
  if (!d || !ivc) return VIMZ_ERR_INVALID;
  DeciderWitness wit;
  { const int rc = decider_witness(d, ivc, chains_on_gpu != 0, wit); if (rc) return rc; }
  const size_t bytes = 32 * wit.z.size();
  if (buf && cap >= bytes) { uint64_t* o = (uint64_t*)buf; for (size_t i = 0; i < wit.z.size(); i++) { const Fe c = Fe::from_mont(wit.z[i]); memcpy(o + 4 * i, c.v, 32); } }
  return (int64_t)bytes;
}
#endif

// Decider::verify (reached from `verify_final_proof`, vimz/src/sonobe_backend/decider.rs:31-50, mod.rs:80): what the contract generated for this key
// does with (steps, z_0, z_i, 25 words) — contracts/ContrastVerifier.sol:685-783 — on the host: steps >= 2, the two folded commitments, their
// KZG openings, the Groth16 proof for the public inputs the words imply.  *result = 0 accepted; else a bit set: 1 fewer than two steps, 2 KZG
// opening of cmW, 4 of cmE, 8 Groth16, 16 a word pair is not a curve point (the contract's precompile would revert).  Host only.
int vimz_decider_verify(const vimz_decider* d, uint64_t steps, const uint64_t* z0, const uint64_t* zi, const uint64_t words[100], uint32_t* result) {
  if (!d || !z0 || !zi || !words || !result) return VIMZ_ERR_INVALID;
  if (aff_is_identity(d->kzg_vk)) return vz_fail(d->ctx, VIMZ_ERR_INVALID, "vimz_decider_verify: the decider was set up without the SRS's verifying key");
  *result = verify_words(key_of(d), steps, z0, zi, words);
  return VIMZ_OK;
}
// the same with the key as bytes (vimz_decider_vk's layout; also how a contract's constants are fed in: tests/test_decider_verify_host.py runs the
// reference's six committed proofs through this with the constants of contracts/*Verifier.sol).  No context, no GPU.
int vimz_decider_verify_key(const uint64_t* key_words, size_t n_key_words, uint64_t steps, const uint64_t* z0, const uint64_t* zi, uint32_t len_z,
                            const uint64_t words[100], uint32_t* result) {
  if (!key_words || !z0 || !zi || !words || !result) return VIMZ_ERR_INVALID;
  VerifierKey K;
  if (!parse_key(key_words, n_key_words, &K) || K.len_z != len_z) return VIMZ_ERR_INVALID;
  *result = verify_words(K, steps, z0, zi, words);
  return VIMZ_OK;
}

}  // extern "C"
