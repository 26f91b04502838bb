// Image hasher: the running Poseidon hash the circuits keep of an image (circuits/src/utils/hashers.circom, image_running_hash.circom),
// the value a proof's final state z_n[0] / z_n[1] holds for its source / target image.  It replaces pyvimz's `image-hasher`
// (pyvimz/pyvimz/image_hasher.py: one circom witness-generator process per row).
//
//   unit digest   d = ArrayHasher(L)(unit) = _WindowFoldHasher(L, 8): Poseidon(min(L, 8)) over the first window, then ceil(L/8) - 1 windows
//                 of Poseidon(k + 1) over (previous digest, next k = min(rest, 7) elements) — t runs from 2 to 9, and the last L - 8 - 7·(ceil(L/8) - 1)
//                 elements are never absorbed
//   running hash  acc_0 = 0, acc_{i+1} = PairHasher(acc_i, d_i)   (HeadTailHasher; a dropped unit contributes PairHasher(acc_i, 0): redact)
//   units         image rows, or 40 x 40 blocks, packed as vimz_pack_pixels packs them (10 pixels per element, R in the low byte)
//
// The digests of every unit of every image of a call are independent chains: ONE launch, k_image_digests, one lane group per chain.  Each chain is
// serial (17 permutations per HD row, 96 per 8K row) and there are few of them (720 at HD), so the kernel is latency-bound: the permutations run in
// the reduced-radix arithmetic of the witness chains (fp29.hpp, witness.hpp: poseidon_group29 — lane i owns state[i], the MDS rows are gathered
// with shuffles, partial rounds in sparse form), 8 lanes per chain when no permutation of it is wider than t = 8, 16 otherwise.  Packing is fused
// into the kernel: a lane reads the 10 pixels of the element it absorbs.  The serial PairHasher chain over the digests is one t = 3 permutation per
// unit and runs on the host (cb::poseidon_hash), one image per thread, as vimz_ivc_chain_from_digests does.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "internal.hpp"
#include "fp29.hpp"
#include "circuit/poseidon_params.hpp"

using namespace vz;

namespace {

typedef Fp29<BnFr> F29;
constexpr int IH_STRIDE = 12;        // words per table element (three 16-byte loads), as witness.hpp's F29_STRIDE
constexpr int IH_WAVE = 64;
constexpr uint32_t IH_MAX_LEN = 1u << 20;        // elements per unit

struct IhTables {        // per width t (index t, 2..9): round constants, MDS, sparse partial rounds, basis change — all in the fp29 form
  const uint32_t* c[10]; const uint32_t* m[10]; const uint32_t* s[10]; const uint32_t* f[10];
  uint32_t rp[10];
};
struct IhImage { const uint8_t* px; const uint32_t* units; uint32_t h, w, ch, block, L, pad; };       // px: pixels (rows from 0) | units: canonical elements
struct IhSeg { uint32_t first_block, n_chains, chain_off, L; };       // chains of one unit length: workgroups [first_block, next segment's)
struct IhChain { uint32_t img, unit; };

__device__ __forceinline__ F29 ih_load29(const uint32_t* __restrict__ base, size_t idx) {
  const uint4* q = reinterpret_cast<const uint4*>(base + (size_t)IH_STRIDE * idx);
  const uint4 a = q[0], b = q[1], c = q[2];
  F29 r; r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w; r.v[8] = c.x;
  return r;
}
__device__ __forceinline__ F29 ih_shfl29(const F29& v, int src_lane) {
  F29 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = __shfl(v.v[k], src_lane);
  return r;
}

// Element e of unit `unit` as x·2^261 mod p (below 1.5 p).  Pixels: the packing of k_pack_pixels (capi.hip) — row r / 40 x 40 block, zero pixels
// past the row's end, channels beyond the third ignored (alpha), a grey value in the R slot.
__device__ __forceinline__ F29 ih_element(const IhImage& I, uint32_t unit, uint32_t e) {
  uint32_t w8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (I.units) {
    const uint4* q = reinterpret_cast<const uint4*>(I.units + 8 * ((size_t)unit * I.L + e));
    const uint4 a = q[0], b = q[1];
    w8[0] = a.x; w8[1] = a.y; w8[2] = a.z; w8[3] = a.w; w8[4] = b.x; w8[5] = b.y; w8[6] = b.z; w8[7] = b.w;
  } else {
    uint32_t row, col0, run;
    if (!I.block) {
      row = unit; col0 = e * 10; run = I.w - col0;          // (e < ceil(w / 10): col0 < w)
    } else {
      const uint32_t bw = (I.w + I.block - 1) / I.block, per_row = (I.block + 9) / 10;
      const uint32_t br = unit / bw, bc = unit % bw, r = e / per_row, c = e % per_row;
      row = br * I.block + r; col0 = bc * I.block + c * 10;
      const uint32_t end = min(I.w, (bc + 1) * I.block);
      run = row < I.h && col0 < end ? end - col0 : 0;
    }
    const uint32_t nc = I.ch < 3 ? I.ch : 3;
    const uint8_t* p = I.px + ((size_t)row * I.w + col0) * I.ch;
#pragma unroll
    for (uint32_t k = 0; k < 10; k++)          // (unrolled: constant byte positions keep w8 in registers)
#pragma unroll
      for (uint32_t c = 0; c < 3; c++) {
        const uint32_t byte = 3 * k + c;
        if (k < run && c < nc) w8[byte >> 2] |= (uint32_t)p[(size_t)k * I.ch + c] << (8 * (byte & 3));
      }
  }
  F29 r2;
#pragma unroll
  for (int i = 0; i < 9; i++) r2.v[i] = F29::R2_29.l[i];
  return F29::mul(F29::pack(w8), r2);      // (x < 2^256 < 6 p, R2 < p: 6·1 <= 64 -> below 1.05 p)
}

// One Poseidon permutation of width T on a group of G lanes (lane li < T owns state[li]); s below 2 p in, below 2 p out.  The rounds of
// witness.hpp's poseidon_group29 without the wires: full rounds with the MDS row gathered by shuffles, partial rounds in sparse form
// (one S-box, a dot product with the first row reduced across the group, a first-column update), the basis change after them.
template <int T>
__device__ __forceinline__ F29 ih_perm(const IhTables& P, F29 s, uint32_t li, int lane_base, int G) {
  const uint32_t* __restrict__ PC = P.c[T];
  const uint32_t* __restrict__ PM = P.m[T];
  const uint32_t* __restrict__ PS = P.s[T];
  const uint32_t* __restrict__ PF = P.f[T];
  const uint32_t rp = P.rp[T];
  const bool mine = li < (uint32_t)T;
  F29 Mrow[T];
#pragma unroll
  for (int j = 0; j < T; j++) Mrow[j] = mine ? ih_load29(PM, (size_t)li * T + j) : F29::zero();
  auto full_round = [&](uint32_t r) {
    if (mine) {
      s = F29::add(s, ih_load29(PC, (size_t)r * T + li));                     // < 3
      const F29 x2 = F29::sqr(s), x4 = F29::sqr(x2);
      s = F29::mul(x4, s);                                                    // 9, 2.25, 4.5 -> each < 1.5
    }
    F29 prod[T];
#pragma unroll
    for (int j = 0; j < T; j++) prod[j] = F29::mul(Mrow[j], ih_shfl29(s, lane_base + j));     // 1 · 1.5
#pragma unroll
    for (int stride = 1; stride < T; stride <<= 1)
#pragma unroll
      for (int j = 0; j + stride < T; j += 2 * stride) prod[j] = F29::add(prod[j], prod[j + stride]);
    s = prod[0].weak_reduce();                                                // T · 1.5 <= 13.5 -> < 1.65
  };
  for (uint32_t r = 0; r < 4; r++) full_round(r);
  const bool l0 = li == 0;
  F29 ct = F29::zero(), rw = F29::zero(), cl = F29::zero();
  if (mine) { const size_t q = 3 * (size_t)li; ct = ih_load29(PS, q); rw = ih_load29(PS, q + 1); cl = ih_load29(PS, q + 2); }
  for (uint32_t r = 0; r < rp; r++) {
    F29 ctn = F29::zero(), rwn = F29::zero(), cln = F29::zero();
    if (mine && r + 1 < rp) { const size_t q = 3 * ((size_t)(r + 1) * T + li); ctn = ih_load29(PS, q); rwn = ih_load29(PS, q + 1); cln = ih_load29(PS, q + 2); }
    s = F29::add(s, ct);                                           // < 3
    const F29 sl0 = ih_shfl29(s, lane_base);
    const F29 m1 = F29::mul(l0 ? s : rw, s);                       // lane 0: x2 (3·3); lane i: row_i·s_i
    const F29 u = F29::mul(l0 ? rw : cl, sl0);                     // lane 0: row_0·s; lane i: col_i·s_0
    F29 x4 = F29::zero();
    if (l0) x4 = F29::sqr(m1);
    const F29 x4b = ih_shfl29(x4, lane_base);
    const F29 m2 = F29::mul(x4b, u);                               // lane 0: row_0·x5; lane i: col_i·x5
    F29 p = l0 ? m2 : (mine ? m1 : F29::zero());
    for (int off = G >> 1; off >= 1; off >>= 1) {                  // (G wave-uniform)
      F29 o;
#pragma unroll
      for (int k = 0; k < 9; k++) o.v[k] = __shfl_xor(p.v[k], off);
      p = F29::add(p, o);                                          // <= T terms below 1.5
    }
    s = (l0 ? p : (mine ? F29::add(s, m2) : s)).weak_reduce();     // 13.5 | 3 + 1.5 -> < 1.65
    ct = ctn; rw = rwn; cl = cln;
  }
  {
    F29 acc = F29::zero();
#pragma unroll
    for (int j = 0; j < T - 1; j++) {
      const F29 sj = ih_shfl29(s, lane_base + 1 + j);
      if (mine && !l0) acc = F29::add(acc, F29::mul(ih_load29(PF, (size_t)(li - 1) * (T - 1) + j), sj));     // <= 8 terms below 1.5
    }
    if (mine && !l0) s = acc.weak_reduce();
  }
  for (uint32_t r = 4 + rp; r < 8 + rp; r++) full_round(r);
  return s;
}

// grid: one 64-lane workgroup per (segment, 64 / G chains); out: one canonical digest (8 words) per chain, in chain order.
__global__ void __launch_bounds__(IH_WAVE) k_image_digests(IhTables P, const IhImage* __restrict__ imgs, const IhSeg* __restrict__ segs, uint32_t n_segs,
                                                           const IhChain* __restrict__ chains, uint32_t* __restrict__ out) {
  uint32_t sg = 0;
  while (sg + 1 < n_segs && blockIdx.x >= segs[sg + 1].first_block) sg++;
  const IhSeg S = segs[sg];
  const int G = S.L >= 8 ? 16 : 8;           // t = 9 needs 9 lanes; a unit of at most 7 elements is one permutation of t <= 8
  const uint32_t li = threadIdx.x & (uint32_t)(G - 1);
  const int lane_base = (int)(threadIdx.x & ~(uint32_t)(G - 1));
  const uint32_t k = (blockIdx.x - S.first_block) * (IH_WAVE / G) + threadIdx.x / G;
  const bool live = k < S.n_chains;
  const IhChain C = chains[S.chain_off + (live ? k : 0)];      // (an idle group of the last workgroup repeats the segment's first chain: shuffles stay convergent)
  const IhImage I = imgs[C.img];
  const uint32_t L = S.L, rounds = (L + 7) / 8;
  F29 h = F29::zero();
  uint32_t done = 0;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t kin = r == 0 ? min(L, 8u) : min(L - done, 7u);
    const uint32_t t = r == 0 ? kin + 1 : kin + 2;
    F29 s = F29::zero();                                     // lane 0: 0; lane 1: the previous window's digest (after the first); then the elements
    if (li >= 1 && li < t) s = (r > 0 && li == 1) ? h : ih_element(I, C.unit, done + li - (r == 0 ? 1 : 2));
    switch (t) {                                             // (wave-uniform: every chain of a workgroup has the same L)
      case 2: s = ih_perm<2>(P, s, li, lane_base, G); break;
      case 3: s = ih_perm<3>(P, s, li, lane_base, G); break;
      case 4: s = ih_perm<4>(P, s, li, lane_base, G); break;
      case 5: s = ih_perm<5>(P, s, li, lane_base, G); break;
      case 6: s = ih_perm<6>(P, s, li, lane_base, G); break;
      case 7: s = ih_perm<7>(P, s, li, lane_base, G); break;
      case 8: s = ih_perm<8>(P, s, li, lane_base, G); break;
      default: s = ih_perm<9>(P, s, li, lane_base, G); break;
    }
    h = ih_shfl29(s, lane_base);
    done += kin;
  }
  if (live && li == 0) {
    F29 one = F29::zero(); one.v[0] = 1;
    const F29 x = F29::mul(h, one).canon();                 // x·2^261 -> x (below 1.02 p), then [0, p)
    uint32_t w8[8]; x.unpack(w8);
    uint4* o = reinterpret_cast<uint4*>(out + 8 * (size_t)k + 8 * (size_t)S.chain_off);
    o[0] = make_uint4(w8[0], w8[1], w8[2], w8[3]); o[1] = make_uint4(w8[4], w8[5], w8[6], w8[7]);
  }
}

// The tables for t = 2..9 in the fp29 form, built once per process (host), uploaded once per context.
struct IhHostTables { std::vector<uint32_t> words; size_t c[10], m[10], s[10], f[10]; uint32_t rp[10]; };
const IhHostTables& ih_host_tables() {
  static const IhHostTables T = [] {
    IhHostTables H{};
    auto put = [&](const std::vector<cb::Fe>& v) {
      const size_t at = H.words.size();
      H.words.resize(at + v.size() * (size_t)IH_STRIDE, 0u);
      for (size_t i = 0; i < v.size(); i++) { const F29 x = F29::from_std(v[i]); for (int k = 0; k < 9; k++) H.words[at + i * IH_STRIDE + k] = x.v[k]; }
      return at;
    };
    for (int t = 2; t <= 9; t++) {
      const cb::PoseidonTable& P = cb::poseidon_table(t);
      const auto& S = cb::poseidon_sparse_t<BnFr>(t);
      std::vector<cb::Fe> packed((size_t)P.rp * t * 3);      // per (round, lane): transformed constant, first-row entry, first-column entry (0 for lane 0)
      for (int r = 0; r < P.rp; r++)
        for (int i = 0; i < t; i++) {
          cb::Fe* q = &packed[3 * ((size_t)r * t + i)];
          q[0] = S.ctil[(size_t)r * t + i]; q[1] = S.row[(size_t)r * t + i]; q[2] = i ? S.col[(size_t)r * (t - 1) + i - 1] : cb::Fe::zero();
        }
      H.c[t] = put(P.C); H.m[t] = put(P.M); H.s[t] = put(packed); H.f[t] = put(S.Pfin); H.rp[t] = (uint32_t)P.rp;
    }
    return H;
  }();
  return T;
}

inline size_t ih_align(size_t x) { return (x + 255) & ~(size_t)255; }

bool ih_below_modulus(const uint64_t* x) {
  const uint32_t* m = BnFr::MOD.w;
  for (int i = 3; i >= 0; i--) {
    const uint64_t mi = (uint64_t)m[2 * i] | (uint64_t)m[2 * i + 1] << 32;
    if (x[i] != mi) return x[i] < mi;
  }
  return false;
}

}  // namespace

static int fail(vimz_ctx* c, int code, const char* what, hipError_t e = hipSuccess) { return vz::vz_fail(c, code, what, e); }

extern "C" int vimz_image_hash(vimz_ctx* c, const vimz_image_desc* imgs, size_t n, uint64_t* out) {
  if (!c) return VIMZ_ERR_INVALID;
  if (!imgs || !out || n == 0 || n > 4096) return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: bad argument (1 to 4096 images, out not NULL)");
  // ---- validate every descriptor before anything touches the device
  std::vector<IhImage> dimg(n);
  std::vector<size_t> units(n), bytes(n);
  size_t total_chains = 0;
  for (size_t i = 0; i < n; i++) {
    const vimz_image_desc& D = imgs[i];
    IhImage& I = dimg[i];
    size_t all = 0, L = 0;
    if (D.pixels) {
      if (!D.height || !D.width || D.height > (1ull << 20) || D.width > (1ull << 20) || D.height * D.width > (1ull << 30) ||
          (D.channels != 1 && D.channels != 3 && D.channels != 4) || D.block < 0 || D.block > 4096)
        return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: bad image (at most 2^20 per dimension and 2^30 pixels, channels 1, 3 or 4, block 0..4096)");
      const size_t b = (size_t)D.block;
      L = b ? b * ((b + 9) / 10) : (D.width + 9) / 10;
      all = b ? ((D.height + b - 1) / b) * ((D.width + b - 1) / b) : D.height;
    } else {
      if (!D.units || !D.n_units || !D.unit_len || D.unit_len > IH_MAX_LEN || D.n_units > (1ull << 24) || D.block != 0)
        return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: bad packed units (units not NULL, 1..2^24 units of 1..2^20 elements, block 0)");
      L = D.unit_len; all = D.n_units;
    }
    if (L > IH_MAX_LEN) return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: units longer than 2^20 elements");
    if (D.max_units > all) return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: max_units exceeds the image's rows / blocks");
    const size_t U = D.max_units ? D.max_units : all;
    if (!D.pixels) {
      if (U * L > (1ull << 28)) return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: more than 2^28 packed elements");
      for (size_t e = 0; e < U * L; e++)
        if (!ih_below_modulus(D.units + 4 * e)) return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: a packed element is not below the field modulus");
      bytes[i] = 32 * U * L;
    } else {
      // only the rows the first U units read travel to the device
      const size_t b = (size_t)D.block, bw = b ? (D.width + b - 1) / b : 1;
      const size_t rows = b ? std::min<size_t>(D.height, ((U + bw - 1) / bw) * b) : U;
      bytes[i] = rows * D.width * (size_t)D.channels;
    }
    units[i] = U;
    I.h = (uint32_t)(D.pixels ? D.height : 0); I.w = (uint32_t)(D.pixels ? D.width : 0); I.ch = (uint32_t)(D.pixels ? D.channels : 0);
    I.block = (uint32_t)(D.pixels ? D.block : 0); I.L = (uint32_t)L; I.pad = 0;
    for (size_t u = 0; u < U; u++) total_chains += D.drop && D.drop[u] ? 0 : 1;
  }
  if (total_chains >= (1ull << 31)) return fail(c, VIMZ_ERR_INVALID, "vimz_image_hash: too many units");

  // ---- the chains, grouped by unit length (one segment per length)
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return dimg[a].L < dimg[b].L; });
  std::vector<IhChain> chains; chains.reserve(total_chains);
  std::vector<IhSeg> segs;
  std::vector<size_t> first_chain(n);      // per image: index of its first (undropped) unit's chain; chains of an image are consecutive
  uint32_t blocks = 0;
  for (size_t oi = 0; oi < n; oi++) {
    const size_t i = order[oi];
    const uint32_t L = dimg[i].L;
    size_t cnt = 0;
    first_chain[i] = chains.size();
    for (size_t u = 0; u < units[i]; u++) if (!(imgs[i].drop && imgs[i].drop[u])) { chains.push_back(IhChain{(uint32_t)i, (uint32_t)u}); cnt++; }
    if (!cnt) continue;
    const uint32_t per = L >= 8 ? IH_WAVE / 16 : IH_WAVE / 8;
    if (!segs.empty() && segs.back().L == L) {
      IhSeg& S = segs.back();
      blocks -= (S.n_chains + per - 1) / per;
      S.n_chains += (uint32_t)cnt;
      blocks += (S.n_chains + per - 1) / per;
    } else {
      segs.push_back(IhSeg{blocks, (uint32_t)cnt, (uint32_t)(chains.size() - cnt), L});
      blocks += (uint32_t)((cnt + per - 1) / per);
    }
  }
  std::vector<uint32_t> digests(8 * chains.size());
  typedef std::chrono::steady_clock clk;
  const clk::time_point t0 = clk::now();

  {
    std::lock_guard<std::mutex> g(c->mu);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, VIMZ_ERR_HIP, "vimz_image_hash: hipSetDevice", e);
    const IhHostTables& HT = ih_host_tables();
    if (!c->image_hash_tables) {
      uint32_t* d = nullptr;
      if ((e = hipMalloc((void**)&d, 4 * HT.words.size())) != hipSuccess) return fail(c, VIMZ_ERR_HIP, "vimz_image_hash: Poseidon tables", e);
      if ((e = hipMemcpyAsync(d, HT.words.data(), 4 * HT.words.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess) {
        hipStreamSynchronize(c->stream); hipFree(d);
        return fail(c, VIMZ_ERR_HIP, "vimz_image_hash: Poseidon tables", e);
      }
      c->image_hash_tables = d;
    }
    IhTables P{};
    for (int t = 2; t <= 9; t++) {
      P.c[t] = c->image_hash_tables + HT.c[t]; P.m[t] = c->image_hash_tables + HT.m[t];
      P.s[t] = c->image_hash_tables + HT.s[t]; P.f[t] = c->image_hash_tables + HT.f[t]; P.rp[t] = HT.rp[t];
    }
    if (!chains.empty()) {
      // one device buffer per context, grown geometrically; the one it replaces is retired, not freed (no device-wide synchronisation: a prover
      // may be folding on this GPU).  (A stream-ordered hipMallocAsync / hipFreeAsync per call was tried first: repeated calls then returned
      // wrong hashes on an MI355X.)
      size_t off = 0;
      const size_t o_img = off; off += ih_align(sizeof(IhImage) * n);
      const size_t o_seg = off; off += ih_align(sizeof(IhSeg) * segs.size());
      const size_t o_chn = off; off += ih_align(sizeof(IhChain) * chains.size());
      const size_t o_out = off; off += ih_align(32 * chains.size());
      std::vector<size_t> o_data(n);
      for (size_t i = 0; i < n; i++) { o_data[i] = off; off += ih_align(bytes[i]); }
      if (off > c->image_hash_bytes) {
        const size_t want = std::max(off, 2 * c->image_hash_bytes);
        void* nb = nullptr;
        if ((e = hipMalloc(&nb, want)) != hipSuccess) return fail(c, VIMZ_ERR_HIP, "vimz_image_hash: device buffer", e);
        if (c->image_hash_buf) c->image_hash_retired.push_back(c->image_hash_buf);
        c->image_hash_buf = nb; c->image_hash_bytes = want;
      }
      uint8_t* buf = (uint8_t*)c->image_hash_buf;
      for (size_t i = 0; i < n; i++) {
        dimg[i].px = imgs[i].pixels ? buf + o_data[i] : nullptr;
        dimg[i].units = imgs[i].pixels ? nullptr : (const uint32_t*)(buf + o_data[i]);
      }
      const char* what = nullptr;
      auto h2d = [&](size_t at, const void* src, size_t nb) {
        if (!what && nb && (e = hipMemcpyAsync(buf + at, src, nb, hipMemcpyHostToDevice, c->stream)) != hipSuccess) what = "vimz_image_hash: upload";
      };
      h2d(o_img, dimg.data(), sizeof(IhImage) * n);
      h2d(o_seg, segs.data(), sizeof(IhSeg) * segs.size());
      h2d(o_chn, chains.data(), sizeof(IhChain) * chains.size());
      for (size_t i = 0; i < n; i++) h2d(o_data[i], imgs[i].pixels ? (const void*)imgs[i].pixels : (const void*)imgs[i].units, bytes[i]);
      if (!what) {
        hipLaunchKernelGGL(k_image_digests, dim3(blocks), dim3(IH_WAVE), 0, c->stream, P, (const IhImage*)(buf + o_img), (const IhSeg*)(buf + o_seg),
                           (uint32_t)segs.size(), (const IhChain*)(buf + o_chn), (uint32_t*)(buf + o_out));
        if ((e = hipGetLastError()) != hipSuccess) what = "vimz_image_hash: k_image_digests";
      }
      if (!what && (e = hipMemcpyAsync(digests.data(), buf + o_out, 32 * chains.size(), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) what = "vimz_image_hash: download";
      const hipError_t es = hipStreamSynchronize(c->stream);
      if (what) return fail(c, VIMZ_ERR_HIP, what, e);
      if (es != hipSuccess) return fail(c, VIMZ_ERR_HIP, "vimz_image_hash: k_image_digests", es);
    }
  }

  const clk::time_point t1 = clk::now();
  // ---- the running hash of each image on the host, one image per thread
  auto chain = [&](size_t i) {
    cb::Fe acc = cb::Fe::zero();
    size_t k = first_chain[i];
    for (size_t u = 0; u < units[i]; u++) {
      cb::Fe in[2] = {acc, cb::Fe::zero()};
      if (!(imgs[i].drop && imgs[i].drop[u])) { cb::Fe d; memcpy(d.v, &digests[8 * k++], 32); in[1] = cb::Fe::to_mont(d); }
      acc = cb::poseidon_hash(in, 2);
    }
    const cb::Fe r = cb::Fe::from_mont(acc);
    memcpy(out + 4 * i, r.v, 32);
  };
  const size_t nt = std::min<size_t>(n, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  if (nt <= 1) {
    for (size_t i = 0; i < n; i++) chain(i);
  } else {
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t k = 0; k < nt; k++) th.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < n;) chain(i); });
    for (auto& x : th) x.join();
  }
  const clk::time_point t2 = clk::now();
  std::lock_guard<std::mutex> g(c->mu);
  c->image_hash_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  c->image_hash_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  return VIMZ_OK;
}

extern "C" int vimz_image_hash_last_profile(vimz_ctx* c, double ms[2]) {
  if (!c || !ms) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  ms[0] = c->image_hash_ms[0]; ms[1] = c->image_hash_ms[1];
  return VIMZ_OK;
}
