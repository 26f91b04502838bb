// Every host-side decision about one MSM, as a pure function of plain values: which of the three paths runs (k_msm_fixed, the fused k_msm_small,
// the general pipeline), the window plan, and every size the launchers (msm.hpp) reserve and launch from.  No HIP and no curve code in here, so the
// decisions are tested on the CPU (tests/native/msm_shape_check.cpp), and the producer of the pinned window sums (msm_launch) and their consumer
// (msm_finish) read how many sums there are, and what they mean, from the same lines (msm_kout and the helpers next to it).
#pragma once
#include <cstdint>
#include <cstddef>
#include <algorithm>

namespace vz {

constexpr int MSM_SUB = 16;          // max entries one thread accumulates in k_accum: the chain of dependent additions per thread;
                                     // the partials of a bucket are then folded by k_combine.  8 / 12 / 16 / 24 give the same steps/s within the run-to-run noise
                                     // (shorter pieces: k_accum wastes fewer lanes at its end, k_combine has more partials to fold —
                                     // in the bench 0.27 + 0.31, 0.29 + 0.25, 0.32 + 0.25, 0.53 + 0.19 ms)
constexpr int MSM_MAX_WINDOWS = 96;
constexpr uint32_t MSM_VWIN = 1024;  // window tables with one shared bucket set: its 2^(c-1) buckets are reduced as virtual windows of this many
constexpr uint32_t MSM_ROWS_MAX = 16;      // rows of one group (msm_launch_rows)

struct MsmPlan {
  int c;            // window bits
  int K;            // windows
  uint32_t nbw;     // buckets per window = 2^(c-1)
  uint32_t nb;      // total buckets
  int split_ones;   // unit scalars summed separately (one more sum after the msm_kout others)
  int tabled;       // 1: window tables, one bucket set, (R_v, S_v) of nbw / MSM_VWIN virtual windows, no Horner; 2: tables of the fused small path (K sums, no Horner);
                    // 3: tables with per-window bucket sets; 4: one bucket set reduced by BIT PLANES (k_reduce_planes: log2(nbw) + 2 sums)
};

// The fused single-launch path for small MSMs (k_msm_small): window, points per workgroup chunk, chunks, size limit.
constexpr int SMALL_C = 7;
constexpr uint32_t SMALL_CHUNK = 1536, SMALL_MAXQ = 32;
constexpr uint32_t SMALL_NBW = 1u << (SMALL_C - 1);
// (measured on MI355X, dense scalars, tools/small_msm_crossover.py: fused 0.22 / 0.29 / 0.31 / 0.35 / 0.45 ms at 16 k / 24.6 k / 27.7 k / 32.8 k / 49 k
//  points against 0.28 / 0.34 / 0.35 / 0.34 / 0.42 ms through the general pipeline: the hand-over is at 20 chunks)
constexpr size_t MSM_SMALL_MAX = (size_t)SMALL_CHUNK * 20;
static_assert(MSM_SMALL_MAX <= (size_t)SMALL_CHUNK * SMALL_MAXQ, "chunk results of a window fit the workspace");
constexpr uint32_t FIXED_PER_THREAD = 4, FIXED_CHUNK = 256 * FIXED_PER_THREAD;      // k_msm_fixed: points per workgroup
constexpr uint32_t SORT_BLOCKS = 256;      // LDS counting sort: at most one workgroup per CU (msm_shape picks fewer for small inputs)
// words of the fixed-size slices every row of a workspace holds (MsmWorkspace::row_bytes): the ticket block, the heavy-bucket list, its tickets
constexpr uint32_t MSM_TOTALS_WORDS = 16, MSM_HEAVY_CAP = 65536, MSM_HEAVY_DONE_WORDS = 1024;
constexpr uint32_t MSM_HEAVY_SCRATCH_POINTS = 1024 * 32;      // partial sums of the split heavy buckets

static inline MsmPlan msm_plan(size_t n, int scalar_bits, int c_override) {
  MsmPlan p;
  p.split_ones = 0; p.tabled = 0;
  int c = c_override;
  if (c <= 0) {
    // Measured on MI355X (profiles/r01_msm_phases.txt): k_accum is throughput-bound (~n*K mixed adds) while
    // k_reduce is a latency-bound serial chain whose depth grows with 2^c / 256, so the optimum sits at a
    // much smaller window than the classic ln(n) rule: c = 11 from 2^15 points up, shrinking below.
    c = n >= (1u << 15) ? 11 : n >= (1u << 12) ? 9 : n >= 256 ? 7 : 5;
  }
  p.c = c;
  p.K = (scalar_bits + 1 + c - 1) / c;
  p.nbw = 1u << (c - 1);
  p.nb = p.nbw * (uint32_t)p.K;
  return p;
}

// What the reduce of a plan writes, read by the launcher (where the sums go, where the unit sum follows) and by msm_finish (how to weigh them):
// a shared bucket set comes back as V virtual windows of vw buckets, (R_v, S_v) each — or, tabled == 4, as log2(nbw) bit planes and two plain halves.
static inline uint32_t msm_vwin(const MsmPlan& p) { return std::min<uint32_t>(p.nbw, MSM_VWIN); }
static inline int msm_vwindows(const MsmPlan& p) { return (int)(p.nbw / msm_vwin(p)); }
static inline uint32_t msm_plane_bits(const MsmPlan& p) { uint32_t P = 0; while ((1u << P) < p.nbw) P++; return P; }
// k_reduce_planes over a bucket set of nbw buckets: Pl = log2 nbw planes, Gp workgroups per plane (256·lpt leaves each, lpt = nbw / (512·Gp)); false where
// the plane workgroups' partial sums do not fit one tree, or the Pl + 2 sums and a unit sum the pinned buffer
static inline bool msm_plane_shape(uint32_t nbw, uint32_t& Pl, uint32_t& Gp) {
  Pl = 0; while ((1u << Pl) < nbw) Pl++;
  Gp = std::min<uint32_t>(16u, nbw / 1024u);
  while (Gp > 1 && (Pl + 2) * Gp > 256) Gp >>= 1;
  return nbw >= 1024 && (1u << Pl) == nbw && (Pl + 2) * Gp <= 256 && (int)Pl + 2 + 1 <= MSM_MAX_WINDOWS;
}
static inline int msm_kout(const MsmPlan& p) { return p.tabled == 4 ? (int)msm_plane_bits(p) + 2 : p.tabled == 1 ? 2 * msm_vwindows(p) : p.K; }
static inline int msm_sums_out(const MsmPlan& p) { return msm_kout(p) + (p.split_ones ? 1 : 0); }      // all sums of the pinned buffer: the unit sum is the last

// VIMZ_TUNE (parsed in msm.hpp, msm_tuning): what an MSM's shape or kernels may be pinned to; results never depend on it
struct MsmTuning { int sort_blocks = 0, combine_lane_bits = -1, ones_dense = 1, reduce_planes = 0, signed_scalars = 1; };
// a key's precomputed tables (BaseTables without its pointers) and the row group of a call (msm_launch_rows), as msm_shape needs them
struct MsmTableDesc { bool present = false; int c = 0, K = 0, own = 0; bool mult = false; size_t n_total = 0; };
struct MsmGroupDesc { bool grouped = false; uint32_t G = 1, n_extra = 0; };

enum MsmPath { MSM_PATH_FIXED, MSM_PATH_SMALL, MSM_PATH_LARGE };
enum { MSM_SHAPE_OK = 0, MSM_SHAPE_INVALID = 1, MSM_SHAPE_NOT_SUPPORTED = 2 /* a shape the grouped chain does not cover: row after row */ };

struct MsmShape {
  MsmPath path = MSM_PATH_LARGE;
  MsmPlan plan = {};      // final: what *plan_out receives, in one assignment
  // fused paths: k_msm_small runs Q chunks of `chunk` points per window, k_msm_fixed Qf workgroups per window
  uint32_t Q = 0, chunk = 0, Qf = 0;
  // general pipeline
  bool lds_sort = false;  // all buckets' counters fit one workgroup's LDS: the contention-free sort (else k_hist / k_scatter with global atomics)
  bool own = false;       // tables with per-window bucket sets
  bool shared = false;    // tables with one bucket set for all windows
  bool planes = false;    // ... reduced by bit planes
  uint32_t sub = 0;       // entries per accumulation thread
  size_t entries = 0, max_subs = 0;      // upper bounds: sort entries, sub-buckets
  uint32_t sort_blocks = 0, lane_bits = 0, heavy_min = 0;
  uint32_t bstride = 0 /* buckets between windows */, pstride = 0 /* table row length */;
  uint32_t vw = 0; int V = 0;            // msm_vwin, msm_vwindows
  uint32_t Pl = 0, Gp = 0;               // bit planes: log2 nbw, workgroups per plane
  int kout = 0;           // sums the reduce writes, before the unit sum (msm_kout)
};

static inline int msm_shape(MsmShape& out, size_t n, int scalar_bits, int c_override, int split_ones, const MsmTableDesc& tb, const MsmGroupDesc& rg,
                            const MsmTuning& tune, bool no_small) {
  MsmShape s;
  if (n == 0 || n >= (1u << 31)) return MSM_SHAPE_INVALID;
  if (rg.grouped && (rg.G == 0 || rg.G > MSM_ROWS_MAX || rg.n_extra > MSM_ROWS_MAX || (split_ones == 0 && rg.n_extra))) return MSM_SHAPE_INVALID;
  // tables made for the fused small path (window SMALL_C): its window sums then only need adding — no Horner on the host
  const bool small_fmt = tb.present && tb.c == SMALL_C;             // (ignored, not an error, when the fused path is switched off)
  const bool small_tb = small_fmt && !no_small && c_override <= 0;
  bool tabled = tb.present && !small_fmt && c_override <= 0;
  // tables with per-window bucket sets only fit the window this size would get anyway; otherwise they are not used
  if (tabled && tb.own && tb.c != msm_plan(n, scalar_bits, 0).c) tabled = false;
  s.own = tabled && tb.own;
  s.shared = tabled && !tb.own;
  if (small_tb && (n > MSM_SMALL_MAX || tb.K != (scalar_bits + SMALL_C) / SMALL_C)) return MSM_SHAPE_INVALID;
  if (!no_small && !tabled && c_override <= 0 && n <= MSM_SMALL_MAX) {      // fused single-launch path
    if (rg.grouped) return MSM_SHAPE_NOT_SUPPORTED;
    MsmPlan& ps = s.plan;
    ps.c = SMALL_C; ps.K = (scalar_bits + SMALL_C) / SMALL_C; ps.nbw = SMALL_NBW; ps.nb = SMALL_NBW * (uint32_t)ps.K; ps.split_ones = 0; ps.tabled = small_tb ? 2 : 0;
    s.kout = msm_kout(ps);
    if (small_tb && tb.mult) {      // every multiple resident: the digits select their points (k_msm_fixed)
      s.path = MSM_PATH_FIXED;
      s.Qf = (uint32_t)((n + FIXED_CHUNK - 1) / FIXED_CHUNK);
    } else {
      s.path = MSM_PATH_SMALL;
      s.Q = (uint32_t)((n + SMALL_CHUNK - 1) / SMALL_CHUNK); s.chunk = (uint32_t)((n + s.Q - 1) / s.Q);
    }
    out = s;
    return MSM_SHAPE_OK;
  }
  s.path = MSM_PATH_LARGE;
  MsmPlan& pl = s.plan;
  pl = msm_plan(n, scalar_bits, tabled ? tb.c : c_override);
  if (tabled) {            // one bucket set shared by all windows — or (own) the usual ones, whose sums then need no Horner
    if (tb.K != pl.K || pl.nbw < 256 || (size_t)tb.K * tb.n_total >= (1u << 31)) return MSM_SHAPE_INVALID;
    if (!s.own && 2 * msm_vwindows(pl) + 1 > MSM_MAX_WINDOWS) return MSM_SHAPE_INVALID;
    if (s.own) pl.tabled = 3; else { pl.nb = pl.nbw; pl.tabled = 1; }
  }
  if (pl.K + 1 > MSM_MAX_WINDOWS || pl.c > 16 || pl.c < 2) return MSM_SHAPE_INVALID;
  pl.split_ones = split_ones;
  // shared bucket set: as virtual windows (k_reduce), or — VIMZ_TUNE=reduce_planes=1 — by bit planes (k_reduce_planes) where the plane workgroups' partial sums fit one tree
  const bool planes_fit = msm_plane_shape(pl.nbw, s.Pl, s.Gp);
  s.planes = s.shared && tune.reduce_planes && planes_fit;
  if (s.planes) pl.tabled = 4;
  s.lds_sort = (size_t)pl.nb * 4 <= 144 * 1024;      // all buckets' counters fit in one workgroup's LDS at the default window (24 x 1024 x 4 B = 96 KiB): contention-free sort
  if (rg.grouped && (s.planes || s.own || !s.lds_sort)) return MSM_SHAPE_NOT_SUPPORTED;
  s.entries = (size_t)pl.K * n;
  // small MSMs are latency-bound (one dependent addition ~ 6-10 us): shorter chains per thread, more threads
  // (a witness commitment — split_ones — of an HD-sized circuit is a few 10^5 entries spread thinly over the buckets: one thread per bucket and a
  //  chain of a dozen additions each on a quarter of the GPU; pieces of 8 give twice the threads half the chain: 1 045-1 061 -> 1 088-1 097 steps/s at
  //  contrast HD, one chain 808 -> 823; at 4K the buckets are three times as full and the long pieces stay (558 against 542).
  //  Longer pieces for the dense MSM(T) — 24 / 32 entries, half the partials for k_combine — measured within the noise at 256 rows and
  //  worse in the 20-row window and on one chain: 842 against 876, 786 against 812; shorter ones were worse too: DESIGN_LOG.md)
  s.sub = n < (1u << 15) ? 8u : split_ones ? (n < (1u << 19) ? 8u : (uint32_t)MSM_SUB) : (uint32_t)MSM_SUB;   // MSM_SUB for everything large
  s.max_subs = s.entries / s.sub + pl.nb + 1;
  // every sort workgroup zeroes, writes out and later re-reads all nb counters (96 KiB at the default window): with one workgroup
  // per CU at 305 k points each handled 1.2 k scalars for 24.5 k counters, and k_block_prefix walked 256 rows — fixed costs.
  // About 4 k scalars per workgroup (75 workgroups here) measured best: one proof 384 -> 394 steps/s, three 599 -> 614.
  s.sort_blocks = tune.sort_blocks > 0 && tune.sort_blocks <= (int)SORT_BLOCKS ? (uint32_t)tune.sort_blocks
                                                                                 : (uint32_t)std::min<size_t>(SORT_BLOCKS, std::max<size_t>(32, n / 4096));
  s.bstride = s.shared ? 0u : pl.nbw; s.pstride = tabled ? (uint32_t)tb.n_total : 0u;
  // lanes per ordinary bucket in k_combine, from the mean number of partials per bucket (upper bound: every digit non-zero): two
  // lanes up to ~24 partials (measured at 312 k dense points, 19 per bucket: 16 lanes 0.28 ms, 8: 0.155, 4: 0.137, 2: 0.117;
  // one lane and a heavy list of every bucket: 3.5 ms); buckets above 16 partials per lane go to the heavy list
  // (a witness — split_ones — has far fewer entries than its upper bound: an eighth is assumed, which gives its buckets two lanes where
  //  the bound gave four: k_combine 31.4 -> 29.1 M instructions per step)
  const size_t mean_parts = (split_ones ? s.entries / 8 : s.entries) / s.sub / pl.nb + 1;
  s.lane_bits = tune.combine_lane_bits >= 0 ? (uint32_t)tune.combine_lane_bits : mean_parts > 96 ? 4u : mean_parts > 48 ? 3u : mean_parts > 24 ? 2u : 1u;
  s.heavy_min = 16u << s.lane_bits;
  s.vw = msm_vwin(pl); s.V = msm_vwindows(pl); s.kout = msm_kout(pl);
  out = s;
  return MSM_SHAPE_OK;
}

}  // namespace vz
