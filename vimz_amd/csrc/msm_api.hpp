// The MSM's host interface: workspace, table descriptors and the entry points that msm_inst_*.hip instantiate per curve.  The pipeline itself is
// described at the top of msm.hpp; the plan and every shape decision are in msm_shape.hpp (no HIP in there).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <algorithm>
#include "ec.hpp"
#include "msm_shape.hpp"

namespace vz {

#define VZ_HIP_CHECK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return _e; } while (0)

// Precomputed window tables of a commitment key: d[j][i] = 2^(c j) * P_i, affine internal form, row length n_total.
// own != 0: every window keeps its own bucket set, as without tables — the tables only spare the host the Horner over the window sums
// (the large-MSM default window, c = 11); own == 0: one bucket set shared by all windows (c = 13..16: fewer entries, deeper reduce).
struct BaseTables {
  const uint32_t* d; size_t n_total; size_t offset; int c, K; int own = 0;
  // fused small path only: every multiple of the table rows — mult[(w·n_total + i)·2^(c−1) + (m−1)] = m·2^(c·w)·P_i, m = 1..2^(c−1) —
  // so that a digit SELECTS its point: no buckets, no sort, the MSM is one sum (k_msm_fixed).  189 KB per base point at c = 7.
  const uint32_t* mult = nullptr;
};

// Row groups (msm_launch_rows): ONE chain of launches commits G vectors of the same length over the same key, the row in blockIdx.y.  Every
// workspace array then holds G slices; these are the distances between consecutive rows' slices, in 32-bit words (all zero: one row, as ever).
struct MsmRowStrides {
  size_t scalars = 0, block_hist = 0, sorted = 0, partial = 0, heavy_scratch = 0, out = 0;
  uint32_t counts = 0, offs = 0 /* bucket_off, sub_off */, totals = 0, heavy = 0, heavy_done = 0;
};
// One unit sum  Σ_{scalar_i = 1} P_i  of a grouped launch (ones_launch_rows): n scalars (Montgomery or not, as the call says) over bases; one XYZZ point to out
struct OnesDesc { const uint32_t* scalars; const uint32_t* bases; uint32_t* out; size_t n; };
struct OnesDescs { OnesDesc d[2 * MSM_ROWS_MAX]; };

struct MsmWorkspace {  // device buffers, grown on demand and reused across calls
  uint32_t* counts = nullptr;      // nb
  uint32_t* cursor = nullptr;      // nb
  uint32_t* bucket_off = nullptr;  // nb + 1
  uint32_t* sub_off = nullptr;     // nb + 1
  uint32_t* sorted = nullptr;      // K * n
  void* partial = nullptr;         // max_subs * sizeof(XYZZ)
  uint32_t* totals = nullptr;      // [0] = total subs
  uint32_t* block_hist = nullptr;  // [256][nb] per-workgroup histograms of the LDS counting sort
  size_t cap_block_hist = 0;
  void* ones_partial = nullptr;    // (16384 + 64) XYZZ partial sums of the unit-scalar path
  uint32_t* heavy = nullptr;       // [0] = count, then ids of buckets with many sub-buckets
  uint32_t* heavy_scratch = nullptr;   // 1024 x 32 partial sums of the split heavy buckets
  uint32_t* heavy_done = nullptr;      // 1024 tickets: the last of a split bucket's 32 workgroups folds its scratch row (k_combine); zero between launches
  uint32_t* plane_scratch = nullptr;   // 256 partial sums of k_reduce_planes
  size_t cap_nb = 0, cap_entries = 0, cap_subs = 0;
  size_t cap_rows = 1;             // row slices every array above holds (msm_launch_rows); the sizes named in the comments are per row
  void* host_pinned = nullptr;     // MSM_MAX_WINDOWS * 128 B
  static constexpr size_t HEAVY_SCRATCH_WORDS = (size_t)XYZZ_WORDS * MSM_HEAVY_SCRATCH_POINTS;

  // device bytes of one row's slices (what a group of G rows costs G times)
  static size_t row_bytes(uint32_t nb, size_t entries, size_t subs, size_t block_hist_words) {
    return 4 * (4 * (size_t)nb + 2 + entries + (size_t)XYZZ_WORDS * subs + block_hist_words + MSM_TOTALS_WORDS + MSM_HEAVY_CAP + 1 + HEAVY_SCRATCH_WORDS + MSM_HEAVY_DONE_WORDS);
  }
  hipError_t reserve(uint32_t nb, size_t entries, size_t subs, size_t rows = 1) {
    if (rows > cap_rows) {      // more row slices than ever: everything anew (the tickets among them, zeroed below)
      hipFree(counts); hipFree(cursor); hipFree(bucket_off); hipFree(sub_off); hipFree(sorted); hipFree(partial); hipFree(totals); hipFree(heavy); hipFree(heavy_scratch);
      hipFree(heavy_done); hipFree(block_hist);
      counts = cursor = bucket_off = sub_off = sorted = totals = heavy = heavy_scratch = heavy_done = block_hist = nullptr; partial = nullptr;
      cap_nb = cap_entries = cap_subs = cap_block_hist = 0;
      cap_rows = rows;
    }
    const size_t R = cap_rows;
    if (nb > cap_nb) {
      hipFree(counts); hipFree(cursor); hipFree(bucket_off); hipFree(sub_off);
      VZ_HIP_CHECK(hipMalloc(&counts, 4 * R * (size_t)nb)); VZ_HIP_CHECK(hipMalloc(&cursor, 4 * R * (size_t)nb));
      VZ_HIP_CHECK(hipMalloc(&bucket_off, 4 * R * ((size_t)nb + 1))); VZ_HIP_CHECK(hipMalloc(&sub_off, 4 * R * ((size_t)nb + 1)));
      cap_nb = nb;
    }
    if (entries > cap_entries) {
      hipFree(sorted); VZ_HIP_CHECK(hipMalloc(&sorted, 4 * R * entries)); cap_entries = entries;
    }
    if (subs > cap_subs) {
      hipFree(partial);
      VZ_HIP_CHECK(hipMalloc(&partial, 4 * XYZZ_WORDS * R * subs)); cap_subs = subs;
    }
    // (totals[2] is the ticket of k_prefix_scan: zero between launches.  hipMemset on device memory is a null-stream operation that may
    //  return before it has run and the MSM streams are non-blocking: synchronise)
    if (!totals) { VZ_HIP_CHECK(hipMalloc(&totals, 4 * R * MSM_TOTALS_WORDS)); VZ_HIP_CHECK(hipMemset(totals, 0, 4 * R * MSM_TOTALS_WORDS)); VZ_HIP_CHECK(hipStreamSynchronize(nullptr)); }
    if (!heavy) VZ_HIP_CHECK(hipMalloc(&heavy, 4 * R * (MSM_HEAVY_CAP + 1)));
    if (!heavy_scratch) VZ_HIP_CHECK(hipMalloc(&heavy_scratch, 4 * R * HEAVY_SCRATCH_WORDS));
    if (!heavy_done) { VZ_HIP_CHECK(hipMalloc(&heavy_done, 4 * R * MSM_HEAVY_DONE_WORDS)); VZ_HIP_CHECK(hipMemset(heavy_done, 0, 4 * R * MSM_HEAVY_DONE_WORDS)); VZ_HIP_CHECK(hipStreamSynchronize(nullptr)); }
    if (!plane_scratch) VZ_HIP_CHECK(hipMalloc(&plane_scratch, 4 * (size_t)XYZZ_WORDS * 256));
    if (!ones_partial) VZ_HIP_CHECK(hipMalloc(&ones_partial, 4 * (size_t)XYZZ_WORDS * (16384 + 64 + 512)));
    if (!host_pinned) VZ_HIP_CHECK(hipHostMalloc(&host_pinned, 4 * XYZZ_WORDS * MSM_MAX_WINDOWS));
    return hipSuccess;
  }
  void* small_buf = nullptr;       // fused small MSM: 128 completion counters, then MSM_MAX_WINDOWS x 16 chunks x 64 bucket sums
  hipError_t reserve_small() {
    if (!host_pinned) VZ_HIP_CHECK(hipHostMalloc(&host_pinned, 4 * XYZZ_WORDS * MSM_MAX_WINDOWS));
    // NOTE: hipMemset on device memory runs on the null stream and may return before it has executed; the MSM streams are
    // non-blocking, so every such fill is followed by a null-stream synchronise (a fill landing after the first kernel's
    // writes cost a day: it zeroed chunk results of the very first small MSM of a prover, only under heavy multi-stream load).
    if (!totals) { VZ_HIP_CHECK(hipMalloc(&totals, 4 * cap_rows * MSM_TOTALS_WORDS)); VZ_HIP_CHECK(hipMemset(totals, 0, 4 * cap_rows * MSM_TOTALS_WORDS)); VZ_HIP_CHECK(hipStreamSynchronize(nullptr)); }
    if (small_buf) return hipSuccess;
    const size_t bytes = 512 + 4 * (size_t)XYZZ_WORDS * MSM_MAX_WINDOWS * SMALL_MAXQ * (1u << (SMALL_C - 1));
    VZ_HIP_CHECK(hipMalloc(&small_buf, bytes));
    VZ_HIP_CHECK(hipMemset(small_buf, 0, 512));          // the completion counters (the chunk results are written before they are read)
    return hipStreamSynchronize(nullptr);
  }
  hipError_t reserve_block_hist(size_t words /* per row; after reserve() */) {
    if (words <= cap_block_hist) return hipSuccess;
    hipFree(block_hist); block_hist = nullptr; cap_block_hist = 0;
    VZ_HIP_CHECK(hipMalloc(&block_hist, 4 * cap_rows * words));
    cap_block_hist = words;
    return hipSuccess;
  }
  void release() {
    hipFree(counts); hipFree(cursor); hipFree(bucket_off); hipFree(sub_off); hipFree(sorted);
    hipFree(partial); hipFree(totals); hipFree(heavy); hipFree(heavy_scratch); hipFree(heavy_done); hipFree(plane_scratch); hipFree(small_buf); hipFree(ones_partial); hipFree(block_hist);
    if (host_pinned) hipHostFree(host_pinned);
    *this = MsmWorkspace();
  }
};

struct MsmStats { int c, K; uint32_t subs, entries; float ms[6]; };  // ms: hist, scan, scatter, accum, combine, reduce

// Defined in msm.hpp; explicitly instantiated per curve in msm_inst_*.hip.
template <class C>
hipError_t msm_launch(hipStream_t stream, MsmWorkspace& ws, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n,
                      int scalars_mont, int c_override, void* pinned_dst, MsmPlan* plan_out, hipEvent_t* ev, int split_ones,
                      const BaseTables* tb = nullptr);
// G vectors of n scalars each (row r at d_scalars + 8·r·scalar_row_stride) over the SAME bases, committed by one chain of launches: the kernels of
// msm_launch with the row in blockIdx.y and a slice of every workspace array per row; row r's sums go to pinned_dst + r·pinned_row_stride (bytes),
// the plan — one for all rows — to plan_out.  G = 1 issues msm_launch's launches.  Covers the LDS sort with a shared bucket set (tables, c = 13..16)
// or without tables, reduced by k_reduce; any other shape (fused small path, per-window tables, bit planes, the global-atomics sort) is issued
// by msm_launch row after row.  split_ones: the rows' unit sums — and `extra`, n_extra more unit sums of the caller's — by ones_launch_rows.
// max_rows: the largest G this workspace will see (its arrays are sized for it once: growing them synchronises the device).
template <class C>
hipError_t msm_launch_rows(hipStream_t stream, MsmWorkspace& ws, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n, size_t scalar_row_stride, uint32_t G,
                           int scalars_mont, void* pinned_dst, size_t pinned_row_stride, MsmPlan* plan_out, int split_ones, const BaseTables* tb,
                           const OnesDesc* extra = nullptr, uint32_t n_extra = 0, uint32_t max_rows = 0);
// device bytes one more row of such a group costs its workspace (0: this shape is issued row by row)
template <class C>
size_t msm_rows_row_bytes(size_t n, int split_ones, const BaseTables* tb);
// count (<= 2·MSM_ROWS_MAX) unit sums in two launches: every workgroup of the first folds its 256 partial sums, the second finishes each sum into its `out`
template <class C>
hipError_t ones_launch_rows(hipStream_t stream, MsmWorkspace& ws, const OnesDesc* descs, uint32_t count, int scalars_mont);
template <class C>
hipError_t build_tables(hipStream_t stream, const uint32_t* d_bases, size_t n, int c, int K, uint32_t* d_tables);
// d_mult[(w·n + i)·2^(c−1) + (m−1)] = m·d_tables[w][i] for m = 1..2^(c−1)  (n·K·2^(c−1) affine points)
template <class C>
hipError_t build_multiples(hipStream_t stream, const uint32_t* d_tables, size_t n, int c, int K, uint32_t* d_mult);
template <class C>
Affine<typename C::Base> msm_finish(const MsmPlan& pl, const void* pinned);
template <class C>
hipError_t msm_run(hipStream_t stream, MsmWorkspace& ws, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n,
                   int scalars_mont, int c_override, Affine<typename C::Base>* out_affine_mont, MsmStats* stats,
                   hipEvent_t* ev /* 7 events or nullptr */, int split_ones, const BaseTables* tb = nullptr);
// Σ_{scalar_i = 1} P_i alone: one XYZZ point (device form) at pinned_dst; ones_finish converts it
template <class C>
hipError_t ones_launch(hipStream_t stream, MsmWorkspace& ws, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n, int scalars_mont, void* pinned_dst);
template <class C>
XYZZ<typename C::Base> ones_finish(const void* pinned);

}  // namespace vz
