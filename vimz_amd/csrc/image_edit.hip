// Image editor: pyvimz's image-editor transformations (pyvimz/pyvimz/img/transformations.py) on the device, bit for bit as
// vimz_amd/image_editor.py restates them, with the packing of the prover's input (build_input's "original" / "transformed") fused in.
//
// One launch per descriptor, k_image_edit<OP>, on the context's stream, so a descriptor whose source is an earlier one's edited image reads it
// after it is written.  A thread owns one packed element: 10 consecutive pixels of a row.  Threads [0, n_tgt) compute the 10 edited pixels of
// their element, store them and, when wanted, their packed element; threads [n_tgt, n_tgt + n_src) pack 10 source pixels (the zero rows of
// blur / sharpness included).  Redact's 40 x 40 blocks are 4 elements wide, so the row-wise thread layout writes the block layout directly
// (ed_elem_index).  The call is transfer-bound: the kernels read and write each byte a few times through L1 / L2, the PCIe copies move
// every byte once.
//
// Float64: numpy rounds after every ufunc, so (c - 128.0) * f + 128.0 and resize's A*wt + B*wt + ... are evaluated one rounded operation at
// a time.  hipcc would contract a*b + c into one FMA (one rounding), which changes the truncated byte for some (factor, pixel) pairs
// (f = 0.55, c = 8: numpy 62, an FMA 61).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "internal.hpp"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t ED_THREADS = 256;
constexpr uint32_t ED_BLOCK = 40;        // redact's block side (compress_by_blocks)
constexpr size_t ED_MAX_DESCS = VIMZ_EDIT_MAX_DESCS;

struct EdJob {
  const uint8_t* src;      // source pixels (h x w x ch)
  uint8_t* dst;            // edited pixels (oh x ow x och)
  uint32_t* tgt;           // packed edited image, or nullptr
  uint32_t* spk;           // packed source, or nullptr
  const uint8_t* flags;    // redact: one flag per full block, or nullptr (checkerboard)
  double factor, xr, yr;   // brightness / contrast; resize's w / new_w and h / new_h
  uint32_t h, w, ch, oh, ow, och;
  uint32_t x, y;           // crop
  uint32_t pad;            // zero rows above and below the packed source (blur, sharpness)
  uint32_t blocks;         // packed as 40 x 40 blocks (redact: h, w multiples of 40)
  uint32_t n_tgt, n_src;   // threads of the two parts
  uint32_t h720;           // resize: the source is 720 rows high (HD -> SD weights)
};

// where element j of row `row` goes: row-major, or in its 40 x 40 block (4 elements per block row, blocks row-major)
__host__ __device__ __forceinline__ size_t ed_elem_index(uint32_t row, uint32_t j, uint32_t per, uint32_t blocks) {
  if (!blocks) return (size_t)row * per + j;
  const uint32_t bw = per / 4;
  return ((size_t)(row / ED_BLOCK) * bw + j / 4) * (ED_BLOCK * 4) + (row % ED_BLOCK) * 4 + (j % 4);
}

__host__ __device__ __forceinline__ uint32_t ed_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ uint32_t ed_px(const EdJob& J, uint32_t r, uint32_t c, uint32_t k) {
  return J.src[((size_t)r * J.w + c) * J.ch + k];
}
// a neighbour of the 3 x 3 stencils: zero outside the image
__host__ __device__ __forceinline__ int ed_nb(const EdJob& J, int r, int c, uint32_t k) {
  return r < 0 || c < 0 || r >= (int)J.h || c >= (int)J.w ? 0 : (int)ed_px(J, (uint32_t)r, (uint32_t)c, k);
}
__host__ __device__ __forceinline__ uint32_t ed_trunc(double d) {       // np.clip(d, 0, 255).astype(np.uint8) of a finite d
  d = d < 0.0 ? 0.0 : d;
  d = d > 255.0 ? 255.0 : d;
  return (uint32_t)d;
}

// channel k of edited pixel (row, col)
template <int OP>
__host__ __device__ __forceinline__ uint32_t ed_value(const EdJob& J, uint32_t row, uint32_t col, uint32_t k) {
  if constexpr (OP == VIMZ_EDIT_HASH) {
    return ed_px(J, row, col, k);
  } else if constexpr (OP == VIMZ_EDIT_GRAYSCALE) {
    return (19595u * ed_px(J, row, col, 0) + 38470u * ed_px(J, row, col, 1) + 7471u * ed_px(J, row, col, 2) + 32768u) >> 16;
  } else if constexpr (OP == VIMZ_EDIT_BRIGHTNESS) {
    const double p = (double)ed_px(J, row, col, k) * J.factor;
    return ed_trunc(p);
  } else if constexpr (OP == VIMZ_EDIT_CONTRAST) {
    const double d = (double)ed_px(J, row, col, k) - 128.0;
    const double p = d * J.factor;
    const double t = p + 128.0;
    return ed_trunc(t);
  } else if constexpr (OP == VIMZ_EDIT_BLUR) {
    int s = 0;
    for (int dr = -1; dr <= 1; dr++)
      for (int dc = -1; dc <= 1; dc++) s += ed_nb(J, (int)row + dr, (int)col + dc, k);
    return (uint32_t)(s / 9);
  } else if constexpr (OP == VIMZ_EDIT_SHARPNESS) {
    const int r = (int)row, c = (int)col;
    const int s = 5 * ed_nb(J, r, c, k) - ed_nb(J, r - 1, c, k) - ed_nb(J, r + 1, c, k) - ed_nb(J, r, c - 1, k) - ed_nb(J, r, c + 1, k);
    return (uint32_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
  } else if constexpr (OP == VIMZ_EDIT_RESIZE) {
    const uint32_t yl = (uint32_t)((double)row * J.yr), xl = (uint32_t)((double)col * J.xr);
    const double wt = J.h720 ? ((row & 1) ? 1.0 / 3 : 2.0 / 3) : 0.5;
    const double wb = 1.0 - wt;
    const double A = ed_px(J, yl, xl, k), B = ed_px(J, yl, xl + 1, k), C = ed_px(J, yl + 1, xl, k), D = ed_px(J, yl + 1, xl + 1, k);
    const double a = A * wt, b = B * wt, cc = C * wb, dd = D * wb;
    double s = a + b;
    s = s + cc;
    s = s + dd;
    return (uint32_t)(s / 2);
  } else if constexpr (OP == VIMZ_EDIT_CROP) {
    return ed_px(J, J.y + row, J.x + col, k);
  } else {      // VIMZ_EDIT_REDACT
    const uint32_t by = row / ED_BLOCK, bx = col / ED_BLOCK, nby = J.h / ED_BLOCK, nbx = J.w / ED_BLOCK;
    const bool red = by < nby && bx < nbx && (J.flags ? J.flags[(size_t)by * nbx + bx] != 0 : ((by + bx) & 1) != 0);
    return red ? 0u : ed_px(J, row, col, k);
  }
}

__host__ __device__ __forceinline__ void ed_put(uint32_t (&w8)[8], uint32_t byte, uint32_t v) { w8[byte >> 2] |= v << (8 * (byte & 3)); }
__host__ __device__ __forceinline__ void ed_store_element(uint32_t* out, size_t idx, const uint32_t (&w8)[8]) {
  uint4* o = reinterpret_cast<uint4*>(out + 8 * idx);
  o[0] = make_uint4(w8[0], w8[1], w8[2], w8[3]);
  o[1] = make_uint4(w8[4], w8[5], w8[6], w8[7]);
}

// thread t of a descriptor's launch (also compiled for the host: tests/test_image_edit_host.py steps it on the CPU against numpy)
template <int OP>
__host__ __device__ __forceinline__ void ed_thread(const EdJob& J, uint32_t t) {
  uint32_t w8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t < J.n_tgt) {
    const uint32_t per = (J.ow + 9) / 10, row = t / per, j = t % per, col0 = 10 * j, np = ed_min(10u, J.ow - col0);
    uint8_t* d = J.dst + ((size_t)row * J.ow + col0) * J.och;
#pragma unroll
    for (uint32_t p = 0; p < 10; p++) {
      if (p < np) {
        if (J.och == 1) {
          const uint32_t v = ed_value<OP>(J, row, col0 + p, 0);
          d[p] = (uint8_t)v;
          ed_put(w8, 3 * p, v);
        } else {
#pragma unroll
          for (uint32_t k = 0; k < 3; k++) {
            const uint32_t v = ed_value<OP>(J, row, col0 + p, k);
            d[3 * p + k] = (uint8_t)v;
            ed_put(w8, 3 * p + k, v);
          }
        }
      }
    }
    if (J.tgt) ed_store_element(J.tgt, ed_elem_index(row, j, per, J.blocks), w8);
  } else if (t - J.n_tgt < J.n_src) {
    const uint32_t s = t - J.n_tgt, per = (J.w + 9) / 10, prow = s / per, j = s % per, col0 = 10 * j, np = ed_min(10u, J.w - col0);
    const uint32_t nc = J.ch < 3 ? J.ch : 3;
    const bool live = prow >= J.pad && prow - J.pad < J.h;
    if (live) {
      const uint32_t row = prow - J.pad;
#pragma unroll
      for (uint32_t p = 0; p < 10; p++)
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
          if (p < np && k < nc) ed_put(w8, 3 * p + k, ed_px(J, row, col0 + p, k));
    }
    ed_store_element(J.spk, J.blocks ? ed_elem_index(prow, j, per, 1) : (size_t)s, w8);
  }
}

template <int OP>
__global__ void __launch_bounds__(ED_THREADS) k_image_edit(EdJob J) {
  ed_thread<OP>(J, blockIdx.x * ED_THREADS + threadIdx.x);
}

// what a descriptor resolves to: its source (host pixels or an earlier edit), its edited image and its packed shapes
struct EdPlan {
  uint32_t h, w, ch, oh, ow, och, pad, blocks;
  size_t su, sl, tu, tl;
  double xr, yr;
};

inline size_t ed_align(size_t x) { return (x + 255) & ~(size_t)255; }

bool ed_needs_rgb(int op) { return op != VIMZ_EDIT_HASH && op != VIMZ_EDIT_CROP && op != VIMZ_EDIT_REDACT; }

int ed_plan(vimz_ctx* c, const vimz_edit_desc* descs, size_t n, std::vector<EdPlan>& plans) {
  if (!descs || n == 0 || n > ED_MAX_DESCS) return vz::vz_fail(c, VIMZ_ERR_INVALID, "vimz_image_edit: bad argument (1 to 4096 descriptors)");
  plans.assign(n, EdPlan{});
  for (size_t i = 0; i < n; i++) {
    const vimz_edit_desc& D = descs[i];
    EdPlan& P = plans[i];
    auto bad = [&](const char* why) { return vz::vz_fail(c, VIMZ_ERR_INVALID, ("vimz_image_edit: edit " + std::to_string(i) + ": " + why).c_str()); };
    if (D.op < VIMZ_EDIT_HASH || D.op > VIMZ_EDIT_REDACT) return bad("unknown op");
    if (D.pixels) {
      if (!D.height || !D.width || D.height > (1ull << 20) || D.width > (1ull << 20) || D.height * D.width > (1ull << 30))
        return bad("bad source size (1 to 2^20 per dimension, at most 2^30 pixels)");
      if (D.channels != 1 && D.channels != 3 && D.channels != 4) return bad("source channels must be 1, 3 or 4");
      P.h = (uint32_t)D.height; P.w = (uint32_t)D.width; P.ch = (uint32_t)D.channels;
    } else {
      if (D.source < 0 || (uint64_t)D.source >= i) return bad("the source is neither host pixels nor an earlier edit of the call");
      const EdPlan& S = plans[(size_t)D.source];
      P.h = S.oh; P.w = S.ow; P.ch = S.och;
    }
    if (ed_needs_rgb(D.op) && P.ch == 1) return bad("this op needs an RGB source, the source is grey");
    P.oh = P.h; P.ow = P.w;
    P.och = D.op == VIMZ_EDIT_GRAYSCALE || P.ch == 1 ? 1 : 3;
    P.pad = D.op == VIMZ_EDIT_BLUR || D.op == VIMZ_EDIT_SHARPNESS ? 1 : 0;
    P.blocks = D.op == VIMZ_EDIT_REDACT ? 1 : 0;
    if ((D.op == VIMZ_EDIT_BRIGHTNESS || D.op == VIMZ_EDIT_CONTRAST) && !std::isfinite(D.factor)) return bad("factor is not finite");
    if (D.op == VIMZ_EDIT_CROP) {
      if (!D.new_width || !D.new_height || D.x > P.w || D.new_width > P.w - D.x || D.y > P.h || D.new_height > P.h - D.y)
        return bad("the crop window is empty or not inside the image");
      P.ow = (uint32_t)D.new_width; P.oh = (uint32_t)D.new_height;
    }
    if (D.op == VIMZ_EDIT_RESIZE) {
      if (!D.new_width || !D.new_height || D.new_width > (1ull << 20) || D.new_height > (1ull << 20) || D.new_width * D.new_height > (1ull << 30))
        return bad("bad resize target (1 to 2^20 per dimension, at most 2^30 pixels)");
      // the last output row / column reads source row yl + 1 / column xl + 1 (the indices grow with the output's): numpy raises an IndexError
      // where that is outside the image
      P.xr = (double)P.w / (double)D.new_width; P.yr = (double)P.h / (double)D.new_height;
      const double yl = (double)(D.new_height - 1) * P.yr, xl = (double)(D.new_width - 1) * P.xr;
      if ((size_t)yl + 1 >= P.h || (size_t)xl + 1 >= P.w) return bad("resize reads past the source's last row or column (xl + 1 or yl + 1 outside the image)");
      P.ow = (uint32_t)D.new_width; P.oh = (uint32_t)D.new_height;
    }
    const size_t nby = P.h / ED_BLOCK, nbx = P.w / ED_BLOCK;
    // NULL flags with n_redact = 0 ask for the checkerboard; any other count must be the block count, an empty list included (a caller's
    // zero flags are not "no flags": they must not turn into blocks the caller did not ask for)
    if (D.op == VIMZ_EDIT_REDACT && !D.redact && D.n_redact) return bad("redact: n_redact flags given, but the flag array is NULL");
    if (D.op == VIMZ_EDIT_REDACT && D.redact && D.n_redact != nby * nbx) return bad("redact needs one flag per full 40 x 40 block");
    if (P.blocks) {
      const bool whole = P.h % ED_BLOCK == 0 && P.w % ED_BLOCK == 0;
      P.su = P.tu = whole ? nby * nbx : 0;
      P.sl = P.tl = ED_BLOCK * ED_BLOCK / 10;
      if (!whole && (D.out_source || D.out_target)) return bad("redact packs 40 x 40 blocks: height and width must be multiples of 40");
    } else {
      P.su = P.h + 2 * P.pad; P.sl = (P.w + 9) / 10;
      P.tu = D.op == VIMZ_EDIT_HASH ? 0 : P.oh; P.tl = D.op == VIMZ_EDIT_HASH ? 0 : (P.ow + 9) / 10;
      if (D.op == VIMZ_EDIT_HASH && D.out_target) return bad("hash has no edited image to pack (out_target must be NULL)");
    }
  }
  return VIMZ_OK;
}

// the launch parameters of a planned descriptor over its buffers (spk / tgt nullptr: not wanted)
EdJob ed_job(const vimz_edit_desc& D, const EdPlan& P, const uint8_t* src, uint8_t* dst, uint32_t* spk, uint32_t* tgt, const uint8_t* flags) {
  EdJob J{};
  J.src = src; J.dst = dst; J.tgt = tgt; J.spk = spk; J.flags = flags;
  J.factor = D.factor; J.xr = P.xr; J.yr = P.yr;
  J.h = P.h; J.w = P.w; J.ch = P.ch; J.oh = P.oh; J.ow = P.ow; J.och = P.och;
  J.x = (uint32_t)D.x; J.y = (uint32_t)D.y;
  J.pad = P.pad; J.blocks = P.blocks; J.h720 = P.h == 720;
  J.n_tgt = P.oh * ((P.ow + 9) / 10);
  J.n_src = spk ? (uint32_t)(P.su * P.sl) : 0;
  return J;
}

template <int OP>
void ed_launch(const EdJob& J, hipStream_t s) {
  const uint32_t threads = J.n_tgt + J.n_src;
  hipLaunchKernelGGL(k_image_edit<OP>, dim3((threads + ED_THREADS - 1) / ED_THREADS), dim3(ED_THREADS), 0, s, J);
}
void ed_launch_op(int op, const EdJob& J, hipStream_t s) {
  switch (op) {
    case VIMZ_EDIT_HASH: ed_launch<VIMZ_EDIT_HASH>(J, s); break;
    case VIMZ_EDIT_GRAYSCALE: ed_launch<VIMZ_EDIT_GRAYSCALE>(J, s); break;
    case VIMZ_EDIT_BRIGHTNESS: ed_launch<VIMZ_EDIT_BRIGHTNESS>(J, s); break;
    case VIMZ_EDIT_CONTRAST: ed_launch<VIMZ_EDIT_CONTRAST>(J, s); break;
    case VIMZ_EDIT_BLUR: ed_launch<VIMZ_EDIT_BLUR>(J, s); break;
    case VIMZ_EDIT_SHARPNESS: ed_launch<VIMZ_EDIT_SHARPNESS>(J, s); break;
    case VIMZ_EDIT_RESIZE: ed_launch<VIMZ_EDIT_RESIZE>(J, s); break;
    case VIMZ_EDIT_CROP: ed_launch<VIMZ_EDIT_CROP>(J, s); break;
    default: ed_launch<VIMZ_EDIT_REDACT>(J, s); break;
  }
}

}  // namespace

static int fail(vimz_ctx* c, int code, const char* what, hipError_t e = hipSuccess) { return vz::vz_fail(c, code, what, e); }

extern "C" int vimz_image_edit_shapes(vimz_ctx* c, const vimz_edit_desc* descs, size_t n, vimz_edit_shape* out) {
  if (!c) return VIMZ_ERR_INVALID;
  if (!out) return fail(c, VIMZ_ERR_INVALID, "vimz_image_edit_shapes: out is NULL");
  std::vector<EdPlan> plans;
  const int rc = ed_plan(c, descs, n, plans);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) {
    const EdPlan& P = plans[i];
    out[i] = vimz_edit_shape{P.oh, P.ow, (int)P.och, P.su, P.sl, P.tu, P.tl};
  }
  return VIMZ_OK;
}

extern "C" int vimz_image_edit(vimz_ctx* c, const vimz_edit_desc* descs, size_t n) {
  if (!c) return VIMZ_ERR_INVALID;
  std::vector<EdPlan> plans;
  int rc = ed_plan(c, descs, n, plans);
  if (rc) return rc;
  // the call's device buffer: per descriptor its uploaded source (host pixels), its redact flags, its edited pixels and the packed outputs
  std::vector<size_t> o_in(n), o_flags(n), o_dst(n), o_spk(n), o_tgt(n);
  std::vector<size_t> in_bytes(n), dst_bytes(n), spk_bytes(n), tgt_bytes(n);
  size_t off = 0;
  for (size_t i = 0; i < n; i++) {
    const vimz_edit_desc& D = descs[i];
    const EdPlan& P = plans[i];
    in_bytes[i] = D.pixels ? (size_t)P.h * P.w * P.ch : 0;
    dst_bytes[i] = (size_t)P.oh * P.ow * P.och;
    spk_bytes[i] = D.out_source ? 32 * P.su * P.sl : 0;
    tgt_bytes[i] = D.out_target ? 32 * P.tu * P.tl : 0;
    o_in[i] = off; off += ed_align(in_bytes[i]);
    o_flags[i] = off; off += ed_align(D.op == VIMZ_EDIT_REDACT && D.redact ? D.n_redact : 0);
    o_dst[i] = off; off += ed_align(dst_bytes[i]);
    o_spk[i] = off; off += ed_align(spk_bytes[i]);
    o_tgt[i] = off; off += ed_align(tgt_bytes[i]);
  }
  typedef std::chrono::steady_clock clk;
  std::lock_guard<std::mutex> g(c->mu);
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(c, VIMZ_ERR_HIP, "vimz_image_edit: hipSetDevice", e);
  // one device buffer per context, grown geometrically; the one it replaces is retired, not freed (a hipFree waits for the whole device,
  // for the folds of other contexts on it)
  if (off > c->image_edit_bytes) {
    const size_t want = std::max(off, 2 * c->image_edit_bytes);
    void* nb = nullptr;
    if ((e = hipMalloc(&nb, want)) != hipSuccess) return fail(c, VIMZ_ERR_HIP, "vimz_image_edit: device buffer", e);
    if (c->image_edit_buf) c->image_edit_retired.push_back(c->image_edit_buf);
    c->image_edit_buf = nb; c->image_edit_bytes = want;
  }
  uint8_t* buf = (uint8_t*)c->image_edit_buf;
  const char* what = nullptr;
  auto copy = [&](void* dst, const void* src, size_t nb, hipMemcpyKind kind, const char* w) {
    if (!what && nb && (e = hipMemcpyAsync(dst, src, nb, kind, c->stream)) != hipSuccess) what = w;
  };
  auto sync = [&](const char* w) {
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (!what && es != hipSuccess) { what = w; e = es; }
  };
  const clk::time_point t0 = clk::now();
  for (size_t i = 0; i < n; i++) {
    const vimz_edit_desc& D = descs[i];
    copy(buf + o_in[i], D.pixels, in_bytes[i], hipMemcpyHostToDevice, "vimz_image_edit: upload");
    if (D.op == VIMZ_EDIT_REDACT && D.redact) copy(buf + o_flags[i], D.redact, D.n_redact, hipMemcpyHostToDevice, "vimz_image_edit: upload");
  }
  sync("vimz_image_edit: upload");
  const clk::time_point t1 = clk::now();
  for (size_t i = 0; i < n && !what; i++) {
    const vimz_edit_desc& D = descs[i];
    const EdPlan& P = plans[i];
    const EdJob J = ed_job(D, P, D.pixels ? buf + o_in[i] : buf + o_dst[(size_t)D.source], buf + o_dst[i],
                           D.out_source ? (uint32_t*)(buf + o_spk[i]) : nullptr, D.out_target ? (uint32_t*)(buf + o_tgt[i]) : nullptr,
                           D.op == VIMZ_EDIT_REDACT && D.redact ? buf + o_flags[i] : nullptr);
    ed_launch_op(D.op, J, c->stream);
    if ((e = hipGetLastError()) != hipSuccess) what = "vimz_image_edit: k_image_edit";
  }
  sync("vimz_image_edit: k_image_edit");
  const clk::time_point t2 = clk::now();
  for (size_t i = 0; i < n; i++) {
    const vimz_edit_desc& D = descs[i];
    if (D.out_pixels) copy(D.out_pixels, buf + o_dst[i], dst_bytes[i], hipMemcpyDeviceToHost, "vimz_image_edit: download");
    if (D.out_source) copy(D.out_source, buf + o_spk[i], spk_bytes[i], hipMemcpyDeviceToHost, "vimz_image_edit: download");
    if (D.out_target) copy(D.out_target, buf + o_tgt[i], tgt_bytes[i], hipMemcpyDeviceToHost, "vimz_image_edit: download");
  }
  sync("vimz_image_edit: download");
  const clk::time_point t3 = clk::now();
  if (what) return fail(c, VIMZ_ERR_HIP, what, e);
  c->image_edit_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
  c->image_edit_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  c->image_edit_ms[2] = std::chrono::duration<double, std::milli>(t3 - t2).count();
  return VIMZ_OK;
}

extern "C" int vimz_image_edit_last_profile(vimz_ctx* c, double ms[3]) {
  if (!c || !ms) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < 3; i++) ms[i] = c->image_edit_ms[i];
  return VIMZ_OK;
}
