// image_edit.hip's per-thread code on the CPU: ed_plan and ed_thread compiled for the host and run thread by thread over host buffers, so
// tests/test_image_edit_host.py can check the kernels' logic (edits, fused packing, chains, refusals) against numpy without a GPU.
// Built by vimz_amd/csrc/Makefile (target `all`) into build/libimage_edit_host.so.  The same two entry points as the product's
// vimz_image_edit_shapes / vimz_image_edit, without a context.
#include <cstdio>
#include <cstring>
#include <string>

#include <hip/hip_runtime.h>

struct vimz_ctx;
namespace vz {
static std::string g_host_err;
int vz_fail(vimz_ctx*, int code, const char* what, hipError_t) { g_host_err = what; return code; }
}  // namespace vz

#include "image_edit.hip"

namespace {
template <int OP>
void ed_host_run(const EdJob& J) {
  for (uint32_t t = 0; t < J.n_tgt + J.n_src; t++) ed_thread<OP>(J, t);
}
}  // namespace

extern "C" const char* edit_host_last_error(void) { return vz::g_host_err.c_str(); }

extern "C" int edit_host_shapes(const vimz_edit_desc* descs, size_t n, vimz_edit_shape* out) {
  std::vector<EdPlan> plans;
  const int rc = ed_plan(nullptr, descs, n, plans);
  if (rc) return rc;
  for (size_t i = 0; i < n; i++) {
    const EdPlan& P = plans[i];
    out[i] = vimz_edit_shape{P.oh, P.ow, (int)P.och, P.su, P.sl, P.tu, P.tl};
  }
  return VIMZ_OK;
}

extern "C" int edit_host_run(const vimz_edit_desc* descs, size_t n) {
  std::vector<EdPlan> plans;
  const int rc = ed_plan(nullptr, descs, n, plans);
  if (rc) return rc;
  std::vector<std::vector<uint8_t>> dst(n);
  for (size_t i = 0; i < n; i++) {
    const vimz_edit_desc& D = descs[i];
    const EdPlan& P = plans[i];
    dst[i].resize((size_t)P.oh * P.ow * P.och);
    const EdJob J = ed_job(D, P, D.pixels ? D.pixels : dst[(size_t)D.source].data(), dst[i].data(), (uint32_t*)D.out_source,
                           (uint32_t*)D.out_target, D.op == VIMZ_EDIT_REDACT ? D.redact : nullptr);
    switch (D.op) {
      case VIMZ_EDIT_HASH: ed_host_run<VIMZ_EDIT_HASH>(J); break;
      case VIMZ_EDIT_GRAYSCALE: ed_host_run<VIMZ_EDIT_GRAYSCALE>(J); break;
      case VIMZ_EDIT_BRIGHTNESS: ed_host_run<VIMZ_EDIT_BRIGHTNESS>(J); break;
      case VIMZ_EDIT_CONTRAST: ed_host_run<VIMZ_EDIT_CONTRAST>(J); break;
      case VIMZ_EDIT_BLUR: ed_host_run<VIMZ_EDIT_BLUR>(J); break;
      case VIMZ_EDIT_SHARPNESS: ed_host_run<VIMZ_EDIT_SHARPNESS>(J); break;
      case VIMZ_EDIT_RESIZE: ed_host_run<VIMZ_EDIT_RESIZE>(J); break;
      case VIMZ_EDIT_CROP: ed_host_run<VIMZ_EDIT_CROP>(J); break;
      default: ed_host_run<VIMZ_EDIT_REDACT>(J); break;
    }
    if (D.out_pixels) std::memcpy(D.out_pixels, dst[i].data(), dst[i].size());
  }
  return VIMZ_OK;
}
