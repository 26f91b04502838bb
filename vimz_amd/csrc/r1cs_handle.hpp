// The handle behind vimz_r1cs (include/vimz_hip.h): a caller-supplied R1CS shape resident on the device, as r1cs_capi.hip uploads it.
#pragma once
#include <vector>
#include "r1cs_ops.hpp"

struct vimz_r1cs {
  int field = 0;
  size_t nrows = 0, ncols = 0, nnz[3] = {0, 0, 0};
  vz::CsrDev M[3] = {};
  uint32_t* dict = nullptr; size_t ndict = 0;
  uint32_t* long_items = nullptr; uint32_t n_long = 0, n_med = 0;
  uint32_t* scratch = nullptr;          // 6 x nrows elements: (A,B,C)·z1 and (A,B,C)·z2 of commit_T
  std::vector<void*> owned;
};
