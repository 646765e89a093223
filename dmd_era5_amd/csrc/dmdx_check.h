// The argument-check basics of libdmdx.so, free of HIP: dmdx_common.h includes this, and so can a host-only program.
#pragma once

#include <stdint.h>

#include "../../include/dmdx.h"

void dmdx_set_error(const char* fmt, ...);

#define DMDX_CHECK_ARG(cond, ...)        \
  do {                                   \
    if (!(cond)) {                       \
      dmdx_set_error(__VA_ARGS__);       \
      return DMDX_E_INVALID;             \
    }                                    \
  } while (0)

constexpr int64_t kMaxSize = int64_t(1) << 31;   // every size and leading dimension of a streaming kernel is below
constexpr unsigned kQuietNaN = 0x7FC00000u;      // the bits of the NaN a kernel writes for "no value"
