// Error plumbing shared by the host translation units of libcessec (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/cess_ec.h"

namespace cec {

// Records `msg` as the calling thread's cec_last_error and returns `code` (cess_ec.cpp).
int set_error(int code, const std::string& msg);

// The error of the launches issued since the last check, as a return code.
inline int check_launch(const char* what = "kernel launch") {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(CEC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return CEC_OK;
}

}  // namespace cec

#define CEC_HIP_TRY(expr)                                                                  \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return cec::set_error(_e == hipErrorOutOfMemory ? CEC_ENOMEM : CEC_EHIP,             \
                            std::string(#expr) + ": " + hipGetErrorString(_e));            \
  } while (0)
