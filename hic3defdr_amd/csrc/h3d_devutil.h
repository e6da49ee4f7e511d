// Device helpers shared by the diagnostics and evaluation kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace h3dint {

// order-preserving key of a double, ascending (-0.0 and +0.0 one value), and
// its inverse
__device__ inline uint64_t asc_key(double x) {
  const uint64_t b = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ inline double asc_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

}  // namespace h3dint
