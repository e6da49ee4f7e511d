// libh3d.so's hipcub instantiations, the scans, the reduction and the select
// (h3d_cub.h: these units alone include hipcub, so no other unit compiles
// rocprim's kernels).
#include <hipcub/hipcub.hpp>

#include "h3d_cub.h"

namespace {

// (min is exact: any association of the scan gives the same bits)
struct MinOp {
  __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};

}  // namespace

namespace h3dint {

hipError_t inclusive_sum(void* tmp, size_t& bytes, int32_t* in, int32_t* out, int n,
                         hipStream_t s) {
  return hipcub::DeviceScan::InclusiveSum(tmp, bytes, in, out, n, s);
}

hipError_t inclusive_sum(void* tmp, size_t& bytes, int64_t* in, int64_t* out, int n,
                         hipStream_t s) {
  return hipcub::DeviceScan::InclusiveSum(tmp, bytes, in, out, n, s);
}

hipError_t exclusive_sum(void* tmp, size_t& bytes, int32_t* in, int32_t* out, int n,
                         hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, n, s);
}

hipError_t exclusive_sum(void* tmp, size_t& bytes, const int32_t* in, int32_t* out, int n,
                         hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, n, s);
}

hipError_t inclusive_min(void* tmp, size_t& bytes, double* in, double* out, int n,
                         hipStream_t s) {
  return hipcub::DeviceScan::InclusiveScan(tmp, bytes, in, out, MinOp(), n, s);
}

hipError_t reduce_sum(void* tmp, size_t& bytes, int32_t* in, int32_t* out, int n,
                      hipStream_t s) {
  return hipcub::DeviceReduce::Sum(tmp, bytes, in, out, n, s);
}

hipError_t select_flagged_indices(void* tmp, size_t& bytes, const uint8_t* flags, int32_t* out,
                                  int32_t* n_selected, int n, hipStream_t s) {
  hipcub::CountingInputIterator<int32_t> it(0);
  return hipcub::DeviceSelect::Flagged(tmp, bytes, it, flags, out, n_selected, n, s);
}

}  // namespace h3dint
