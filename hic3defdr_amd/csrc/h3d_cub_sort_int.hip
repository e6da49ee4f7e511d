// libh3d.so's hipcub instantiations, the other radix sorts of integer keys
// (h3d_cub.h: the h3d_cub_*.hip units alone include hipcub, so no other unit
// compiles rocprim's kernels).
#include <hipcub/hipcub.hpp>

#include "h3d_cub.h"

namespace h3dint {

#define H3D_SORT_PAIRS(K, V)                                                            \
  hipError_t sort_pairs(void* tmp, size_t& bytes, const K* keys_in, K* keys_out,        \
                        const V* vals_in, V* vals_out, int n, int begin_bit,            \
                        int end_bit, hipStream_t s) {                                   \
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in,   \
                                              vals_out, n, begin_bit, end_bit, s);      \
  }

H3D_SORT_PAIRS(int32_t, int32_t)
H3D_SORT_PAIRS(int64_t, int32_t)
H3D_SORT_PAIRS(uint64_t, uint8_t)

hipError_t sort_keys(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                     int n, int begin_bit, int end_bit, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys_in, keys_out, n, begin_bit, end_bit,
                                           s);
}

}  // namespace h3dint
