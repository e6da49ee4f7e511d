// libh3d.so's hipcub instantiations, the radix sorts of unsigned keys with
// int32 index values: estimate_disp's prep, group sums, rank average
// (h3d_cub.h: the h3d_cub_*.hip units alone include hipcub, so no other unit
// compiles rocprim's kernels). The two stay in one unit, as they were in
// h3d_api.hip: the compiler's register allocation of one rocprim kernel
// (the u64 block sort) depends on what else its module holds.
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

H3D_SORT_PAIRS(uint32_t, int32_t)
H3D_SORT_PAIRS(uint64_t, int32_t)

}  // namespace h3dint
