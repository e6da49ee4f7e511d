// The hipcub operations libh3d.so uses, as plain functions: one per
// (operation, argument types) that some unit calls, defined in the
// h3d_cub_*.hip units -- the only sources that include hipcub / rocprim, so
// each of rocprim's kernels is compiled once (a radix sort instantiation is
// ~220 of them) and not again by every unit that sorts or scans.
//
// Each keeps hipcub's two-phase shape: tmp = nullptr only reports the temp
// size in `bytes`; callers go through cub_call / cub_bytes (h3d_ctx.h). The
// argument types are those of the call sites, const included: rocprim's
// kernels are instantiated on the iterator types, so a `const int32_t*`
// input is another set of kernels than an `int32_t*` one.
//
// A new (operation, types) is a new declaration here and a definition in the
// unit of its kind. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace h3dint {

// DeviceRadixSort::SortPairs / SortKeys: stable, ascending, over the key bits
// [begin_bit, end_bit)
// ---- h3d_cub_sort_idx.hip: unsigned keys, int32 index values --------------
hipError_t sort_pairs(void* tmp, size_t& bytes, const uint32_t* keys_in, uint32_t* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);
hipError_t sort_pairs(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);

// ---- h3d_cub_sort_int.hip: the other integer keys -------------------------
hipError_t sort_pairs(void* tmp, size_t& bytes, const int32_t* keys_in, int32_t* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);
hipError_t sort_pairs(void* tmp, size_t& bytes, const int64_t* keys_in, int64_t* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);
hipError_t sort_pairs(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                      const uint8_t* vals_in, uint8_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);
hipError_t sort_keys(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                     int n, int begin_bit, int end_bit, hipStream_t s);

// ---- h3d_cub_sort_f64.hip: double keys ------------------------------------
hipError_t sort_pairs(void* tmp, size_t& bytes, const double* keys_in, double* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);
hipError_t sort_pairs(void* tmp, size_t& bytes, const double* keys_in, double* keys_out,
                      const int64_t* vals_in, int64_t* vals_out, int n, int begin_bit,
                      int end_bit, hipStream_t s);
// DeviceSegmentedRadixSort::SortKeys: segment k is [seg_begin[k], seg_end[k])
hipError_t segmented_sort_keys(void* tmp, size_t& bytes, const double* keys_in,
                               double* keys_out, int n, int n_segments, int64_t* seg_begin,
                               int64_t* seg_end, int begin_bit, int end_bit, hipStream_t s);

// ---- h3d_cub_scan.hip: DeviceScan, DeviceReduce, DeviceSelect -------------
hipError_t inclusive_sum(void* tmp, size_t& bytes, int32_t* in, int32_t* out, int n,
                         hipStream_t s);
hipError_t inclusive_sum(void* tmp, size_t& bytes, int64_t* in, int64_t* out, int n,
                         hipStream_t s);
hipError_t exclusive_sum(void* tmp, size_t& bytes, int32_t* in, int32_t* out, int n,
                         hipStream_t s);
hipError_t exclusive_sum(void* tmp, size_t& bytes, const int32_t* in, int32_t* out, int n,
                         hipStream_t s);
// InclusiveScan with min(a, b) (b < a ? b : a)
hipError_t inclusive_min(void* tmp, size_t& bytes, double* in, double* out, int n,
                         hipStream_t s);
// DeviceReduce::Sum: *out = the sum of in[0 .. n)
hipError_t reduce_sum(void* tmp, size_t& bytes, int32_t* in, int32_t* out, int n,
                      hipStream_t s);
// DeviceSelect::Flagged over the counting iterator 0, 1, ..: out = the i in
// [0, n) with flags[i] != 0, in order; *n_selected = their count
hipError_t select_flagged_indices(void* tmp, size_t& bytes, const uint8_t* flags, int32_t* out,
                                  int32_t* n_selected, int n, hipStream_t s);

}  // namespace h3dint
