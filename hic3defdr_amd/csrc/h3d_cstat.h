// Per-cluster statistics of a sparse table (cluster_table.py:192-332): the
// plain host + device pieces. h3d_cstat.hip runs them one wave per task,
// h3d_hosttest_cstat.cpp serially, so the association of every sum is checkable
// without a GPU and the device can be held to the host build with ==.
//
// The table is n pixels (row[i], col[i]) with K float64 values each; cluster
// k is a list of pixels. A cluster pixel takes the table's K values at its
// (row, col), or 0.0 where the table has no such pixel; the m values of a
// column are reduced to their mean, max and min (np.mean / np.max / np.min:
// the divisor is m, a NaN among the m makes max and min NaN).
//
// The order of every operation, fixed here:
//   - a task is a chunk of at most kChunk consecutive pixels of one cluster
//     (task_count); a cluster's tasks depend on its size alone;
//   - lane l of the task's kLanes lanes folds the task's pixels l, l + kLanes,
//     ... in that order into an Acc that starts at acc_init();
//   - the lanes are folded by lanes_fold: for o = kLanes / 2 .. 1, lane l < o
//     becomes acc_fold(lane l, lane l + o); lane 0 is the task's partial;
//   - the cluster's partials are folded in task order into an acc_init();
//   - mean = sum / (double)m; a NaN result is stored as kNaNBits (canon), so
//     the x86 and the gfx950 default NaN compare equal.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define H3D_CSTAT_HD __host__ __device__ inline
#else
#define H3D_CSTAT_HD inline
#endif

namespace h3dcstat {

constexpr int kLanes = 64;
constexpr int kChunk = 2048;  // pixels per task
constexpr int kMaxK = 256;    // data columns per call
constexpr int kColBlock = 8;  // columns a lane holds in registers at once
constexpr int64_t kMaxCoord = ((int64_t)1 << 31) - 1;
constexpr int64_t kMaxN = ((int64_t)1 << 31) - 2;
constexpr uint64_t kNaNBits = 0x7ff8000000000000ull;
constexpr uint64_t kBadKey = ~0ull;

// the bits of *flags (H3D_CSTAT_* of h3d.h) and of `want` (H3D_CSTAT_MEAN ..)
constexpr int kFlagRepeat = 1;  // a table pixel twice, or outside [0, 2^31)
constexpr int kFlagOrder = 2;   // `sorted` promised, (row, col) not increasing
constexpr int kFlagPixel = 4;   // a cluster pixel outside [0, n_rows) x [0, n_cols)
constexpr int kFlagStarts = 8;  // starts[0] != 0 or a cluster without pixels
constexpr int kWantMean = 1, kWantMax = 2, kWantMin = 4;

// row << 32 | col (k_mem_set_keys' packing); kBadKey for a coordinate
// outside [0, 2^31), which is above every valid key
H3D_CSTAT_HD uint64_t pixel_key(int64_t row, int64_t col) {
  const uint64_t r = (uint64_t)row, c = (uint64_t)col;
  return (r <= (uint64_t)kMaxCoord && c <= (uint64_t)kMaxCoord) ? ((r << 32) | c) : kBadKey;
}

// what table pixel i (key cur, its predecessor's key prev) does to *flags
// under the `sorted` promise
H3D_CSTAT_HD int sorted_flags(uint64_t prev, uint64_t cur, bool has_prev) {
  if (cur == kBadKey) return kFlagRepeat;
  if (!has_prev || prev == kBadKey) return 0;  // the predecessor reports itself
  return prev == cur ? kFlagRepeat : (prev > cur ? kFlagOrder : 0);
}

// tasks of a cluster of m pixels (m >= 1)
H3D_CSTAT_HD int32_t task_count(int64_t m) { return (int32_t)((m + kChunk - 1) / kChunk); }

// the first position of the n ascending keys whose key is >= key.
// Terminates: hi - lo shrinks by at least one every step.
H3D_CSTAT_HD int64_t lower_bound(const uint64_t* keys, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The table index of cluster pixel (r, c), -1 where the table has none; idx
// is the sort's payload (NULL: the table came sorted, position = index).
// *bad is set for a pixel outside [0, n_rows) x [0, n_cols), which never
// searches.
H3D_CSTAT_HD int32_t lookup(int64_t r, int64_t c, int64_t n_rows, int64_t n_cols,
                            const uint64_t* keys, const int32_t* idx, int64_t n, int* bad) {
  if (r < 0 || r >= n_rows || c < 0 || c >= n_cols) {
    *bad = 1;
    return -1;
  }
  const uint64_t key = pixel_key(r, c);  // n_rows, n_cols <= 2^31: a valid key
  const int64_t pos = lower_bound(keys, n, key);
  if (pos >= n || keys[pos] != key) return -1;
  return idx ? idx[pos] : (int32_t)pos;
}

// np.max / np.min of two values: a NaN wins. Compares only, so the host and
// the device build take the same branch on the same bits.
H3D_CSTAT_HD double nan_max(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a > b ? a : b;
}
H3D_CSTAT_HD double nan_min(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a < b ? a : b;
}

H3D_CSTAT_HD double from_bits(uint64_t u) {
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
}
H3D_CSTAT_HD double canon(double v) { return v != v ? from_bits(kNaNBits) : v; }

struct Acc {
  double sum, mx, mn;
};
H3D_CSTAT_HD Acc acc_init() {
  return Acc{0.0, from_bits(0xfff0000000000000ull), from_bits(0x7ff0000000000000ull)};
}
H3D_CSTAT_HD void acc_add(Acc& a, double v) {
  a.sum = a.sum + v;
  a.mx = nan_max(a.mx, v);
  a.mn = nan_min(a.mn, v);
}
H3D_CSTAT_HD Acc acc_fold(const Acc& a, const Acc& b) {
  return Acc{a.sum + b.sum, nan_max(a.mx, b.mx), nan_min(a.mn, b.mn)};
}

// the lanes' fold written serially over an array of kLanes values (the device
// does it with __shfl_down); the result is lane[0]
template <typename T, typename Fold>
inline void lanes_fold(T* lane, Fold fold) {
  for (int o = kLanes / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) lane[l] = fold(lane[l], lane[l + o]);
}

}  // namespace h3dcstat
