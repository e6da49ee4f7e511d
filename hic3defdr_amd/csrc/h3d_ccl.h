// Run-based connected-component labelling of a banded pixel list: the plain
// host + device pieces (no memory model in here). h3d_clusters.hip runs them
// under a lock-free union-find, h3d_hosttest.cpp under a serial one, so all
// but the concurrency is checkable without a GPU.
//
// Input: pixels (row[i], col[i]) in strictly increasing (row, col) order,
// coordinates in [0, 2^31), and a class byte per pixel (kAbsent = no pixel).
// Two pixels connect when they are adjacent (connectivity 1: an edge, 2: an
// edge or a corner) and of equal class: the partition of clusters.py:69-97
// per class. A run is a maximal stretch of consecutive columns of one row
// and one class; runs come out in pixel order, so a run's id orders it by
// its first pixel.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define H3D_CCL_HD __host__ __device__ inline
#else
#define H3D_CCL_HD inline
#endif

namespace h3dccl {

constexpr uint8_t kAbsent = 255;
constexpr int kMaxClasses = 254;  // C of argmax_class: 254 stays a class byte
constexpr int64_t kMaxCoord = ((int64_t)1 << 31) - 1;

H3D_CCL_HD uint64_t pixel_key(int64_t row, int64_t col) {
  return ((uint64_t)row << 32) | (uint64_t)col;
}

// pixel i breaks the input rule: a coordinate outside [0, 2^31), or not
// after pixel i - 1 in (row, col) order (a repeat included)
H3D_CCL_HD bool bad_pixel(const int64_t* row, const int64_t* col, int64_t i) {
  const uint64_t r = (uint64_t)row[i], c = (uint64_t)col[i];
  if (r > (uint64_t)kMaxCoord || c > (uint64_t)kMaxCoord) return true;
  if (i == 0) return false;
  const uint64_t pr = (uint64_t)row[i - 1], pc = (uint64_t)col[i - 1];
  if (pr > (uint64_t)kMaxCoord || pc > (uint64_t)kMaxCoord) return false;  // i - 1 reports itself
  return pixel_key((int64_t)pr, (int64_t)pc) >= pixel_key((int64_t)r, (int64_t)c);
}

// pixel i (i >= 1) continues the run of pixel i - 1
H3D_CCL_HD bool run_continues(const int64_t* row, const int64_t* col, const uint8_t* cls,
                              int64_t i) {
  return cls[i] != kAbsent && cls[i - 1] == cls[i] && row[i - 1] == row[i] &&
         col[i - 1] + 1 == col[i];
}
H3D_CCL_HD bool run_head(const int64_t* row, const int64_t* col, const uint8_t* cls, int64_t i) {
  return cls[i] != kAbsent && !(i > 0 && run_continues(row, col, cls, i));
}
H3D_CCL_HD bool run_tail(const int64_t* row, const int64_t* col, const uint8_t* cls, int64_t i,
                         int64_t n) {
  return cls[i] != kAbsent && !(i + 1 < n && run_continues(row, col, cls, i + 1));
}

// The run records, one array per field, in run-id order: the index of the
// first pixel, the keys of the first and the last pixel (row << 32 | col)
// and the class. Runs of one row are disjoint and ascending, so key0 and
// key1 are both strictly increasing.
struct Runs {
  const int32_t* first;
  const uint64_t* key0;
  const uint64_t* key1;
  const uint8_t* cls;
  int32_t count;
};

// the first run whose last pixel is at or after `key` (count if none).
// Terminates: hi - lo shrinks by at least one every step.
H3D_CCL_HD int32_t first_run_ending_at_or_after(const Runs& runs, uint64_t key) {
  int32_t lo = 0, hi = runs.count;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (runs.key1[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// unite(r, j) for every run j of the row above run r that touches r's column
// span (widened by a column on each side at connectivity 2) and has r's
// class. Backward links only: an edge is seen from its later run. Terminates:
// j only increases and stops at r at the latest (run r's row is not the row
// above).
template <typename Unite>
H3D_CCL_HD void for_each_link(const Runs& runs, int32_t r, int connectivity, Unite unite) {
  const uint64_t k0 = runs.key0[r], k1 = runs.key1[r];
  const uint64_t row = k0 >> 32;
  if (row == 0) return;
  const uint64_t widen = connectivity == 2 ? 1 : 0;
  const uint64_t c0 = k0 & 0xffffffffull, c1 = k1 & 0xffffffffull;
  const uint64_t lo = ((row - 1) << 32) | (c0 >= widen ? c0 - widen : 0);
  const uint64_t hi = ((row - 1) << 32) | (c1 + widen);  // c1 + 1 <= 2^31: stays in the low word
  const uint8_t cls = runs.cls[r];
  for (int32_t j = first_run_ending_at_or_after(runs, lo); j < r && runs.key0[j] <= hi; ++j)
    if (runs.cls[j] == cls) unite(r, j);
}

// the class byte of threshold (thresholding.py:7-41): q < fdr -> 0 (sig),
// q >= fdr -> 1 (insig), NaN -> in neither
H3D_CCL_HD uint8_t q_class(double q, double fdr) {
  return q < fdr ? 0 : (q >= fdr ? 1 : kAbsent);
}

// np.argmax of v[0 .. C): the first maximum, and the first NaN wins
// (classification.py:7-49); 1 <= C <= kMaxClasses
H3D_CCL_HD uint8_t argmax_class(const double* v, int C) {
  int best = 0;
  for (int j = 0; j < C; ++j) {
    if (v[j] != v[j]) return (uint8_t)j;
    if (v[j] > v[best]) best = j;
  }
  return (uint8_t)best;
}

}  // namespace h3dccl
