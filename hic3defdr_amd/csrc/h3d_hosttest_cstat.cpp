// libh3d_hosttest.so: the host twin of the per-cluster statistics, for CPU
// unit tests ONLY (a translation unit of its own beside h3d_hosttest.cpp; the
// product never loads this library).
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "h3d_cstat.h"

extern "C" {

// h3d_cluster_stats (h3d_cstat.hip) written serially: the same keys, order
// check, lookup, tasks, lane striding, lane fold and task-order fold
// (h3d_cstat.h), so every sum associates as on the device. Returns the
// H3D_CSTAT_* flag bits (the outputs are then untouched), -1 for a bad
// argument, 0 otherwise. Outputs may be NULL.
int h3dt_cluster_stats(const int64_t* row, const int64_t* col, const double* data, int64_t n,
                       int K, int sorted, int64_t n_rows, int64_t n_cols, const int64_t* prow,
                       const int64_t* pcol, const int64_t* starts, int64_t n_clusters,
                       double* mean, double* vmax, double* vmin, int32_t* found) {
  using namespace h3dcstat;
  if (n < 0 || n > kMaxN || K < 1 || K > kMaxK || n_clusters < 0 || n_clusters > kMaxN) return -1;
  if (n_rows < 0 || n_rows > kMaxCoord + 1 || n_cols < 0 || n_cols > kMaxCoord + 1) return -1;
  if (n_clusters == 0) return 0;
  if ((n && (!row || !col || !data)) || !prow || !pcol || !starts) return -1;
  int flags = 0;
  std::vector<uint64_t> keys((size_t)n);
  std::vector<int32_t> idx;
  for (int64_t i = 0; i < n; ++i) {
    keys[i] = pixel_key(row[i], col[i]);
    if (sorted)
      flags |= sorted_flags(i > 0 ? keys[i - 1] : 0, keys[i], i > 0);
    else if (keys[i] == kBadKey)
      flags |= kFlagRepeat;
  }
  if (!sorted) {
    idx.resize((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int32_t a, int32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> ks((size_t)n);
    for (int64_t i = 0; i < n; ++i) ks[i] = keys[idx[i]];
    keys.swap(ks);
    for (int64_t i = 1; i < n; ++i)
      if (keys[i] == keys[i - 1]) flags |= kFlagRepeat;
  }
  for (int64_t k = 0; k < n_clusters; ++k)
    if (!((k == 0 ? starts[k] == 0 : starts[k] > 0) && starts[k + 1] > starts[k]))
      flags |= kFlagStarts;
  if (flags) return flags;
  const int64_t n_pix = starts[n_clusters];
  if (n_pix > kMaxN) return -1;
  std::vector<int32_t> loc((size_t)n_pix);
  int bad = 0;
  for (int64_t p = 0; p < n_pix; ++p)
    loc[p] = lookup(prow[p], pcol[p], n_rows, n_cols, keys.data(), sorted ? nullptr : idx.data(),
                    n, &bad);
  if (bad) return kFlagPixel;
  for (int64_t k = 0; k < n_clusters; ++k) {
    const int64_t m = starts[k + 1] - starts[k];
    const int32_t nt = task_count(m);
    int32_t f = 0;
    for (int c = 0; c < K; ++c) {
      Acc a = acc_init();
      for (int32_t t = 0; t < nt; ++t) {  // the cluster's partials in task order
        const int64_t p0 = starts[k] + (int64_t)t * kChunk;
        const int64_t p1 = std::min(p0 + kChunk, starts[k + 1]);
        Acc lane[kLanes];
        int32_t cnt[kLanes];
        for (int l = 0; l < kLanes; ++l) {
          lane[l] = acc_init();
          cnt[l] = 0;
          for (int64_t p = p0 + l; p < p1; p += kLanes) {
            const int32_t i = loc[p];
            cnt[l] += i >= 0;
            acc_add(lane[l], i >= 0 ? data[(int64_t)i * K + c] : 0.0);
          }
        }
        lanes_fold(lane, [](const Acc& x, const Acc& y) { return acc_fold(x, y); });
        lanes_fold(cnt, [](int32_t x, int32_t y) { return x + y; });
        a = acc_fold(a, lane[0]);
        if (c == 0) f += cnt[0];
      }
      if (mean) mean[k * K + c] = canon(a.sum / (double)m);
      if (vmax) vmax[k * K + c] = canon(a.mx);
      if (vmin) vmin[k * K + c] = canon(a.mn);
    }
    if (found) found[k] = f;
  }
  return 0;
}

}  // extern "C"
