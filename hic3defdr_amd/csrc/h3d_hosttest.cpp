// Host build of the device numerics, for CPU unit tests ONLY.
//
// The same headers the gfx950 kernels include (h3d_special.h, h3d_model.h,
// h3d_philox.h, h3d_sample.h, h3d_ccl.h)
// compiled with g++ and exported over a flat C ABI so tests/ can check them
// against scipy / the oracle without a GPU. The product never loads this
// library (hic3defdr_amd loads libh3d.so and fails loudly without it).
//
// The entries it shares with the gfx950 build are defined once, in
// h3d_unit_abi.h, against the backend below: the buffers are the caller's
// arrays and for_each is the serial loop. The entries after the include
// exist in this build alone.
#include <cstdint>
#include <vector>

#include "h3d_ccl.h"

#define H3DT_BODY

namespace {

template <typename T>
struct In {
  const T* p;
  In(const T* host, int64_t) : p(host) {}
  operator const T*() const { return p; }
};

template <typename T>
struct Out {
  T* p;
  Out(T* host, int64_t, T) : p(host) {}
  operator T*() const { return p; }
  bool fetch() const { return true; }
};

template <typename F>
int for_each(int64_t n, F body) {
  int flags = 0;
  for (int64_t i = 0; i < n; ++i) flags |= body(i);
  return flags;
}

}  // namespace

#include "h3d_unit_abi.h"

extern "C" {

// exp_fast's gfx950 straight line evaluated here (host build only)
H3DT_UNARY(exp_fast_straight, exp_fast_straight)

// Host emulation of the multi-rank estimate_disp driver (h3d_disp_per_dist_dev
// with an all-reduce hook): this rank's pixels, stable-ordered by distance;
// per data pass every active segment's local NLL total, summed across ranks
// by `reduce`, then the shared qcml/Brent state machines advance. Used by the
// gloo world_size-2 tests to check the sharded algorithm on CPU.
typedef int (*h3dt_reduce_fn)(double* buf, int64_t count, void* user);

int h3dt_disp_rounds(int64_t n, int R, int C, const int32_t* raw,
                     const double* f, const int32_t* dist,
                     const int32_t* cond_of_rep, int D, h3dt_reduce_fn reduce,
                     void* user, double* out, int32_t* flags_out) {
  const int S = D * C;
  std::vector<int> nrep(C, 0), rep_idx(C * M, 0);
  for (int r = 0; r < R; ++r) rep_idx[cond_of_rep[r] * M + nrep[cond_of_rep[r]]++] = r;
  std::vector<std::vector<int64_t>> px(D);
  for (int64_t i = 0; i < n; ++i) px[dist[i]].push_back(i);
  std::vector<double> cnt(S, 0.0), tot(S, 0.0);
  for (int d = 0; d < D; ++d)
    for (int c = 0; c < C; ++c) cnt[d * C + c] = (double)px[d].size();
  if (reduce && reduce(cnt.data(), S, user)) return -2;
  std::vector<h3d::SegState> st(S);
  for (int s = 0; s < S; ++s) h3d::seg_init(&st[s], (long long)cnt[s], nrep[s % C]);
  std::vector<double> pd((size_t)n * R, 0.0);
  for (int guard = 0; guard < 200000; ++guard) {
    bool any = false;
    for (int s = 0; s < S; ++s) any |= st[s].phase != h3d::kDone;
    if (!any) break;
    for (int s = 0; s < S; ++s) {
      tot[s] = 0.0;
      if (st[s].phase == h3d::kDone) continue;
      const int d = s / C, c = s % C, nr = nrep[c];
      for (int64_t i : px[d]) {
        double x[M], fv[M], dd[M];
        for (int k = 0; k < nr; ++k) {
          const int r = rep_idx[c * M + k];
          x[k] = raw[i * R + r];
          fv[k] = f[i * R + r];
          dd[k] = pd[i * R + r];
        }
        if (st[s].phase == h3d::kEqualize) {
          st[s].flags |= h3d::equalize_pixel<M>(x, fv, nr, st[s].disp, dd);
          for (int k = 0; k < nr; ++k) pd[i * R + rep_idx[c * M + k]] = dd[k];
        }
        tot[s] += h3d::nll_pixel<M>(dd, nr, st[s].k);
      }
    }
    if (reduce && reduce(tot.data(), S, user)) return -2;
    for (int s = 0; s < S; ++s)
      if (st[s].phase != h3d::kDone) h3d::seg_step(&st[s], tot[s], nrep[s % C]);
  }
  for (int s = 0; s < S; ++s) {
    out[s] = st[s].result;
    if (flags_out) flags_out[s] = st[s].flags;
  }
  return 0;
}

// h3d_label_components (h3d_clusters.hip) with a serial union-find in place
// of the CAS: the same input check, run-head / run-tail predicates and link
// enumeration (h3d_ccl.h), run ids from a serial count, labels by first
// pixel. Returns 16 (H3D_FLAG_BADIN; label all -1, *n_clusters 0) where the
// input breaks the (row, col) rule, -1 for a bad argument, 0 otherwise.
int h3dt_ccl_labels(const int64_t* row, const int64_t* col, const uint8_t* cls, int64_t n,
                    int connectivity, int32_t* label, int64_t* n_clusters) {
  using namespace h3dccl;
  if (n < 0 || n > (((int64_t)1 << 31) - 2) || !n_clusters) return -1;
  if (connectivity != 1 && connectivity != 2) return -1;
  *n_clusters = 0;
  if (n == 0) return 0;
  if (!row || !col || !cls || !label) return -1;
  bool bad = false;
  for (int64_t i = 0; i < n; ++i) {
    bad = bad || bad_pixel(row, col, i);
    label[i] = -1;
  }
  if (bad) return 16;
  std::vector<int32_t> incl((size_t)n), first;
  std::vector<uint64_t> key0, key1;
  std::vector<uint8_t> rcls;
  int32_t count = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (run_head(row, col, cls, i)) {
      ++count;
      first.push_back((int32_t)i);
      key0.push_back(pixel_key(row[i], col[i]));
      key1.push_back(0);
      rcls.push_back(cls[i]);
    }
    incl[i] = count;
    if (run_tail(row, col, cls, i, n)) key1[count - 1] = pixel_key(row[i], col[i]);
  }
  if (count == 0) return 0;
  std::vector<int32_t> parent((size_t)count);
  for (int32_t r = 0; r < count; ++r) parent[r] = r;
  auto find = [&](int32_t x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  const Runs runs{first.data(), key0.data(), key1.data(), rcls.data(), count};
  for (int32_t r = 0; r < count; ++r)
    for_each_link(runs, r, connectivity, [&](int32_t a, int32_t b) {
      a = find(a), b = find(b);
      if (a != b) parent[a > b ? a : b] = a > b ? b : a;  // the smaller id stays the root
    });
  std::vector<int32_t> rank((size_t)count);
  int32_t n_roots = 0;
  for (int32_t r = 0; r < count; ++r) rank[r] = find(r) == r ? n_roots++ : -1;
  for (int64_t i = 0; i < n; ++i)
    if (cls[i] != kAbsent) label[i] = rank[find(incl[i] - 1)];
  *n_clusters = n_roots;
  return 0;
}

// q_class / argmax_class of h3d_ccl.h over n pixels (value (n, C) row-major)
void h3dt_q_class(int64_t n, const double* q, double fdr, uint8_t* cls) {
  for (int64_t i = 0; i < n; ++i) cls[i] = h3dccl::q_class(q[i], fdr);
}
void h3dt_argmax_class(int64_t n, int C, const double* value, const uint8_t* member,
                       uint8_t* cls) {
  for (int64_t i = 0; i < n; ++i)
    cls[i] = member[i] ? h3dccl::argmax_class(value + i * C, C) : h3dccl::kAbsent;
}

}  // extern "C"
