// libh3d.so: the calls on the GPU -- connected-component labelling of the
// thresholded / classified pixels (threshold(gpu=True), classify(gpu=True)).
//
//   h3d_threshold_classes_dev  thresholding.py:7-41: the class byte of a
//                              q-value (sig / insig / in neither);
//   h3d_argmax_classes_dev     classification.py:7-49: np.argmax of a member
//                              pixel's alt-model means;
//   h3d_label_components       clusters.py:69-97 as a partition: pixels of
//                              equal class that touch get one label; labels
//                              rank the clusters by their first pixel;
//   h3d_cluster_lists          per cluster size, class, bounding box; the
//                              kept clusters' members in pixel order.
//
// The labelling is run-based (h3d_ccl.h): run heads -> inclusive sum = run
// ids -> run records -> one lane per run unites it with the touching runs of
// the row above -> roots -> exclusive sum of the root flags = cluster rank.
// The default path's DirectedDisjointSet replay (h3d_calls.cpp) yields the
// same sets in the reference's order; here the order is canonical: clusters
// by first pixel, pixels in (row, col) order.
//
// The union-find over run ids follows ECL-CC (Jaiganesh & Burtscher, HPDC'18):
// parent[x] <= x always, a root is hooked by a device-scope CAS of the larger
// root onto the smaller, find halves paths. What it relies on:
//   - every value ever stored in parent[x] is x or an ancestor of x with a
//     smaller id, so a stale load (another XCD's L2, this CU's L1) yields an
//     older ancestor of the same tree: more steps, never a wrong tree;
//   - a root changes by CAS alone, so two hooks of one root cannot both win;
//   - no kernel waits for another workgroup; phases that need each other's
//     results (links -> roots -> labels) are separate launches;
//   - a tree's root is its smallest id, so labels do not depend on scheduling.
// Integer atomics only. n <= 2^31 - 2.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "h3d.h"
#include "h3d_ccl.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_errors.h"

using namespace h3dint;
using h3derr::fail;

namespace h3dclu {

using namespace h3dccl;

constexpr int kBlock = kLaunchBlock;
constexpr int64_t kMaxN = ((int64_t)1 << 31) - 2;

#define H3D_GRID_STRIDE(i, n)                                          \
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (n); \
       i += (int64_t)gridDim.x * kBlock)

// ---- class bytes ----------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_q_class(const double* __restrict__ q, int64_t n,
                                                    double fdr, uint8_t* __restrict__ cls) {
  H3D_GRID_STRIDE(i, n) cls[i] = q_class(q[i], fdr);
}

__global__ __launch_bounds__(kBlock) void k_argmax_class(const double* __restrict__ value,
                                                         int64_t n, int C,
                                                         const uint8_t* __restrict__ member,
                                                         uint8_t* __restrict__ cls) {
  H3D_GRID_STRIDE(i, n) cls[i] = member[i] ? argmax_class(value + i * C, C) : kAbsent;
}

// ---- runs -------------------------------------------------------------------------

// head[i] = 1 where pixel i starts a run; *flag |= 1 where the input breaks
// the (row, col) rule
__global__ __launch_bounds__(kBlock) void k_run_heads(const int64_t* __restrict__ row,
                                                      const int64_t* __restrict__ col,
                                                      const uint8_t* __restrict__ cls, int64_t n,
                                                      int32_t* __restrict__ head,
                                                      int* __restrict__ flag) {
  int bad = 0;
  H3D_GRID_STRIDE(i, n) {
    bad |= bad_pixel(row, col, i) ? 1 : 0;
    head[i] = run_head(row, col, cls, i) ? 1 : 0;
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}

// incl = the inclusive sum of head: a present pixel belongs to run
// incl[i] - 1. The head writes the run's first index, first key, class and
// parent (itself); the tail writes the last key.
__global__ __launch_bounds__(kBlock) void k_run_records(
    const int64_t* __restrict__ row, const int64_t* __restrict__ col,
    const uint8_t* __restrict__ cls, int64_t n, const int32_t* __restrict__ incl,
    int32_t* __restrict__ first, uint64_t* __restrict__ key0, uint64_t* __restrict__ key1,
    uint8_t* __restrict__ rcls, int32_t* __restrict__ parent) {
  H3D_GRID_STRIDE(i, n) {
    if (cls[i] == kAbsent) continue;
    const int32_t r = incl[i] - 1;
    if (run_head(row, col, cls, i)) {
      first[r] = (int32_t)i;
      key0[r] = pixel_key(row[i], col[i]);
      rcls[r] = cls[i];
      parent[r] = r;
    }
    if (run_tail(row, col, cls, i, n)) key1[r] = pixel_key(row[i], col[i]);
  }
}

// ---- union-find over run ids ------------------------------------------------------

__device__ inline int32_t uf_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this lane can see it, halving the path.
// Terminates: a non-root's parent is smaller than it, so x strictly
// decreases every trip and is bounded by 0. The halving store writes a
// grandparent, which is an ancestor of x: the invariant of the file head.
__device__ inline int32_t uf_find(int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = uf_load(parent + x);
    if (p == x) return x;
    const int32_t g = uf_load(parent + p);
    if (g == p) return p;
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
}

// One tree out of a's and b's. Terminates: a failed CAS returns parent[a],
// which is smaller than a (a was no root any more), and find never returns
// more than its argument, so a + b strictly decreases every trip. b may be a
// stale root: hooking the root a under any smaller node of the other tree
// still merges the two and keeps parent[a] < a.
__device__ inline void uf_unite(int32_t* parent, int32_t a, int32_t b) {
  a = uf_find(parent, a);
  b = uf_find(parent, b);
  while (a != b) {
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicCAS(parent + a, a, b);  // device scope
    if (old == a) return;
    a = uf_find(parent, old);
  }
}

// one lane per run: unite with the touching runs of the row above
__global__ __launch_bounds__(kBlock) void k_run_links(Runs runs, int connectivity,
                                                      int32_t* __restrict__ parent) {
  H3D_GRID_STRIDE(r, runs.count)
  for_each_link(runs, (int32_t)r, connectivity,
                [&](int32_t a, int32_t b) { uf_unite(parent, a, b); });
}

// A launch of its own, read-only on parent: root[r] and the root flag.
// Terminates: parent[x] < x for every non-root.
__global__ __launch_bounds__(kBlock) void k_run_roots(const int32_t* __restrict__ parent,
                                                      int32_t n_runs, int32_t* __restrict__ root,
                                                      int32_t* __restrict__ is_root) {
  H3D_GRID_STRIDE(r, n_runs) {
    int32_t x = (int32_t)r;
    for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[r] = x;
    is_root[r] = x == (int32_t)r ? 1 : 0;
  }
}

// rank = the exclusive sum of is_root: the cluster's number by first pixel
__global__ __launch_bounds__(kBlock) void k_pixel_labels(
    const uint8_t* __restrict__ cls, int64_t n, const int32_t* __restrict__ incl,
    const int32_t* __restrict__ root, const int32_t* __restrict__ rank,
    const int32_t* __restrict__ is_root, int32_t n_runs, int32_t* __restrict__ label,
    int64_t* __restrict__ n_clusters) {
  H3D_GRID_STRIDE(i, n) label[i] = cls[i] == kAbsent ? -1 : rank[root[incl[i] - 1]];
  if (blockIdx.x == 0 && threadIdx.x == 0)
    *n_clusters = (int64_t)rank[n_runs - 1] + is_root[n_runs - 1];
}

__global__ __launch_bounds__(kBlock) void k_fill_i32(int32_t* __restrict__ out, int64_t n,
                                                     int32_t v) {
  H3D_GRID_STRIDE(i, n) out[i] = v;
}

// device pointers; synchronises the stream. *flags gets H3D_FLAG_BADIN (and
// label all -1, *n_clusters 0) where the input breaks the rule.
int label_dev(h3d_ctx* ctx, const int64_t* d_row, const int64_t* d_col, const uint8_t* d_cls,
              int64_t n, int connectivity, int32_t* d_label, int64_t* n_clusters, int* flags) {
  hipStream_t s = ctx->stream;
  Scratch sc{ctx};
  int32_t* head = sc.get<int32_t>("ccl_head", (size_t)n);
  int32_t* incl = sc.get<int32_t>("ccl_incl", (size_t)n);
  // status: [0] the input flag, [1] unused, then the cluster count (int64)
  int32_t* d_st = sc.get<int32_t>("ccl_status", 4);
  if (!sc.ok) return fail(H3D_ENOMEM, "labelling buffers");
  ProfScope ps(ctx, "ccl_label", n);
  HIP_TRY(hipMemsetAsync(d_st, 0, 16, s));
  hipLaunchKernelGGL(k_run_heads, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_row, d_col, d_cls,
                     n, head, (int*)d_st);
  if (int rc = cub_call(ctx, "cub_tmp_ccl", [&](void* tmp, size_t& bytes) {
        return inclusive_sum(tmp, bytes, head, incl, (int)n, s);
      }))
    return rc;
  HIP_TRY(hipGetLastError());
  // the input flag and the run count in one read
  HIP_TRY(hipMemcpyAsync(d_st + 1, incl + (n - 1), 4, hipMemcpyDeviceToDevice, s));
  int32_t st[2] = {0, 0};
  if (int rc = d2h_sync(ctx, st, d_st, 8, s)) return rc;
  const int32_t n_runs = st[1];
  if (st[0] || n_runs == 0) {
    if (st[0]) *flags |= H3D_FLAG_BADIN;
    hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_label, n, -1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  }
  int32_t* first = sc.get<int32_t>("ccl_run_first", (size_t)n_runs);
  uint64_t* key0 = sc.get<uint64_t>("ccl_run_key0", (size_t)n_runs);
  uint64_t* key1 = sc.get<uint64_t>("ccl_run_key1", (size_t)n_runs);
  uint8_t* rcls = sc.get<uint8_t>("ccl_run_cls", (size_t)n_runs);
  int32_t* parent = sc.get<int32_t>("ccl_parent", (size_t)n_runs);
  int32_t* root = sc.get<int32_t>("ccl_root", (size_t)n_runs);
  int32_t* is_root = sc.get<int32_t>("ccl_is_root", (size_t)n_runs);
  int32_t* rank = sc.get<int32_t>("ccl_rank", (size_t)n_runs);
  if (!sc.ok) return fail(H3D_ENOMEM, "run buffers");
  hipLaunchKernelGGL(k_run_records, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_row, d_col,
                     d_cls, n, incl, first, key0, key1, rcls, parent);
  const Runs runs{first, key0, key1, rcls, n_runs};
  hipLaunchKernelGGL(k_run_links, dim3(grid_for(ctx, n_runs)), dim3(kBlock), 0, s, runs,
                     connectivity, parent);
  hipLaunchKernelGGL(k_run_roots, dim3(grid_for(ctx, n_runs)), dim3(kBlock), 0, s, parent, n_runs,
                     root, is_root);
  if (int rc = cub_call(ctx, "cub_tmp_ccl", [&](void* tmp, size_t& bytes) {
        return exclusive_sum(tmp, bytes, is_root, rank, (int)n_runs, s);
      }))
    return rc;
  int64_t* d_ncl = (int64_t*)(d_st + 2);
  hipLaunchKernelGGL(k_pixel_labels, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_cls, n, incl,
                     root, rank, is_root, n_runs, d_label, d_ncl);
  HIP_TRY(hipGetLastError());
  return d2h_sync(ctx, n_clusters, d_ncl, 8, s);
}

int check_label(const void* ctx, const void* row, const void* col, const void* cls, int64_t n,
                int connectivity, const void* label, const void* n_clusters, const void* flags) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0 || n > kMaxN) return fail(H3D_EARG, "n=%lld outside [0, 2^31 - 2]", (long long)n);
  if (connectivity != 1 && connectivity != 2)
    return fail(H3D_EARG, "connectivity=%d, not 1 or 2", connectivity);
  if (!n_clusters || !flags) return fail(H3D_EARG, "null n_clusters / flags");
  if (n && (!row || !col || !cls || !label)) return fail(H3D_EARG, "null pixel array");
  return 0;
}

// ---- cluster lists ----------------------------------------------------------------

// bounds is (4, n_clusters): min row, max row, min col, max col
__global__ __launch_bounds__(kBlock) void k_stats_init(int32_t n_clusters,
                                                       int32_t* __restrict__ size,
                                                       int32_t* __restrict__ first,
                                                       int32_t* __restrict__ bounds) {
  H3D_GRID_STRIDE(k, n_clusters) {
    size[k] = 0;
    first[k] = INT_MAX;
    bounds[k] = INT_MAX;
    bounds[(int64_t)n_clusters + k] = -1;
    bounds[2 * (int64_t)n_clusters + k] = INT_MAX;
    bounds[3 * (int64_t)n_clusters + k] = -1;
  }
}

__device__ inline void stats_add(int32_t nc, int32_t l, int32_t cnt, int32_t idx, int32_t r0,
                                 int32_t r1, int32_t c0, int32_t c1, int32_t* size,
                                 int32_t* first, int32_t* bounds) {
  atomicAdd(size + l, cnt);
  atomicMin(first + l, idx);
  atomicMin(bounds + l, r0);
  atomicMax(bounds + (int64_t)nc + l, r1);
  atomicMin(bounds + 2 * (int64_t)nc + l, c0);
  atomicMax(bounds + 3 * (int64_t)nc + l, c1);
}

// Size, first member and bounding box per cluster by integer atomics. The
// pixels come in (row, col) order, so most of a wave's 64 pixels are of one
// or two clusters: a label held by many lanes is reduced in registers and
// issues one set of atomics (the giant insig component would otherwise send
// every pixel's six atomics to the same six words, also from the waves a few
// sig pixels are sprinkled into). A label outside [-1, n_clusters) sets *flag.
constexpr int kGroups = 3, kMinGroup = 8;

__global__ __launch_bounds__(kBlock) void k_cluster_stats(
    const int32_t* __restrict__ label, const int64_t* __restrict__ row,
    const int64_t* __restrict__ col, int64_t n, int32_t n_clusters, int32_t* __restrict__ size,
    int32_t* __restrict__ first, int32_t* __restrict__ bounds, int* __restrict__ flag) {
  int bad = 0;
  // every lane of the block takes every trip (the bound is block-uniform)
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n;
       base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    int32_t l = i < n ? label[i] : -1;
    if (l < -1 || l >= n_clusters) {
      bad = 1;
      l = -1;
    }
    const int32_t r = l >= 0 ? (int32_t)row[i] : 0, c = l >= 0 ? (int32_t)col[i] : 0;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(l >= 0);
    // up to kGroups labels of the wave with at least kMinGroup lanes each
    // are reduced in registers, their first lane adding the result
    for (int g = 0; g < kGroups && todo; ++g) {
      const int lead = __ffsll((long long)todo) - 1;
      const int32_t lg = __shfl(l, lead, 64);
      const unsigned long long grp = __ballot(l == lg) & todo;
      const int cnt = __popcll(grp);
      if (cnt < kMinGroup) break;  // wave-uniform
      const bool in = (grp >> lane) & 1;
      int32_t r0 = in ? r : INT_MAX, r1 = in ? r : -1, c0 = in ? c : INT_MAX, c1 = in ? c : -1;
      for (int o = 32; o > 0; o >>= 1) {
        r0 = min(r0, __shfl_xor(r0, o, 64));
        r1 = max(r1, __shfl_xor(r1, o, 64));
        c0 = min(c0, __shfl_xor(c0, o, 64));
        c1 = max(c1, __shfl_xor(c1, o, 64));
      }
      if (lane == lead)  // the group's first lane: its smallest index
        stats_add(n_clusters, l, cnt, (int32_t)i, r0, r1, c0, c1, size, first, bounds);
      todo &= ~grp;
    }
    if ((todo >> lane) & 1)
      stats_add(n_clusters, l, 1, (int32_t)i, r, r, c, c, size, first, bounds);
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void k_cluster_keep(int32_t n_clusters, int32_t min_size,
                                                         const int32_t* __restrict__ size,
                                                         int32_t* __restrict__ keep,
                                                         int32_t* __restrict__ ksize) {
  H3D_GRID_STRIDE(k, n_clusters) {
    const int32_t kp = size[k] >= min_size && size[k] > 0 ? 1 : 0;
    keep[k] = kp;
    ksize[k] = kp ? size[k] : 0;
  }
}

// krank / kstart = the exclusive sums of keep / ksize. starts of the kept
// clusters, every cluster's class (of its first member) and the totals
// tot = {n_kept, n_members}.
__global__ __launch_bounds__(kBlock) void k_cluster_starts(
    int32_t n_clusters, const int32_t* __restrict__ keep, const int32_t* __restrict__ krank,
    const int32_t* __restrict__ ksize, const int32_t* __restrict__ kstart,
    const int32_t* __restrict__ first, const uint8_t* __restrict__ cls,
    int64_t* __restrict__ starts, uint8_t* __restrict__ cls_of, int64_t* __restrict__ tot) {
  H3D_GRID_STRIDE(k, n_clusters) {
    if (keep[k]) starts[krank[k]] = kstart[k];
    cls_of[k] = first[k] != INT_MAX ? cls[first[k]] : kAbsent;
    if (k == n_clusters - 1) {
      tot[0] = (int64_t)krank[k] + keep[k];
      tot[1] = (int64_t)kstart[k] + ksize[k];
      starts[tot[0]] = tot[1];
    }
  }
}

// sort key of pixel i: its kept cluster's rank, n_kept for the rest
__global__ __launch_bounds__(kBlock) void k_member_keys(const int32_t* __restrict__ label,
                                                        int64_t n, int32_t n_clusters,
                                                        const int32_t* __restrict__ keep,
                                                        const int32_t* __restrict__ krank,
                                                        int32_t n_kept, int32_t* __restrict__ keys) {
  H3D_GRID_STRIDE(i, n) {
    const int32_t l = label[i];
    keys[i] = (l >= 0 && l < n_clusters && keep[l]) ? krank[l] : n_kept;
  }
}

// device pointers; synchronises the stream
int lists_dev(h3d_ctx* ctx, const int32_t* d_label, const uint8_t* d_cls, const int64_t* d_row,
              const int64_t* d_col, int64_t n, int64_t n_clusters, int64_t min_size,
              int32_t* d_size, uint8_t* d_cls_of, int32_t* d_bounds, int32_t* d_members,
              int64_t* d_starts, int64_t* n_kept, int64_t* n_members) {
  hipStream_t s = ctx->stream;
  const int32_t nc = (int32_t)n_clusters;
  const int32_t ms = (int32_t)(min_size > INT_MAX ? INT_MAX : (min_size < 1 ? 1 : min_size));
  *n_kept = *n_members = 0;
  if (nc == 0) {
    HIP_TRY(hipMemsetAsync(d_starts, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  }
  Scratch sc{ctx};
  int32_t* first = sc.get<int32_t>("ccl_cl_first", (size_t)nc);
  int32_t* keep = sc.get<int32_t>("ccl_cl_keep", (size_t)nc);
  int32_t* krank = sc.get<int32_t>("ccl_cl_krank", (size_t)nc);
  int32_t* ksize = sc.get<int32_t>("ccl_cl_ksize", (size_t)nc);
  int32_t* kstart = sc.get<int32_t>("ccl_cl_kstart", (size_t)nc);
  int64_t* d_tot = sc.get<int64_t>("ccl_cl_tot", 3);  // n_kept, n_members, the label flag
  if (!sc.ok) return fail(H3D_ENOMEM, "cluster list buffers");
  ProfScope ps(ctx, "ccl_lists", n);
  HIP_TRY(hipMemsetAsync(d_tot, 0, 24, s));
  hipLaunchKernelGGL(k_stats_init, dim3(grid_for(ctx, nc)), dim3(kBlock), 0, s, nc, d_size, first,
                     d_bounds);
  hipLaunchKernelGGL(k_cluster_stats, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_label, d_row,
                     d_col, n, nc, d_size, first, d_bounds, (int*)(d_tot + 2));
  hipLaunchKernelGGL(k_cluster_keep, dim3(grid_for(ctx, nc)), dim3(kBlock), 0, s, nc, ms, d_size,
                     keep, ksize);
  if (int rc = cub_call(ctx, "cub_tmp_ccl", [&](void* tmp, size_t& bytes) {
        return exclusive_sum(tmp, bytes, keep, krank, (int)nc, s);
      }))
    return rc;
  if (int rc = cub_call(ctx, "cub_tmp_ccl", [&](void* tmp, size_t& bytes) {
        return exclusive_sum(tmp, bytes, ksize, kstart, (int)nc, s);
      }))
    return rc;
  hipLaunchKernelGGL(k_cluster_starts, dim3(grid_for(ctx, nc)), dim3(kBlock), 0, s, nc, keep,
                     krank, ksize, kstart, first, d_cls, d_starts, d_cls_of, d_tot);
  HIP_TRY(hipGetLastError());
  int64_t tot[3] = {0, 0, 0};
  if (int rc = d2h_sync(ctx, tot, d_tot, 24, s)) return rc;
  if (tot[2]) return fail(H3D_EARG, "a label outside [-1, n_clusters)");
  *n_kept = tot[0];
  *n_members = tot[1];
  if (tot[1] == 0) return 0;
  // a stable sort by kept rank leaves every cluster in index order; the
  // dropped and absent pixels sort behind the n_members kept ones
  int32_t* keys = sc.get<int32_t>("ccl_cl_keys", (size_t)n);
  int32_t* keys_s = sc.get<int32_t>("ccl_cl_keys_s", (size_t)n);
  int32_t* vals = sc.get<int32_t>("ccl_cl_vals", (size_t)n);
  if (!sc.ok) return fail(H3D_ENOMEM, "member sort buffers");
  const int32_t nk = (int32_t)tot[0];
  hipLaunchKernelGGL(k_member_keys, dim3(grid_for(ctx, n)), dim3(kBlock), 0, s, d_label, n, nc,
                     keep, krank, nk, keys);
  launch_iota(ctx, s, vals, n);
  int bits = 1;
  while (bits < 31 && ((int64_t)1 << bits) <= nk) ++bits;
  if (int rc = cub_call(ctx, "cub_tmp_ccl", [&](void* tmp, size_t& bytes) {
        return sort_pairs(tmp, bytes, (const int32_t*)keys, keys_s, (const int32_t*)vals,
                          d_members, (int)n, 0, bits, s);
      }))
    return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int check_lists(const void* ctx, int64_t n, int64_t n_clusters, bool arrays, bool outputs,
                const void* n_kept, const void* n_members) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0 || n > kMaxN) return fail(H3D_EARG, "n=%lld outside [0, 2^31 - 2]", (long long)n);
  if (n_clusters < 0 || n_clusters > n)
    return fail(H3D_EARG, "n_clusters=%lld outside [0, n]", (long long)n_clusters);
  if (!n_kept || !n_members) return fail(H3D_EARG, "null n_kept / n_members");
  if (n && !arrays) return fail(H3D_EARG, "null pixel array");
  if (!outputs) return fail(H3D_EARG, "null output");
  return 0;
}

}  // namespace h3dclu

extern "C" {

int h3d_threshold_classes_dev(h3d_ctx* ctx, const double* d_q, int64_t n, double fdr,
                              uint8_t* d_cls) {
  using namespace h3dclu;
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0 || n > kMaxN) return fail(H3D_EARG, "n=%lld outside [0, 2^31 - 2]", (long long)n);
  if (n == 0) return 0;
  if (!d_q || !d_cls) return fail(H3D_EARG, "null q / cls");
  HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_q_class, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, d_q, n, fdr,
                     d_cls);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int h3d_argmax_classes_dev(h3d_ctx* ctx, const double* d_value, int64_t n, int C,
                           const uint8_t* d_member, uint8_t* d_cls) {
  using namespace h3dclu;
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0 || n > kMaxN) return fail(H3D_EARG, "n=%lld outside [0, 2^31 - 2]", (long long)n);
  if (C < 1 || C > kMaxClasses) return fail(H3D_EARG, "C=%d outside [1, %d]", C, kMaxClasses);
  if (n == 0) return 0;
  if (!d_value || !d_member || !d_cls) return fail(H3D_EARG, "null value / member / cls");
  HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_argmax_class, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, d_value,
                     n, C, d_member, d_cls);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int h3d_label_components_dev(h3d_ctx* ctx, const int64_t* d_row, const int64_t* d_col,
                             const uint8_t* d_cls, int64_t n, int connectivity, int32_t* d_label,
                             int64_t* n_clusters, int* flags) {
  using namespace h3dclu;
  if (int rc = check_label(ctx, d_row, d_col, d_cls, n, connectivity, d_label, n_clusters, flags))
    return rc;
  *n_clusters = 0;
  *flags = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  return label_dev(ctx, d_row, d_col, d_cls, n, connectivity, d_label, n_clusters, flags);
}

int h3d_label_components(h3d_ctx* ctx, const int64_t* row, const int64_t* col, const uint8_t* cls,
                         int64_t n, int connectivity, int32_t* label, int64_t* n_clusters,
                         int* flags) {
  using namespace h3dclu;
  if (int rc = check_label(ctx, row, col, cls, n, connectivity, label, n_clusters, flags))
    return rc;
  *n_clusters = 0;
  *flags = 0;
  if (n == 0) return 0;
  HostCall hc(ctx);
  int64_t* d_row = hc.in("ccl_in_row", row, (size_t)n);
  int64_t* d_col = hc.in("ccl_in_col", col, (size_t)n);
  uint8_t* d_cls = hc.in("ccl_in_cls", cls, (size_t)n);
  int32_t* d_label = hc.out<int32_t>("ccl_out_label", (size_t)n);
  if (int rc = hc.ready("labelling buffers")) return rc;
  if (int rc = label_dev(ctx, d_row, d_col, d_cls, n, connectivity, d_label, n_clusters, flags))
    return rc;
  hc.back(label, d_label, (size_t)n);
  return hc.finish();
}

int h3d_cluster_lists_dev(h3d_ctx* ctx, const int32_t* d_label, const uint8_t* d_cls,
                          const int64_t* d_row, const int64_t* d_col, int64_t n,
                          int64_t n_clusters, int64_t min_size, int32_t* d_size,
                          uint8_t* d_cls_of, int32_t* d_bounds, int32_t* d_members,
                          int64_t* d_starts, int64_t* n_kept, int64_t* n_members) {
  using namespace h3dclu;
  if (int rc = check_lists(ctx, n, n_clusters, d_label && d_cls && d_row && d_col,
                           d_starts && (n_clusters == 0 || (d_size && d_cls_of && d_bounds)) &&
                               (n == 0 || d_members),
                           n_kept, n_members))
    return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return lists_dev(ctx, d_label, d_cls, d_row, d_col, n, n_clusters, min_size, d_size, d_cls_of,
                   d_bounds, d_members, d_starts, n_kept, n_members);
}

int h3d_cluster_lists(h3d_ctx* ctx, const int32_t* label, const uint8_t* cls, const int64_t* row,
                      const int64_t* col, int64_t n, int64_t n_clusters, int64_t min_size,
                      int32_t* size, uint8_t* cls_of, int32_t* bounds, int32_t* members,
                      int64_t* starts, int64_t* n_kept, int64_t* n_members) {
  using namespace h3dclu;
  if (int rc = check_lists(ctx, n, n_clusters, label && cls && row && col,
                           starts && (n_clusters == 0 || (size && cls_of && bounds)) &&
                               (n == 0 || members),
                           n_kept, n_members))
    return rc;
  *n_kept = *n_members = 0;
  if (n_clusters == 0) {
    starts[0] = 0;
    return 0;
  }
  const size_t nc = (size_t)n_clusters;
  HostCall hc(ctx);
  int32_t* d_label = hc.in("ccl_in_label", label, (size_t)n);
  uint8_t* d_cls = hc.in("ccl_in_cls", cls, (size_t)n);
  int64_t* d_row = hc.in("ccl_in_row", row, (size_t)n);
  int64_t* d_col = hc.in("ccl_in_col", col, (size_t)n);
  int32_t* d_size = hc.out<int32_t>("ccl_out_size", nc);
  uint8_t* d_cls_of = hc.out<uint8_t>("ccl_out_cls_of", nc);
  int32_t* d_bounds = hc.out<int32_t>("ccl_out_bounds", 4 * nc);
  int32_t* d_members = hc.out<int32_t>("ccl_out_members", (size_t)n);
  int64_t* d_starts = hc.out<int64_t>("ccl_out_starts", nc + 1);
  if (int rc = hc.ready("cluster list buffers")) return rc;
  if (int rc = lists_dev(ctx, d_label, d_cls, d_row, d_col, n, n_clusters, min_size, d_size,
                         d_cls_of, d_bounds, d_members, d_starts, n_kept, n_members))
    return rc;
  hc.back(size, d_size, nc);
  hc.back(cls_of, d_cls_of, nc);
  hc.back(bounds, d_bounds, 4 * nc);
  hc.back(members, d_members, (size_t)*n_members);
  hc.back(starts, d_starts, (size_t)*n_kept + 1);
  return hc.finish();
}

}  // extern "C"
