// libh3d.so: C ABI (include/h3d.h) + orchestration of the gfx950 kernels:
// context, profiling, the estimate_disp driver, cml, bh. The lrt entries live
// in h3d_lrt.hip, prepare_data's in h3d_prepare_api.hip (separate TUs,
// compiled in parallel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <optional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_cub.h"
#include "h3d_errors.h"
#include "h3d_host.h"
#include "h3d_kernels.h"

using namespace h3d;
using namespace h3dint;
using h3derr::fail;

namespace {

// H3D_TIMING=1: host-side stage stamps of the estimate_disp driver (stderr)
struct HostStamps {
  bool on = std::getenv("H3D_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char* what) const {
    if (on)
      fprintf(stderr, "[h3d timing] %8.1f us %s\n",
              std::chrono::duration<double, std::micro>(
                  std::chrono::steady_clock::now() - t0).count(), what);
  }
};

// workgroups of `kernel` (`block` threads, `dyn_lds` bytes of dynamic LDS)
// that fit on one CU at once, queried once per kernel (every device of a
// process is a gfx950)
template <typename K>
int resident_blocks(h3d_ctx* ctx, K kernel, int block, size_t dyn_lds = 0) {
  int& nb = ctx->resident[(const void*)kernel];
  if (nb == 0 &&
      (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, dyn_lds) != hipSuccess ||
       nb < 1))
    nb = 1;
  return nb;
}

// grid = one full wave of resident workgroups (the kernels grid-stride over
// the work list), at most one workgroup per item
template <typename K>
int work_grid(h3d_ctx* ctx, K kernel, size_t max_items) {
  const size_t wave = (size_t)ctx->n_cu * resident_blocks(ctx, kernel, kBlock);
  return (int)std::max<size_t>(1, std::min<size_t>(max_items, wave));
}

// The kernels' replicate slot width M -- the smallest of 2, 4, 8, 16, 32 that
// holds the largest condition -- and their kFull forms (M = 2 only, see
// k_brent) are template arguments: fn(integral_constant<int, M>,
// bool_constant<kFull>) runs with the call's pair.
template <typename F>
auto with_width(int mslot, bool nll_full, F&& fn) {
  using std::integral_constant;
  if (mslot == 2 && nll_full) return fn(integral_constant<int, 2>{}, std::true_type{});
  if (mslot == 2) return fn(integral_constant<int, 2>{}, std::false_type{});
  if (mslot == 4) return fn(integral_constant<int, 4>{}, std::false_type{});
  if (mslot == 8) return fn(integral_constant<int, 8>{}, std::false_type{});
  if (mslot == 16) return fn(integral_constant<int, 16>{}, std::false_type{});
  return fn(integral_constant<int, 32>{}, std::false_type{});
}

// the whole Brent search of every freshly equalized segment (single rank)
// (kFull: every condition has exactly M replicates, see k_brent)
template <int M, bool kFull = false>
void launch_brent(h3d_ctx* ctx, const double* pd, int64_t n, const int64_t* seg_start,
                  int S, int C, const int32_t* rep_idx, const int32_t* n_rep,
                  SegState* st, const int* seg_flags, double* result, int* queue,
                  const int32_t* gate_meta = nullptr, int live_min = 0,
                  const int* gang_abort = nullptr, bool queue_zeroed = false) {
  ProfScope ps(ctx, "disp_nll", 0);
  auto k = k_brent<M, kFull>;
  constexpr int kBrentBlock = brent_block<M>();
  // LDS staging of each segment's head: the workgroup's whole share of the
  // CU's LDS (one 1024-thread workgroup per CU), minus the static part
  // (M >= 16: 512-thread workgroups, two per CU -- staging would halve that)
  const size_t lds_bytes = M <= 8 ? (size_t)ctx->brent_lds_kb * 1024 : 0;
  if (lds_bytes && !ctx->resident.count((const void*)k))
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
  const int grid =
      std::max(1, std::min(S, ctx->n_cu * resident_blocks(ctx, k, kBrentBlock, lds_bytes)));
  // (whole blocks of pixels: thread t then adds pixels t, t + block, ... of
  // the segment in that order wherever the head ends, so the sum's bits do
  // not depend on H3D_BRENT_LDS_KB; the default and every measured size
  // already were -- 16 KB at M = 4, 512 pixels, gave other last bits)
  const int64_t lds_px =
      (int64_t)(lds_bytes / (8 * (size_t)M)) / kBrentBlock * kBrentBlock;
  if (!queue_zeroed) (void)hipMemsetAsync(queue, 0, sizeof(int), ctx->stream);
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBrentBlock), lds_px ? lds_px * 8 * M : 0,
                     ctx->stream, pd, n, seg_start, S, C, rep_idx, n_rep, st, seg_flags,
                     result, queue, ctx->work_count, lds_px, gate_meta, live_min, gang_abort,
                     ctx->nll_ranges);
#ifdef H3D_BRENT_CLOCK
  unsigned long long clk[38];
  (void)hipMemcpyFromSymbolAsync(clk, HIP_SYMBOL(g_brent_clk), sizeof(clk), 0,
                                 hipMemcpyDeviceToHost, ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  fprintf(stderr, "[brent_clk] sum %llu bar1 %llu step %llu bar2 %llu stage %llu total %llu\n",
          clk[0], clk[1], clk[2], clk[3], clk[4], clk[5]);
  fprintf(stderr, "[brent_clk_wave] sum");
  for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", clk[6 + i]);
  fprintf(stderr, " bar1");
  for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", clk[22 + i]);
  fprintf(stderr, "\n");
#endif
}

// the gang variant (k_brent_gang): every live segment's search over the
// co-resident workgroups of its slices.
struct GangTables {
  int32_t* task_seg = nullptr;
  int32_t* task_g = nullptr;
  int T = 0, gmax = 1, grid = 0;
  int64_t P = 0;
  double* part = nullptr;
  int* tag = nullptr;
  int* abort = nullptr;
  long long timeout = 0;
};

// next tag epoch of the gang exchange: the tags are cleared when their
// buffer is new -- another pointer, or the same pointer handed out again by
// a grown allocation (scratch frees and reallocates: the grown tail would
// hold stale device words), i.e. another (pointer, capacity) -- or the epoch
// wraps (tag = epoch << 10 | evaluation + 1). The whole allocation is
// cleared, so a later call with another layout (S, gmax) inside the same
// allocation only ever finds zeros or tags of older epochs.
int gang_next_epoch(h3d_ctx* ctx, const GangTables& g, int S) {
  const size_t cap = ctx->bufs["gang_tag"].second;
  if (ctx->gang_tag_buf != (void*)g.tag || ctx->gang_tag_cap != cap ||
      ctx->gang_epoch >= (1 << 20)) {
    const size_t bytes = std::max(cap, (size_t)2 * S * g.gmax * 4);
    if (hipMemsetAsync(g.tag, 0, bytes, ctx->stream) != hipSuccess) return -1;
    ctx->gang_tag_buf = (void*)g.tag;
    ctx->gang_tag_cap = cap;
    ctx->gang_epoch = 0;
  }
  return ++ctx->gang_epoch;
}

// spin bound of a gang wait: 0.5 s of the constant-rate wall clock
long long gang_timeout(h3d_ctx* ctx) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) !=
          hipSuccess ||
      khz <= 0)
    khz = 100000;
  return (long long)khz * 500;
}

// room for n_tasks tasks and the exchange of S segments in g->gmax slices
int gang_buffers(h3d_ctx* ctx, GangTables* g, size_t n_tasks, int S) {
  Scratch sc{ctx};
  g->task_seg = sc.get<int32_t>("gang_seg", n_tasks);
  g->task_g = sc.get<int32_t>("gang_g", n_tasks);
  g->part = sc.get<double>("gang_part", (size_t)2 * S * g->gmax);
  g->tag = sc.get<int>("gang_tag", (size_t)2 * S * g->gmax);
  g->abort = sc.get<int>("gang_abort", 1);
  return sc.ok ? 0 : fail(H3D_ENOMEM, "gang tables");
}

// The host-built gang tables (H3D_BRENT=2: every search in gangs). Returns 1
// (nothing set up) when a gang would not fit the resident grid.
template <int M>
int gang_setup(h3d_ctx* ctx, const std::vector<int64_t>& seg_start, int D, int C,
               GangTables* g) {
  g->grid = ctx->n_cu * resident_blocks(ctx, k_brent_gang<M>, kGangThreads);
  int64_t total = 0;
  for (int d = 0; d < D; ++d) total += (seg_start[d + 1] - seg_start[d]) * C;
  // slices: about two resident grids of them over the whole call, at least
  // 1024 pixels (4 per thread)
  int64_t P = (total + 2 * (int64_t)g->grid - 1) / (2 * (int64_t)g->grid);
  P = std::max<int64_t>(1024, (P + kGangThreads - 1) / kGangThreads * kGangThreads);
  std::vector<int32_t> ts, tg;
  int gmax = 1;
  for (int d = 0; d < D; ++d) {
    const int64_t np = seg_start[d + 1] - seg_start[d];
    if (np == 0) continue;
    const int G = (int)((np + P - 1) / P);
    if (G > g->grid) return 1;  // cannot be co-resident: plain k_brent
    gmax = std::max(gmax, G);
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < G; ++j) {
        ts.push_back(d * C + c);
        tg.push_back(j);
      }
  }
  const int S = D * C;
  g->T = (int)ts.size();
  g->gmax = gmax;
  g->P = P;
  if (int rc = gang_buffers(ctx, g, std::max<size_t>(1, ts.size()), S)) return rc;
  if (g->T) {
    HIP_TRY(hipMemcpyAsync(g->task_seg, ts.data(), ts.size() * 4, hipMemcpyHostToDevice,
                           ctx->stream));
    HIP_TRY(hipMemcpyAsync(g->task_g, tg.data(), tg.size() * 4, hipMemcpyHostToDevice,
                           ctx->stream));
  }
  HIP_TRY(hipMemsetAsync(g->abort, 0, 4, ctx->stream));
  // the host vectors die here: the copies must have read them
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  g->timeout = gang_timeout(ctx);
  return 0;
}

// Device-built gang tables (the dev_tables path, no host sync): the slice
// size from the call's pixel count alone -- about two resident grids of
// slices over all segments, at least 1024 pixels, and few enough slices per
// segment to be co-resident (G <= grid) --, room for the task table
// (k_disp_tables fills it) and the exchange buffers sized for the largest
// possible segment (all n pixels).
template <int M>
int gang_setup_dev(h3d_ctx* ctx, int64_t n, int D, int C, GangTables* g) {
  g->grid = ctx->n_cu * resident_blocks(ctx, k_brent_gang<M>, kGangThreads);
  const int64_t total = n * C;
  int64_t P = (total + 2 * (int64_t)g->grid - 1) / (2 * (int64_t)g->grid);
  P = std::max<int64_t>(P, (n + g->grid - 1) / g->grid);
  P = std::max<int64_t>(1024, (P + kGangThreads - 1) / kGangThreads * kGangThreads);
  if (ctx->gang_px > 0)
    P = std::max<int64_t>(std::max<int64_t>(64, ctx->gang_px), (n + g->grid - 1) / g->grid);
  g->P = P;
  g->gmax = (int)std::max<int64_t>(1, (n + P - 1) / P);
  g->T = (int)std::min<int64_t>(INT32_MAX, (int64_t)C * (g->gmax + D));
  const int S = D * C;
  if (int rc = gang_buffers(ctx, g, (size_t)g->T, S)) return rc;
  // (task_seg's tail and abort are set by k_disp_tables, which fills the
  // table)
  g->timeout = gang_timeout(ctx);
  return 0;
}

template <int M, bool kFull = false>
void launch_brent_gang(h3d_ctx* ctx, const double* pd, int64_t n, const int64_t* seg_start,
                       int S, int C, const int32_t* rep_idx, const int32_t* n_rep,
                       SegState* st, const int* seg_flags, double* result, int* queue,
                       const GangTables& g, const int32_t* gate_meta = nullptr,
                       int live_max = 0, bool queue_zeroed = false) {
  ProfScope ps(ctx, "disp_nll", 0);
  if (!queue_zeroed) (void)hipMemsetAsync(queue, 0, sizeof(int), ctx->stream);
  const int epoch = gang_next_epoch(ctx, g, S);
  const int grid = std::max(1, std::min(g.T, g.grid));
  auto k = k_brent_gang<M, kFull>;
  if constexpr (kFull) {
    // the slices and the resident grid were sized for k_brent_gang<M>
    // (gang_setup*; the slice size decides the sum's association, so it is
    // the same for both instantiations): the kFull one runs only where as
    // many of its workgroups are resident
    if (ctx->n_cu * resident_blocks(ctx, k, kGangThreads) < g.grid) k = k_brent_gang<M, false>;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(kGangThreads), 0, ctx->stream, pd,
                     n, seg_start, S, C, rep_idx, n_rep, st, seg_flags, result, queue,
                     g.task_seg, g.task_g, g.T, g.P, g.part, g.tag, g.gmax, g.abort,
                     g.timeout, ctx->work_count, epoch, gate_meta, live_max,
                     ctx->nll_ranges);
}

// algorithmic HBM bytes of the disp_work launches so far: an equalize
// pixel-replicate reads raw (4 B) + f (8 B) and writes pseudodata (8 B); an
// NLL pixel-replicate reads pseudodata (8 B)
int64_t disp_work_bytes(h3d_ctx* ctx, bool nll) {
  unsigned long long c[2] = {0, 0};
  if (!ctx->work_count) return 0;
  (void)hipMemcpyAsync(c, ctx->work_count, sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  return nll ? (int64_t)(c[1] * 8ull) : (int64_t)(c[0] * 20ull);
}

// ---------------------------------------------------------------------------
// estimate_disp: the driver. disp_per_dist_core reads as its stages; what
// they share travels in a DispCall.
// ---------------------------------------------------------------------------

// H3D_DEBUG: the first launch error of the estimate_disp driver, by site
void dbg_launch(const char* where) {
  static const bool on = std::getenv("H3D_DEBUG") != nullptr;
  if (!on) return;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fprintf(stderr, "[h3d] launch error at %s: %s\n", where, hipGetErrorString(e));
}

// h3d_estimate_disp_dev's request: the smoothed tables of the result, on the
// device, enqueued behind the result copies
struct TableReq {
  int weighted;
  double frac, aff;
  double* d_tables;
};

struct DispCall {
  h3d_ctx* ctx = nullptr;
  hipStream_t s = nullptr;
  // the request
  const int32_t* d_raw = nullptr;
  const double* d_f = nullptr;
  const int32_t* d_dist = nullptr;
  int64_t n = 0;
  int R = 0, C = 0, D = 0;
  h3d_allreduce_fn reduce = nullptr;
  void* user = nullptr;
  const TableReq* treq = nullptr;
  // the plan: S segments, the kernels' replicate slot width and whether
  // every condition fills it (with_width)
  int S = 0, mslot = 0;
  bool nll_full = false;
  std::vector<int> nrep;
  std::vector<int32_t> rep_idx;
  // The per-call tables built on the device (k_disp_tables), no host sync
  // before the qcml loop: a single rank with pixels, unless H3D_BRENT=2 asks
  // for gangs throughout (their task table the host builds from the segment
  // bounds). Any number of live segments: the Brent mode is chosen on the
  // device per qcml iteration (dual). The host builds the tables for the
  // multi-rank driver, a call without pixels and H3D_BRENT=2.
  bool dev_tables = false;
  // dev_tables with H3D_BRENT=1: k_brent and k_brent_gang are both launched
  // every qcml iteration and the DEVICE picks one by the live-segment count
  // (one workgroup per segment while they fill the CUs, gangs for the tail
  // iterations, whose few live segments left most CUs idle: cfg2's fourth
  // iteration ran ~55 searches on 55 CUs for 0.36 ms); the gang task table
  // comes from k_disp_tables. Cleared when a gang aborts.
  bool dual = false;
  HostStamps stamp;
  // the pixels sorted by distance, replicate-major rows; pseudodata
  int32_t* raw_s = nullptr;
  double *f_s = nullptr, *pd = nullptr;
  // H3D_EQ_GATHER on the packed path of the single-rank driver: the prep
  // only sorts, and the first equalize launch gathers the rows itself, from
  // every condition's sort order (perm + c n) and packed records (packed +
  // c n); gather_rows is cleared once that launch is enqueued
  bool gather_rows = false;
  const int32_t* perm = nullptr;
  const CondPack2* packed = nullptr;
  int64_t* d_seg = nullptr;         // D + 1 segment bounds
  std::vector<int64_t> seg_start;   // their host copy (host-built tables)
  // chunk and segment tables, work list, per-segment state and results
  int n_chunks = 0;
  size_t max_items = 0;
  int64_t *d_cs = nullptr, *d_lpx = nullptr;
  int32_t *d_cl = nullptr, *d_cd = nullptr, *d_scb = nullptr, *d_sce = nullptr;
  int32_t *d_nrep = nullptr, *d_repidx = nullptr;
  SegState* d_st = nullptr;
  int32_t *d_list = nullptr, *d_meta = nullptr, *d_slb = nullptr, *d_sle = nullptr;
  double *d_partial = nullptr, *d_total = nullptr, *d_res = nullptr;
  int *d_flags = nullptr, *d_bad = nullptr, *d_queue = nullptr;
  GangTables gang;
  // the pinned result zone (ctx->h_res): dispersions, final states, the
  // device's distance check; h_meta: the polled work meta
  int32_t* h_meta = nullptr;
  double* h_resd = nullptr;
  SegState* h_sst = nullptr;
  int* h_bad = nullptr;
  bool have_res = false;  // the results of the final poll are in h_res
  // the prep's profile scope: it ends with sort_and_gather, or -- a forked
  // prep -- behind the join
  std::optional<ProfScope> prep_scope;
  // the prep's side branch (conditions 1 .. C-1 on ctx->prep_side) has not
  // joined s yet
  bool forked = false;
  // The side branch back into s (nothing to do unless forked): s waits for
  // all that the side stream holds, then disp_prep ends. The destructor
  // joins on every path out of the call that did not get there, so no
  // side-stream kernel outlives the call's claim on the scratch; where the
  // wait cannot be enqueued, the host waits for the side stream instead.
  void join_prep() {
    if (forked) {
      forked = false;
      if (hipEventRecord(ctx->prep_join, ctx->prep_side) != hipSuccess ||
          hipStreamWaitEvent(s, ctx->prep_join, 0) != hipSuccess)
        (void)hipStreamSynchronize(ctx->prep_side);
    }
    prep_scope.reset();
  }
  DispCall() = default;
  DispCall(const DispCall&) = delete;
  DispCall& operator=(const DispCall&) = delete;
  ~DispCall() { join_prep(); }
};

// the equalize pass (heavy: q2qnbinom) over the active work list, then
// (NLL: the multi-rank driver) the NLL-only pass (light)
// (kFull: every condition has exactly M replicates -- k_disp_work's
// replicate count is the constant M, see k_brent)
// (c.gather_rows: the call's first equalize launch, which gathers the rows it
// works on -- k_disp_work's kGather -- and leaves them for the later ones)
template <int M, bool NLL, bool kFull = false>
void launch_disp_work(DispCall& c) {
  h3d_ctx* ctx = c.ctx;
  auto launch = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(work_grid(ctx, k, c.max_items)), dim3(kBlock), 0, c.s, c.raw_s,
                       c.f_s, c.pd, c.n, c.d_cs, c.d_cl, c.d_cd, c.C, c.d_repidx, c.d_nrep,
                       c.d_st, c.d_flags, c.d_list, c.d_meta, c.d_partial, ctx->eq_static8,
                       c.perm, c.packed);
  };
  {
    ProfScope ps(ctx, "disp_work", 0, 1);
    // the equalize register budget: 4 waves per SIMD up to M = 8 (the sweeps
    // are in DESIGN.md, "Settled switches")
    bool gathered = false;
    if constexpr (M == 2 && !NLL)
      if (c.gather_rows) {
        launch(k_disp_work<M, 4, kEqualize, NLL, kFull, true>);
        c.gather_rows = false;
        gathered = true;
      }
    if (!gathered) launch(k_disp_work<M, (M <= 8 ? 4 : 1), kEqualize, NLL, kFull>);
  }
  if constexpr (NLL) {
    ProfScope ps(ctx, "disp_nll", 0);
    launch(k_disp_work<M, 1, kNll>);
  }
}

// stable radix sort of (key, value) pairs over key bits [begin_bit, end_bit)
// on stream s, its hipcub temp out of the slot tmp_slot
template <typename K>
int radix_sort_pairs(h3d_ctx* ctx, const char* tmp_slot, hipStream_t s, const K* keys_in,
                     K* keys_out, const int32_t* vals_in, int32_t* vals_out, int64_t n,
                     int begin_bit, int end_bit) {
  return cub_call(ctx, tmp_slot, [&](void* tmp, size_t& bytes) {
    return sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (int)n, begin_bit, end_bit,
                      s);
  });
}

// the temp bytes radix_sort_pairs<K> takes for n pairs (reserved ahead of
// the prep's fork: cub_call then finds its slot large enough)
template <typename K>
int radix_sort_temp_bytes(int64_t n, int begin_bit, int end_bit, size_t* bytes) {
  return cub_bytes(
      [&](void* tmp, size_t& b) {
        return sort_pairs(tmp, b, (const K*)nullptr, (K*)nullptr, (const int32_t*)nullptr,
                          (int32_t*)nullptr, (int)n, begin_bit, end_bit, (hipStream_t) nullptr);
      },
      bytes);
}

// The side stream and the two events of a forked prep, created on first use
// (false: they cannot be had, the prep stays on one stream).
bool prep_side_ready(h3d_ctx* ctx) {
  if (!ctx->prep_side &&
      hipStreamCreateWithFlags(&ctx->prep_side, hipStreamNonBlocking) != hipSuccess)
    ctx->prep_side = nullptr;
  if (!ctx->prep_fork &&
      hipEventCreateWithFlags(&ctx->prep_fork, hipEventDisableTiming) != hipSuccess)
    ctx->prep_fork = nullptr;
  if (!ctx->prep_join &&
      hipEventCreateWithFlags(&ctx->prep_join, hipEventDisableTiming) != hipSuccess)
    ctx->prep_join = nullptr;
  const bool ok = ctx->prep_side && ctx->prep_fork && ctx->prep_join;
  if (!ok) (void)hipGetLastError();  // (not this call's error: it runs on one stream)
  return ok;
}

int validate_and_plan(DispCall& c, const int32_t* cond_of_rep, int estimator) {
  h3d_ctx* ctx = c.ctx;
  const int64_t n = c.n;
  if (n < 0 || c.D < 1) return fail(H3D_EARG, "n=%lld D=%d", (long long)n, c.D);
  if (n > 0 && (!c.d_raw || !c.d_f || !c.d_dist)) return fail(H3D_EARG, "null device input");
  if (n >= (int64_t)1 << 31) return fail(H3D_EARG, "n=%lld exceeds 2^31 pixels per call", (long long)n);
  if (estimator != H3D_EST_QCML)
    return fail(H3D_EARG, "estimator %d: only qcml runs on the GPU path (the reference's cml/mme divide an int64 array in place and raise)", estimator);
  if (int rc = check_cond(cond_of_rep, c.R, c.C, &c.nrep, &c.rep_idx)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  if (std::getenv("H3D_DEBUG")) {
    const hipError_t pe = hipGetLastError();
    if (pe != hipSuccess)
      fprintf(stderr, "[h3d] estimate_disp entry: pending HIP error %s\n", hipGetErrorString(pe));
  }
  c.s = ctx->stream;
  c.S = c.D * c.C;
  // (an M = 6 instantiation for cfg4's R_c = 6 measured equal to M = 8:
  // 111.5 vs 110.5 ms equalize per step, profiles/r02/q2)
  const int maxnr = *std::max_element(c.nrep.begin(), c.nrep.end());
  c.mslot = maxnr <= 2 ? 2 : maxnr <= 4 ? 4 : maxnr <= 8 ? 8 : maxnr <= 16 ? 16 : 32;
  // every condition has exactly mslot replicates: the kFull instantiations
  // of the equalize pass and the Brent kernels (M = 2 only, see k_brent;
  // H3D_NLL_FULL=0: never)
  c.nll_full = ctx->nll_full && c.mslot == 2 &&
               std::all_of(c.nrep.begin(), c.nrep.end(), [&](int r) { return r == c.mslot; });
  c.dev_tables = !c.reduce && n > 0 && ctx->brent_gang != 2;
  c.dual = c.dev_tables && ctx->brent_gang == 1;
  return 0;
}

// One (distance, max, min count) order per condition: per condition a key
// pass over its replicates' counts, a stable radix sort and a gather of just
// those replicates' rows (profiles/r02/sortab). K = uint32_t while the
// distance fits 16 bits: (distance, 8-bit min / max count codes), sorted over
// end_bit + 16 bits (cfg2: 24 bits, three radix passes). (A stable scatter
// into distance buckets, then each bucket sorted in LDS, gave the same order
// but measured slower: prep 0.55 -> 1.19 ms per cfg2 step, r06aj / r06ak --
// the scatter's 4-byte writes to ~250 buckets are uncoalesced (195 us) and
// the LDS bitonic sorts LDS-bound (555 us); the radix passes stage their
// scatter through LDS.) A distance outside the key's range, a negative one
// included, saturates to the largest code, which is >= D: such pixels sort
// behind every segment and the segment check rejects the call. The segment
// bounds are searched in condition 0's sorted keys (k_seg_bounds). idx_out:
// n entries, or (c.gather_rows) C x n, a sort order per condition that the
// first equalize launch gathers through instead of a gather kernel here.
template <typename K>
int sort_by_condition(DispCall& c, int end_bit, const int32_t* idx_in, int32_t* idx_out) {
  h3d_ctx* ctx = c.ctx;
  hipStream_t s = c.s;
  const int64_t n = c.n;
  const int R = c.R, C = c.C;
  constexpr bool k32 = sizeof(K) == 4;
  const int cbits = k32 ? 16 : 64 - end_bit;
  const int sort_bits = k32 ? end_bit + 16 : 64;
  Scratch sc{ctx};
  int32_t* d_reps = sc.get<int32_t>("sort_reps", (size_t)C * kMaxReps);
  if (!sc.ok) return fail(H3D_ENOMEM, "sort buffers");
  if (int rc = h2d_pinned(ctx, d_reps, c.rep_idx.data(), (size_t)C * kMaxReps * 4, s)) return rc;
  // every condition of <= 2 replicates: one key pass for all of them, and
  // the gathers read its packed (raw, f) records -- one 32-byte sector per
  // pixel instead of a raw and an f line (k_dist_cond_keys_pack2)
  const bool pack = k32 && c.mslot == 2;
  int32_t* d_nrep = nullptr;
  CondPack2* packed = nullptr;
  // c.gather_rows (sort_and_gather, implies pack): the prep only sorts, each
  // condition into a sort order of its own (idx_out + c n), which with the
  // records stays as it is until the first equalize launch has gathered
  // through it (k_disp_work's kGather)
  const bool fused = c.gather_rows;
  if (pack) {
    d_nrep = sc.get<int32_t>("sort_nrep", (size_t)C);
    packed = sc.get<CondPack2>("cond_pack2", (size_t)C * n);
    if (!sc.ok) return fail(H3D_ENOMEM, "packed gather rows");
    if (int rc = h2d_pinned(ctx, d_nrep, c.nrep.data(), (size_t)C * 4, s)) return rc;
  }
  K* keys = sc.template get<K>("dkeys", (pack ? (size_t)C : 1) * n);
  K* keys_s = sc.template get<K>("dkeys_s", n);
  if (!sc.ok) return fail(H3D_ENOMEM, "sort keys");
  // A branch of the prep: its stream and what its conditions, one after the
  // other, write. idx_in, the packed records and their per-condition keys
  // are only read after the key pass and are shared; the unpacked path's one
  // key buffer is rewritten per condition, so the side branch has its own.
  struct Branch {
    hipStream_t s;
    K *keys, *keys_s;
    int32_t* idx_out;
    const char* tmp_slot;
  };
  const Branch main{s, keys, keys_s, idx_out, "cub_tmp"};
  Branch side = main;
  // H3D_PREP_STREAMS=2: conditions 1 .. C-1 on the side stream. Every buffer
  // of both branches, the hipcub temps included, is taken here, before the
  // fork: no slot is regrown while a stream works on it. Without the extra
  // buffers (or the stream) the prep stays on one stream, and so does a call
  // of more than kPrepForkMaxPx pixels: the overlap wins a fixed amount per
  // call (the sorts' short fill and histogram kernels, k_seg_bounds, launch
  // gaps) and loses in proportion to n, since sort passes and gathers that
  // each fill the chip slow each other down. Parent
  // against two streams, prep per step: cfg2 (3.8 M pixels) 0.60 -> 0.51 ms,
  // cfg4 (13 M, C = 3) 5.61 -> 5.44, cfg3 (46 M) 5.73 -> 6.04 (r10b).
  constexpr int64_t kPrepForkMaxPx = (int64_t)1 << 24;
  bool two = ctx->prep_streams == 2 && C > 1 && n <= kPrepForkMaxPx;
  if (two) {
    Scratch sb{ctx};
    size_t tmp_bytes = 0;
    side.keys_s = sb.template get<K>("dkeys_s_b", n);
    if (!fused) side.idx_out = sb.template get<int32_t>("idx_out_b", n);
    if (!pack) side.keys = sb.template get<K>("dkeys_b", n);
    side.tmp_slot = "cub_tmp_b";
    two = sb.ok && radix_sort_temp_bytes<K>(n, 0, sort_bits, &tmp_bytes) == 0 &&
          scratch(ctx, main.tmp_slot, tmp_bytes) && scratch(ctx, side.tmp_slot, tmp_bytes) &&
          prep_side_ready(ctx);
    if (two) {
      side.s = ctx->prep_side;
    } else {
      (void)hipGetLastError();  // (a failed allocation is not this call's error)
      side = main;
    }
  }
  auto key_pass = [&](int cc, const Branch& b) {
    if (!pack)
      hipLaunchKernelGGL(k_dist_cond_keys<K>, dim3(grid_for(ctx, n)), dim3(kBlock), 0, b.s,
                         c.d_dist, c.d_raw, n, R, d_reps + cc * kMaxReps, c.nrep[cc], cbits,
                         b.keys);
    else if (cc == 0)  // (pack implies K = uint32_t)
      hipLaunchKernelGGL(k_dist_cond_keys_pack2, dim3(grid_for(ctx, n)), dim3(kBlock), 0, b.s,
                         c.d_dist, c.d_raw, c.d_f, n, R, C, d_reps, d_nrep,
                         reinterpret_cast<uint32_t*>(keys), packed);
  };
  auto sort_gather = [&](int cc, const Branch& b) -> int {
    const K* keys_c = pack ? keys + (size_t)cc * n : b.keys;
    int32_t* perm_c = fused ? idx_out + (size_t)cc * n : b.idx_out;
    if (int rc = radix_sort_pairs<K>(ctx, b.tmp_slot, b.s, keys_c, b.keys_s, idx_in, perm_c, n, 0,
                                     sort_bits))
      return rc;
    SoaRows rows;
    for (int j = 0; j < c.nrep[cc]; ++j) {
      const int r = c.rep_idx[(size_t)cc * kMaxReps + j];
      rows.raw[j] = c.raw_s + (size_t)r * n;
      rows.f[j] = c.f_s + (size_t)r * n;
    }
    if (fused) {
      // (no gather here: the first equalize launch fills the rows)
    } else if (pack) {
      hipLaunchKernelGGL(k_gather_pack2, dim3(grid_for(ctx, n)), dim3(kBlock), 0, b.s, perm_c,
                         packed + (size_t)cc * n, n, c.nrep[cc], rows);
    } else {
      const int64_t tiles = (n + kGatherTile - 1) / kGatherTile;
      const int grid =
          (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)ctx->n_cu * 8));
      hipLaunchKernelGGL(k_gather_cond_tile, dim3(grid), dim3(256), 0, b.s, perm_c, c.d_raw,
                         c.d_f, n, R, d_reps + cc * kMaxReps, c.nrep[cc], rows);
    }
    // the segment bounds out of condition 0's sorted keys, the distance above
    // their cbits count bits, before the branch's next sort rewrites them
    if (cc == 0)
      hipLaunchKernelGGL(k_seg_bounds<K>, dim3((c.D + 1 + 255) / 256), dim3(256), 0, b.s,
                         (const K*)b.keys_s, n, cbits, c.D, c.d_seg);
    return 0;
  };
  key_pass(0, main);
  if (two) {
    // the fork: the side stream starts behind k_iota, the design uploads and
    // the (first) key pass; c.join_prep() brings it back
    HIP_TRY(hipEventRecord(ctx->prep_fork, s));
    HIP_TRY(hipStreamWaitEvent(ctx->prep_side, ctx->prep_fork, 0));
    c.forked = true;
  }
  if (int rc = sort_gather(0, main)) return rc;
  for (int cc = 1; cc < C; ++cc) {
    key_pass(cc, side);
    if (int rc = sort_gather(cc, side)) return rc;
  }
  if (fused) {
    c.perm = idx_out;
    c.packed = packed;
  }
  return 0;
}

// Stage (n > 0): the pixels sorted by distance into SoA rows (gather_rows:
// their sort orders, the rows left to the first equalize launch), the
// segment bounds, and -- host-built tables -- the bounds on the host, checked.
int sort_and_gather(DispCall& c) {
  h3d_ctx* ctx = c.ctx;
  const int64_t n = c.n;
  const int R = c.R, D = c.D;
  // disp_prep ends with this stage; a forked prep's side branch may run on
  // under the table kernels, and the scope stays open until it has joined
  // (start_qcml): it measures the critical path on the call's stream
  c.prep_scope.emplace(ctx, "disp_prep", n);
  struct ScopeEnd {
    DispCall& c;
    ~ScopeEnd() {
      if (!c.forked) c.prep_scope.reset();
    }
  } scope_end{c};
  Scratch sc{ctx};
  int end_bit = 1;
  while ((1 << end_bit) <= D) ++end_bit;
  // H3D_EQ_GATHER: on the packed path (32-bit keys, <= 2 replicates per
  // condition) of the single-rank driver the prep only sorts, into one sort
  // order per condition, and the first equalize launch gathers
  c.gather_rows = ctx->eq_gather && !c.reduce && end_bit <= 16 && c.mslot == 2;
  int32_t* idx_in = sc.get<int32_t>("idx_in", n);
  int32_t* idx_out = c.gather_rows ? sc.get<int32_t>("cond_perm", (size_t)c.C * n)
                                   : sc.get<int32_t>("idx_out_c", n);
  c.raw_s = sc.get<int32_t>("raw_s", n * R);
  c.f_s = sc.get<double>("f_s", n * R);
  c.pd = sc.get<double>("pd", n * R);
  c.d_seg = sc.get<int64_t>("seg_start", D + 1);
  if (!sc.ok) return fail(H3D_ENOMEM, "device allocation failed (n=%lld)", (long long)n);
  launch_iota(ctx, c.s, idx_in, n);
  if (int rc = end_bit <= 16 ? sort_by_condition<uint32_t>(c, end_bit, idx_in, idx_out)
                             : sort_by_condition<uint64_t>(c, end_bit, idx_in, idx_out))
    return rc;
  c.stamp("prep launched");
  if (c.dev_tables) return 0;  // k_disp_tables checks the bounds
  HIP_TRY(hipMemcpyAsync(c.seg_start.data(), c.d_seg, (D + 1) * 8, hipMemcpyDeviceToHost, c.s));
  HIP_TRY(hipStreamSynchronize(c.s));
  if (c.seg_start[0] != 0 || c.seg_start[D] != n) {
    c.stamp("seg_start synced (dist check failed)");
    // pixels with dist < 0 or >= D
    return fail(H3D_EARG, "dist outside [0, %d)", D);
  }
  return 0;
}

// the chunk and segment tables the host builds from the segment bounds
struct HostTables {
  std::vector<int64_t> cs, lpx;
  std::vector<int32_t> cl, cd, scb, sce;
  std::vector<SegState> st;
};

int host_tables(DispCall& c, HostTables* t) {
  h3d_ctx* ctx = c.ctx;
  const int D = c.D, C = c.C, S = c.S;
  const std::vector<int64_t>& seg_start = c.seg_start;
  t->scb.resize(D);
  t->sce.resize(D);
  for (int d = 0; d < D; ++d) {
    t->scb[d] = (int32_t)t->cl.size();
    for (int64_t a = seg_start[d]; a < seg_start[d + 1]; a += kChunk) {
      t->cs.push_back(a);
      t->cl.push_back((int32_t)std::min<int64_t>(kChunk, seg_start[d + 1] - a));
      t->cd.push_back(d);
    }
    t->sce[d] = (int32_t)t->cl.size();
  }
  c.n_chunks = (int)t->cl.size();
  if (c.n_chunks == 0) {
    // (n = 0: the staging below keeps room for one chunk and copies it)
    t->cs.push_back(0);
    t->cl.push_back(0);
    t->cd.push_back(0);
  }
  // pixel counts per segment: this rank's, and over all ranks
  t->lpx.resize(S);
  for (int d = 0; d < D; ++d)
    for (int cc = 0; cc < C; ++cc) t->lpx[d * C + cc] = seg_start[d + 1] - seg_start[d];
  std::vector<double> cnt(t->lpx.begin(), t->lpx.end());
  Scratch sc{ctx};
  double* d_cnt = sc.get<double>("seg_cnt", S);
  if (!sc.ok) return fail(H3D_ENOMEM, "seg_cnt");
  if (c.reduce) {
    HIP_TRY(hipMemcpyAsync(d_cnt, cnt.data(), S * 8, hipMemcpyHostToDevice, c.s));
    if (c.reduce(d_cnt, S, c.user)) return fail(H3D_EHIP, "allreduce callback failed");
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, S * 8, hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
  }
  t->st.resize(S);
  for (int sg = 0; sg < S; ++sg)
    seg_init(&t->st[sg], (long long)cnt[sg], c.nrep[sg % C], ctx->qcml_tol);
  return 0;
}

// Stage: the per-call tables on the device -- host-built and uploaded, or
// (dev_tables) only the design uploaded and the rest built by k_disp_tables
// -- and the scratch of the qcml loop.
int segment_tables(DispCall& c) {
  h3d_ctx* ctx = c.ctx;
  hipStream_t s = c.s;
  const int D = c.D, C = c.C, S = c.S;
  HostTables t;
  if (c.dev_tables)
    c.n_chunks = (int)std::min<int64_t>(c.n / kChunk + D + 1, INT32_MAX);  // an upper bound
  else if (int rc = host_tables(c, &t))
    return rc;
  // the tables go up as ONE copy from a pinned staging buffer (nine pageable
  // copies cost ~0.3 ms of host-side gaps per cfg2 step: each staged and
  // launched its own blit)
  std::vector<int32_t> nrep32(c.nrep.begin(), c.nrep.end());
  struct Part {
    const void* src;
    size_t bytes, off;
  };
  // (dev_tables: the chunk / segment tables are k_disp_tables' outputs, only
  // their room is reserved and nothing of them is copied)
  const size_t nch = (size_t)std::max(c.n_chunks, 1);
  Part parts[] = {{t.cs.data(), nch * 8, 0},
                  {t.cl.data(), nch * 4, 0},
                  {t.cd.data(), nch * 4, 0},
                  {t.scb.data(), (size_t)D * 4, 0},
                  {t.sce.data(), (size_t)D * 4, 0},
                  {nrep32.data(), (size_t)C * 4, 0},
                  {c.rep_idx.data(), c.rep_idx.size() * 4, 0},
                  {t.st.data(), (size_t)S * sizeof(SegState), 0},
                  {t.lpx.data(), (size_t)S * 8, 0}};
  size_t blob = 0;
  for (Part& q : parts) {
    q.off = blob;
    blob += (q.bytes + 255) & ~(size_t)255;
  }
  // the parts that go up: all of them, or (dev_tables) nrep + rep_idx only
  const int q_lo = c.dev_tables ? 5 : 0, q_hi = c.dev_tables ? 7 : 9;
  const size_t up_lo = parts[q_lo].off, up_hi = q_hi < 9 ? parts[q_hi].off : blob;
  if (!ctx->h_stage_done)
    HIP_TRY(hipEventCreateWithFlags(&ctx->h_stage_done, hipEventDisableTiming));
  else
    HIP_TRY(hipEventSynchronize(ctx->h_stage_done));  // the previous copy has read it
  if (int rc = ctx->h_stage.grow(blob)) return rc;
  Scratch sc{ctx};
  char* d_blob = sc.get<char>("disp_tables", blob);
  if (!sc.ok) return fail(H3D_ENOMEM, "disp tables");
  char* h_stage = (char*)ctx->h_stage.p;
  for (int qi = q_lo; qi < q_hi; ++qi)
    if (parts[qi].bytes) std::memcpy(h_stage + parts[qi].off, parts[qi].src, parts[qi].bytes);
  HIP_TRY(hipMemcpyAsync(d_blob + up_lo, h_stage + up_lo, up_hi - up_lo,
                         hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(ctx->h_stage_done, s));
  c.d_cs = (int64_t*)(d_blob + parts[0].off);
  c.d_cl = (int32_t*)(d_blob + parts[1].off);
  c.d_cd = (int32_t*)(d_blob + parts[2].off);
  c.d_scb = (int32_t*)(d_blob + parts[3].off);
  c.d_sce = (int32_t*)(d_blob + parts[4].off);
  c.d_nrep = (int32_t*)(d_blob + parts[5].off);
  c.d_repidx = (int32_t*)(d_blob + parts[6].off);
  c.d_st = (SegState*)(d_blob + parts[7].off);
  c.d_lpx = (int64_t*)(d_blob + parts[8].off);
  c.max_items = nch * C;
  c.d_list = sc.get<int32_t>("work_list", c.max_items);
  // len, active, eq_len, live; k_disp_work's task heads (kTaskHeadStride apart)
  c.d_meta = sc.get<int32_t>("work_meta", kWorkMetaInts);
  c.d_slb = sc.get<int32_t>("seg_lb", S);
  c.d_sle = sc.get<int32_t>("seg_le", S);
  c.d_partial = sc.get<double>("partial", c.max_items * kWavesPerBlock);
  c.d_total = sc.get<double>("seg_total", S);
  c.d_flags = sc.get<int>("seg_flags", S);
  c.d_res = sc.get<double>("seg_result", S);
  c.d_bad = sc.get<int>("dist_bad", 1);
  if (!sc.ok) return fail(H3D_ENOMEM, "disp scratch");
  if (!c.dev_tables) {
    HIP_TRY(hipMemsetAsync(c.d_flags, 0, S * 4, s));  // else k_disp_tables
  } else {
    if (c.dual)
      if (int rc = with_width(c.mslot, false, [&](auto m, auto) {
            return gang_setup_dev<decltype(m)::value>(ctx, c.n, D, C, &c.gang);
          }))
        return rc;
    hipLaunchKernelGGL(k_disp_tables, dim3(1), dim3(1024), 0, s, c.d_seg, D, C, c.n, c.d_nrep,
                       c.d_cs, c.d_cl, c.d_cd, c.d_scb, c.d_sce, c.d_st, c.d_lpx, c.d_bad,
                       c.dual ? c.gang.P : (int64_t)1, c.dual ? c.gang.task_seg : nullptr,
                       c.dual ? c.gang.task_g : nullptr, ctx->qcml_tol, c.dual ? c.gang.T : 0,
                       c.d_flags, c.dual ? c.gang.abort : nullptr);
    dbg_launch("k_disp_tables");
  }
  c.stamp("tables uploaded");
  return 0;
}

// k_seg_update: (step, multi-rank) advances every active segment's state
// machine with its reduced total, then rebuilds the active work list; init:
// the first list of a call. It also zeroes the single-rank Brent kernels'
// work queues.
void launch_seg_update(DispCall& c, int init, int step) {
  ProfScope ps(c.ctx, "disp_update", 0, init ? 3 : 2);  // (the first list is not timed)
  hipLaunchKernelGGL(k_seg_update, dim3(1), dim3(1024), 0, c.s, c.d_st, c.d_total, c.d_flags,
                     c.S, c.C, c.d_nrep, c.d_scb, c.d_sce, c.d_list, c.d_slb, c.d_sle, c.d_res,
                     c.d_meta, init, step, c.d_lpx, c.ctx->work_count,
                     step ? nullptr : c.d_queue, c.dual ? c.gang.P : (int64_t)1,
                     c.dual ? c.gang.task_seg : nullptr, c.dual ? c.gang.task_g : nullptr);
}

// Stage: the first active list and the pinned zone the results land in.
int start_qcml(DispCall& c) {
  h3d_ctx* ctx = c.ctx;
  Scratch sc{ctx};
  c.d_queue = sc.get<int>("brent_queue", 2);
  if (!sc.ok) return fail(H3D_ENOMEM, "brent queue");
  launch_seg_update(c, 1, 0);
  // the join of a forked prep: k_disp_tables, the table upload, the gang
  // setup and the list above need only the segment bounds; the equalize pass
  // that comes next reads every condition's rows (gather_rows: its sort
  // order)
  c.join_prep();
  if (!ctx->h_meta) HIP_TRY(hipHostMalloc((void**)&ctx->h_meta, 32, hipHostMallocDefault));
  c.h_meta = ctx->h_meta;
  const size_t res_bytes = (size_t)c.S * 8 + (size_t)c.S * sizeof(SegState) + 8;
  if (int rc = ctx->h_res.grow(res_bytes)) return rc;
  c.h_resd = (double*)ctx->h_res.p;
  c.h_sst = (SegState*)(c.h_resd + c.S);
  c.h_bad = (int*)(c.h_sst + c.S);
  *c.h_bad = 0;
  return 0;
}

// the results into the pinned zone (enqueued; the caller waits)
hipError_t copy_results(DispCall& c) {
  hipError_t e = hipMemcpyAsync(c.h_resd, c.d_res, (size_t)c.S * 8, hipMemcpyDeviceToHost, c.s);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c.h_sst, c.d_st, (size_t)c.S * sizeof(SegState), hipMemcpyDeviceToHost,
                       c.s);
  if (e == hipSuccess && c.dev_tables)
    e = hipMemcpyAsync(c.h_bad, c.d_bad, 4, hipMemcpyDeviceToHost, c.s);
  return e;
}

// One poll of the single-rank loop: the live-segment count and,
// speculatively, what follows a final poll -- the result copies (pinned) and
// the requested smoother behind them, so a final poll costs one host round
// trip (r03s trace: ~0.12 ms of host gaps after the fifth iteration); a poll
// that finds live segments simply runs them, and a later poll redoes both.
int poll_single_rank(DispCall& c, bool gangs) {
  h3d_ctx* ctx = c.ctx;
  hipEvent_t copied = ev_get(ctx);
  int rc = 0;
  if (hipMemcpyAsync(c.h_meta, c.d_meta, 16, hipMemcpyDeviceToHost, c.s) != hipSuccess ||
      (gangs && hipMemcpyAsync(c.h_meta + 4, c.gang.abort, 4, hipMemcpyDeviceToHost, c.s) !=
                    hipSuccess) ||
      copy_results(c) != hipSuccess || hipEventRecord(copied, c.s) != hipSuccess) {
    ctx->event_pool.push_back(copied);
    return fail(H3D_EHIP, "disp round copies failed: %s", hipGetErrorString(hipGetLastError()));
  }
  // (speculatively only where the smoother is the device's, enqueued without
  // a wait; the host smoother of D > kTableMaxD runs once, on the final
  // result -- on an intermediate poll it would block and could reject a
  // table that is not final)
  if (c.treq && c.D <= kTableMaxD)
    rc = h3d_disp_tables_dev(ctx, c.d_res, c.D, c.C, c.treq->weighted, c.treq->frac,
                             c.treq->aff, c.treq->d_tables);
  const hipError_t ce = hipEventSynchronize(copied);
  ctx->event_pool.push_back(copied);
  if (rc) return rc;
  if (ce != hipSuccess) return fail(H3D_EHIP, "disp round sync failed: %s", hipGetErrorString(ce));
  c.have_res = true;
  c.stamp("poll");
  return 0;
}

// Stage, single rank: one equalize pass per qcml iteration over every segment
// that needs one, then k_brent (or gangs, k_brent_gang) runs each such
// segment's whole Brent search in-kernel, then k_seg_update rebuilds the
// equalize list. The host polls the live-segment count every `batch`
// iterations (an iteration with nothing to do costs three empty launches).
int qcml_single_rank(DispCall& c) {
  h3d_ctx* ctx = c.ctx;
  if (c.n == 0) {
    Scratch sc{ctx};
    c.d_seg = sc.get<int64_t>("seg_start", c.D + 1);
    if (!sc.ok) return fail(H3D_ENOMEM, "brent scratch");
    HIP_TRY(hipMemsetAsync(c.d_seg, 0, (c.D + 1) * 8, c.s));
  }
  // H3D_BRENT=2 (host-built tables): every search in gangs
  bool use_gang = ctx->brent_gang == 2 && c.n > 0;
  if (use_gang) {
    const int grc = with_width(c.mslot, false, [&](auto m, auto) {
      return gang_setup<decltype(m)::value>(ctx, c.seg_start, c.D, c.C, &c.gang);
    });
    if (grc == 1) use_gang = false;
    else if (grc) return grc;
  }
  // first poll after 5 iterations (cfg2's searches end after 5; a poll is a
  // host sync plus the relaunch latency, ~50 us of idle GPU -- r03 host
  // stamps), then every 2
  int rounds = 0, batch = 5;
  while (true) {
    for (int b = 0; b < batch; ++b) {
      dbg_launch("before qcml iteration");
      with_width(c.mslot, c.nll_full, [&](auto m, auto full) {
        constexpr int M = decltype(m)::value;
        constexpr bool kFull = decltype(full)::value;
        auto brent = [&](const int32_t* gate_meta, int live_min, const int* gang_abort) {
          launch_brent<M, kFull>(ctx, c.pd, c.n, c.d_seg, c.S, c.C, c.d_repidx, c.d_nrep,
                                 c.d_st, c.d_flags, c.d_res, c.d_queue, gate_meta, live_min,
                                 gang_abort, true);
        };
        auto gang = [&](const int32_t* gate_meta, int live_max) {
          launch_brent_gang<M, kFull>(ctx, c.pd, c.n, c.d_seg, c.S, c.C, c.d_repidx, c.d_nrep,
                                      c.d_st, c.d_flags, c.d_res, c.d_queue + 1, c.gang,
                                      gate_meta, live_max, true);
        };
        launch_disp_work<M, false, kFull>(c);
        dbg_launch("equalize");
        if (c.dual) {
          brent(c.d_meta, ctx->n_cu, c.gang.abort);
          dbg_launch("k_brent (dual)");
          gang(c.d_meta, ctx->n_cu);
          dbg_launch("k_brent_gang (dual)");
        } else if (use_gang) {
          gang(nullptr, 0);
        } else {
          brent(nullptr, 0, nullptr);
        }
      });
      launch_seg_update(c, 0, 0);
      ++rounds;
    }
    const bool gangs = use_gang || c.dual;
    if (int rc = poll_single_rank(c, gangs)) return rc;
    if (std::getenv("H3D_DEBUG"))
      fprintf(stderr, "[h3d] qcml iterations=%d live_segments=%d gang=%d abort=%d\n", rounds,
              c.h_meta[3], use_gang ? 1 : c.dual ? 2 : 0, gangs ? c.h_meta[4] : 0);
    if (c.dual && c.h_meta[4]) {
      // a gang aborted: k_brent (gated on the same flag) already took over
      // the following iterations on the device; launch it alone from here
      c.dual = false;
      ctx->gang_aborts += 1;
    }
    if (use_gang && c.h_meta[4]) {
      // a gang's wait timed out (CUs held elsewhere): its segments stayed
      // in kEqualize and repeat their iteration; finish with k_brent
      use_gang = false;
      ctx->gang_aborts += 1;
      continue;
    }
    if (c.h_meta[3] == 0) return 0;
    if (rounds > 2000) return fail(H3D_ENOCONV, "estimate_disp did not terminate");
    batch = 2;
  }
}

// Stage, multi-rank: per Brent evaluation an equalize / NLL pass, this
// rank's per-segment sums (k_seg_reduce), the cross-rank all-reduce, and
// k_seg_update stepping the (identical) state machines. Polled after 2, 4,
// then every 8 rounds.
int qcml_multi_rank(DispCall& c) {
  int rounds = 0, batch = 2;
  while (true) {
    for (int b = 0; b < batch; ++b) {
      // every width the single-rank driver picks (mslot 2 fell through to
      // the M = 32 instantiation here: 13.1 vs 5.5 ms of equalize per cfg2
      // step, bench --noop-reduce)
      with_width(c.mslot, false,
                 [&](auto m, auto) { launch_disp_work<decltype(m)::value, true>(c); });
      {
        ProfScope ps(c.ctx, "disp_reduce", 0);
        hipLaunchKernelGGL(k_seg_reduce, dim3((c.S + 3) / 4), dim3(256), 0, c.s, c.d_partial,
                           c.d_slb, c.d_sle, c.S, c.d_total, nullptr, c.d_flags, c.d_nrep, c.C,
                           c.d_res);
      }
      if (c.reduce(c.d_total, c.S, c.user)) return fail(H3D_EHIP, "allreduce callback failed");
      launch_seg_update(c, 0, 1);
      ++rounds;
    }
    if (hipMemcpyAsync(c.h_meta, c.d_meta, 16, hipMemcpyDeviceToHost, c.s) != hipSuccess ||
        hipStreamSynchronize(c.s) != hipSuccess)
      return fail(H3D_EHIP, "disp round sync failed: %s", hipGetErrorString(hipGetLastError()));
    if (std::getenv("H3D_DEBUG"))
      fprintf(stderr, "[h3d] disp rounds=%d active_items=%d live_segments=%d\n", rounds,
              c.h_meta[1], c.h_meta[3]);
    // terminate on the genome-wide live-segment count (identical on every
    // rank), not on this rank's own work-list length: a rank without pixels
    // in the still-active segments must keep joining the collective reduce
    if (c.h_meta[3] == 0) return 0;
    if (rounds > 200000) return fail(H3D_ENOCONV, "estimate_disp did not terminate");
    batch = std::min(batch * 2, 8);
  }
}

// Stage: the results to the caller, the kernels' status, the smoother.
int collect_results(DispCall& c, double* disp_per_dist, int32_t* seg_flags_out) {
  h3d_ctx* ctx = c.ctx;
  const TableReq* treq = c.treq;
  // a launch error of the qcml loop is this call's, not a later call's
  HIP_TRY(hipGetLastError());
  if (!c.have_res) {
    // (the multi-rank path) the results into the pinned zone; the smoother
    // runs behind the copies, the host waits for the copies only
    HIP_TRY(copy_results(c));
    hipEvent_t copied = ev_get(ctx);
    HIP_TRY(hipEventRecord(copied, c.s));
    const int trc = treq ? h3d_disp_tables_dev(ctx, c.d_res, c.D, c.C, treq->weighted,
                                               treq->frac, treq->aff, treq->d_tables)
                         : 0;
    const hipError_t e = hipEventSynchronize(copied);
    ctx->event_pool.push_back(copied);
    if (trc) return trc;
    if (e != hipSuccess) return fail(H3D_EHIP, "result copy: %s", hipGetErrorString(e));
  }
  std::memcpy(disp_per_dist, c.h_resd, (size_t)c.S * 8);
  ctx->last_S = c.S;
  c.stamp("results");
  if (c.dev_tables && *c.h_bad) return fail(H3D_EARG, "dist outside [0, %d)", c.D);
  int all = 0;
  for (int sg = 0; sg < c.S; ++sg) {
    all |= c.h_sst[sg].flags;
    if (seg_flags_out) seg_flags_out[sg] = c.h_sst[sg].flags;
  }
  if (const int frc = flags_to_code(all)) return frc;
  if (c.have_res && treq && c.D > kTableMaxD)
    // the host smoother (h3d_disp_tables_dev's D > kTableMaxD branch), once,
    // on the final result
    return h3d_disp_tables_dev(ctx, c.d_res, c.D, c.C, treq->weighted, treq->frac, treq->aff,
                               treq->d_tables);
  return 0;
}

int disp_per_dist_core(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                       const int32_t* d_dist, int64_t n, int R, int C,
                       const int32_t* cond_of_rep, int D, int estimator,
                       double* disp_per_dist, int32_t* seg_flags_out,
                       h3d_allreduce_fn reduce, void* user, const TableReq* treq) {
  if (!ctx || !cond_of_rep || !disp_per_dist) return fail(H3D_EARG, "null argument");
  DispCall c;
  c.ctx = ctx;
  c.d_raw = d_raw;
  c.d_f = d_f;
  c.d_dist = d_dist;
  c.n = n;
  c.R = R;
  c.C = C;
  c.D = D;
  c.reduce = reduce;
  c.user = user;
  c.treq = treq;
  if (int rc = validate_and_plan(c, cond_of_rep, estimator)) return rc;
  c.seg_start.assign(D + 1, 0);
  if (n > 0)
    if (int rc = sort_and_gather(c)) return rc;
  c.stamp("seg_start synced");
  if (int rc = segment_tables(c)) return rc;
  if (int rc = start_qcml(c)) return rc;
  if (int rc = reduce ? qcml_multi_rank(c) : qcml_single_rank(c)) return rc;
  return collect_results(c, disp_per_dist, seg_flags_out);
}

}  // namespace

extern "C" {

int h3d_version(void) { return 1; }

const char* h3d_last_error(void) { return h3derr::last(); }

int h3d_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

h3d_ctx* h3d_open(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    fail(H3D_ENODEV, "no HIP device visible");
    return nullptr;
  }
  if (device < 0 || device >= n) {
    fail(H3D_EARG, "device %d of %d", device, n);
    return nullptr;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    fail(H3D_EHIP, "hipGetDeviceProperties failed");
    return nullptr;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fail(H3D_ENODEV, "device %d is %s, libh3d is built for gfx950", device,
         prop.gcnArchName);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    fail(H3D_EHIP, "hipSetDevice failed");
    return nullptr;
  }
  h3d_ctx* ctx = new h3d_ctx();
  ctx->device = device;
  ctx->n_cu = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    fail(H3D_EHIP, "stream create failed");
    return nullptr;
  }
  ctx->stream = ctx->own;
  if (const char* e = std::getenv("H3D_EQ_STATIC8"))
    ctx->eq_static8 = std::max(0, std::min(8, std::atoi(e)));
  if (const char* e = std::getenv("H3D_BRENT")) ctx->brent_gang = std::atoi(e);
  if (const char* e = std::getenv("H3D_BRENT_LDS_KB")) ctx->brent_lds_kb = std::atoi(e);
  if (const char* e = std::getenv("H3D_NLL_FULL")) ctx->nll_full = std::atoi(e);
  if (const char* e = std::getenv("H3D_NLL_RANGES")) ctx->nll_ranges = std::atoi(e);
  if (const char* e = std::getenv("H3D_PREP_STREAMS")) ctx->prep_streams = std::atoi(e);
  if (const char* e = std::getenv("H3D_EQ_GATHER")) ctx->eq_gather = std::atoi(e);
  if (const char* e = std::getenv("H3D_GANG_P")) ctx->gang_px = std::atoi(e);
  if (hipMalloc((void**)&ctx->work_count, 2 * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(ctx->work_count, 0, 2 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipStreamDestroy(ctx->own);
    delete ctx;
    fail(H3D_ENOMEM, "counter allocation failed");
    return nullptr;
  }
  // The prep's side stream, now rather than with the first fork: HIP maps
  // streams onto a few hardware queues, a stream created once they are all
  // taken shares one, and two streams on one queue run in enqueue order.
  // Created lazily it shared the benchmark's queue with the call's stream
  // (no overlap); a stream that cannot be had now is tried again by the call.
  if (ctx->prep_streams == 2) (void)prep_side_ready(ctx);
  return ctx;
}

void h3d_close(h3d_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->prep_side) (void)hipStreamSynchronize(ctx->prep_side);
  prof_collect(ctx);
  for (auto& kv : ctx->bufs)
    if (kv.second.first) (void)hipFree(kv.second.first);
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  if (ctx->work_count) (void)hipFree(ctx->work_count);
  if (ctx->h_meta) (void)hipHostFree(ctx->h_meta);
  if (ctx->h_stage_done) (void)hipEventDestroy(ctx->h_stage_done);
  if (ctx->bounce_ev) (void)hipEventDestroy(ctx->bounce_ev);
  if (ctx->prep_fork) (void)hipEventDestroy(ctx->prep_fork);
  if (ctx->prep_join) (void)hipEventDestroy(ctx->prep_join);
  if (ctx->prep_side) (void)hipStreamDestroy(ctx->prep_side);
  if (ctx->own) (void)hipStreamDestroy(ctx->own);
  delete ctx;  // (the PinnedBufs free themselves)
}

int h3d_set_stream(h3d_ctx* ctx, void* stream) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  ctx->stream = stream ? (hipStream_t)stream : ctx->own;
  return 0;
}

int h3d_set_qcml_tol(h3d_ctx* ctx, double tol) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (!(tol >= 0.0) || !(tol < INFINITY)) return fail(H3D_EARG, "qcml tol %g", tol);
  ctx->qcml_tol = tol;
  return 0;
}

int h3d_profile_enable(h3d_ctx* ctx, int on) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  prof_collect(ctx);
  ctx->prof = on < 0 ? 0 : on > 2 ? 2 : on;
  return 0;
}

int h3d_profile_reset(h3d_ctx* ctx) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  prof_collect(ctx);
  ctx->stats.clear();
  HIP_TRY(hipMemsetAsync(ctx->work_count, 0, 2 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

// Section clock ticks of the equalize pass (a -DH3D_SECPROF build only,
// h3d_special.h; tools/secprof.py): copies the 32 counters out, then zeroes
// them when reset. Returns -1 (H3D_EARG) in a normal build. Not part of
// include/h3d.h: a measurement hook of profiling builds.
extern "C" int h3d_secprof(int reset, unsigned long long* out32) {
#if defined(H3D_SECPROF)
  if (out32)
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_h3d_secprof), 32 * 8, 0,
                                hipMemcpyDeviceToHost));
  if (reset) {
    static const unsigned long long zeros[32] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_h3d_secprof), zeros, 32 * 8, 0,
                              hipMemcpyHostToDevice));
  }
  return 0;
#else
  (void)reset;
  (void)out32;
  return fail(H3D_EARG, "not a -DH3D_SECPROF build");
#endif
}

int h3d_profile_read(h3d_ctx* ctx, const char* name, double* total_ms,
                     int64_t* launches, int64_t* units) {
  if (!ctx || !name) return fail(H3D_EARG, "null argument");
  prof_collect(ctx);
  if (std::strcmp(name, "gang_aborts") == 0) {
    // gang Brent waits that hit their wall-clock bound (the searches then
    // finished under k_brent): a count over the ctx's life, not a timing
    if (total_ms) *total_ms = 0.0;
    if (launches) *launches = ctx->gang_aborts;
    if (units) *units = 0;
    return 0;
  }
  auto it = ctx->stats.find(name);
  ProfEntry e = (it == ctx->stats.end()) ? ProfEntry() : it->second;
  if (total_ms) *total_ms = e.ms;
  if (launches) *launches = e.launches;
  // disp_work / disp_nll units = algorithmic bytes; lrt / disp_prep = pixels
  if (units)
    *units = std::strcmp(name, "disp_work") == 0   ? disp_work_bytes(ctx, false)
             : std::strcmp(name, "disp_nll") == 0 ? disp_work_bytes(ctx, true)
                                                   : e.units;
  return 0;
}

// ---------------------------------------------------------------------------
// estimate_disp (the driver: disp_per_dist_core, above)
// ---------------------------------------------------------------------------

int h3d_disp_per_dist_dev(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                          const int32_t* d_dist, int64_t n, int R, int C,
                          const int32_t* cond_of_rep, int D, int estimator,
                          double* disp_per_dist, int32_t* seg_flags_out,
                          h3d_allreduce_fn reduce, void* user) {
  return disp_per_dist_core(ctx, d_raw, d_f, d_dist, n, R, C, cond_of_rep, D, estimator,
                            disp_per_dist, seg_flags_out, reduce, user, nullptr);
}

int h3d_estimate_disp_dev(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                          const int32_t* d_dist, int64_t n, int R, int C,
                          const int32_t* cond_of_rep, int D, int weighted, double frac,
                          double auto_frac_factor, double* disp_per_dist,
                          int32_t* seg_flags_out, double* d_tables_out) {
  if (!d_tables_out) return fail(H3D_EARG, "null d_tables_out");
  const TableReq req{weighted, frac, auto_frac_factor, d_tables_out};
  return disp_per_dist_core(ctx, d_raw, d_f, d_dist, n, R, C, cond_of_rep, D, H3D_EST_QCML,
                            disp_per_dist, seg_flags_out, nullptr, nullptr, &req);
}

int h3d_disp_per_dist(h3d_ctx* ctx, const int64_t* raw, const double* f,
                      const int32_t* dist, int64_t n, int R, int C,
                      const int32_t* cond_of_rep, int D, int estimator,
                      double* disp_per_dist, int32_t* seg_flags) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n > 0 && (!raw || !f || !dist)) return fail(H3D_EARG, "null input");
  HIP_TRY(hipSetDevice(ctx->device));
  int32_t* d_raw = nullptr;
  double* d_f = nullptr;
  int32_t* d_dist = nullptr;
  if (n > 0) {  // the counts are checked before the driver starts
    HostCall hc(ctx);
    d_raw = hc.counts(raw, n * R, "raw counts must be in [0, 2^31)");
    d_f = hc.in("in_f", f, n * R);
    d_dist = hc.in("in_dist", dist, n);
    if (int rc = hc.ready("inputs")) return rc;
    if (int rc = hc.finish()) return rc;
  }
  return h3d_disp_per_dist_dev(ctx, d_raw, d_f, d_dist, n, R, C, cond_of_rep, D,
                               estimator, disp_per_dist, seg_flags, nullptr, nullptr);
}

int h3d_disp_table(const double* col, int D, int weighted, double frac,
                   double auto_frac_factor, double* table_out) {
  if (!col || !table_out || D < 1) return fail(H3D_EARG, "null argument / D");
  std::vector<double> x, y, xs(D);
  for (int d = 0; d < D; ++d) {
    xs[d] = d;
    if (std::isfinite(col[d])) {
      x.push_back(d);
      y.push_back(col[d]);
    }
  }
  if (x.size() < 2) return fail(H3D_EARG, "fewer than two finite dispersion points");
  std::vector<double> out;
  int rc;
  if (weighted)
    rc = h3dhost::weighted_lowess_fit_eval(x, y, y[0], frac, auto_frac_factor, xs, &out,
                                           /*pinned_min_weight=*/weighted != 2);
  else
    rc = h3dhost::lowess_fit_eval(x, y, y[0], frac >= 0 ? frac : 0.3, 0.01, xs, &out);
  if (rc) return fail(H3D_ENOCONV, "lowess fit failed (degenerate dispersion table)");
  std::memcpy(table_out, out.data(), D * 8);
  return 0;
}

// every condition's table in one call: (D, C) row-major in and out, one
// host thread per condition (the smoother is serial per condition); one
// ctypes call instead of a Python thread pool, whose dispatch cost more than
// the smoothing (r03: 1.36 ms for two conditions vs 0.75 ms in sequence on
// the container's CPU)
int h3d_disp_tables(const double* disp_per_dist, int D, int C, int weighted,
                    double frac, double auto_frac_factor, double* tables_out) {
  if (!disp_per_dist || !tables_out || D < 1 || C < 1 || C > kMaxConds)
    return fail(H3D_EARG, "null argument / D / C");
  std::vector<std::vector<double>> cols(C, std::vector<double>(D)), outs(C, std::vector<double>(D));
  for (int c = 0; c < C; ++c)
    for (int d = 0; d < D; ++d) cols[c][d] = disp_per_dist[(size_t)d * C + c];
  std::vector<int> rcs(C, 0);
  std::vector<std::string> errs(C);
  auto one = [&](int c) {
    rcs[c] = h3d_disp_table(cols[c].data(), D, weighted, frac, auto_frac_factor,
                            outs[c].data());
    if (rcs[c]) errs[c] = h3derr::last();   // the message is thread-local
  };
  std::vector<std::thread> pool;
  for (int c = 1; c < C; ++c) pool.emplace_back(one, c);
  one(0);
  for (auto& t : pool) t.join();
  for (int c = 0; c < C; ++c)
    if (rcs[c]) return fail(rcs[c], "condition %d: %s", c, errs[c].c_str());
  for (int c = 0; c < C; ++c)
    for (int d = 0; d < D; ++d) tables_out[(size_t)d * C + c] = outs[c][d];
  return 0;
}

int h3d_disp_seg_stats(h3d_ctx* ctx, int S, int32_t* qiter, int32_t* evals) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (S != ctx->last_S || !ctx->h_res.p)
    return fail(H3D_EARG, "no estimate_disp result of %d segments (last: %d)", S, ctx->last_S);
  const SegState* h_sst = (const SegState*)((const double*)ctx->h_res.p + S);
  for (int s = 0; s < S; ++s) {
    if (qiter) qiter[s] = h_sst[s].qiter;
    if (evals) evals[s] = h_sst[s].evals;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// cml on given data (util/dispersion.py:46-80)
// ---------------------------------------------------------------------------

int h3d_cml(h3d_ctx* ctx, const double* data, int64_t n, int r, double* disp_out) {
  if (!ctx || !data || !disp_out) return fail(H3D_EARG, "null argument");
  if (n < 1 || r < 1 || r > kMaxReps) return fail(H3D_EARG, "n=%lld r=%d", (long long)n, r);
  if (n >= (int64_t)1 << 31) return fail(H3D_EARG, "n too large");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // replicate-major (SoA) copy of the data: the pseudodata layout k_brent reads
  std::vector<double> soa((size_t)n * r);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < r; ++k) soa[(size_t)k * n + i] = data[i * r + k];
  SegState st;
  seg_init(&st, n, r);  // phase kEqualize: the first evaluation is at x0
  std::vector<int32_t> rep_idx(kMaxReps);
  for (int k = 0; k < kMaxReps; ++k) rep_idx[k] = k;
  const int64_t seg[2] = {0, n};
  const int32_t nrep = r;
  HostCall hc(ctx);
  double* d_pd = hc.in("cml_pd", soa.data(), (size_t)n * r);
  int64_t* d_seg = hc.in("cml_seg", seg, 2);
  int32_t* d_ri = hc.in("cml_ri", rep_idx.data(), kMaxReps);
  int32_t* d_nr = hc.in("cml_nr", &nrep, 1);
  SegState* d_st = hc.in("cml_st", &st, 1);
  int* d_fl = hc.out<int>("cml_fl", 1);
  double* d_res = hc.out<double>("cml_res", 1);
  int* d_q = hc.out<int>("cml_queue", 1);
  if (int rc = hc.ready("cml scratch")) return rc;
  HIP_TRY(hipMemsetAsync(d_fl, 0, 4, s));
  with_width(r <= 4 ? 4 : r <= 8 ? 8 : r <= 16 ? 16 : 32, false, [&](auto m, auto) {
    launch_brent<decltype(m)::value>(ctx, d_pd, n, d_seg, 1, 1, d_ri, d_nr, d_st, d_fl, d_res,
                                     d_q);
  });
  HIP_TRY(hipGetLastError());
  hc.back(&st, d_st, 1);
  if (int rc = hc.finish()) return rc;
  if (st.flags & kFlagBrentFail)
    return fail(H3D_ENOCONV, "bounded minimisation failed (reference: assert res.success)");
  // the search ended in seg_step's qcml update: disp = delta / (1 - delta)
  *disp_out = st.disp;
  return 0;
}

// ---------------------------------------------------------------------------
// bh
// ---------------------------------------------------------------------------

int h3d_bh(const double* p, int64_t n, double* q) {
  if (n < 0 || (n > 0 && (!p || !q))) return fail(H3D_EARG, "null argument");
  h3dhost::bh(p, n, q);
  return 0;
}

}  // extern "C"

