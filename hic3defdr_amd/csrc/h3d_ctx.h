// libh3d internals shared by its HIP translation units: the context behind
// the C ABI's opaque h3d_ctx handle, the launch and argument helpers and the
// staging of the host-buffer entry points (HostCall). The bodies of what is
// declared here live in h3d_ctx.hip (h3d_api.hip is the hot path only). Not
// part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "h3d.h"
#include "h3d_errors.h"

#define HIP_TRY(expr)                                                      \
  do {                                                                     \
    hipError_t e_ = (expr);                                                \
    if (e_ != hipSuccess)                                                  \
      return h3derr::fail(H3D_EHIP, "%s failed: %s (%s:%d)", #expr,        \
                          hipGetErrorString(e_), __FILE__, __LINE__);      \
  } while (0)

namespace h3d {

// prepare_data state between h3d_union_count and h3d_union_fill
struct PrepUnion {
  int R = 0, n_bins = 0;
  int64_t n_entries = 0, n_px = 0;
  // device
  int64_t* keys_sorted = nullptr;  // n_entries
  int32_t* ent_sorted = nullptr;   // n_entries
  int32_t* run_of = nullptr;       // n_entries (exclusive-scanned heads)
  int32_t* px_of_run = nullptr;    // runs -> pixel (or -1)
  int64_t* run_start = nullptr;    // runs + 1
  double* ent_val = nullptr;       // raw value per entry (summed duplicates not needed: canonical CSR)
  int32_t* ent_rep = nullptr;      // replicate per entry
  double* bias = nullptr;          // (n_bins, R)
  int64_t n_runs = 0;
};

}  // namespace h3d

namespace h3dint {

struct ProfEntry {
  double ms = 0.0;
  int64_t launches = 0;
  int64_t units = 0;
};

// a device dispersion table enqueued by h3d_disp_tables_dev whose status
// has not been read yet (h3d_lrt_dev_tab / h3d_disp_tables_wait settle it)
struct TablePending {
  const double* dpd = nullptr;
  double* tables = nullptr;
  int D = 0, C = 0, weighted = 1;
  double frac = -1.0, aff = 15.0;
  int active = 0, on_host = 0;
};

// grow-only pinned host buffer of the ctx, freed with it (a per-call
// hipHostFree would synchronise the device)
struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  // room for `bytes`: a smaller block is freed first and replaced by one of
  // max(bytes, min_cap) -- its contents are not kept
  int grow(size_t bytes, size_t min_cap = 0) {
    if (cap >= bytes) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = bytes > min_cap ? bytes : min_cap;
    HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return 0;
  }
};

}  // namespace h3dint

struct h3d_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  int n_cu = 256;
  std::map<const void*, int> resident;  // kernel -> resident workgroups / CU
  // 0 off; 1: the roofline kernels only ("disp_work", "lrt"); 2: every
  // scope. Events are collected lazily (profile_read / reset / close), so
  // the launch path never waits on them.
  int prof = 0;
  std::map<std::string, h3dint::ProfEntry> stats;
  std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> pending;
  std::vector<int64_t> pending_units;
  std::vector<hipEvent_t> event_pool;
  // grow-only device scratch, by slot
  std::map<std::string, std::pair<void*, size_t>> bufs;
  // prepare_data state between h3d_union_count and h3d_union_fill
  h3d::PrepUnion prep;
  // [equalize, nll] pixel-replicates processed by disp_work (measurement)
  unsigned long long* work_count = nullptr;
  // pinned host word the disp loop polls (active work items), kept for the
  // ctx's lifetime (a per-call hipHostFree would synchronise the device)
  int32_t* h_meta = nullptr;
  // pinned staging of estimate_disp's per-call tables (one H2D copy)
  h3dint::PinnedBuf h_stage;
  // pinned landing zone of estimate_disp's results (per-segment dispersion,
  // state, the distance check): pageable device-to-host copies blocked the
  // host one after another at the end of every call
  h3dint::PinnedBuf h_res;
  // recorded after each H2D copy out of h_stage: the next call waits on it
  // before rewriting (or freeing) the buffer, whichever way the last call
  // returned
  hipEvent_t h_stage_done = nullptr;
  // pinned bounce buffers for the small host<->device copies of the host
  // entry points (h2d_pinned / pinned_rd): a copy from or to pageable memory
  // is staged by the HIP runtime behind every other pageable copy in flight
  // -- e.g. the class's background result copies -- and a 4-byte flag read
  // waited tens of ms behind them (r06an)
  h3dint::PinnedBuf bounce;
  size_t bounce_off = 0;
  hipEvent_t bounce_ev = nullptr;
  hipStream_t bounce_stream = nullptr;
  h3dint::PinnedBuf land;
  // tuning knobs (env at h3d_open; the settled ones are listed in DESIGN.md,
  // "Settled switches")
  // k_disp_work: eighths of the task rounds dealt statically (the rest from
  // a device counter); H3D_EQ_STATIC8
  int eq_static8 = 4;
  // H3D_BRENT: 1 = gang Brent searches (k_brent_gang) where one workgroup
  // per segment leaves CUs idle, 2 = always, 0 = k_brent only
  int brent_gang = 1;
  int gang_aborts = 0;  // gang waits that timed out (fell back to k_brent)
  // H3D_BRENT_LDS_KB: LDS per k_brent workgroup for the segment's staged
  // head (0 = stream every evaluation from memory). With the log table in
  // LDS too, r03am: 64 / 96 / 128 KB 2.62-2.66 ms of Brent per cfg2 step,
  // 80 / 112 / 144 KB 2.73-2.80 (the replicate rows' LDS stride), 0 KB 2.67
  int brent_lds_kb = 128;
  // H3D_NLL_FULL: a call whose conditions all have exactly two replicates
  // (M = 2) runs the kFull instantiations of the equalize pass and the Brent
  // kernels (the replicate count a constant, predicate-free Brent trips; the
  // same bits); 0 = always the general ones
  int nll_full = 1;
  // H3D_NLL_RANGES: the Brent kernels take the r >= 5 form of the NLL term
  // (nll_pixel_r5, h3d_model.h nll_mode) for the evaluations it covers (the
  // same bits); 0 = the large / mid / general dispatch only
  int nll_ranges = 1;
  // H3D_PREP_STREAMS: 2 = estimate_disp's prep sorts and gathers conditions
  // 1 .. C-1 on prep_side while condition 0's chain and the table kernels
  // run on `stream` (fork / join through the two events; a
  // call too large to gain from it stays on `stream`, sort_by_condition);
  // 1 = everything on `stream`, one condition after the other
  int prep_streams = 2;
  // H3D_EQ_GATHER: 1 = on the packed path of the single-rank driver (32-bit
  // keys, every condition <= 2 replicates) the prep only sorts and the first
  // equalize launch gathers the sorted rows itself (k_disp_work's kGather;
  // the same bits); 0 = a gather kernel per condition in the prep
  int eq_gather = 1;
  // created by h3d_open with the switch at 2 (early: a stream created when
  // the process's hardware queues are all taken shares one, and two streams
  // on one queue run in enqueue order), destroyed with the ctx
  hipStream_t prep_side = nullptr;
  hipEvent_t prep_fork = nullptr, prep_join = nullptr;
  double qcml_tol = 1e-4;  // h3d_set_qcml_tol (qcml's tol, dispersion.py:10)
  // gang Brent slice (pixels; 0 = sized from the call, gang_setup_dev)
  int gang_px = 0;
  // k_brent_gang tag epoch (tags carry it, so they need no clearing between
  // launches) and the tag buffer it is valid for
  int gang_epoch = 0;
  void* gang_tag_buf = nullptr;
  size_t gang_tag_cap = 0;  // the tag allocation's capacity when last cleared
  // segments of the last estimate_disp call whose final states are in h_res
  // (h3d_disp_seg_stats)
  int last_S = 0;
  h3dint::TablePending tab_pending;
};

namespace h3dint {

constexpr int kLaunchBlock = 256;
// distances per condition the device smoother holds in LDS (h3d_table.hip);
// beyond it h3d_disp_tables_dev runs the host smoother inside the call
constexpr int kTableMaxD = 1024;

// grow-only device buffer of the ctx, by slot name (nullptr on OOM)
void* scratch(h3d_ctx* ctx, const char* slot, size_t bytes);
// the same, but a grown buffer keeps its first `keep` bytes (stream-ordered
// copy; growth at least doubles the capacity)
void* scratch_keep(h3d_ctx* ctx, const char* slot, size_t bytes, size_t keep);

// a call's device buffers out of the ctx's slots, counted in elements; `ok`
// turns false at the first failed allocation, so a group of buffers is
// checked once: if (!sc.ok) return fail(H3D_ENOMEM, ...)
struct Scratch {
  h3d_ctx* ctx;
  bool ok = true;
  template <typename T>
  T* get(const char* slot, size_t count) {
    T* p = (T*)scratch(ctx, slot, count * sizeof(T));
    ok = ok && p;
    return p;
  }
  // scratch_keep: a grown buffer keeps its first keep_count elements
  template <typename T>
  T* keep(const char* slot, size_t count, size_t keep_count) {
    T* p = (T*)scratch_keep(ctx, slot, count * sizeof(T), keep_count * sizeof(T));
    ok = ok && p;
    return p;
  }
};

// One host-buffer entry point's staging on the ctx's device and stream:
// uploads, the call's slots, downloads, one synchronisation. Every operation
// enqueues at once; the first error sticks (`err`) and ready() / finish()
// report it. A HostCall that leaves scope with a copy in flight and without
// finish() drains the stream, so no early return leaves a copy running into
// or out of memory the caller gets back.
struct HostCall {
  h3d_ctx* ctx;
  Scratch sc;
  int err = 0;
  bool in_flight = false;  // a copy was enqueued and finish() has not run
  int* d_ovf = nullptr;    // counts(): the overflow word, its host copy and
  int ovf = 0;             // the message of a set one
  const char* ovf_msg = nullptr;

  explicit HostCall(h3d_ctx* c);  // hipSetDevice
  HostCall(const HostCall&) = delete;
  ~HostCall() {
    if (in_flight) (void)hipStreamSynchronize(ctx->stream);
  }
  void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
  template <typename T>  // a slot of `count` elements, without a copy
  T* out(const char* slot, size_t count) {
    return sc.get<T>(slot, count);
  }
  template <typename T>  // host -> device of `count` elements into (part of) a slot
  void up(T* d, const T* src, size_t count) {
    if (d && src) copy(d, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  // a slot of count + pad elements and the upload of `count` into it; an
  // absent (NULL) src takes no slot and gives NULL
  template <typename T>
  T* in(const char* slot, const T* src, size_t count, size_t pad = 0) {
    T* d = src ? sc.get<T>(slot, count + pad) : nullptr;
    up(d, src, count);
    return d;
  }
  // raw counts, uploaded and converted to int32; a count outside [0, 2^31)
  // fails finish() with H3D_EINPUT and `msg`
  int32_t* counts(const int64_t* raw64, int64_t count, const char* msg);
  template <typename T>  // device -> host of `count` elements into caller memory
  void back(T* dst, const T* d_src, size_t count) {
    if (dst) copy(dst, d_src, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  // ahead of the launches: the first error, or H3D_ENOMEM "<what>"
  int ready(const char* what);
  // one stream synchronisation, the count check, the first error
  int finish();
  // the same with a small result: `bytes` into dst through pinned_rd
  int finish(void* dst, const void* d_src, size_t bytes);
};

// hipcub's two-phase calls. op(tmp, bytes) is the operation, one of
// h3d_cub.h's (hipError_t(void*, size_t&)): with tmp = nullptr it only reports its temp
// size. cub_bytes is that query alone; cub_call queries, takes the temp out
// of the ctx slot (grow-only: a slot reserved larger beforehand is reused as
// it is) and runs the operation.
template <typename Op>
int cub_bytes(Op op, size_t* bytes) {
  *bytes = 0;
  HIP_TRY(op(nullptr, *bytes));
  return 0;
}
template <typename Op>
int cub_call(h3d_ctx* ctx, const char* tmp_slot, Op op) {
  size_t bytes = 0;
  if (int rc = cub_bytes(op, &bytes)) return rc;
  void* tmp = scratch(ctx, tmp_slot, bytes);
  if (!tmp) return h3derr::fail(H3D_ENOMEM, "hipcub temp (%s, %zu bytes)", tmp_slot, bytes);
  HIP_TRY(op(tmp, bytes));
  return 0;
}

// Raw counts arrive as int64 and every kernel reads int32. counts_to_i32
// (enqueued on the ctx stream) clears *d_ovf and converts `count` device
// values, setting *d_ovf where one is outside [0, 2^31); HostCall::counts
// does so for a host array, through the slots "in_raw64" / "in_raw" / "ovf",
// and HostCall::finish reads the word (H3D_EINPUT).
int counts_to_i32(h3d_ctx* ctx, const int64_t* d_raw64, int32_t* d_raw, int64_t count,
                  int* d_ovf);
// out[i] = i for i in [0, n), enqueued on s (k_iota, h3d_ctx.hip)
void launch_iota(h3d_ctx* ctx, hipStream_t s, int32_t* out, int64_t n);
hipEvent_t ev_get(h3d_ctx* ctx);
// host -> device copy of `bytes` through the ctx's pinned bounce buffer,
// stream-ordered on s (the source may be reused at once)
int h2d_pinned(h3d_ctx* ctx, void* d_dst, const void* src, size_t bytes, hipStream_t s);
// a pinned landing zone of >= bytes for device -> host copies (grow-only;
// one user at a time: the caller synchronises before reading it and before
// its next call), nullptr on failure
void* pinned_rd(h3d_ctx* ctx, size_t bytes);
// device -> host copy through the pinned landing zone, synchronous on s
int d2h_sync(h3d_ctx* ctx, void* dst, const void* d_src, size_t bytes, hipStream_t s);
// folds the recorded event pairs into ctx->stats (synchronises the stream)
void prof_collect(h3d_ctx* ctx);
// grid of a grid-stride elementwise kernel over n items
int grid_for(h3d_ctx* ctx, int64_t n, int per_cu = 8);
// validates a replicate -> condition map; per-condition replicate counts and
// replicate indices (C x kMaxReps, design order)
int check_cond(const int32_t* cond_of_rep, int R, int C, std::vector<int>* nrep,
               std::vector<int32_t>* rep_idx);
// kernel status flags -> H3D_E* code (+ message)
int flags_to_code(int fl);
// ctx not NULL and n in [0, 2^31)
int check_count(const void* ctx, int64_t n);
// lets `kernel` take up to `bytes` of dynamic LDS: set once per process and
// device, a no-op afterwards
int allow_dynamic_lds(h3d_ctx* ctx, const void* kernel, int bytes);
// the device table of h3d_disp_tables_dev (h3d_table.hip): copy its status
// (before the stream sync), settle it (after): 1 = redone on the host
int table_status_copy(h3d_ctx* ctx, int* h_st);
int table_settle(h3d_ctx* ctx, const int* h_st);

// wraps one kernel launch with HIP events on the ctx stream when profiling
struct ProfScope {
  h3d_ctx* ctx;
  const char* name;
  int64_t units;
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  ProfScope(h3d_ctx* c, const char* n, int64_t u, int level = 2)
      : ctx(c), name(n), units(u), on(c->prof >= level) {
    // bound the pending list (collecting synchronises the stream)
    if (on && ctx->pending.size() > 16384) prof_collect(ctx);
    if (on) {
      a = ev_get(ctx);
      b = ev_get(ctx);
      (void)hipEventRecord(a, ctx->stream);
    }
  }
  ~ProfScope() {
    if (on) {
      (void)hipEventRecord(b, ctx->stream);
      ctx->pending.push_back({name, {a, b}});
      ctx->pending_units.push_back(units);
    }
  }
};

}  // namespace h3dint
