// libh3d.so: the bodies of what h3d_ctx.h declares -- the ctx's slots and
// pinned buffers, profiling events, the launch and argument helpers every
// unit shares, and the staging of the host-buffer entry points (HostCall).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <set>
#include <utility>

#include "h3d.h"
#include "h3d_ctx.h"
#include "h3d_errors.h"
#include "h3d_model.h"

using namespace h3d;
using h3derr::fail;

namespace h3d {

// raw counts int64 -> int32; *overflow = 1 where one is outside [0, 2^31)
static __global__ void k_i64_to_i32(const int64_t* __restrict__ in,
                             int32_t* __restrict__ out, int64_t n,
                             int* __restrict__ overflow) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = in[i];
    if (v < 0 || v > 0x7fffffffLL) atomicOr(overflow, 1);
    out[i] = (int32_t)v;
  }
}

static __global__ void k_iota(int32_t* __restrict__ out, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int32_t)i;
}

}  // namespace h3d

namespace h3dint {

void* scratch(h3d_ctx* ctx, const char* slot, size_t bytes) {
  auto& b = ctx->bufs[slot];
  if (b.second >= bytes && b.first) return b.first;
  if (b.first) (void)hipFree(b.first);
  b.first = nullptr;
  b.second = 0;
  void* p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
  b.first = p;
  b.second = std::max<size_t>(bytes, 256);
  return p;
}

void* scratch_keep(h3d_ctx* ctx, const char* slot, size_t bytes, size_t keep) {
  auto& b = ctx->bufs[slot];
  if (b.first && b.second >= bytes) return b.first;
  const size_t cap = std::max<size_t>(std::max(bytes, 2 * b.second), 256);
  void* p = nullptr;
  if (hipMalloc(&p, cap) != hipSuccess) return nullptr;
  if (b.first) {
    if (keep) (void)hipMemcpyAsync(p, b.first, std::min(keep, b.second),
                                   hipMemcpyDeviceToDevice, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(b.first);
  }
  b.first = p;
  b.second = cap;
  return p;
}

int h2d_pinned(h3d_ctx* ctx, void* d_dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return 0;
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (!ctx->bounce_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->bounce_ev, hipEventDisableTiming));
  // the buffer is rewritten only after every earlier copy out of it has
  // read it: wrap-around, growth and a change of stream wait on the last one
  const bool wrap = ctx->bounce_off + need > ctx->bounce.cap;
  if ((wrap || (ctx->bounce_stream && ctx->bounce_stream != s)) && ctx->bounce_stream) {
    HIP_TRY(hipEventSynchronize(ctx->bounce_ev));
    ctx->bounce_off = 0;
    ctx->bounce_stream = nullptr;
  }
  if (need > ctx->bounce.cap) {
    if (int rc = ctx->bounce.grow(need, (size_t)1 << 20)) return rc;
    ctx->bounce_off = 0;
  }
  char* b = (char*)ctx->bounce.p + ctx->bounce_off;
  std::memcpy(b, src, bytes);
  HIP_TRY(hipMemcpyAsync(d_dst, b, bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(ctx->bounce_ev, s));
  ctx->bounce_stream = s;
  ctx->bounce_off += need;
  return 0;
}

void* pinned_rd(h3d_ctx* ctx, size_t bytes) {
  return ctx->land.grow(bytes, 4096) ? nullptr : ctx->land.p;
}

int counts_to_i32(h3d_ctx* ctx, const int64_t* d_raw64, int32_t* d_raw, int64_t count,
                  int* d_ovf) {
  HIP_TRY(hipMemsetAsync(d_ovf, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_i64_to_i32, dim3(grid_for(ctx, count)), dim3(kLaunchBlock), 0, ctx->stream,
                     d_raw64, d_raw, count, d_ovf);
  return 0;
}

void launch_iota(h3d_ctx* ctx, hipStream_t s, int32_t* out, int64_t n) {
  hipLaunchKernelGGL(k_iota, dim3(grid_for(ctx, n)), dim3(kLaunchBlock), 0, s, out, n);
}

int d2h_sync(h3d_ctx* ctx, void* dst, const void* d_src, size_t bytes, hipStream_t s) {
  void* l = pinned_rd(ctx, bytes);
  if (!l) return fail(H3D_ENOMEM, "pinned landing zone");
  HIP_TRY(hipMemcpyAsync(l, d_src, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(dst, l, bytes);
  return 0;
}

hipEvent_t ev_get(h3d_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

void prof_collect(h3d_ctx* ctx) {
  if (ctx->pending.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (size_t i = 0; i < ctx->pending.size(); ++i) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->pending[i].second.first,
                              ctx->pending[i].second.second);
    auto& e = ctx->stats[ctx->pending[i].first];
    e.ms += ms;
    e.launches += 1;
    e.units += ctx->pending_units[i];
    ctx->event_pool.push_back(ctx->pending[i].second.first);
    ctx->event_pool.push_back(ctx->pending[i].second.second);
  }
  ctx->pending.clear();
  ctx->pending_units.clear();
}

int grid_for(h3d_ctx* ctx, int64_t n, int per_cu) {
  int64_t g = (n + kLaunchBlock - 1) / kLaunchBlock;
  g = std::min<int64_t>(g, (int64_t)ctx->n_cu * per_cu);
  return (int)std::max<int64_t>(g, 1);
}

int check_cond(const int32_t* cond_of_rep, int R, int C, std::vector<int>* nrep,
               std::vector<int32_t>* rep_idx) {
  if (R < 1 || R > kMaxReps) return fail(H3D_EARG, "R=%d outside [1, %d]", R, kMaxReps);
  if (C < 1 || C > kMaxConds) return fail(H3D_EARG, "C=%d outside [1, %d]", C, kMaxConds);
  nrep->assign(C, 0);
  rep_idx->assign((size_t)C * kMaxReps, 0);
  for (int r = 0; r < R; ++r) {
    const int c = cond_of_rep[r];
    if (c < 0 || c >= C) return fail(H3D_EARG, "cond_of_rep[%d]=%d", r, c);
    (*rep_idx)[(size_t)c * kMaxReps + (*nrep)[c]] = r;
    (*nrep)[c] += 1;
  }
  for (int c = 0; c < C; ++c)
    if ((*nrep)[c] == 0) return fail(H3D_EARG, "condition %d has no replicates", c);
  return 0;
}

int flags_to_code(int fl) {
  if (fl & kFlagBadInput) return fail(H3D_EINPUT, "non-positive or non-finite dispersion / scaling factor (status %d)", fl);
  if (fl & (kFlagNoRoot | kFlagNoConv)) return fail(H3D_ENOCONV, "mean MLE failed (status %d)", fl);
  if (fl & (kFlagBrentFail | kFlagQcmlGuard)) return fail(H3D_ENOCONV, "dispersion optimisation failed (status %d)", fl);
  return 0;
}

int check_count(const void* ctx, int64_t n) {
  if (!ctx) return fail(H3D_EARG, "null ctx");
  if (n < 0 || n > (((int64_t)1 << 31) - 1))
    return fail(H3D_EARG, "n=%lld outside [0, 2^31)", (long long)n);
  return 0;
}

int allow_dynamic_lds(h3d_ctx* ctx, const void* kernel, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({ctx->device, kernel})) return 0;
  HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert({ctx->device, kernel});
  return 0;
}

HostCall::HostCall(h3d_ctx* c) : ctx(c), sc{c} {
  const hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) err = fail(H3D_EHIP, "hipSetDevice failed: %s", hipGetErrorString(e));
}

void HostCall::copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (err || bytes == 0) return;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
  in_flight = true;
  if (e != hipSuccess)
    err = fail(H3D_EHIP, "hipMemcpyAsync of %zu bytes failed: %s", bytes, hipGetErrorString(e));
}

int32_t* HostCall::counts(const int64_t* raw64, int64_t count, const char* msg) {
  ovf_msg = msg;
  int64_t* d_raw64 = in("in_raw64", raw64, count);
  int32_t* d_raw = out<int32_t>("in_raw", count);
  d_ovf = out<int>("ovf", 1);
  if (!err && !sc.ok) err = fail(H3D_ENOMEM, "raw counts");
  if (!err) err = counts_to_i32(ctx, d_raw64, d_raw, count, d_ovf);
  if (err) d_ovf = nullptr;
  return d_raw;
}

int HostCall::ready(const char* what) {
  if (!err && !sc.ok) err = fail(H3D_ENOMEM, "%s", what);
  return err;
}

int HostCall::finish() {
  if (d_ovf) copy(&ovf, d_ovf, 4, hipMemcpyDeviceToHost);
  in_flight = false;
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (err) return err;
  if (e != hipSuccess)
    return fail(H3D_EHIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  if (ovf) return fail(H3D_EINPUT, "%s", ovf_msg);
  return 0;
}

int HostCall::finish(void* dst, const void* d_src, size_t bytes) {
  void* l = pinned_rd(ctx, bytes);
  if (!l && !err) err = fail(H3D_ENOMEM, "pinned landing zone");
  copy(l, d_src, bytes, hipMemcpyDeviceToHost);
  if (int rc = finish()) return rc;
  std::memcpy(dst, l, bytes);
  return 0;
}

}  // namespace h3dint
