// gfx950 build of the device numerics, for GPU unit tests ONLY.
//
// libh3d_selftest.so exports the same flat C ABI as the host build
// (h3d_hosttest.cpp: h3dt_*), but every entry point runs the device code of
// h3d_special.h / h3d_model.h in a gfx950 kernel -- OCML exp/log, the
// contracted NLL lgamma, device-side branch structure -- so tests/ can hold
// the kernels' numerics to the reference's unit goldens at the same
// tolerances as the host build (tests/test_special_host.py, parametrized
// over both libraries). The product never loads this library.
//
// The entries are those of h3d_unit_abi.h, the same text the host build
// compiles; this file is the backend under them. Host pointers in, host
// pointers out: each call stages its arrays through device buffers
// (synchronous; sizes are unit-test sized) and runs its body in k_each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#define H3DT_BODY __device__

namespace {

constexpr int kBlock = 256;

// set by the first HIP call that fails, and never cleared: from then on
// nothing is launched, every call reports -2 and every output holds its fill
bool g_failed = false;

bool ok(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    std::fprintf(stderr, "[h3d_selftest] %s: %s\n", what, hipGetErrorString(e));
    g_failed = true;
  }
  return e == hipSuccess;
}

template <typename T>
T* dev_alloc(int64_t count) {
  T* p = nullptr;
  const size_t bytes = std::max<int64_t>(count, 1) * sizeof(T);
  if (ok(hipMalloc((void**)&p, bytes), "hipMalloc")) ok(hipMemset(p, 0, bytes), "memset");
  return p;
}

// Device copy of a host array. The object the entry declares owns the
// allocation; the copies a body captures (and the kernel receives) only
// carry its pointer. A NULL host array reads as zeros.
template <typename T>
struct In {
  const T* p;
  bool owner = true;
  In(const T* host, int64_t count) : p(dev_alloc<T>(count)) {
    if (p && host && count > 0)
      ok(hipMemcpy((void*)p, host, count * sizeof(T), hipMemcpyHostToDevice), "H2D");
  }
  In(const In& o) : p(o.p), owner(false) {}
  ~In() {
    if (owner && p) (void)hipFree((void*)p);
  }
  __host__ __device__ operator const T*() const { return p; }
};

// Device buffer of a host output array: copied back when the entry returns
// (or at fetch()), or `fill` in every element once anything has failed.
template <typename T>
struct Out {
  T* p = nullptr;
  T* host;
  int64_t n;
  T fill;
  bool owner = true;
  Out(T* host_, int64_t count, T fill_) : host(host_), n(count), fill(fill_) {
    if (host) p = dev_alloc<T>(n);
  }
  Out(const Out& o) : p(o.p), host(o.host), n(o.n), fill(o.fill), owner(false) {}
  bool fetch() const {
    return !g_failed && (!host || n <= 0 ||
                         ok(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost), "D2H"));
  }
  ~Out() {
    if (!owner) return;
    if (!fetch() && host) std::fill(host, host + std::max<int64_t>(n, 0), fill);
    if (p) (void)hipFree(p);
  }
  __host__ __device__ operator T*() const { return p; }
};

template <typename F>
__global__ void k_each(int64_t n, F body, int* __restrict__ flags) {
  int fl = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    fl |= body(i);
  if (fl) atomicOr(flags, fl);
}

template <typename F>
int for_each(int64_t n, F body) {
  int fl = 0;
  Out<int> flags(&fl, 1, 0);
  if (g_failed) return -2;  // a buffer of this call, or an earlier call
  const int grid = (int)std::min<int64_t>(std::max<int64_t>((n + kBlock - 1) / kBlock, 1), 4096);
  hipLaunchKernelGGL(k_each<F>, dim3(grid), dim3(kBlock), 0, 0, n, body, (int*)flags);
  if (!ok(hipGetLastError(), "launch") || !ok(hipDeviceSynchronize(), "sync") || !flags.fetch())
    return -2;
  return fl;
}

}  // namespace

#include "h3d_unit_abi.h"

// 1 when a device is visible and every call so far succeeded
extern "C" int h3dt_device_ok(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return 0;
  return g_failed ? 0 : 1;
}
