// Philox4x32-10 (Salmon, Moraes, Dror & Shaw, "Parallel random numbers: as
// easy as 1, 2, 3", SC'11; the Random123 constants), host + device, and the
// counter layout of the simulation stream (simulate(gpu=True), DESIGN.md §1
// F9): every draw is a pure function of (seed, stream, replicate, pixel
// index) -- nothing depends on block size, grid size or launch order.
#pragma once

#include <cstdint>

#include "h3d_special.h"

namespace h3d {

struct Philox4 {
  uint32_t w0, w1, w2, w3;
};

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// ten rounds on counter c under key (k0, k1); the key steps by the Weyl
// increments between rounds
H3D_HD Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c.w0;
    const uint64_t p1 = (uint64_t)kPhiloxM1 * c.w2;
    Philox4 n;
    n.w0 = (uint32_t)(p1 >> 32) ^ c.w1 ^ k0;
    n.w1 = (uint32_t)p1;
    n.w2 = (uint32_t)(p0 >> 32) ^ c.w3 ^ k1;
    n.w3 = (uint32_t)p0;
    c = n;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}

// a uniform from two words: the top 52 bits of (hi << 32 | lo) as an integer
// m, u = (m + 1/2) 2^-52. m + 1/2 has at most 53 significant bits, so u is
// exact, lies in [2^-53, 1 - 2^-53] -- strictly inside (0, 1) -- and 1 - u =
// ((2^52 - 1 - m) + 1/2) 2^-52 is exact too. (53 bits + 1/2 would need 54
// significant bits: its largest value rounds to 1.)
H3D_HD double philox_uniform(uint32_t lo, uint32_t hi) {
  const uint64_t m = (((uint64_t)hi << 32) | lo) >> 12;
  return ((double)m + 0.5) * 0x1p-52;
}

// the two uniforms of one draw: key = the seed's (low, high) words, counter =
// {pixel index low, pixel index high, replicate, stream id}; u1 from words
// 0 and 1, u2 from words 2 and 3
H3D_HD void sim_uniforms(uint64_t seed, uint32_t stream, uint32_t rep, uint64_t pixel,
                         double* u1, double* u2) {
  Philox4 c;
  c.w0 = (uint32_t)pixel;
  c.w1 = (uint32_t)(pixel >> 32);
  c.w2 = rep;
  c.w3 = stream;
  const Philox4 o = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  *u1 = philox_uniform(o.w0, o.w1);
  *u2 = philox_uniform(o.w2, o.w3);
}

}  // namespace h3d
