// dm_threshold_util.h — FairShare round 2 by sorted thresholds: the helpers k_general
// (dm_tick_general.hip) and the chain's heterogeneous kernels (dm_tick_large_het.h) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dm {

constexpr int kGenMaxT = 256;
constexpr int kGenBuckets = 2 * kGenMaxT + 1;
constexpr uint64_t kGenEmpty = ~0ull;  // a NaN pattern: never a finite threshold's bits

// ascending bitonic sort of one key per lane across the wave
__device__ __forceinline__ uint32_t wave_sort64(uint32_t key) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)key, j, 64);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      key = keep_min ? (key < other ? key : other) : (key > other ? key : other);
    }
  }
  return key;
}

// m = number of thresholds below w; bucket 2m (strictly between) or 2m+1 (== T_m+1)
__device__ __forceinline__ int gen_bucket(const double* T, int K, double w) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] < w)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < K && T[lo] == w) ? 2 * lo + 1 : 2 * lo;
}

__device__ __forceinline__ int gen_index(const double* T, int K, double t) {  // T[k] == t
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] < t)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace dm
