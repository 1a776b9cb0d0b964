// dm_clean.hip — Clean (store.go:169-181) over the whole device store (dm_store_clean):
// the rows whose lease has lapsed are found, listed in ascending row order and, unless
// the call only peeks, released exactly as dm_store_release releases them.
//
// The shape is the re-layout's compact mode (dm_relayout.hip), over the same scan blocks
// of 4096 rows (one 256-thread workgroup each, every wave 16 x 64 consecutive rows):
//   k_cl_count   lapsed rows per block, and the block's earliest expiry among the rows
//                that stay: 4 B per row, + 8 B where the row carries its own expiry
//   k_rl_scan    exclusive prefix of the block counts (one workgroup; dm_relayout.hip)
//   k_cl_min     the blocks' minima reduced next to the total (one workgroup): the host
//                reads both in one 16-B copy and sizes the list from the total
//   k_cl_apply   lapsed row i to list[blk_pre[block] + rank in the block], and the row
//                body of k_release (release_row, the deltas through wave_seg_add);
//                skipped when nothing lapsed
// No atomics on the row path but the ones a release needs (running sums, dense masks).
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_update_util.h"

namespace dm {

namespace {

constexpr int kClWaveRows = kRlBlkRows / 4;  // 4 waves per workgroup
constexpr int kClIter = kClWaveRows / 64;    // rows per lane
static_assert(kClIter == 16, "a wave's lapsed-row masks are kept in 16 registers");
constexpr int64_t kNoExpiry = INT64_MAX;     // DM_NO_EXPIRY

// Row i as Clean sees it: whether it lapses at a.now, its expiry if it stays (else
// kNoExpiry), and its resource where the lookup was needed (a follower), else -1.
__device__ __forceinline__ bool cl_row(const CleanArgs& a, int64_t i, int32_t* raw, int* seg, int64_t* stay) {
  *raw = a.sub[i];
  *seg = -1;
  *stay = kNoExpiry;
  if (sub_released(*raw)) return false;
  int64_t e;
  if (*raw < 0) {
    e = a.expiry[i];
    if (e == kReleased) return false;  // a free row as dm_store_load and the re-layout hold it
  } else {
    *seg = seg_of_row(a.ix, i);
    e = a.agg[*seg].follow_exp;
  }
  if (a.now > e) return true;  // strict After (store.go:174)
  *stay = e;
  return false;
}

__device__ __forceinline__ int64_t cl_wave_min(int64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t o = __shfl_xor((long long)v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_cl_count(CleanArgs a) {
  __shared__ int32_t wtot[4];
  __shared__ int64_t wmin[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kRlBlkRows + (int64_t)w * kClWaveRows;
  int total = 0;
  int64_t mn = kNoExpiry;
#pragma unroll 4
  for (int k = 0; k < kClIter; ++k) {
    const int64_t i = row0 + k * 64 + lane;
    bool lapsed = false;
    if (i < a.N) {
      int32_t raw;
      int seg;
      int64_t stay;
      lapsed = cl_row(a, i, &raw, &seg, &stay);
      mn = stay < mn ? stay : mn;
    }
    total += __popcll(__ballot(lapsed));
  }
  mn = cl_wave_min(mn);
  if (lane == 0) {
    wtot[w] = total;
    wmin[w] = mn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.blk_pre[blockIdx.x] = (int64_t)wtot[0] + wtot[1] + wtot[2] + wtot[3];
    int64_t m = wmin[0];
    for (int v = 1; v < 4; ++v) m = wmin[v] < m ? wmin[v] : m;
    a.blk_min[blockIdx.x] = m;
  }
}

// out[0] = min of v[0, n): one workgroup (n is the number of scan blocks)
__global__ __launch_bounds__(1024) void k_cl_min(const int64_t* __restrict__ v, int64_t n, int64_t* out) {
  __shared__ int64_t s[16];
  int64_t mn = kNoExpiry;
  for (int64_t i = threadIdx.x; i < n; i += 1024) mn = v[i] < mn ? v[i] : mn;
  mn = cl_wave_min(mn);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) mn = s[w] < mn ? s[w] : mn;
    out[0] = mn;
  }
}

template <bool PEEK>
__global__ __launch_bounds__(256) void k_cl_apply(CleanArgs a, DenseUpd du) {
  __shared__ int32_t wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kRlBlkRows + (int64_t)w * kClWaveRows;
  unsigned long long m[kClIter];
  int segs[kClIter];
  int total = 0;
#pragma unroll
  for (int k = 0; k < kClIter; ++k) {
    const int64_t i = row0 + k * 64 + lane;
    bool lapsed = false;
    segs[k] = -1;
    if (i < a.N) {
      int32_t raw;
      int64_t stay;
      lapsed = cl_row(a, i, &raw, &segs[k], &stay);
    }
    m[k] = __ballot(lapsed);
    total += __popcll(m[k]);
  }
  if (lane == 0) wtot[w] = total;
  __syncthreads();
  int64_t run = a.blk_pre[blockIdx.x];
  for (int v = 0; v < w; ++v) run += wtot[v];
#pragma unroll
  for (int k = 0; k < kClIter; ++k) {
    if (m[k] == 0) continue;  // wave-uniform
    const int64_t i = row0 + k * 64 + lane;
    const bool lapsed = (m[k] >> lane) & 1;
    int seg = 0;
    double dh = 0.0, dw = 0.0;
    long long ds = 0;
    if (lapsed) {
      const int64_t at = run + lanes_below(m[k]);
      if (at < a.list_n) a.list[at] = i;
      if constexpr (!PEEK) {
        seg = segs[k] >= 0 ? segs[k] : seg_of_row(a.ix, i);
        release_row(a.ix, seg, i, a.has, a.wants, a.sub, a.expl, du, &dh, &dw, &ds);
      }
    }
    if constexpr (!PEEK) wave_seg_add(a.agg, lapsed, seg, dh, dw, ds, true, true);
    run += __popcll(m[k]);
  }
}

// The count pass, stream-ordered: a.blk_pre[blocks] = the lapsed rows, a.blk_pre[blocks + 1]
// = the earliest expiry among the rows that stay (kNoExpiry if none).
hipError_t launch_clean_count(const CleanArgs& a, hipStream_t st) {
  const int64_t nb = (a.N + kRlBlkRows - 1) / kRlBlkRows;
  if (nb <= 0) return hipSuccess;
  k_cl_count<<<(unsigned)nb, 256, 0, st>>>(a);
  hipError_t e = launch_rl_scan(a.blk_pre, nb, st);
  if (e != hipSuccess) return e;
  k_cl_min<<<1, 1024, 0, st>>>(a.blk_min, nb, a.blk_pre + nb + 1);
  return hipGetLastError();
}

// The apply pass; a.list holds a.list_n = a.blk_pre[blocks] entries.
hipError_t launch_clean_apply(const CleanArgs& a, const DenseUpd& du, bool peek, hipStream_t st) {
  const int64_t nb = (a.N + kRlBlkRows - 1) / kRlBlkRows;
  if (nb <= 0) return hipSuccess;
  if (peek)
    k_cl_apply<true><<<(unsigned)nb, 256, 0, st>>>(a, du);
  else
    k_cl_apply<false><<<(unsigned)nb, 256, 0, st>>>(a, du);
  return hipGetLastError();
}

}  // namespace dm
