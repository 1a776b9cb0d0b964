// dm_load.hip — a store loaded from, and read into, device memory (dm_store_load_device,
// dm_read_store_sums_device): what dm_store_load's serial host loops do, over columns that
// never leave HBM.
//
//   k_ld_check     the caller's rows before anything of the context is touched: a subclients
//                  value outside [0, kSubMax] (rejects the call) and whether every row has
//                  count 1 or is released (all_sub_one); 8 B read per row, 16 where the count is not 1
//   k_ld_sub       the subclients column, 8 B per row in, 4 B out, every row explicit
//   k_ld_res_lane  resources of at most kLdLaneRows rows, one lane each
//   k_ld_res_wave  the longer ones, one wave each
// (wants, has and expiry_ns are device-to-device copies: the host enqueues them.)
//
// The two resource kernels write a resource's running sums -- the given agg_* carried, or
// one Assign per row in row order (store.go:156-158) -- and find what scan_maybe_general
// (dm_store.cpp) finds.  The order of the additions is fixed: from +0.0, sum += has[i] for i
// ascending, so one resource's additions are a serial chain, whoever loads the rows.  A wave
// loads 64 rows per column coalesced, the next 64 while it works on these, and feeds them to
// the chains in lane order through readlanes: no lane ever waits on a load that depends on
// its own previous one, and a 10^6-row resource is ~15.6k such steps of one wave.  The count
// is an integer: lane partials, reduced once.  Built with -ffp-contract=off like every
// unit; the chains hold additions only.
//
// Flags are reduced per wave (ballots), per workgroup (LDS), and at most one atomic per
// workgroup goes onto the flags word.
//
//   k_ld_unpack    ResAgg (32-B records) into the three arrays of dm_read_store_sums_device
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dm_kernel_util.h"
#include "dm_launch.h"

namespace dm {

namespace {

constexpr int kLdLaneRows = 32;      // longer resources take a wave each
constexpr int64_t kLdMaxBlocks = 8192;  // every kernel here strides over its rows or resources

// Flag bits the lanes of a workgroup hold, onto the flags word: one atomic at most.
__device__ __forceinline__ void ld_raise(uint32_t f, uint32_t* flags, uint32_t* lds) {
  uint32_t wf = 0;
  for (uint32_t bit = 1; bit <= kLdGeneral; bit <<= 1)
    if (__ballot(f & bit)) wf |= bit;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) lds[w] = wf;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t all = lds[0] | lds[1] | lds[2] | lds[3];
    if (all) atomicOr(flags, all);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void k_ld_check(LoadArgs a) {
  __shared__ uint32_t lds[4];
  uint32_t f = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.N; i += stride) {
    const int64_t s = a.sub[i];
    if (s < 0 || s > kSubMax) f |= kLdBadSub;
    // released rows never take part in a tick, so they do not count against all_sub_one
    if (s != 1 && a.expiry[i] != kReleased) f |= kLdNotOne;
  }
  ld_raise(f, a.flags, lds);
}

// Every loaded row keeps its own expiry (explicit, dm_device.h); a writeback tick turns the
// live ones into followers of their resource's expiry.
__global__ __launch_bounds__(256) void k_ld_sub(const int64_t* __restrict__ sub, int64_t N, int32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride)
    out[i] = (int32_t)((uint32_t)sub[i] | kSubExplicit);
}

// A row of a resource of more than kSmallMax rows, as scan_maybe_general counts it: not
// released, and a NaN wants or a subclients value that differs from the first such row's.
__device__ __forceinline__ bool ld_general_row(double w, int64_t s, int64_t* s0) {
  if (*s0 < 0) *s0 = s;
  return w != w || s != *s0;
}

template <bool SUMS>
__global__ __launch_bounds__(256) void k_ld_res_lane(LoadArgs a, const int64_t* __restrict__ off, ResAgg* agg) {
  __shared__ uint32_t lds[4];
  uint32_t f = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.R; r += stride) {
    const int64_t o0 = off[r], o1 = off[r + 1];
    if (o1 - o0 > kLdLaneRows) continue;  // k_ld_res_wave's
    const bool scan = o1 - o0 > kSmallMax;
    int64_t cnt = 0, s0 = -1;
    double sh = 0.0, sw = 0.0;
    for (int64_t i = o0; i < o1; ++i) {
      const double w = a.wants[i];
      const int64_t s = a.sub[i];
      if constexpr (SUMS) {
        sh += a.has[i];
        sw += w;
        cnt += s;
      }
      if (scan && a.expiry[i] != kReleased && ld_general_row(w, s, &s0)) f = kLdGeneral;
    }
    if constexpr (SUMS)
      agg[r] = ResAgg{cnt, sh, sw, 0};
    else
      agg[r] = ResAgg{a.agg_count[r], a.agg_sum_has[r], a.agg_sum_wants[r], 0};
  }
  ld_raise(f, a.flags, lds);
}

namespace {

struct LdRows {  // a lane's row of the 64 a wave holds
  double w, h;
  int64_t s, e;
};

// Row i of a resource that ends at `end` (> its first row), or past the end a row that adds
// nothing.  The loads are unconditional (a lane past the end loads the last row and drops
// it), so the wait before a step's chains can leave the next step's loads in flight.
template <bool SUMS>
__device__ __forceinline__ LdRows ld_rows(const LoadArgs& a, int64_t i, int64_t end) {
  const bool in = i < end;
  const int64_t j = in ? i : end - 1;
  LdRows v{a.wants[j], 0.0, a.sub[j], a.expiry[j]};
  if constexpr (SUMS) v.h = a.has[j];
  if (!in) v = LdRows{0.0, 0.0, 0, kReleased};
  return v;
}

}  // namespace

template <bool SUMS>
__global__ __launch_bounds__(256) void k_ld_res_wave(LoadArgs a, const int64_t* __restrict__ off, ResAgg* agg) {
  __shared__ uint32_t lds[4];
  uint32_t f = 0;
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + uniform((int)(threadIdx.x >> 6)), nw = (int64_t)gridDim.x * 4;
  for (int64_t r = w0; r < a.R; r += nw) {
    const int64_t o0 = off[r], o1 = off[r + 1];
    if (o1 - o0 <= kLdLaneRows) continue;  // k_ld_res_lane's
    int64_t cnt = 0, s0 = -1;
    double sh = 0.0, sw = 0.0;
    LdRows cur = ld_rows<SUMS>(a, o0 + lane, o1);
    for (int64_t b = o0; b < o1; b += 64) {
      const LdRows nxt = ld_rows<SUMS>(a, b + 64 + lane, o1);  // in flight while the chains run
      const bool live = cur.e != kReleased;  // (a lane past the end holds kReleased)
      const unsigned long long m = __ballot(live);
      if (m) {  // (kLdLaneRows >= kSmallMax: every resource here is scanned)
        if (s0 < 0) s0 = readlane_any(cur.s, __ffsll(m) - 1);
        if (__ballot(live && (cur.w != cur.w || cur.s != s0))) f = kLdGeneral;
      }
      if constexpr (SUMS) {
        cnt += cur.s;  // (0 past the end)
        if (o1 - b >= 64) {
#pragma unroll
          for (int l = 0; l < 64; ++l) {
            sh += readlane_any(cur.h, l);
            sw += readlane_any(cur.w, l);
          }
        } else {
          const int rows = uniform((int)(o1 - b));
          for (int l = 0; l < rows; ++l) {
            sh += readlane_any(cur.h, l);
            sw += readlane_any(cur.w, l);
          }
        }
      }
      cur = nxt;
    }
    if constexpr (SUMS) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor((long long)cnt, d, 64);
      if (lane == 0) agg[r] = ResAgg{cnt, sh, sw, 0};
    } else {
      if (lane == 0) agg[r] = ResAgg{a.agg_count[r], a.agg_sum_has[r], a.agg_sum_wants[r], 0};
    }
  }
  ld_raise(f, a.flags, lds);
}

__global__ __launch_bounds__(256) void k_ld_unpack(const ResAgg* __restrict__ agg, int64_t n, int64_t* count,
                                                   double* sum_has, double* sum_wants) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const ResAgg g = agg[i];
    if (count) count[i] = g.count;
    if (sum_has) sum_has[i] = g.sum_has;
    if (sum_wants) sum_wants[i] = g.sum_wants;
  }
}

// --------------------------------------------------------------------------
// host-side launchers (called by dm_store.cpp)
// --------------------------------------------------------------------------
static unsigned ld_grid(int64_t items, int per_block) {
  return (unsigned)std::min<int64_t>((items + per_block - 1) / per_block, kLdMaxBlocks);
}

hipError_t launch_load_check(const LoadArgs& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.flags, 0, sizeof(uint32_t), st);
  if (e != hipSuccess || a.N <= 0) return e;
  k_ld_check<<<ld_grid(a.N, 256), 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_load_sub(const LoadArgs& a, int32_t* sub32, hipStream_t st) {
  if (a.N <= 0) return hipSuccess;
  k_ld_sub<<<ld_grid(a.N, 256), 256, 0, st>>>(a.sub, a.N, sub32);
  return hipGetLastError();
}

hipError_t launch_load_resources(const LoadArgs& a, const int64_t* seg_off, ResAgg* agg, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  if (a.agg_count) {
    k_ld_res_lane<false><<<ld_grid(a.R, 256), 256, 0, st>>>(a, seg_off, agg);
    k_ld_res_wave<false><<<ld_grid(a.R, 4), 256, 0, st>>>(a, seg_off, agg);
  } else {
    k_ld_res_lane<true><<<ld_grid(a.R, 256), 256, 0, st>>>(a, seg_off, agg);
    k_ld_res_wave<true><<<ld_grid(a.R, 4), 256, 0, st>>>(a, seg_off, agg);
  }
  return hipGetLastError();
}

hipError_t launch_unpack_sums(const ResAgg* agg, int64_t n, int64_t* count, double* sum_has, double* sum_wants,
                              hipStream_t st) {
  if (n <= 0 || (!count && !sum_has && !sum_wants)) return hipSuccess;
  k_ld_unpack<<<ld_grid(n, 256), 256, 0, st>>>(agg, n, count, sum_has, sum_wants);
  return hipGetLastError();
}

}  // namespace dm
