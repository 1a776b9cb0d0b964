// dm_relayout.hip — the device store re-laid out in HBM (dm_store_relayout): resources
// grow, shrink, are compacted or appended without a row crossing PCIe.
//
// The reference grows a resource's map one client at a time (store.go:153-167) and
// creates resources on first use (resource.go:153-163); here a resource is a segment of
// the columnar table, so a new layout is a gather of every row that stays into fresh
// columns (28 B read, 28 B written per row).  The old columns are left untouched: the
// host swaps the fresh ones in only when no kernel flagged a rejection.
//
//   k_rl_blkseg   the new table's block index (RowIndex::blk_seg) from the new seg_off
//   k_rl_agg      the running sums carried bit for bit, zero for appended resources
//   k_rl_fill     free rows of the new table: the rows no old row moves to
//   k_rl_scatter  every old row to its new place, as an explicit-expiry row
// and, in compact mode, before the scatter:
//   k_rl_count    moved (not released) rows per scan block of 4096 old rows, and for every
//                 resource the moved rows of its first row's block before that row
//   k_rl_scan     exclusive prefix of the block counts (one workgroup)
// A moved row's rank among its resource's moved rows is then
//   blk_pre[block] + rank in the block  -  (blk_pre[block of the resource's first row] + seg_local[r]),
// whatever the resource's size: a resource inside one block or spanning thousands takes
// the same path.  No atomics on the row path (the rejection flags only).
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_update_util.h"

namespace dm {

namespace {

constexpr int kRlWaveRows = kRlBlkRows / 4;   // 4 waves per workgroup
constexpr int kRlIter = kRlWaveRows / 64;     // rows per lane
static_assert(kRlIter == 16, "a wave's moved-row masks are kept in 16 registers");

// A row as dm_read_store reports it: its resource and its resolved expiry
// (k_resolve_rows); a row is released when that expiry is DM_RELEASED.
__device__ __forceinline__ void rl_row(const RelayoutArgs& a, int64_t i, int32_t* raw, int* seg, int64_t* e) {
  *raw = a.sub[i];
  *seg = seg_of_row(a.ix, i);
  *e = sub_released(*raw) ? kReleased : (*raw < 0 ? a.expiry[i] : a.agg[*seg].follow_exp);
}

__device__ __forceinline__ void rl_reject(const RelayoutArgs& a, uint32_t why, int seg) {
  atomicOr(a.flags, why);
  atomicMin(a.bad, (unsigned long long)seg);
}

}  // namespace

__global__ void k_rl_blkseg(const int64_t* __restrict__ off, int64_t R, int64_t N, int64_t nb, int32_t* blk) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  int64_t lo = 0;
  if (R > 0) {
    int64_t row = b << kRowBlkShift;
    const int64_t last = N > 0 ? N - 1 : 0;
    if (row > last) row = last;
    int64_t hi = R;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= row)
        lo = mid;
      else
        hi = mid;
    }
  }
  blk[b] = (int32_t)lo;
}

// Running sums carried, not recomputed; the followers' expiry starts over (every row
// leaves the re-layout with an expiry of its own), as after dm_store_load.
__global__ void k_rl_agg(const ResAgg* __restrict__ old, int64_t R, ResAgg* out, int64_t Rn) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Rn) return;
  ResAgg g{0, 0.0, 0.0, 0};
  if (r < R) {
    g = old[r];
    g.follow_exp = 0;
  }
  out[r] = g;
}

// Free rows of the new table, four per thread (16-B stores where all four are free):
// has 0, wants 0, subclients 0, expiry DM_RELEASED, as dm_store_load holds such a row.
// all: every row (compact mode, whose scatter then overwrites the moved ones); else the
// rows past the old length of their resource (the scatter writes the others).
__global__ __launch_bounds__(256) void k_rl_fill(RelayoutArgs a, RowIndex nix, int all) {
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= a.Nn) return;
  bool fr[4] = {true, true, true, true};
  if (!all) {
    const int64_t last = j + 3 < a.Nn ? j + 3 : a.Nn - 1;
    const int r0 = seg_of_row(nix, j), r3 = seg_of_row(nix, last);
    for (int q = 0; q < 4; ++q) {
      const int64_t row = j + q;
      if (row >= a.Nn) break;
      const int r = r0 == r3 ? r0 : seg_of_row(nix, row);
      fr[q] = r >= a.R || row - a.new_off[r] >= a.ix.seg_off[r + 1] - a.ix.seg_off[r];
    }
  }
  if (j + 3 < a.Nn && fr[0] && fr[1] && fr[2] && fr[3]) {
    const double2 z{0.0, 0.0};
    const longlong2 rel{(long long)kReleased, (long long)kReleased};
    const int se = (int)kSubExplicit;
    *(double2*)(a.n_wants + j) = z;
    *(double2*)(a.n_wants + j + 2) = z;
    *(double2*)(a.n_has + j) = z;
    *(double2*)(a.n_has + j + 2) = z;
    *(int4*)(a.n_sub + j) = int4{se, se, se, se};
    *(longlong2*)(a.n_expiry + j) = rel;
    *(longlong2*)(a.n_expiry + j + 2) = rel;
    return;
  }
  for (int q = 0; q < 4; ++q) {
    const int64_t row = j + q;
    if (row >= a.Nn || !fr[q]) continue;
    a.n_wants[row] = 0.0;
    a.n_has[row] = 0.0;
    a.n_sub[row] = (int32_t)kSubExplicit;
    a.n_expiry[row] = kReleased;
  }
}

// Compact mode: the rows that move are the rows not released.
__global__ __launch_bounds__(256) void k_rl_count(RelayoutArgs a) {
  __shared__ int32_t wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kRlBlkRows + (int64_t)w * kRlWaveRows;
  unsigned long long m[kRlIter];
  int segs[kRlIter];
  uint32_t first = 0;
  int total = 0;
#pragma unroll
  for (int k = 0; k < kRlIter; ++k) {
    const int64_t i = row0 + k * 64 + lane;
    bool moved = false;
    segs[k] = 0;
    if (i < a.N) {
      int32_t raw;
      int64_t e;
      rl_row(a, i, &raw, &segs[k], &e);
      moved = e != kReleased;
      if (i == a.ix.seg_off[segs[k]]) first |= 1u << k;
    }
    m[k] = __ballot(moved);
    total += __popcll(m[k]);
  }
  if (lane == 0) wtot[w] = total;
  __syncthreads();
  int run = 0;
  for (int v = 0; v < w; ++v) run += wtot[v];
#pragma unroll
  for (int k = 0; k < kRlIter; ++k) {
    if (first >> k & 1) a.seg_local[segs[k]] = run + lanes_below(m[k]);
    run += __popcll(m[k]);
  }
  if (threadIdx.x == 0) a.blk_pre[blockIdx.x] = (int64_t)wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// Exclusive prefix of v[0, n) in place, the total in v[n]: one workgroup (n is the number
// of scan blocks: ~30k for 125M rows).
__global__ __launch_bounds__(1024) void k_rl_scan(int64_t* v, int64_t n) {
  __shared__ int64_t s[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t lo = (int64_t)t * per < n ? (int64_t)t * per : n;
  const int64_t hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += v[i];
  s[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t x = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  int64_t run = s[t] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t x = v[i];
    v[i] = run;
    run += x;
  }
  if (t == 1023) v[n] = s[1023];
}

// (for the other scans over blocks of kRlBlkRows rows: dm_clean.hip)
hipError_t launch_rl_scan(int64_t* v, int64_t n, hipStream_t st) {
  k_rl_scan<<<1, 1024, 0, st>>>(v, n);
  return hipGetLastError();
}

// One old row to its place in the new table.  rank: (compact mode) the moved rows before
// it in the whole table.
template <bool COMPACT>
__device__ __forceinline__ void rl_move(const RelayoutArgs& a, int64_t i, int32_t raw, int seg, int64_t e,
                                        int64_t rank) {
  const int64_t o0 = a.ix.seg_off[seg], olen = a.ix.seg_off[seg + 1] - o0;
  const int64_t n0 = a.new_off[seg], nlen = a.new_off[seg + 1] - n0;
  const bool released = e == kReleased;
  int64_t k = 0;
  bool moved;
  if constexpr (!COMPACT) {
    k = i - o0;
    moved = k < nlen;
    if (!moved && !released) rl_reject(a, kRlDrop, seg);
  } else {
    moved = !released;
    if (moved) {
      k = rank - (a.blk_pre[o0 >> kRowBlkShift] + a.seg_local[seg]);
      if (k < 0) {
        rl_reject(a, kRlInternal, seg);
        moved = false;
      } else if (k >= nlen) {
        rl_reject(a, kRlOver, seg);
        moved = false;
      }
    }
  }
  const int64_t dest = n0 + k;
  if (moved) {
    const double wv = a.wants[i];
    const int sv = sub_value(raw);
    a.n_wants[dest] = wv;
    a.n_has[dest] = a.has[i];
    a.n_sub[dest] = (int32_t)((uint32_t)sv | kSubExplicit);
    a.n_expiry[dest] = e;
    // a resource that leaves the small tiles (which decide any rows) for the bins, which
    // hand heterogeneous subclients and NaN wants to k_general: the host then prepares for it
    if (olen <= kSmallMax && nlen > kSmallMax && !released && (sv != 1 || wv != wv)) atomicOr(a.flags, kRlGeneral);
  }
  if (a.row_map) a.row_map[i] = moved ? dest : -1;
}

template <bool COMPACT>
__global__ __launch_bounds__(256) void k_rl_scatter(RelayoutArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kRlBlkRows + (int64_t)w * kRlWaveRows;
  if constexpr (!COMPACT) {
#pragma unroll 4
    for (int k = 0; k < kRlIter; ++k) {
      const int64_t i = row0 + k * 64 + lane;
      if (i >= a.N) break;
      int32_t raw;
      int seg;
      int64_t e;
      rl_row(a, i, &raw, &seg, &e);
      rl_move<false>(a, i, raw, seg, e, 0);
    }
  } else {
    __shared__ int32_t wtot[4];
    unsigned long long m[kRlIter];
    int32_t raws[kRlIter];
    int segs[kRlIter];
    int64_t es[kRlIter];
    int total = 0;
#pragma unroll
    for (int k = 0; k < kRlIter; ++k) {
      const int64_t i = row0 + k * 64 + lane;
      raws[k] = (int32_t)kSubReleased;
      segs[k] = 0;
      es[k] = kReleased;
      if (i < a.N) rl_row(a, i, &raws[k], &segs[k], &es[k]);
      m[k] = __ballot(es[k] != kReleased);
      total += __popcll(m[k]);
    }
    if (lane == 0) wtot[w] = total;
    __syncthreads();
    int64_t run = a.blk_pre[blockIdx.x];
    for (int v = 0; v < w; ++v) run += wtot[v];
#pragma unroll
    for (int k = 0; k < kRlIter; ++k) {
      const int64_t i = row0 + k * 64 + lane;
      if (i < a.N) rl_move<true>(a, i, raws[k], segs[k], es[k], run + lanes_below(m[k]));
      run += __popcll(m[k]);
    }
  }
}

// Every launch of one re-layout, stream-ordered.  nblk: the new table's block index
// ((Nn >> kRowBlkShift) + 2 entries), n_agg: its running sums (Rn entries).
hipError_t launch_relayout(const RelayoutArgs& a, int32_t* nblk, ResAgg* n_agg, bool compact, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.flags, 0, sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.bad, 0xFF, sizeof(unsigned long long), st)) != hipSuccess) return e;
  const int64_t nnb = (a.Nn >> kRowBlkShift) + 2;
  k_rl_blkseg<<<(unsigned)((nnb + 255) / 256), 256, 0, st>>>(a.new_off, a.Rn, a.Nn, nnb, nblk);
  if (a.Rn > 0) k_rl_agg<<<(unsigned)((a.Rn + 255) / 256), 256, 0, st>>>(a.agg, a.R, n_agg, a.Rn);
  const int64_t nb = (a.N + kRlBlkRows - 1) / kRlBlkRows;
  if (compact && nb > 0) {
    k_rl_count<<<(unsigned)nb, 256, 0, st>>>(a);
    k_rl_scan<<<1, 1024, 0, st>>>(a.blk_pre, nb);
  }
  if (a.Nn > 0) {
    const RowIndex nix{a.new_off, nblk, a.Rn};
    const int64_t quads = (a.Nn + 3) / 4;
    k_rl_fill<<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(a, nix, compact ? 1 : 0);
  }
  if (nb > 0) {
    if (compact)
      k_rl_scatter<true><<<(unsigned)nb, 256, 0, st>>>(a);
    else
      k_rl_scatter<false><<<(unsigned)nb, 256, 0, st>>>(a);
  }
  return hipGetLastError();
}

}  // namespace dm
