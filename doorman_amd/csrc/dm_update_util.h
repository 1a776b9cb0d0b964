// Device helpers shared by the kernels that change stored rows outside a tick: the store
// updates (dm_update.hip), the re-layout (dm_relayout.hip) and Clean (dm_clean.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"

namespace dm {

// resource owning row r: last s with seg_off[s] <= r.  A coarse index (the
// resource holding the first row of every 2^kRowBlkShift-row block) narrows the
// binary search to the few resources of r's block.
__device__ __forceinline__ int seg_of_row(const RowIndex& ix, int64_t r) {
  const int64_t* __restrict__ seg_off = ix.seg_off;
  const int64_t b = r >> kRowBlkShift;
  int64_t lo = ix.blk_seg[b];
  int64_t hi = (int64_t)ix.blk_seg[b + 1] + 1;  // invariant: seg_off[lo] <= r < seg_off[hi]
  if (hi > ix.R) hi = ix.R;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (seg_off[mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  return (int)lo;
}

// The key-clearing builds of the wants-refresh kernels (dm_update.hip, dm_device.h
// KeyClear): resource seg's fixed-point key, if it has one, becomes invalid.  A plain
// vector store of zeros: keys are cleared only by stores of this one value, so any number
// of waves may clear the same key.  (The bin's array by selects, not by an index into the
// kernel argument, which would put the four pointers into scratch.)
__device__ __forceinline__ void clear_key(const KeyClear& kc, int seg) {
  const int32_t io = kc.item_of[seg];
  if (io < 0) return;
  const int bin = io >> 24;
  FixKey* k = bin == 3 ? kc.keys[0] : bin == 4 ? kc.keys[1] : bin == 5 ? kc.keys[2] : kc.keys[3];
  if (k) k[io & 0xFFFFFF] = FixKey{0, 0, 0};
}

// Add per-row deltas to their resources' running sums: lanes of a wave that hit
// the same resource are summed first (DPP) and add once; a wave whose rows spread
// over many resources adds per lane.  Every lane of the wave must call this.
// KEYS (the key-clearing builds): `changed` says that the lane's row changed its wants
// bits; the lane that adds for a run of a resource also clears the resource's key when some
// lane of the run changed -- one store per run at most, on the spread-out path too, where
// the run is the consecutive active lanes of one resource behind a head.
template <bool KEYS = false>
__device__ __forceinline__ void wave_seg_add(ResAgg* agg, bool active, int seg, double dh, double dw, long long ds,
                                             bool with_has, bool with_count, bool changed = false,
                                             const KeyClear& kc = KeyClear{}) {
  const int lane = threadIdx.x & 63;
  const unsigned long long act = __ballot(active);
  const int prev = __shfl(seg, lane > 0 ? lane - 1 : 0, 64);
  const bool head = active && (lane == 0 || !((act >> (lane - 1)) & 1) || prev != seg);
  const unsigned long long heads = __ballot(head);
  unsigned long long chg = 0ull;
  if constexpr (KEYS) chg = __ballot(active && changed);
  if (__popcll(heads) > 8) {
    if (active) {
      if (with_has) atomicAdd(&agg[seg].sum_has, dh);
      atomicAdd(&agg[seg].sum_wants, dw);
      if (with_count) atomicAdd((unsigned long long*)&agg[seg].count, (unsigned long long)ds);
    }
    if constexpr (KEYS) {
      if (head) {  // the run: this lane up to the next head or inactive lane
        const unsigned long long above = lane == 63 ? 0ull : ~0ull << (lane + 1);
        const unsigned long long stop = (heads | ~act) & above;
        const unsigned long long upto = stop ? (1ull << __builtin_ctzll(stop)) - 1ull : ~0ull;
        if (chg & upto & ~((1ull << lane) - 1ull)) clear_key(kc, seg);
      }
    }
    return;
  }
  unsigned long long rem = act;
  while (rem) {
    const int h = __builtin_ctzll(rem);
    const int s0 = __builtin_amdgcn_readlane(seg, h);
    const unsigned long long m = __ballot(active && seg == s0) & rem;
    const bool in = (m >> lane) & 1;
    AggR v{in ? ds : 0, in ? dh : 0.0, in ? dw : 0.0};
    v = wave_reduce(v, OpR());
    if (lane == h) {
      if (with_has) atomicAdd(&agg[s0].sum_has, v.h);
      atomicAdd(&agg[s0].sum_wants, v.w);
      if (with_count) atomicAdd((unsigned long long*)&agg[s0].count, (unsigned long long)v.cnt);
      if constexpr (KEYS) {
        if (chg & m) clear_key(kc, s0);
      }
    }
    rem &= ~m;
  }
}

// one byte of a dense resource's masks (dm_device.h mask_pos), atomically: rows of one
// resource share the mask words
__device__ __forceinline__ void mask_bit(uint8_t* base, int32_t off, int32_t bit, bool set) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(base + off);
  unsigned* w = reinterpret_cast<unsigned*>(a & ~uintptr_t(3));
  const unsigned m = 1u << (bit + 8 * (int)(a & 3));
  if (set)
    atomicOr(w, m);
  else
    atomicAnd(w, ~m);
}

// The row's place in its dense resource's masks, or false when the resource is not in
// a dense state its item describes (dm_device.h DenseUpd).
__device__ __forceinline__ bool dense_row(const DenseUpd& du, const RowIndex& ix, int seg, int64_t r, uint8_t state,
                                          MaskPos* mp, WorkItem** item) {
  if (state < 2 || !du.item_of) return false;
  const int32_t io = du.item_of[seg];
  if (io < 0) return false;
  const int bin = io >> 24;
  WorkItem* it = du.bins[bin - 3] + (io & 0xFFFFFF);
  if (((it->n >> 16) & 0xFF) != state - 1) return false;  // the hint is the state's (a new shape clears hints)
  int G, R;
  bin_shape(bin, du.bin4_wave, du.bin6_wide, &G, &R);
  const int64_t lo = ix.seg_off[seg];
  *mp = mask_pos(G, R, (int)(r - lo));
  *item = it;
  return true;
}

// Release (store.go:142-151) of stored row r of resource seg, as k_release and Clean
// (dm_clean.hip) apply it: the row zeroed and marked released, and what it held returned
// negated, for the resource's running sums (wave_seg_add).
__device__ __forceinline__ void release_row(const RowIndex& ix, int seg, int64_t r, double* s_has, double* s_wants,
                                            int32_t* s_sub, uint8_t* expl, const DenseUpd& du, double* dh, double* dw,
                                            long long* ds) {
  *dh = -s_has[r];
  *dw = -s_wants[r];
  *ds = -(long long)sub_value(s_sub[r]);
  s_has[r] = 0.0;
  s_wants[r] = 0.0;
  s_sub[r] = (int32_t)kSubReleased;  // the mark every reader decodes first: the expiry column is left alone
  MaskPos mp;
  WorkItem* it;
  const uint8_t st = expl[seg];
  if (dense_row(du, ix, seg, r, st, &mp, &it)) {  // stays dense: the row into the released-row mask
    uint8_t* mb = du.rmask + rel_mask_offset(ix.seg_off[seg]);
    mask_bit(mb, mp.roff, mp.rbit, true);
    mask_bit(mb, mp.aoff, mp.abit, false);  // (a row that arrived since the last tick)
    atomicOr(&it->n, 1 << 24);
  } else if (st >= 2) {
    expl[seg] = 0;  // no longer dense: the next tick reads the subclients column
  }
}

// lanes below this one whose bit is set in a wave's ballot
__device__ __forceinline__ int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

}  // namespace dm
