// dm_tick_steady.h — the split form's dense-side kernels, each stated once as a template over
// its build (dm_tick_group.h Build), and the launch code of each role.  dm_tick_group.hip
// instantiates the unmasked builds and dm_tick_masked.hip the masked ones: two code objects.
#pragma once
#include <algorithm>

#include "dm_tick_group.h"

namespace dm {

// The workgroup bins split by the dense hint (launch_bin_dense / launch_bin_rest):
// k_block_dense decides the items whose hint is set without the subclients column
// (128 x 8: 73 VGPRs, 6 waves per SIMD instead of 5; its steady builds 66 and 7: 14336
// rows in flight per CU) and queues the others; k_block_rest decides the queue with the
// mixed body, a grid striding over it (sized from the last split tick's queue; an empty queue costs
// one small launch).  qcnt is a two-slot ring: this tick's count in qcnt[par], and
// k_block_rest clears qcnt[par ^ 1] for the next tick (stream order); host_count
// (host-mapped) tells the host how many items went to the queue (its choice of
// split or mixed), written only when the count differs from the last one written
// (qcnt[2]): a system-scope store to host memory keeps an otherwise empty launch
// alive ~2 us longer, every tick of a dense store.
// When the host skips k_block_rest (every item of the bin verified dense in this row
// epoch, dm_tick.cpp), `guard` (host-mapped) is set should the dense kernel queue
// an item after all, which the host reports as DM_E_INTERNAL (and refuses the store)
// instead of leaving the item undecided unnoticed.  The tick's last kernel (this one,
// or the rest kernel) is launched with the tick's stop event when another queue waits
// for the tick (dm_ctx.h tick_ev).
// (128 x 8 held to 7 waves per SIMD: 71 VGPRs + 20 B of spill, C3 430 -> 590 us; round 5.)
// kSkip: the build a writeback tick in place runs (group_segment: unchanged runs of gets
// are not stored); every other tick runs the build without it.
// kSteady: the builds for a part the host knows to hold only dense items without released
// rows or arrivals, outside recompute mode (group_segment: Clean's result is known; an item
// it is not known for is queued, so the rest kernel follows every steady launch).  As a
// run-time branch in one build the two bodies need 84-87 VGPRs (5 waves per SIMD).
// kFixed: the steady build of a part ticking in place.  Each item has a key (dm_device.h
// FixKey; `keys` runs parallel to `items`, read by this build alone) that the build sets when
// the item's tick changed nothing, and clears when it did or hands the item to other code; with
// use_keys (the part's last tick was this build too and no call has written rows since:
// dm_ctx.h fix_live) an item whose key still matches its capacity and kind loads no row.
// kMasked: a part under DM_KEEP_FREE_SLOTS whose density record shows items with mask bits
// (dm_split_form.h PartForm::masked).  The key rules do not change.
template <int G, int R, Build BUILD>
__global__ __launch_bounds__(G) void k_block_dense(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                   int32_t* queue, int32_t* qcnt, int par,
                                                   int32_t* general_list, int32_t* general_count,
                                                   int32_t* guard, FixKey* __restrict__ keys, int use_keys) {
  constexpr bool FIXED = has_build(BUILD, kFixed);
  __shared__ Lds<G> lds;
  if ((int)blockIdx.x < nitems) {
    const WorkItem wi = items[blockIdx.x];
    // (two statements of the branch, not one over conditional arguments: that moves the builds' code)
    if constexpr (FIXED) {
      const FixKey fk = keys[blockIdx.x];
      if ((wi.n >> 16) == 0) {
        if (threadIdx.x == 0)
          hand_off<true>(keys + blockIdx.x, fk, use_keys, queue, qcnt, par, (int32_t)blockIdx.x, nitems, guard);
      } else {
        group_segment<G, R, kDenseOnly, BUILD>(p, wi, items + blockIdx.x, threadIdx.x, lds, general_list,
                                               general_count, queue, qcnt + par, (int32_t)blockIdx.x, guard, nitems,
                                               keys + blockIdx.x, fk, use_keys);
      }
    } else if ((wi.n >> 16) == 0) {
      if (threadIdx.x == 0)
        hand_off<false>(nullptr, FixKey{0, 0, 0}, 0, queue, qcnt, par, (int32_t)blockIdx.x, nitems, guard);
    } else {
      group_segment<G, R, kDenseOnly, BUILD>(p, wi, items + blockIdx.x, threadIdx.x, lds, general_list, general_count,
                                             queue, qcnt + par, (int32_t)blockIdx.x, guard, nitems);
    }
  }
}

// The sweep's append: a ballot and prefix within the wave, one LDS step across the waves, one
// returning atomicAdd per 1,024 items on the count word (one per item or
// wave on one word).  The lane's slot in the list, or nitems and beyond for none.
__device__ __forceinline__ int sweep_slot(bool app, int32_t* lcnt, int par, int* wtot) {
  const uint64_t bal = __ballot(app);
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int pre = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wtot[wave] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {  // the waves' totals -> their first slots in the list
    int tot = 0;
    for (int w = 0; w < 16; ++w) tot += wtot[w];
    int base = tot > 0 ? atomicAdd(lcnt + par, tot) : 0;
    for (int w = 0; w < 16; ++w) {
      const int c = wtot[w];
      wtot[w] = base;
      base += c;
    }
  }
  __syncthreads();
  return wtot[wave] + pre;  // (below nitems: the slot's count started at zero)
}

// The sweep: a kFixed launch with keys in use spends a workgroup on every item only to find,
// from two scalar loads, that most need no rows (C3: 69,400 of 100,000; such a launch over
// items all at their fixed point runs 55 us with no row loaded, profiles/sweep_share.md).  That
// test is a lane's work.  k_sweep takes one lane per item of the part (sweep_lane,
// dm_tick_group.h): an item that passes every test is done, any other is appended to the
// part's worklist with its key in memory cleared.  k_block_list then runs the kFixed build
// over the worklist alone: every item it sees has an invalid key in memory, so it loads none
// (FixKey{0, 0, 0}), loads its rows at once and stores a key only for an item that turns out
// fixed.  Everything behind the key test (the rest queue, k_general's list, the keys) is
// group_segment's code.  The list's order varies from run to run; no result depends on it
// (resources are independent, each one's sums stay in its workgroup's fixed order).
// lcnt is a two-slot ring as qcnt is: this tick's count in lcnt[par], the sweep clears
// lcnt[par ^ 1]; the list kernel tells the host the count (tell_count: lcnt[2], lcnt[3]).
// CYCLE: a steady writeback tick that writes the alternate column (dm_device.h CycAux: the
// key's states and the proof; dm_split_form.h: when; cycle_step: what a lane does).  A listed
// item's entry carries what the row kernel must know before its loads (SweepEntry::pad): whether
// to load the destination rows and whether the back-off goes on.  Without use_keys (the part's
// last tick was no cycle-form tick, or a call wrote rows since) every key counts as state 0:
// every item is listed, stores every run and gets a fresh key.  In place aux and use_keys are
// unused.  MASKED: on the alternate column a masked row's destination value joins the probe's
// comparison like any other row's, and the first cycle-form tick stores every run.
template <bool CYCLE, bool MASKED>
__global__ __launch_bounds__(1024) void k_sweep(DevParams p, const WorkItem* __restrict__ items, int nitems,
                                                FixKey* __restrict__ keys, CycAux* __restrict__ aux,
                                                SweepEntry* __restrict__ list, int32_t* lcnt, int par, int use_keys) {
  __shared__ int wtot[16];
  const int i = (int)(blockIdx.x * 1024u + threadIdx.x);
  if (i == 0) lcnt[par ^ 1] = 0;
  bool app = false;
  LaneClass c{false, false, 0, 0};
  WorkItem wi{0, 0, 0};
  if (i < nitems) {
    wi = items[i];
    const FixKey fk = keys[i];
    CycAux ax{0, 0, 0};
    if constexpr (CYCLE) ax = aux[i];
    c = sweep_lane<CYCLE, MASKED, false>(p, wi, fk, CYCLE && !use_keys ? 0 : fk.valid, CYCLE ? aux + i : nullptr, ax);
    if (!c.done) {
      app = true;
      if (fk.valid) keys[i] = FixKey{0, 0, 0};
    }
  }
  const int slot = sweep_slot(app, lcnt, par, wtot);
  if (app && slot < nitems) list[slot] = SweepEntry{wi.seg, wi.n, wi.lo, i, {c.probe, c.carry, 0}};
}

// (the cycle form's: stamp, the host's stamp of this launch; tell, the count is told whether it
// changed or not, while the host waits to judge the form by a count of a known tick: CycleAuto)
template <int G, int R, bool CYCLE, bool MASKED>
__global__ __launch_bounds__(G) void k_block_list(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                  const SweepEntry* __restrict__ list, int32_t* lcnt, int lpar,
                                                  unsigned long long* host_count, unsigned long long epoch,
                                                  int32_t* queue, int32_t* qcnt, int par, int32_t* general_list,
                                                  int32_t* general_count, FixKey* __restrict__ keys,
                                                  CycAux* __restrict__ aux, unsigned stamp, int tell) {
  constexpr Build BUILD = (CYCLE ? kCycle : kFixed | kList) | (MASKED ? kMasked : 0u);
  __shared__ Lds<G> lds;
  const int count = min(lcnt[lpar], nitems);
  SweepEntry e = list[blockIdx.x];  // with the count (the grid is at most nitems: in the list, used only below count)
  tell_count(blockIdx.x == 0 && threadIdx.x == 0, lcnt + 2, count, host_count, epoch, CYCLE ? stamp : 0u, CYCLE && tell);
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    if (q != (int)blockIdx.x) e = uniform(list[q]);
    const WorkItem wi{e.seg, e.n, e.lo};
    // (the lane index anew for every item: what the compiler derives from it once for the
    // whole loop stays in VGPRs across the item's passes: 103 against 65)
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    if ((wi.n >> 16) == 0) {  // (its key is invalid in memory: the sweep saw to it)
      if (threadIdx.x == 0) hand_off<false>(nullptr, FixKey{0, 0, 0}, 0, queue, qcnt, par, e.idx, nitems, nullptr);
    } else {
      CycAux ax{0, 0, 0};
      if constexpr (CYCLE) ax = uniform(aux[e.idx]);
      group_segment<G, R, kDenseOnly, BUILD>(p, wi, items + e.idx, t, lds, general_list, general_count, queue,
                                             qcnt + par, e.idx, nullptr, nitems, keys + e.idx, FixKey{0, 0, 0},
                                             CYCLE ? 0 : 1, CYCLE ? aux + e.idx : nullptr, ax, e.pad[0], e.pad[1]);
    }
    __syncthreads();  // the next item reuses the single-use LDS slots
  }
}

// The launch code of launch_bin_dense, launch_bin_sweep and launch_bin_cycle (dm_launch.h), by
// MASKED: dm_tick_group.hip defines the three over the unmasked halves and hands a masked
// launch to the two functions dm_tick_masked.hip defines over the masked ones.
template <bool MASKED>
static hipError_t launch_dense_build(const BinItems& w, const DevParams& p, const SplitArgs& a, hipEvent_t done,
                                     bool steady, FixKey* keys, bool use_keys, hipStream_t st) {
  const int n = w.n;
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)n);
  // in place (the gets go to the column the has came from): the build that skips unchanged runs
  const bool skip = p.writeback && p.out_gets == p.has;
  if (keys && !(skip && steady)) return hipErrorInvalidValue;
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    auto launch = [&](auto build) {
      hipExtLaunchKernelGGL((k_block_dense<G, R, decltype(build)::value>), grid, dim3(G), 0, st, nullptr, done, 0, p,
                            w.items, n, a.queue, a.qcnt, a.par, a.glist, a.gcount, a.guard, keys, use_keys ? 1 : 0);
    };
    constexpr Build kM = MASKED ? kMasked : 0u;
    if (keys) return launch(std::integral_constant<Build, kFixed | kM>{});
    with_bool(skip, [&](auto sk) {
      constexpr Build kS = decltype(sk)::value ? kSkip : 0u;
      if (MASKED || steady) return launch(std::integral_constant<Build, kS | kSteady | kM>{});
      if constexpr (!MASKED) launch(std::integral_constant<Build, kS>{});
    });
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

// The sweep (in place; aux null, keys in use) or the cycle form, and the row kernel.
template <bool CYCLE, bool MASKED>
static hipError_t launch_list_build(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw,
                                    CycAux* aux, bool use_keys, unsigned stamp, bool tell, hipStream_t st) {
  const int n = w.n;
  if (n <= 0) return hipSuccess;
  if (!p.writeback || (p.out_gets != p.has) != CYCLE || !sw.keys || (CYCLE && !aux)) return hipErrorInvalidValue;
  const dim3 lg((unsigned)std::max(1, std::min(n, use_keys ? sw.list_grid : n)));
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    k_sweep<CYCLE, MASKED><<<dim3((unsigned)((n + 1023) / 1024)), dim3(1024), 0, st>>>(
        p, w.items, n, sw.keys, aux, sw.list, sw.lcnt, sw.lpar, use_keys ? 1 : 0);
    k_block_list<G, R, CYCLE, MASKED><<<lg, dim3(G), 0, st>>>(p, w.items, n, sw.list, sw.lcnt, sw.lpar, sw.host_count,
                                                             sw.epoch, a.queue, a.qcnt, a.par, a.glist, a.gcount,
                                                             sw.keys, aux, stamp, tell ? 1 : 0);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

// dm_tick_masked.hip
hipError_t launch_dense_masked(const BinItems& w, const DevParams& p, const SplitArgs& a, hipEvent_t done,
                               FixKey* keys, bool use_keys, hipStream_t st);
hipError_t launch_list_masked(bool cycle, const BinItems& w, const DevParams& p, const SplitArgs& a,
                              const SweepArgs& sw, CycAux* aux, bool use_keys, unsigned stamp, bool tell,
                              hipStream_t st);

}  // namespace dm
