// dm_tick_fused.hip — the fused form of a steady dense tick (dm_split_form.h PartForm::fused):
// the sweep, the row kernel over its worklist and the rest kernel as one launch.  A unit, and so
// a code object, of its own, as dm_tick_masked.hip is: dm_tick_group.hip's device code is what
// it is without it.
//
// A part at its fixed point (or in a proven two-tick cycle) launches k_sweep (in its cycle
// build), then a row kernel over an empty list and a rest kernel over an empty queue:
// two launches that read one count each, because only the device knows the lists are empty
// (lease lengths, templates and learning ends change there).  Each costs the host and the
// stream a launch (profiles/cycle_ab.md: 16.1 us a step against 12.7 us of enqueue).
// k_block_fused makes the empty case cost nothing: a workgroup sweeps a chunk of the part's
// items, one per lane, by the sweeps' tests, and decides the few items that need rows or the
// rest body itself, with the same group_segment calls the list kernels and k_block_rest make.
// No workgroup waits for another and there is no word that every workgroup updates: a workgroup
// adds its counts to the device words only when they are not zero.
#include "dm_hier_round.h"
#include "dm_tick_group.h"

namespace dm {

// Items per workgroup, one per lane of the sweep step: G by default (C3: 782 workgroups of two
// waves, as many waves as k_sweep's 98 x 16).  DM_FUSED_CHUNK builds a variant with fewer
// (profiles/fused_ab.md).
#ifndef DM_FUSED_CHUNK
#define DM_FUSED_CHUNK 0
#endif
template <int G>
constexpr int kFusedChunk = (DM_FUSED_CHUNK > 0 && DM_FUSED_CHUNK < G) ? DM_FUSED_CHUNK : G;

// One listed item of a workgroup's chunk, in LDS: the work item, its index in the part, what the
// sweep step decided (rest: k_block_rest's body; else the row kernel's, with the cycle form's
// probe and carry: SweepEntry::pad) and the item's CycAux as the sweep step left it.
struct FusedEntry {
  int32_t seg, n;
  int64_t lo;
  int32_t idx;
  int32_t flags;  // bit 0: rest; bit 1: probe; bit 2: carry
  int32_t wait, skip;
  uint64_t prev_has;
};
static_assert(sizeof(FusedEntry) == 40, "ten dwords");

// fcnt: the form's own count words (SplitSlot::fu_cnt).  [2 s]: the items listed (row and rest
// items together, what the sweeps' worklist counts) by the fused tick of ring slot s; [4], [5]:
// the listed count and row epoch last told the host; [7]: never read (the count word of a
// hand-off that cannot happen).  This tick adds into slot par; workgroup 0 reads slot par ^ 1,
// the previous fused tick's total, complete by stream order, tells the host when it differs
// from what was last told (SplitSlot::sweep as k_block_list tells it, tell_count, without a stamp)
// and zeroes the slot.  fresh: the part's previous tick was not fused, so the slot holds an
// older tick's total, which is dropped, and the next fused tick tells whatever this one counts.
// host_rest (host-mapped, SplitSlot::fused_queued): the rest items, a two-slot ring as well, but
// added to by the workgroups that have some, in this tick's slot, so that the host knows of a
// lapse before its next choice as it does from k_block_rest (try_split: a part most of whose
// items are rest items runs the mixed kernel); workgroup 0 zeroes the other slot for the next
// fused tick, when fcnt[2 s + 1], the same count on the device, says it is not zero.
//
// ROOT: the launch also carries the root's exchange round of the previous step (dm_carry_rule.h
// has the rule and why no order is lost; RootRound, dm_launch.h).  Every lane that holds an item
// decides the round for that item's resource, rest items and items without a hint word included
// (dm_hier_round.h, K = 1): its loads are issued with the item's own, before the first of
// either is consumed, so the two dependency chains are in flight together, and its registers
// are dead before step 2.  The round reads the block the previous tick published and the root's
// store and configuration, and writes the root's rows and sums and a free template slot: nothing
// this tick's sweep touches, and nothing of another lane's.  Workgroup 0 writes the round's
// status word as k_hier_tick's does.  The builds without it take an empty argument and keep
// their device code.
struct NoRound {};
template <bool ROOT>
using RoundArg = std::conditional_t<ROOT, RootRound, NoRound>;

template <int G, int R, bool CYCLE, bool ROOT>
__global__ __launch_bounds__(G) void k_block_fused(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                   FixKey* __restrict__ keys, CycAux* __restrict__ aux, int32_t* fcnt,
                                                   int par, int fresh, unsigned long long* host_count,
                                                   unsigned long long epoch, int32_t* host_rest,
                                                   int32_t* general_list, int32_t* general_count,
                                                   RoundArg<ROOT> rnd) {
  constexpr int C = kFusedChunk<G>, W = G / 64;
  static_assert(G >= 64 && C <= G, "one item per lane");
  __shared__ Lds<G> lds;
  __shared__ FusedEntry ent[C];
  __shared__ int wtot[W];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if constexpr (ROOT)  // the round's flags (dm_hier_status)
      rnd.ha.status_out[0] = pub_flags(rnd.ha.gathered[0].x);
    int32_t* prev = fcnt + 2 * (par ^ 1);
    const int listed = prev[0], rest = prev[1];
    if (fresh)
      fcnt[4] = -1;
    else
      tell_count(true, fcnt + 4, listed, host_count, epoch, 0u, false);
    if (listed) prev[0] = 0;
    if (rest) {  // (a store to host memory keeps an otherwise empty launch alive ~2 us longer: only when needed)
      prev[1] = 0;
      __hip_atomic_store(host_rest + (par ^ 1), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }

  // ---- step 1: classify (the sweep's lane, sweep_lane, with the `rest` test made for the items
  // the sweep leaves to the row kernel as well) ----
  const int i = (int)(blockIdx.x * (unsigned)C + threadIdx.x);
  bool app = false;
  LaneClass lc{false, false, 0, 0};
  WorkItem wi{0, 0, 0};
  [[maybe_unused]] CycAux ax{0, 0, 0};
  if ((int)threadIdx.x < C && i < nitems) {
    wi = items[i];
    const FixKey fk = keys[i];
    if constexpr (CYCLE) ax = aux[i];
    [[maybe_unused]] HierLane rln;
    [[maybe_unused]] HierLoads rld;
    if constexpr (ROOT) {  // the round's loads, ahead of the item's own
      rln = hier_lane_one(rnd.ha, rnd.ha.leaf_lo + wi.seg);
      rld = hier_round_load(rnd.p, rnd.ha, rln);
    }
    const int hw = wi.n >> 16;
    lc = sweep_lane<CYCLE, false, true>(p, wi, fk, fk.valid, CYCLE ? aux + i : nullptr, ax);
    if (!lc.done) {
      app = true;
      // the key in memory as the two-kernel form leaves it before the item's rows are read:
      // the sweep clears a valid key, and the cycle form's row kernel (which does not use the
      // keys) overwrites whatever the array holds when it hands an item with a hint word off
      const bool dirty = CYCLE && lc.to_rest && hw != 0 && (fk.cbits != 0 || fk.kind != 0);
      if (fk.valid || dirty) keys[i] = FixKey{0, 0, 0};
    }
    if constexpr (ROOT) hier_round_decide<true>(rnd.p, rnd.ha, rln, rld);
  }

  // ---- step 2: compact the listed items into LDS (a ballot per wave, one LDS step across) ----
  const uint64_t bal = __ballot(app), balr = __ballot(lc.to_rest);
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  if (lane == 0) wtot[wave] = __popcll(bal) | __popcll(balr) << 16;
  __syncthreads();
  int base = 0, tot = 0, nrest = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int c = wtot[w];
    base += w < wave ? c & 0xFFFF : 0;
    tot += c & 0xFFFF;
    nrest += c >> 16;
  }
  if (tot == 0) return;  // (uniform) the steady case
  if (threadIdx.x == 0) {
    atomicAdd(fcnt + 2 * par, tot);
    if (nrest) {
      atomicAdd(fcnt + 2 * par + 1, nrest);
      __hip_atomic_fetch_add(host_rest + par, nrest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (app)
    ent[base + __popcll(bal & ((1ull << lane) - 1ull))] =
        FusedEntry{wi.seg, wi.n, wi.lo, i, (lc.to_rest ? 1 : 0) | lc.probe << 1 | lc.carry << 2, ax.wait, ax.skip, ax.prev_has};
  __syncthreads();

  // ---- step 3: the whole workgroup decides them, one after another ----
  for (int q = 0; q < tot; ++q) {
    const FusedEntry e = uniform(ent[q]);
    const WorkItem it{e.seg, e.n, e.lo};
    int t = (int)threadIdx.x;  // (anew for every item: k_block_list)
    asm volatile("" : "+v"(t));
    if (e.flags & 1) {
      group_segment<G, R, kRest>(p, it, items + e.idx, t, lds, general_list, general_count);
    } else if constexpr (CYCLE) {
      // (its own `rest` test is false: no hand-off; the queue arguments are never used)
      group_segment<G, R, kDenseOnly, kCycle>(
          p, it, items + e.idx, t, lds, general_list, general_count, fcnt, fcnt + 7, e.idx, nullptr, 0, keys + e.idx,
          FixKey{0, 0, 0}, 0, aux + e.idx, CycAux{e.prev_has, e.wait, e.skip}, e.flags >> 1 & 1, e.flags >> 2 & 1);
    } else {
      group_segment<G, R, kDenseOnly, kFixed | kList>(p, it, items + e.idx, t, lds, general_list, general_count, fcnt,
                                                      fcnt + 7, e.idx, nullptr, 0, keys + e.idx, FixKey{0, 0, 0}, 1);
    }
    __syncthreads();  // the next item reuses the single-use LDS slots
  }
}

// The launch is the part's last kernel of the tick: it completes `done` (hipExtLaunchKernel's
// stop event) as the rest launch does in the other forms.
//
// The ROOT builds are a unit, and so a code object, of their own (dm_tick_fused_root.hip, which
// includes this file with DM_FUSED_ROOT_UNIT set and defines launch_bin_fused_root): the
// kernels of this unit are then what they are without them (twice the callers of group_segment
// in one unit changed the compiler's inlining, and with it the registers of the builds here).
template <bool ROOT>
static hipError_t launch_fused_build(const BinItems& w, const DevParams& p, const FusedArgs& a,
                                     const RoundArg<ROOT>& round, hipEvent_t done, hipStream_t st) {
  const int n = w.n;
  if (n <= 0) return hipSuccess;
  const bool cycle = p.out_gets != p.has;
  if (!p.writeback || !a.keys || !a.fcnt || !a.host_rest || (cycle && !a.aux)) return hipErrorInvalidValue;
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    const dim3 grid((unsigned)((n + kFusedChunk<G> - 1) / kFusedChunk<G>));
    with_bool(cycle, [&](auto cy) {
      hipExtLaunchKernelGGL((k_block_fused<G, R, decltype(cy)::value, ROOT>), grid, dim3(G), 0, st, nullptr, done, 0, p,
                            w.items, n, a.keys, a.aux, a.fcnt, a.par, a.fresh ? 1 : 0, a.host_count, a.epoch,
                            a.host_rest, a.glist, a.gcount, round);
    });
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

#ifndef DM_FUSED_ROOT_UNIT
hipError_t launch_bin_fused(const BinItems& w, const DevParams& p, const FusedArgs& a, const RootRound* round,
                            hipEvent_t done, hipStream_t st) {
  if (round) return launch_bin_fused_root(w, p, a, *round, done, st);
  return launch_fused_build<false>(w, p, a, NoRound{}, done, st);
}
#else
hipError_t launch_bin_fused_root(const BinItems& w, const DevParams& p, const FusedArgs& a, const RootRound& round,
                                 hipEvent_t done, hipStream_t st) {
  // a carried round: one server, one root row per resource, and an item for every resource
  const HierArgs& ha = round.ha;
  if (ha.K != 1 || ha.G != 1 || ha.server != 0 || ha.r_hi - ha.r_lo != w.n || ha.r_lo != ha.leaf_lo)
    return hipErrorInvalidValue;
  return launch_fused_build<true>(w, p, a, round, done, st);
}
#endif

}  // namespace dm
