// dm_tick_masked.hip — the masked builds of the steady workgroup-bin kernels (dm_keep_keys'
// DM_KEEP_FREE_SLOTS, dm_split_form.h PartForm::masked): a sibling of each steady kernel of
// dm_tick_group.hip, instantiating group_segment (dm_tick_group.h) with MASKED set, and their
// launchers.  A unit, and so a code object, of their own: dm_tick_group.hip's is what it is
// without them, the order and placement of its kernels included.
#include "dm_tick_group.h"

namespace dm {

// The masked builds (group_segment MASKED), for a part under DM_KEEP_FREE_SLOTS whose density
// record shows items with mask bits (dm_split_form.h PartForm::masked): a sibling of each
// steady kernel above, under a name of its own so that every kernel above stays the code it
// was.  Each is its twin's text with MASKED set, and the sweeps' lane tests are group_segment's
// masked `rest` test, as write_fixed's comment demands of the unmasked pair: the released-row
// bit passes, the arrival bit and an item without a live row (a running count of 0) do not.
// The key rules are the twins': FIXED's conditions and the cycle states do not change.  On the
// alternate column a masked row's destination value joins the probe's comparison like any
// other row's, and the first cycle-form tick stores every run (dm_device.h CycAux).
// k_block_dense_masked: the plain steady build (a non-writeback tick, or DM_FIXED=0).
template <int G, int R, bool SKIP>
__global__ __launch_bounds__(G) void k_block_dense_masked(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                          int32_t* queue, int32_t* qcnt, int par,
                                                          int32_t* general_list, int32_t* general_count,
                                                          int32_t* guard) {
  __shared__ Lds<G> lds;
  if ((int)blockIdx.x < nitems) {
    const WorkItem wi = items[blockIdx.x];
    if ((wi.n >> 16) == 0) {
      if (threadIdx.x == 0)
        hand_off<false>(nullptr, FixKey{0, 0, 0}, 0, queue, qcnt, par, (int32_t)blockIdx.x, nitems, guard);
    } else {
      group_segment<G, R, kDenseOnly, SKIP, true, false, false, false, true>(
          p, wi, items + blockIdx.x, threadIdx.x, lds, general_list, general_count, queue, qcnt + par,
          (int32_t)blockIdx.x, guard, nitems);
    }
  }
}

template <int G, int R>
__global__ __launch_bounds__(G) void k_block_dense_fixed_masked(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                                int32_t* queue, int32_t* qcnt, int par,
                                                                int32_t* general_list, int32_t* general_count,
                                                                int32_t* guard, FixKey* __restrict__ keys,
                                                                int use_keys) {
  __shared__ Lds<G> lds;
  if ((int)blockIdx.x < nitems) {
    const WorkItem wi = items[blockIdx.x];
    const FixKey fk = keys[blockIdx.x];
    if ((wi.n >> 16) == 0) {
      if (threadIdx.x == 0)
        hand_off<true>(keys + blockIdx.x, fk, use_keys, queue, qcnt, par, (int32_t)blockIdx.x, nitems, guard);
    } else {
      group_segment<G, R, kDenseOnly, true, true, true, false, false, true>(
          p, wi, items + blockIdx.x, threadIdx.x, lds, general_list, general_count, queue, qcnt + par,
          (int32_t)blockIdx.x, guard, nitems, keys + blockIdx.x, fk, use_keys);
    }
  }
}

// The two sweeps' appends (k_fixed_sweep has the account): the lane's slot in the list, or
// nitems and beyond for none.
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

__global__ __launch_bounds__(1024) void k_fixed_sweep_masked(DevParams p, const WorkItem* __restrict__ items,
                                                             int nitems, FixKey* __restrict__ keys,
                                                             SweepEntry* __restrict__ list, int32_t* lcnt, int par) {
  __shared__ int wtot[16];
  const int i = (int)(blockIdx.x * 1024u + threadIdx.x);
  if (i == 0) lcnt[par ^ 1] = 0;
  bool app = false;
  WorkItem wi{0, 0, 0};
  if (i < nitems) {
    wi = items[i];
    const FixKey fk = keys[i];
    const int hw = wi.n >> 16;
    bool done = false;
    if (hw != 0 && fk.valid) {
      const Res rs = load_res(p, wi.seg);
      const int hint = hw & 0xFF;
      const bool rest = dense_subclients(rs) != hint || (hw >> 8 & 2) != 0 || p.now > rs.follow_exp || p.recompute ||
                        rs.agg_count == 0;
      if (!rest && fk.cbits == (uint64_t)__double_as_longlong(rs.C) && fk.kind == rs.kind && !rs.learning) {
        write_fixed(p, wi.seg, rs, hint);
        done = true;
      }
    }
    if (!done) {
      app = true;
      if (fk.valid) keys[i] = FixKey{0, 0, 0};
    }
  }
  const int slot = sweep_slot(app, lcnt, par, wtot);
  if (app && slot < nitems) list[slot] = SweepEntry{wi.seg, wi.n, wi.lo, i, {0, 0, 0}};
}

template <int G, int R>
__global__ __launch_bounds__(G) void k_block_dense_list_masked(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                               const SweepEntry* __restrict__ list, int32_t* lcnt,
                                                               int lpar, unsigned long long* host_count,
                                                               unsigned long long epoch, int32_t* queue, int32_t* qcnt,
                                                               int par, int32_t* general_list, int32_t* general_count,
                                                               FixKey* __restrict__ keys) {
  __shared__ Lds<G> lds;
  const int count = min(lcnt[lpar], nitems);
  SweepEntry e = list[blockIdx.x];  // with the count (the grid is at most nitems: in the list, used only below count)
  if (blockIdx.x == 0 && threadIdx.x == 0 && (lcnt[2] != count || lcnt[3] != (int32_t)epoch)) {
    __hip_atomic_store(host_count, (unsigned long long)(unsigned)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host_count + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    lcnt[2] = count;
    lcnt[3] = (int32_t)epoch;
  }
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    if (q != (int)blockIdx.x) e = uniform(list[q]);
    const WorkItem wi{e.seg, e.n, e.lo};
    int t = (int)threadIdx.x;  // (anew for every item: k_block_dense_list)
    asm volatile("" : "+v"(t));
    if ((wi.n >> 16) == 0) {  // (its key is invalid in memory: the sweep saw to it)
      if (threadIdx.x == 0) hand_off<false>(nullptr, FixKey{0, 0, 0}, 0, queue, qcnt, par, e.idx, nitems, nullptr);
    } else {
      group_segment<G, R, kDenseOnly, true, true, true, true, false, true>(
          p, wi, items + e.idx, t, lds, general_list, general_count, queue, qcnt + par, e.idx, nullptr, nitems,
          keys + e.idx, FixKey{0, 0, 0}, 1);
    }
    __syncthreads();  // the next item reuses the single-use LDS slots
  }
}

__global__ __launch_bounds__(1024) void k_cycle_sweep_masked(DevParams p, const WorkItem* __restrict__ items,
                                                             int nitems, FixKey* __restrict__ keys,
                                                             CycAux* __restrict__ aux, SweepEntry* __restrict__ list,
                                                             int32_t* lcnt, int par, int use_keys) {
  __shared__ int wtot[16];
  const int i = (int)(blockIdx.x * 1024u + threadIdx.x);
  if (i == 0) lcnt[par ^ 1] = 0;
  bool app = false;
  int probe = 0, carry = 0;
  WorkItem wi{0, 0, 0};
  if (i < nitems) {
    wi = items[i];
    const FixKey fk = keys[i];
    const CycAux ax = aux[i];
    const int hw = wi.n >> 16;
    const int state = use_keys ? fk.valid : 0;
    bool done = false;
    if (hw != 0 && state != 0) {
      const Res rs = load_res(p, wi.seg);
      const int hint = hw & 0xFF;
      const bool rest = dense_subclients(rs) != hint || (hw >> 8 & 2) != 0 || p.now > rs.follow_exp || p.recompute ||
                        rs.agg_count == 0;
      if (!rest && fk.cbits == (uint64_t)__double_as_longlong(rs.C) && fk.kind == rs.kind && !rs.learning) {
        if (state == 2) {
          write_resource(p, wi.seg, rs, Clean{rs.agg_count, __longlong_as_double((long long)ax.prev_has), rs.agg_wants},
                         0.0, hint);
          const uint64_t was = (uint64_t)__double_as_longlong(rs.agg_has);
          if (ax.prev_has != was) aux[i].prev_has = was;
          done = true;
        } else if (ax.skip > 0) {
          aux[i].skip = ax.skip - 1;
          carry = 1;
        } else {
          probe = carry = 1;
        }
      }
    }
    if (!done) {
      app = true;
      if (fk.valid) keys[i] = FixKey{0, 0, 0};
    }
  }
  const int slot = sweep_slot(app, lcnt, par, wtot);
  if (app && slot < nitems) list[slot] = SweepEntry{wi.seg, wi.n, wi.lo, i, {probe, carry, 0}};
}

template <int G, int R>
__global__ __launch_bounds__(G) void k_block_cycle_list_masked(DevParams p, WorkItem* __restrict__ items, int nitems,
                                                               const SweepEntry* __restrict__ list, int32_t* lcnt,
                                                               int lpar, unsigned long long* host_count,
                                                               unsigned long long epoch, int32_t* queue, int32_t* qcnt,
                                                               int par, int32_t* general_list, int32_t* general_count,
                                                               FixKey* __restrict__ keys, CycAux* __restrict__ aux,
                                                               unsigned stamp, int tell) {
  __shared__ Lds<G> lds;
  const int count = min(lcnt[lpar], nitems);
  SweepEntry e = list[blockIdx.x];  // with the count (the grid is at most nitems: in the list, used only below count)
  if (blockIdx.x == 0 && threadIdx.x == 0 && (tell || lcnt[2] != count || lcnt[3] != (int32_t)epoch)) {
    __hip_atomic_store(host_count, (unsigned long long)(unsigned)count | (unsigned long long)stamp << 32,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host_count + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    lcnt[2] = count;
    lcnt[3] = (int32_t)epoch;
  }
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    if (q != (int)blockIdx.x) e = uniform(list[q]);
    const WorkItem wi{e.seg, e.n, e.lo};
    int t = (int)threadIdx.x;  // (anew for every item: k_block_dense_list)
    asm volatile("" : "+v"(t));
    if ((wi.n >> 16) == 0) {  // (its key is invalid in memory: the sweep saw to it)
      if (threadIdx.x == 0) hand_off<false>(nullptr, FixKey{0, 0, 0}, 0, queue, qcnt, par, e.idx, nitems, nullptr);
    } else {
      const CycAux ax = uniform(aux[e.idx]);
      group_segment<G, R, kDenseOnly, true, true, true, true, true, true>(
          p, wi, items + e.idx, t, lds, general_list, general_count, queue, qcnt + par, e.idx, nullptr, nitems,
          keys + e.idx, FixKey{0, 0, 0}, 0, aux + e.idx, ax, e.pad[0], e.pad[1]);
    }
    __syncthreads();  // the next item reuses the single-use LDS slots
  }
}

// --------------------------------------------------------------------------
// host-side launchers (called by dm_tick.cpp): launch_bin_dense's steady builds,
// launch_bin_sweep and launch_bin_cycle (dm_tick_group.hip) with the masked kernels, under
// the same conditions; the rest launch follows each.
// --------------------------------------------------------------------------
hipError_t launch_bin_dense_masked(const BinItems& w, const DevParams& p, const SplitArgs& a, hipEvent_t done,
                                   FixKey* keys, bool use_keys, hipStream_t st) {
  const int n = w.n;
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)n);
  const bool skip = p.writeback && p.out_gets == p.has;
  if (keys && !skip) return hipErrorInvalidValue;
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    if (keys) {
      hipExtLaunchKernelGGL((k_block_dense_fixed_masked<G, R>), grid, dim3(G), 0, st, nullptr, done, 0, p, w.items, n,
                            a.queue, a.qcnt, a.par, a.glist, a.gcount, a.guard, keys, use_keys ? 1 : 0);
      return;
    }
    with_bool(skip, [&](auto sk) {
      hipExtLaunchKernelGGL((k_block_dense_masked<G, R, decltype(sk)::value>), grid, dim3(G), 0, st, nullptr, done, 0,
                            p, w.items, n, a.queue, a.qcnt, a.par, a.glist, a.gcount, a.guard);
    });
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_bin_sweep_masked(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw,
                                   hipStream_t st) {
  const int n = w.n;
  if (n <= 0) return hipSuccess;
  if (!(p.writeback && p.out_gets == p.has) || !sw.keys) return hipErrorInvalidValue;
  const dim3 lg((unsigned)std::max(1, std::min(n, sw.list_grid)));
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    k_fixed_sweep_masked<<<dim3((unsigned)((n + 1023) / 1024)), dim3(1024), 0, st>>>(p, w.items, n, sw.keys, sw.list,
                                                                                     sw.lcnt, sw.lpar);
    k_block_dense_list_masked<G, R><<<lg, dim3(G), 0, st>>>(p, w.items, n, sw.list, sw.lcnt, sw.lpar, sw.host_count,
                                                            sw.epoch, a.queue, a.qcnt, a.par, a.glist, a.gcount,
                                                            sw.keys);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_bin_cycle_masked(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw,
                                   CycAux* aux, bool use_keys, unsigned stamp, bool tell, hipStream_t st) {
  const int n = w.n;
  if (n <= 0) return hipSuccess;
  if (!(p.writeback && p.out_gets != p.has) || !sw.keys || !aux) return hipErrorInvalidValue;
  const dim3 lg((unsigned)std::max(1, std::min(n, use_keys ? sw.list_grid : n)));
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    k_cycle_sweep_masked<<<dim3((unsigned)((n + 1023) / 1024)), dim3(1024), 0, st>>>(
        p, w.items, n, sw.keys, aux, sw.list, sw.lcnt, sw.lpar, use_keys ? 1 : 0);
    k_block_cycle_list_masked<G, R><<<lg, dim3(G), 0, st>>>(p, w.items, n, sw.list, sw.lcnt, sw.lpar, sw.host_count,
                                                            sw.epoch, a.queue, a.qcnt, a.par, a.glist, a.gcount,
                                                            sw.keys, aux, stamp, tell ? 1 : 0);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace dm
