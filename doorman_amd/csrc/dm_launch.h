// dm_launch.h — the host-side launchers the kernel units define and the runtime's host units
// (dm_ctx.h and the .cpp files around it) call.
// Every unit that defines one includes this header, so a definition that drifts from its
// declaration fails to compile instead of failing to link.
#pragma once
#include <hip/hip_runtime.h>

#include "dm_device.h"
#include "dm_large_form.h"

namespace dm {
// dm_tick_group.hip
hipError_t launch_tile_small(const DevParams& p, const Tile* tiles, const TileEntry* list, int n, hipStream_t st);
// The workgroup bins' launchers (bins 3-6) take the launch's items as one argument, and
// the split form's take the device side of the part's split slot (dm_ctx.h SplitSlot) as
// another.  Host-side only: each launcher unpacks them into its kernel's own arguments.
struct BinItems {
  int bin;  // the shape: the bin, or kBin4Wave / kBin6Wide
  WorkItem* items;
  int n;
};
struct SplitArgs {
  int32_t *queue, *qcnt;  // the rest queue and its count ring ...
  int par;                // ... and this tick's slot of it
  int32_t *glist, *gcount;  // k_general's worklist and its count
  int32_t* guard;  // (host-mapped, or null) set should the launch queue an item
};
struct SweepArgs {
  FixKey* keys;
  SweepEntry* list;  // the sweep's worklist, ...
  int32_t* lcnt;     // ... its count ring ...
  int lpar;          // ... and this tick's slot of it
  unsigned long long *host_count, epoch;  // (host-mapped) where the row kernel tells {count, row epoch}
  int list_grid;  // the row kernel's workgroups, a hint (it strides over the list)
};
hipError_t launch_bin(const BinItems& w, const DevParams& p, int32_t* glist, int32_t* gcount, hipStream_t st);
hipError_t launch_subs(const DevParams& p, const SubBins& sb, int32_t* glist, int32_t* gcount, hipStream_t st);
// The split form's dense side.  masked: the form's masked builds (PartForm::masked, which
// implies steady; dm_tick_masked.hip holds them).
// done (optional): an event the launch itself completes (hipExtLaunchKernel's stop event: no
// marker packet of its own on the queue), for another stream to wait on.  steady: the builds
// that take Clean's result as known and queue every item it is not known for (group_segment
// kSteady); the caller launches the rest kernel after them.  keys (optional; only with steady,
// on a writeback tick in place): the kFixed build, over the keys of these items; use_keys:
// valid keys may be trusted (else every key is rewritten).
hipError_t launch_bin_dense(const BinItems& w, const DevParams& p, const SplitArgs& a, hipEvent_t done, bool steady,
                            bool masked, FixKey* keys, bool use_keys, hipStream_t st);
// A kFixed launch with keys in use (a writeback tick in place), as the sweep and the row
// kernel over its worklist (k_sweep, k_block_list): the rest launch follows as after
// launch_bin_dense's steady builds.
hipError_t launch_bin_sweep(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw, bool masked,
                            hipStream_t st);
// The cycle form: a steady writeback tick on the alternate column, through the same two
// kernels' cycle builds.  The first such launch of a part (use_keys false) lists and rewrites
// every item; the rest launch follows either.
hipError_t launch_bin_cycle(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw, bool masked,
                            CycAux* aux, bool use_keys, unsigned stamp, bool tell, hipStream_t st);
hipError_t launch_count_keys(const FixKey* keys, int n, int32_t* out, hipStream_t st);
hipError_t launch_count_cycle(const FixKey* keys, const CycAux* aux, const WorkItem* items, const ResAgg* agg, int n,
                              int32_t* out, hipStream_t st);
hipError_t launch_count_undense(const WorkItem* items, int n, unsigned long long* rec, unsigned long long epoch,
                                hipStream_t st);
hipError_t launch_bin_rest(const BinItems& w, const DevParams& p, const SplitArgs& a, int32_t* host_count,
                           int rest_grid, hipEvent_t done, hipStream_t st);
// dm_tick_fused.hip: the sweep or the cycle form (by the tick's output column) with keys in
// use, the row kernel and the rest kernel as one launch (PartForm::fused); `done` as
// launch_bin_rest's
struct FusedArgs {
  FixKey* keys;
  CycAux* aux;    // the cycle form's half of the keys (unused in place)
  int32_t* fcnt;  // the form's own count words (SplitSlot::fu_cnt) ...
  int par;        // ... and this tick's slot of their ring
  bool fresh;     // the part's previous tick was not fused: the other slot's totals are not told
  unsigned long long *host_count, epoch;  // (host-mapped) {count, row epoch}, as SweepArgs'
  int32_t* host_rest;                     // (host-mapped) the rest items' two-slot ring (SplitSlot::fused_queued)
  int32_t *glist, *gcount;                // k_general's worklist and its count
};
// A root round that rides in the launch (dm_carry_rule.h; k_block_fused's ROOT build): the
// DevParams / HierArgs pair launch_hier_tick would have taken, the round's own `now` in p.now.
// One server, one root row per resource (K = 1), and the launch's items are every resource of
// the leaf: the lane of leaf item i decides root resource ha.leaf_lo + items[i].seg.
struct RootRound {
  DevParams p;
  HierArgs ha;
};
// round: null, or the round the launch carries (launch_bin_fused_root, dm_tick_fused_root.hip)
hipError_t launch_bin_fused_root(const BinItems& w, const DevParams& p, const FusedArgs& a, const RootRound& round,
                                 hipEvent_t done, hipStream_t st);
hipError_t launch_bin_fused(const BinItems& w, const DevParams& p, const FusedArgs& a, const RootRound* round,
                            hipEvent_t done, hipStream_t st);
// dm_tick_large.hip
int redo_blocks_per_cu();
// The chain's one launcher takes the phase (dm_large_form.h LargePhase: each names its
// kernel) and what the chain's kernels share as one argument.  Host-side only: the launcher
// unpacks it into the kernel's own arguments.  The grid is the phase's (dm_large_chain.h
// LargeChain::grid), and S is read by the speculative form's phases alone.
struct LargeArgs {
  const Chunk* chunks;
  const LargeSeg* ls;
  Partials P;
  SpecArgs S;
  int32_t *glist, *gcount;  // k_general's worklist and its count
};
hipError_t launch_large(LargePhase ph, dim3 grid, const DevParams& p, const LargeArgs& a, hipStream_t st);
// dm_tick_general.hip
hipError_t launch_general(const DevParams& p, const int32_t* glist, const int32_t* gcount, int blocks,
                          hipStream_t st);
// dm_update.hip
// The store's columns as the update launchers take them (dm_ctx::store_cols builds it).
// Host-side only: each launcher unpacks it into its kernel's own arguments.
struct StoreCols {
  RowIndex ix;
  double *has, *wants;
  int32_t* sub;
  int64_t* expiry;
  ResAgg* agg;
  uint8_t* expl;
  const ResCfg* cfg;
};
// kc (the upsert, release and refresh launchers): null launches the plain kernel; else its
// key-clearing build (dm_row_epoch.h row_write_start_mode says when)
hipError_t launch_upsert(int64_t n, const int64_t* rows, const double* has, const double* wants, const int64_t* sub,
                         const int32_t* sub32, const int64_t* expiry, int64_t now, const StoreCols& s,
                         const uint32_t* flags, const DenseUpd& du, const KeyClear* kc, hipStream_t st);
hipError_t launch_release(int64_t n, const int64_t* rows, const StoreCols& s, const uint32_t* flags,
                          const DenseUpd& du, const KeyClear* kc, hipStream_t st);
hipError_t launch_check_rows(int64_t n, const int64_t* rows, int64_t N, uint32_t* bitmap, const double* wants,
                             const int64_t* sub, const int32_t* sub32, uint32_t* flags, hipStream_t st);
hipError_t launch_clear_rows(int64_t n, const int64_t* rows, int64_t N, uint32_t* bitmap, hipStream_t st);
hipError_t launch_resolve_rows(int64_t n, const int64_t* rows, int64_t off, const int32_t* sub, const int64_t* expiry,
                               const RowIndex& ix, const ResAgg* agg, int64_t* out_exp, int64_t* out_sub,
                               hipStream_t st);
hipError_t launch_gather_leases(int64_t n, const int64_t* rows, const double* gets, const int64_t* expiry,
                               double* out_gets, int64_t* out_exp, hipStream_t st);
hipError_t launch_update_wants(int64_t n, const int64_t* rows, const double* wants, const StoreCols& s,
                               const uint32_t* flags, const KeyClear* kc, hipStream_t st);
// phase 0: the mask's count and scan; 1: the apply of the values [vlo, vhi); 2: both
hipError_t launch_update_wants_mask(int64_t nwords, const uint64_t* mask, int64_t first_row, int64_t N,
                                    int64_t n_values, const double* wants, int64_t* block_sums, int32_t* word_pre,
                                    const StoreCols& s, uint32_t* flags, int phase, int64_t vlo, int64_t vhi,
                                    const KeyClear* kc, hipStream_t st);
hipError_t launch_refresh_dense(int64_t n, int64_t first_row, const double* wants, const StoreCols& s, uint32_t* flags,
                                unsigned long long* count, const KeyClear* kc, hipStream_t st);
hipError_t launch_carry_reject(const uint32_t* from, uint32_t* to, hipStream_t st);
// dm_hier.hip
hipError_t launch_publish(int64_t R, const ResAgg* agg, void* dst, uint32_t* sync, hipStream_t st);
hipError_t launch_hier_tick(const DevParams& p, const HierArgs& ha, hipStream_t st);
// dm_round.hip
hipError_t launch_decide(const DevParams& p, const ReqItem* items, int nitems, const ReqArgs& q, hipStream_t st);
// dm_decide_fast.hip
hipError_t fd_rows(const DevParams& p, const ReqItem& it, const FastItem& fi, int slot, const ReqArgs& q,
                   const FastArgs& fa, hipStream_t st);
hipError_t fd_item(const DevParams& p, const ReqItem& it, const FastItem& fi, int slot, const ReqArgs& q,
                   const FastArgs& fa, FdScan* part, hipStream_t st);
hipError_t fd_item_sorted(const DevParams& p, const ReqItem& it, const FastItem& fi, int slot, const ReqArgs& q,
                          const FastArgs& fa, FdScan* part, hipStream_t st);
hipError_t fd_sort_keys(void* temp, size_t* bytes, const double* in, double* out, int64_t n, hipStream_t st);
hipError_t fd_sort_pairs(void* temp, size_t* bytes, const double* kin, double* kout, const int32_t* vin,
                         int32_t* vout, int64_t n, int nseg, const int64_t* begin, const int64_t* end,
                         hipStream_t st);
// dm_decide_assign.hip: the selected requests' values into the compact columns; the safe
// capacity of each of n requests' resources (rows: the requests' rows, in the store's range)
hipError_t launch_assign_gather(const ReqArgs& q, const AssignArgs& a, hipStream_t st);
hipError_t launch_safe_capacity(int64_t n, const int64_t* rows, const RowIndex& ix, const ResCfg* cfg,
                                const ResCold* cold, const ResAgg* agg, double* safe, hipStream_t st);
// dm_relayout.hip (launch_rl_scan: the in-place scan dm_clean.hip shares)
hipError_t launch_rl_scan(int64_t* v, int64_t n, hipStream_t st);
hipError_t launch_relayout(const RelayoutArgs& a, int32_t* nblk, ResAgg* n_agg, bool compact, hipStream_t st);
// dm_clean.hip
hipError_t launch_clean_count(const CleanArgs& a, hipStream_t st);
hipError_t launch_clean_apply(const CleanArgs& a, const DenseUpd& du, bool peek, hipStream_t st);
// dm_load.hip
// A snapshot whose columns are device memory (dm_store_load_device), as its kernels take it:
// the caller's columns, read only, and the context's flags word.
struct LoadArgs {
  int64_t R, N;
  const double *wants, *has;
  const int64_t *sub, *expiry;
  const int64_t* agg_count;  // the three running sums, or all null: one Assign per row in row order
  const double *agg_sum_has, *agg_sum_wants;
  uint32_t* flags;
};
constexpr uint32_t kLdBadSub = 1u;   // a subclients value outside [0, kSubMax]: the load is rejected
constexpr uint32_t kLdNotOne = 2u;   // some row that is not released has a count other than 1 (all_sub_one is false)
constexpr uint32_t kLdGeneral = 4u;  // some non-small resource may need k_general (maybe_general)
// the check zeroes the flags word, then reads the caller's rows only; the other two write
// the context's columns: sub32 [N], agg [R], with seg_off the context's copy of the offsets
hipError_t launch_load_check(const LoadArgs& a, hipStream_t st);
hipError_t launch_load_sub(const LoadArgs& a, int32_t* sub32, hipStream_t st);
hipError_t launch_load_resources(const LoadArgs& a, const int64_t* seg_off, ResAgg* agg, hipStream_t st);
hipError_t launch_unpack_sums(const ResAgg* agg, int64_t n, int64_t* count, double* sum_has, double* sum_wants,
                              hipStream_t st);
}  // namespace dm
