// dm_ctx.h — what the host units of the runtime share: the context (one per GPU: the
// device-resident columnar lease store, its dispatch plan, streams and policy state), the
// types that own its device memory, pinned host memory and events, the four owners of its
// cross-stream order (StreamOrder, TickDone, TemplatePipe, QueueCalibration: they carry out
// what dm_tick_order.h decides), the large-resource chain's owner (dm_large_chain.h), the
// store updates' staging (dm_update_stage.h: UpdateStage, RowBitmap; what their flags mean:
// dm_update_outcome.h), the owner of a round of requests' buffers (dm_decide_round.h, sized
// by dm_decide_plan.h's plan), the entry macros of the C-ABI calls, and the functions that
// cross a unit boundary.  The only definition of dm_ctx; the units around it are
// dm_runtime.cpp (context life, streams, profiling), dm_plan.cpp, dm_tick.cpp, dm_decide.cpp,
// dm_store.cpp, dm_store_update.cpp, dm_store_layout.cpp and dm_hier_host.cpp.  See DESIGN.md §3-§5.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: librccl is loaded when the first communicator is made

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/doorman_hip.h"
#include "dm_carry_rule.h"
#include "dm_decide_assign.h"
#include "dm_device.h"
#include "dm_large_form.h"
#include "dm_launch.h"
#include "dm_row_epoch.h"
#include "dm_split_form.h"
#include "dm_tick_order.h"

struct dm_ctx;

namespace dm {

// the thread's last error, for calls that have no context to keep it in (dm_last_error(NULL))
void set_last_error(const std::string& msg);

// kernel classes for profiling
enum KClass {
  KC_SMALL = 0,
  KC_BIN0,  // wave64 .. 256x16
  KC_LARGE_A = KC_BIN0 + kNumBins,
  KC_LARGE_B,
  KC_LARGE_C,
  KC_LARGE_MAP,
  KC_LARGE_FIN,
  KC_GENERAL,
  KC_UPSERT,
  KC_RELEASE,
  KC_SUBS,
  KC_DENSE3,  // the workgroup bins' split form (bins 3-6): dense kernel, then the rest kernel
  KC_DENSE4,
  KC_DENSE5,
  KC_DENSE6,
  KC_REST3,
  KC_REST4,
  KC_REST5,
  KC_REST6,
  KC_PUBLISH,   // dm_publish_totals
  KC_HIER_ROOT, // dm_hier_root_tick
  KC_LARGE_T,   // heterogeneous FairShare on the chain: thresholds,
  KC_LARGE_CH,  // bucket partials,
  KC_LARGE_E,   // bucket totals,
  KC_LARGE_MH,  // the map
  KC_DECIDE,    // dm_decide: the round's device work (fast path + k_decide)
  KC_LARGE_SPEC, // the speculative chain: k_large_spec,
  KC_LARGE_REDO, // k_large_redo
  KC_HIER_GATHER, // dm_hier_step's gather of the servers' blocks (ncclAllGather, or a rehearsal's copy)
  KC_COUNT
};
// bin 6 (2049-4096 rows) runs on 256 x 16 or 512 x 8 workgroups (kBin6Wide):
// "block2k4k" names the bin, dm_plan_info says which shape ran
inline const char* const kClassNames[KC_COUNT] = {
                                     "small_tiles",  "sub16x4",    "sub32x4",    "wave64x4",   "block128x4",
                                     "block128x8",   "block256x8", "block2k4k",  "sub8x2",    "sub16x2",
                                     "large_a",      "large_b",
                                     "large_c",      "large_map",  "large_fin",  "general",    "store_upsert",
                                     "store_release", "subs_merged", "block128x4_dense",
                                     "block128x8_dense", "block256x8_dense", "block2k4k_dense",
                                     "block128x4_rest", "block128x8_rest", "block256x8_rest", "block2k4k_rest",
                                     "hier_publish",
                                     "hier_root", "large_t", "large_c_het", "large_e", "large_map_het", "decide",
                                     "large_spec", "large_redo", "hier_gather"};

// The owners below free what they hold when their holder goes: a context's members with
// the `delete c` that ends dm_destroy (after every stream has been drained), a local with
// its scope.  None can be copied (the static_asserts after each).

// Device memory.  Move-only: std::swap exchanges two buffers (the ping-pong columns, the
// template slots, a re-layout's fresh table).
template <typename T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};
static_assert(!std::is_copy_constructible<DBuf<int>>::value && !std::is_copy_assignable<DBuf<int>>::value &&
                  std::is_nothrow_move_constructible<DBuf<int>>::value &&
                  std::is_nothrow_move_assignable<DBuf<int>>::value,
              "a device buffer has one owner: moved (std::swap), never copied");

// Host memory from hipHostMalloc: p is the plain host pointer every call site reads
// through, d the device's pointer to the same words when the allocation is mapped
// (hipHostMallocMapped), else nullptr.
template <typename T>
struct HBuf {
  T* p = nullptr;
  T* d = nullptr;
  HBuf() = default;
  HBuf(const HBuf&) = delete;
  HBuf& operator=(const HBuf&) = delete;
  ~HBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t alloc(size_t count, unsigned flags) {
    hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), flags);
    if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer((void**)&d, p, 0);
    return e;
  }
};
static_assert(!std::is_copy_constructible<HBuf<int>>::value && !std::is_copy_assignable<HBuf<int>>::value,
              "a host allocation has one owner");

// An event a context keeps for its whole life (created in dm_create); reads as the
// hipEvent_t it holds.  The profiling pool's and the queue calibration's events come and
// go with their use and are not of this kind.
struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (ev) (void)hipEventDestroy(ev);
  }
  hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&ev, flags); }
  operator hipEvent_t() const { return ev; }
};
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value,
              "an event has one owner");

struct ProfEvent {
  int cls;
  hipEvent_t a, b;
};

// One slot's words of a host-mapped allocation: the host's pointer and the device's.
template <typename T>
struct Mapped {
  T *h = nullptr, *d = nullptr;
};

// The state of one stream part of one workgroup bin (bins 3-6): everything the part's
// ticks (dm_tick.cpp bin_part, in the forms of dm_split_form.h) keep from one to the next.
// dm_ctx::slot(b, j) finds it; a bin that is not in stream parts uses part 0's alone.
struct SplitSlot {
  int b = 3, j = 0;  // its bin and stream part
  const int64_t* lo = nullptr;  // dm_ctx::part_lo[b] + j: its items are bins[b][lo[0] .. lo[1]) ...
  int64_t items() const { return lo[1] - lo[0]; }
  const DBuf<FixKey>* bin_keys = nullptr;  // ... and its keys that range of dm_ctx::fix_keys[b - 3]
  FixKey* keys() const { return bin_keys->p + lo[0]; }
  const DBuf<CycAux>* bin_aux = nullptr;  // ... and the cycle form's half of them (dm_ctx::cyc_aux)
  CycAux* aux() const { return bin_aux->p + lo[0]; }
  // The rest queue (k_block_dense appends, k_block_rest decides), one entry per item at
  // most; qcnt: its two-slot count ring and the last count told the host; qpar: the ring
  // slot of the next split tick.  queued (host-mapped): items the last split tick queued,
  // from which try_split decides with skip (ticks in the one-kernel form since the split
  // was last tried) and wait (ticks before the next try).
  DBuf<int32_t> queue, qcnt;
  int qpar = 0, skip = 0, wait = 64;
  Mapped<int32_t> queued;
  // host-mapped: {undense counts, epoch, arrival count} of the row epoch's density check
  // (k_count_undense, enqueued in ver_epoch; the third word is read only under
  // DM_KEEP_FREE_SLOTS), and the guard a dense kernel sets should
  // it queue an item on a tick whose rest kernel was skipped (dm_ctx::check_device)
  Mapped<uint64_t> rec;
  Mapped<int32_t> guard;
  uint64_t ver_epoch = 0, ver_write = 0;  // the row and write epochs of the last check (check_dense)
  // A kept update (dm_keep_keys' DM_KEEP_UPDATES, dm_ctx::update_kept) withdraws the record:
  // the host zeroes the record's epoch word and keeps the counts it held, with their row
  // epoch (0: none), as an estimate for the forms that the rest launch follows
  // (FormInputs::rec_kept); upd_rows: the rows kept updates wrote since that count; recount:
  // the next writeback tick's check_dense counts again.
  uint64_t kept_counts = 0, kept_epoch = 0, kept_arrivals = 0;
  int64_t upd_rows = 0;
  bool recount = false;
  void withdraw_record(uint64_t row_epoch, int64_t rows) {
    if (!rec.h) return;
    if (__atomic_load_n(rec.h + 1, __ATOMIC_ACQUIRE) == row_epoch) {
      kept_counts = __atomic_load_n(rec.h, __ATOMIC_RELAXED);
      kept_arrivals = __atomic_load_n(rec.h + 2, __ATOMIC_RELAXED);
      kept_epoch = row_epoch;
      upd_rows = 0;
      __atomic_store_n(rec.h + 1, 0, __ATOMIC_RELEASE);
    }
    upd_rows += rows;
    recount = true;
  }
  // The row epoch in which the part's last tick launched the FIXED build, which keeps a
  // key per item (0: it did not): keys are trusted only while this is the current epoch.
  // bin_part assigns it from choose_form's result (PartForm::fix_live has the rule and
  // why the host keeps it); rows_changed() and dm_ctx::reset_keys clear it.
  uint64_t fix_live = 0;
  // The same for the cycle form (PartForm::cyc_live), and when the part asks for the
  // alternate column by itself (dm_split_form.h CycleAuto).
  uint64_t cyc_live = 0;
  CycleAuto cyc;
  // The sweep (k_sweep) lists the items whose key does not hold in sw_list, one
  // entry per item at most.  sw_cnt: the list's two-slot count ring and the last {count,
  // epoch} told the host; lpar: the ring slot of the next sweep; sweep (host-mapped):
  // {count, row epoch}, which sizes the next grids.  Allocated by the first tick that sweeps.
  DBuf<SweepEntry> sw_list;
  DBuf<int32_t> sw_cnt;
  int lpar = 0;
  Mapped<uint64_t> sweep;
  // The fused form (k_block_fused, dm_tick_fused.hip) has count words of its own, so that the
  // two-kernel forms resume where they stopped: fu_cnt, a two-slot ring of the listed items
  // and what was last told the host (through `sweep` above); fused_queued (host-mapped), a
  // two-slot ring of the rest items, which stands in for `queued` after a fused tick; fpar:
  // the ring slot of the next fused tick.  fu_cnt is allocated by the first tick that runs fused.
  DBuf<int32_t> fu_cnt;
  Mapped<int32_t> fused_queued;
  int fpar = 0;
  bool ran_fused = false;  // the part's last split-form tick ran fused (dm_tick.cpp launch_fused: whose told words are current)
  PartForm last;  // its last tick's form (all clear: no launch); dm_plan_info slots 20-22, 24-26 count these
  // What the device last told the host, for the form's choice: each record's epoch first,
  // with acquire order (the device stores the count, then the epoch with release order).
  // Only the words the choice can use are read, as ever: the queued count for a part that
  // may split, the records for one that tries to, the sweep's where keys may be in use.
  int64_t read_queued() const {  // (after a fused tick: the slot that tick added to)
    return __atomic_load_n(ran_fused ? fused_queued.h + (fpar ^ 1) : queued.h, __ATOMIC_RELAXED);
  }
  void read_records(FormInputs& in) {
    in.rec_epoch = __atomic_load_n(rec.h + 1, __ATOMIC_ACQUIRE);
    in.rec_counts = __atomic_load_n(rec.h, __ATOMIC_RELAXED);
    if (in.keep_free) in.rec_arrivals = (int64_t)__atomic_load_n(rec.h + 2, __ATOMIC_RELAXED);
    if (in.rec_epoch == in.row_epoch) {  // a count taken after every kept update: the copy has served
      kept_epoch = 0;
      upd_rows = 0;
    } else if (kept_epoch == in.row_epoch) {
      in.rec_epoch = kept_epoch;
      in.rec_counts = kept_counts;
      if (in.keep_free) in.rec_arrivals = (int64_t)kept_arrivals;
      in.rec_kept = true;
      in.upd_rows = upd_rows;
    }
    if (in.fix_live != in.row_epoch && in.cyc_live != in.row_epoch) return;
    in.sw_epoch = __atomic_load_n(sweep.h + 1, __ATOMIC_ACQUIRE);
    const uint64_t told = __atomic_load_n(sweep.h, __ATOMIC_RELAXED);
    in.sw_told = (int64_t)(uint32_t)told;  // (the high half: the cycle form's stamp of the launch that told it)
    in.sw_stamp = (uint32_t)(told >> 32);
  }
  int reset(dm_ctx* c, hipStream_t st);  // a new plan, or parts turned on or off (dm_plan.cpp)
};
static_assert(!std::is_copy_constructible<SplitSlot>::value, "a split slot owns its queues");

// The four owners of a context's cross-stream state.  dm_tick_order.h decides which stream
// waits for which (plain C++, tested on the CPU); these hold the HIP handles and carry the
// decision out, and the host units ask, then do.

constexpr int kStreamParts = 2;  // dm_ctx::kParts: the stream parts a tick's events are kept for

// The context stream, the auxiliary streams (independent size bins of one tick run
// concurrently on them) and the order between them.
// Cross-stream order between the context's streams (fork / join of a tick's work
// classes, the pipelined hierarchy's template slots, dm_stream_wait): an event
// recorded on the producing stream and waited on by the consuming one.  An event wait
// idles the consuming queue ~12-20 us on the box (tools/xs_probe.py); stream-memory
// tokens (hipStreamWriteValue64 / WaitValue64, which this ROCm runs as blit kernels
// of 3-5 us each plus a dispatch gap) measured no cheaper per step (round 4: 75.0 vs
// 72.2 us per N = 8 shard step) and were retired in round 5, as was the tick-done
// word (the tick's last kernels' stop events replaced it: TickDone below).  A wait on
// a token signalled on the waiting stream itself is skipped (stream order).
struct StreamOrder {
  enum : int {
    XS_FORK = 0,
    XS_JOIN0 = 1,                       // + aux stream
    XS_READY0 = XS_JOIN0 + kAux,        // + template slot: the root round wrote it
    XS_FREE0 = XS_READY0 + kTplSlots,   // + template slot: the ticks that read it are done
    XS_LEAF = XS_FREE0 + kTplSlots,     // leaf stream -> the root round's stream
    XS_ROOT,                            // root stream -> the leaf (unpipelined, separate streams)
    XS_EXT,                             // dm_stream_wait
    XS_N
  };
  struct XsTok {
    int w = 0;
    hipStream_t s = nullptr;  // the stream it was signalled on
    bool rec = false;         // recorded (else the wait records on s first: lazy signal)
  };
  const hipStream_t* main = nullptr;  // the context stream (dm_ctx::stream, which dm_set_stream changes)
  TickSignal* sig = nullptr;          // the context's (TickDone): which auxiliary streams hold unjoined work
  hipStream_t aux[kAux] = {};
  bool aux_own_queue = false;  // each auxiliary stream has a hardware queue of its own (CU mask)
  uint64_t aux_seq = 0;        // the stream set's creation order in the process (take_aux)
  Event xs_ev[XS_N];
  hipError_t xs_signal(int w, hipStream_t s, XsTok* tok) {
    tok->w = w;
    tok->s = s;
    tok->rec = true;
    return hipEventRecord(xs_ev[w], s);
  }
  // A signal recorded only if a wait on another stream needs it, then at that wait:
  // it orders after everything the signalling stream holds by then (never less than
  // at signal time), and a same-stream consumer costs nothing.
  void xs_signal_lazy(int w, hipStream_t s, XsTok* tok) {
    tok->w = w;
    tok->s = s;
    tok->rec = false;
  }
  hipError_t xs_wait(const XsTok& tok, hipStream_t s) {
    if (tok.s == s || tok.s == nullptr) return hipSuccess;  // same stream, or known complete
    if (!tok.rec) return xs_order(tok.w, tok.s, s);
    return hipStreamWaitEvent(s, xs_ev[tok.w], 0);
  }
  hipError_t xs_order(int w, hipStream_t from, hipStream_t to) {
    if (from == to) return hipSuccess;
    XsTok t;
    hipError_t e = xs_signal(w, from, &t);
    return e == hipSuccess ? xs_wait(t, to) : e;
  }
  // A forked tick's work classes run on the auxiliary streams.  Normally they are
  // joined back into the context stream at the end of the tick; with DM_DEFER_JOIN
  // the join waits for the next library call that needs it (each cross-queue hop
  // costs ~20 us on the GPU, so back-to-back ticks keep every class streaming).
  // aux_pending: class work not yet joined into the context stream.
  // main_dirty: the context stream holds work the auxiliary streams have not
  // waited for (the next fork must record an event).
  bool aux_pending = false, main_dirty = true;
  hipError_t join() {
    if (!aux_pending) return hipSuccess;
    aux_pending = false;
    sig->unjoined = 0;
    for (int i = 0; i < kAux; ++i) {
      hipError_t e = xs_order(XS_JOIN0 + i, aux[i], *main);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void main_has_work() { main_dirty = true; }
  bool needs_fork() const { return main_dirty; }
  // Before a forked tick's launches: the class streams wait for what the context stream
  // holds (when it holds any), and `used`, the streams with work this tick, count as
  // unjoined.  After them, forked(): there is class work to join.  Two moments, as they
  // always were: a tick whose launch fails in between leaves no join pending.
  hipError_t fork(unsigned used) {
    if (needs_fork()) {
      XsTok fk;
      hipError_t e = xs_signal(XS_FORK, *main, &fk);
      for (int i = 0; i < kAux && e == hipSuccess; ++i) e = xs_wait(fk, aux[i]);
      if (e != hipSuccess) return e;
      main_dirty = false;
    }
    sig->unjoined |= used;
    return hipSuccess;
  }
  void forked() { aux_pending = true; }
};

// The tick-done signal (dm_tick_order.h TickSignal) and the events it counts: one per tick
// and stream part, in a ring; a tick's last kernels complete them.
struct TickDone {
  TickSignal sig;
  Event ev[kStreamParts][kTickEv];  // per stream part (one part: [0])
  hipEvent_t event(int part) const { return ev[part][sig.seq % kTickEv]; }  // this tick's, for the part's last kernel
  // stream s after tick `seq`: its parts' events
  hipError_t wait(uint64_t seq, hipStream_t s) const {
    const int k = (int)(seq % kTickEv);
    for (int j = 0; j < std::max(sig.nev[k], 1); ++j) {
      hipError_t e = hipStreamWaitEvent(s, ev[j][k], 0);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
};

// A pipelined leaf's templates (dm_hier_pipeline; the host half: dm_tick_order.h
// TemplateQueue): the staged slots and the tokens that order their writers and readers.
// Staged templates from another stream: the host waits for the exchange that made them
// and the leaf's stream gets no barrier (a queue waiting on another queue here costs
// ~12-16 us even when the signal is long set -- the step of an N = 8 shard idled that long
// every tick, tools/step_trace.py); the host stays at most ~one step ahead, the device
// never waits.
struct TemplatePipe {
  TemplateQueue q;
  bool on = false;
  DBuf<ResCfg> cfg[kTplSlots];
  DBuf<ResCold> cold[kTplSlots];
  StreamOrder::XsTok ready[kTplSlots];  // root stream: the slot's templates are written
  StreamOrder::XsTok free[kTplSlots];   // leaf stream: the ticks that read the slot are done
  bool free_rec[kTplSlots] = {};        // free holds a signal
  uint64_t free_seq[kTplSlots] = {};    // a slot is free once this tick's event completed (0: use free)
  void reset() {  // every slot free, none read
    q.reset();
    for (bool& r : free_rec) r = false;
  }
  // Stream s has drained and may not outlive the call: the slots' lazy signals on it are
  // complete, never record on it again.
  void forget_stream(hipStream_t s) {
    for (int i = 0; i < kTplSlots; ++i)
      for (StreamOrder::XsTok* t : {&ready[i], &free[i]})
        if (!t->rec && t->s == s) t->s = nullptr;
  }
};

// The queue calibration's streams and windows (the schedule and the choice:
// dm_tick_order.h QueueCalib; carried out by calib_step, dm_tick.cpp):
// aux[i] = phys[perm[i]].
struct QueueCalibration {
  QueueCalib cal;
  int perm[kAux] = {0, 1, 2, 3};
  hipStream_t phys[kAux] = {};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;  // each window's start and end on the context stream
  QueueCalibration() = default;
  QueueCalibration(const QueueCalibration&) = delete;
  QueueCalibration& operator=(const QueueCalibration&) = delete;
  void free() {
    for (auto& pr : ev) {
      if (pr.first) (void)hipEventDestroy(pr.first);
      if (pr.second) (void)hipEventDestroy(pr.second);
    }
    ev.clear();
  }
};

}  // namespace dm

#include "dm_decide_round.h"
#include "dm_large_chain.h"
#include "dm_update_stage.h"

using namespace dm;

struct dm_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  static constexpr int kAux = dm::kAux;
  // Which stream waits for which (the types above): the streams and their fork and join,
  // the tick-done signal, a pipelined leaf's template slots, the queue calibration.
  StreamOrder order;
  TickDone done;
  TemplatePipe tpl;
  QueueCalibration qcal;
  dm_ctx() {
    order.main = &stream;
    order.sig = &done.sig;
  }
  // auxiliary stream of each work class: bins 0..kNumBins-1, small tiles, large chain
  // (round 4 moved every bin to each other stream in A/Bs: this split won every one)
  // (round 5, with the small tiles: bin 3 on stream 3 112.8-117.3 us, on stream 1
  // 112.8-114.2, bin 6 on stream 3 127-129, against 111.0-112.4 us; profiles/r05_c2_classes.md)
  static constexpr int kClassStream[kNumBins + 2] = {2, 2, 2, 2, 1, 1, 1, 2, 2, 3, 0};  // C2: 200 -> 189 us (small class alone)
  // this store's assignment (plan_streams): kClassStream, except that on a store that
  // leaves some auxiliary stream without work, classes that would share a stream move
  // onto the idle ones (a shard of a Zipf population holds only some classes)
  int class_stream[kNumBins + 2] = {2, 2, 2, 2, 1, 1, 1, 2, 2, 3, 0};
  int64_t h_shape_lo[kSubShapes] = {}, h_shape_n[kSubShapes] = {};  // sub-wave shapes' items within their bins
  hipStream_t cpy = nullptr;  // store-update column copies (overlap a running tick)
  std::string err;

  int64_t R = 0, N = 0;
  bool store_loaded = false, cfg_loaded = false;
  // A device-side invariant failed (a redo workgroup gave up waiting, a dense kernel
  // queued an item on a tick that skipped its rest kernel: the host-mapped words
  // below).  The tick that tripped it may have written wrong leases and sums into the
  // store, so every call that reads, updates or ticks the store refuses it from then
  // on (DM_E_INTERNAL) until dm_store_load replaces it.
  bool store_lost = false;
  std::string lost_msg;
  // the store may hold explicit-expiry rows: set by every call that can write one
  // (load, upserts, decide, the root's tick), cleared by a writeback tick (which
  // turns every live explicit row into a follower).  Without them pass A's
  // speculative round 1 is exact and pass B runs one workgroup per large resource.
  bool expl_rows = true;
  // Row epoch: bumped by every call that writes rows (loads, plans, upserts, releases,
  // wants refreshes, decide, the root's tick) -- never by a tick.  Within one epoch a
  // writeback tick leaves every dense workgroup-bin resource dense (dm_tick_group.hip),
  // so a bin verified all-dense once in the epoch (k_count_undense) can skip its
  // k_block_rest: nothing can be queued.
  // Some writers may leave it alone under dm_keep_keys (dm_row_epoch.h has the rule and why
  // it is safe): a wants refresh, which ends as refresh_kept(), and with DM_KEEP_UPDATES a
  // release, an upsert or a synchronous batch, which end as update_kept().  write_epoch moves with
  // every write, kept or not: what the large chain's light redo asks (LargeChain::redo_epoch).
  uint64_t row_epoch = 1, write_epoch = 1;
  void rows_changed() {
    chain.rows_written();
    row_epoch += 1;
    write_epoch += 1;
    for (SplitSlot& s : split) s.fix_live = s.cyc_live = 0;  // no fixed-point key is trusted across a write (SplitSlot)
  }
  // dm_keep_keys.  kept_refreshes: dm_plan_info slot 23.  kept_rows: values the kept
  // refreshes carried since the last tick, each of which may have cleared a key: the next
  // sweep's row kernel is sized for them (FormInputs::refreshed).
  // keep_mode: the call's bit set (DM_KEEP_REFRESH, DM_KEEP_UPDATES; DM_KEEP_FREE_SLOTS keeps no call
  // and only selects forms: dm_split_form.h).  A kept release, upsert
  // or synchronous batch ends as update_kept(): a kept refresh's effects, its own counter
  // (dm_keep_stats), and every part's density record withdrawn as a proof (SplitSlot::
  // withdraw_record).  The call has waited for the context stream behind DM_ENTER's join of
  // the class streams, so no count is in flight: a record enqueued before the update is never
  // read as one taken after it.  kept_upd_rows: the rows of kept updates since the last tick.
  int keep_mode = 0;
  int64_t kept_refreshes = 0, kept_rows = 0;
  int64_t kept_releases = 0, kept_upserts = 0, kept_batches = 0, kept_upd_rows = 0;
  void refresh_kept(int64_t n) {
    chain.rows_written();
    write_epoch += 1;
    kept_refreshes += 1;
    kept_rows += n;
  }
  void update_kept(RowWrite w, int64_t n) {
    chain.rows_written();
    write_epoch += 1;
    (w == RowWrite::release ? kept_releases : w == RowWrite::upsert ? kept_upserts : kept_batches) += 1;
    kept_rows += n;
    kept_upd_rows += n;
    for (SplitSlot& s : split) s.withdraw_record(row_epoch, n);
  }
  bool keys_in_use() const {
    for (const SplitSlot& s : split)
      if (s.fix_live == row_epoch || s.cyc_live == row_epoch) return true;
    return false;
  }
  std::vector<int64_t> h_seg_off;
  std::vector<int64_t> h_refresh_s;

  // lease table
  DBuf<int64_t> seg_off;
  DBuf<int32_t> blk_seg;  // RowIndex coarse index
  RowIndex row_index() const { return RowIndex{seg_off.p, blk_seg.p, R}; }
  DBuf<double> wants, has;
  DBuf<int32_t> sub;  // subclients, 4 B per lease on the device (the ABI carries int64)
  DBuf<int64_t> expiry;
  // running sums + the followers' expiry, AoS (32 B)
  DBuf<ResAgg> agg;
  DBuf<uint8_t> expl;  // per resource: rows may carry explicit expiries (DevParams::expl)
  DBuf<uint8_t> rmask;  // released-row masks of dense workgroup-bin resources (DevParams::rmask)
  DBuf<int32_t> item_of;  // [R]: bin << 24 | item index for bins 3-6, else -1 (DenseUpd)
  // config, AoS: what every tick reads (32 B), and the rest (safe capacity, refresh)
  DBuf<ResCfg> cfg;
  DBuf<ResCold> cold;
  // outputs of a non-writeback tick
  DBuf<double> out_gets;
  DBuf<int64_t> out_expiry;
  DBuf<ResAgg> res;
  bool last_writeback = false, have_result = false;
  int wb_inplace = -1;  // the store's last writeback tick wrote the has column (1) or the alternate one (0)
  uint64_t wb_epoch = 0;  // row_epoch at the last writeback tick (0: none yet)
  // the workgroup bins' items carry dense hints: set by a writeback tick, kept by the
  // store updates (which keep a dense resource's state or end it: DenseUpd), cleared by
  // a new store
  bool hints_set = false;
  int64_t seg_uniform = 0;  // rows per resource when every resource has the same count, else 0
  // the store-update kernels' view of the dense state (dm_device.h DenseUpd)
  DenseUpd dense_upd() const {
    DenseUpd d{};
    d.item_of = item_of.p;
    for (int b = 3; b <= 6; ++b) d.bins[b - 3] = bins[b].p;
    d.bin4_wave = bin4_wave ? 1 : 0;
    d.bin6_wide = bin6_wide ? 1 : 0;
    d.rmask = rmask.p;
    return d;
  }
  // plan
  std::vector<Tile> h_tiles;  // small resources (n <= kSmallMax) in tiles (k_tile_small)
  std::vector<TileEntry> h_tile_list;  // the list tiles' resources
  DBuf<TileEntry> tile_list;
  std::vector<WorkItem> h_bins[kNumBins];
  std::vector<Chunk> h_chunks;
  std::vector<LargeSeg> h_large;
  DBuf<Tile> tiles;
  DBuf<WorkItem> bins[kNumBins];
  DBuf<Chunk> chunks;
  DBuf<LargeSeg> large;
  // the sub-wave bins run in one launch (k_subs): C2 tick 144-145 -> 138 us against
  // one launch per bin (tools/ab.py, both orders, one box; the per-bin form was
  // retired in round 5)
  // The workgroup bins (3-6) split by the dense hint (k_block_dense + k_block_rest) on a
  // tick that follows a writeback tick (only those set hints), unless the split form's
  // back-off says no (dm_split_form.h try_split).  DM_DENSE_SPLIT=0: never split.
  int dense_split = 0xF;  // bit i: bin 3+i runs in the split form (DM_DENSE_SPLIT: 0 off, 1 all, else the mask)
  static constexpr int kSplitBins = 4;  // bins 3..6
  static bool is_split_bin(int b) { return b >= 3 && b < 3 + kSplitBins; }
  // A split part whose items are all verified dense, none with released rows or arrivals
  // (k_count_undense's two counts), runs the steady builds of k_block_dense outside
  // recompute mode: Clean's result is known, so its pass is left out (dm_tick_group.h
  // group_segment STEADY).  DM_STEADY=0: never; 2 (A/B only): the steady ticks' launches,
  // dense then rest, with the plain builds: what the trailing rest launch costs.
  int steady_ok = 1;
  // Stream parts: a workgroup bin that is the store's only work class, and small enough
  // that a launch's ramp and drain are a visible share of it, runs as kParts launches
  // over contiguous halves of its items on two auxiliary streams, never joined from
  // tick to tick (DM_DEFER_JOIN): each part's next tick starts while the other part
  // drains, so the GPU never idles between ticks (an N = 8 shard of configs[3], 12.5M
  // leases: 57.3 -> 48.8 us per tick, tools/shard_split.py; the whole configs[3], 100M
  // leases: 430 -> 425 us, not worth its cross-queue waits in the exchange).  Every
  // split-bin state is per part: the split slot (SplitSlot) of bin b's part j.
  static constexpr int kParts = kStreamParts;
  static constexpr int kSplitSlots = kSplitBins * kParts;
  SplitSlot split[kSplitSlots];
  static int slot_of(int b, int j) { return (b - 3) * kParts + j; }
  static int slot_bin(int i) { return 3 + i / kParts; }  // slot_of's inverse
  static int slot_part(int i) { return i % kParts; }
  SplitSlot& slot(int b, int j) { return split[slot_of(b, j)]; }
  // DM_FIXED=0: no part runs the FIXED build (SplitSlot::fix_live).  fix_keys[b - 3]: the
  // keys of bin b's items, parallel to bins[b]; each slot sees its part's (SplitSlot::keys).
  int fixed_ok = 1;
  DBuf<FixKey> fix_keys[kSplitBins];
  DBuf<int32_t> fix_count;  // dm_store_stats: the valid keys of one part (two words: k_count_cycle)
  // DM_CYCLE=0: no part runs the cycle form and none asks for the alternate column (the
  // ticks are the ones they were without it).  cyc_aux[b - 3]: the keys' second halves.
  int cycle_ok = 1;
  // DM_FUSED=0: no part runs the fused form (PartForm::fused): every tick's launches are the
  // ones they were without it.  2 (a measuring hook): fused wherever the rule allows, whatever
  // count the device told.
  int fused_ok = 1;
  // DM_CYCLE_BYTES (a test hook, read when the context is created): the store size in bytes
  // (48 per lease) above which a part may ask by itself; kStreamBytes by default.
  int64_t cycle_bytes = kStreamBytes;
  DBuf<CycAux> cyc_aux[kSplitBins];
  bool cycle_asked() const {  // some part asks for the alternate column (CycleAuto)
    for (const SplitSlot& s : split)
      if (s.cyc.on && s.cyc.epoch == row_epoch && s.items() > 0) return true;
    return false;
  }
  // the update launchers' view of the store's columns (dm_launch.h StoreCols)
  StoreCols store_cols() const { return {row_index(), has.p, wants.p, sub.p, expiry.p, agg.p, expl.p, cfg.p}; }
  // the key-clearing refresh and update kernels' view of the keys (dm_device.h KeyClear)
  KeyClear key_clear() const {
    KeyClear k{};
    k.item_of = item_of.p;
    for (int b = 0; b < kSplitBins; ++b) k.keys[b] = fix_keys[b].p;
    return k;
  }
  // Wherever a workgroup bin's items are uploaded, its fixed-point keys start invalid, and
  // no part of it has keys in use.
  hipError_t reset_keys(int b, hipStream_t st) {
    DBuf<FixKey>& k = fix_keys[b - 3];
    hipError_t e = k.ensure(std::max<size_t>(h_bins[b].size(), 1));
    if (e == hipSuccess) e = hipMemsetAsync(k.p, 0, k.n * sizeof(FixKey), st);
    DBuf<CycAux>& a = cyc_aux[b - 3];
    if (e == hipSuccess) e = a.ensure(std::max<size_t>(h_bins[b].size(), 1));
    if (e == hipSuccess) e = hipMemsetAsync(a.p, 0, a.n * sizeof(CycAux), st);
    for (int j = 0; j < kParts; ++j) slot(b, j).fix_live = slot(b, j).cyc_live = 0;
    return e;
  }
  // DM_SWEEP=0: a FIXED launch with keys in use stays k_block_dense's kFixed build over every item.
  int sweep_ok = 1;
  int bin_parts[kNumBins] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
  // off for a leaf whose ticks an exchange on another stream waits for (dm_hier_attach):
  // there the exchange's two waits and the parts' CU share cost more than the parts
  // gain (the N = 8 rehearsal step 58.7 -> 66 us; one wait: 60-62 us; round 5)
  bool parts_ok = true;
  int64_t part_lo[kNumBins][kParts + 1] = {};  // item bounds of each part
  bool bin6_wide = false;  // bin 6 on 512 x 8 workgroups (kBin6Wide): it holds most of the rows
  bool bin4_wave = false;  // bin 4 on one wave per resource (kBin4Wave): most of its resources FairShare
  std::vector<int32_t> h_kind;  // the loaded configuration's kinds (bin 4's shape)
  // The split slots' host-mapped words, one allocation per kind (upload_plan), reached
  // through the slots: a word per slot of h_dq and h_guard, three of h_rec, two of h_sw and h_fq.
  HBuf<int32_t> h_dq, h_guard, h_fq;
  HBuf<uint64_t> h_rec, h_sw;
  void bind_split_slots() {  // once, when the words exist
    for (int i = 0; i < kSplitSlots; ++i) {
      SplitSlot& s = split[i];
      s.b = slot_bin(i), s.j = slot_part(i);
      s.lo = part_lo[s.b] + s.j, s.bin_keys = &fix_keys[s.b - 3], s.bin_aux = &cyc_aux[s.b - 3];
      s.queued = {h_dq.p + i, h_dq.d + i}, s.guard = {h_guard.p + i, h_guard.d + i};
      s.rec = {h_rec.p + 3 * i, h_rec.d + 3 * i}, s.sweep = {h_sw.p + 2 * i, h_sw.d + 2 * i};
      s.fused_queued = {h_fq.p + 2 * i, h_fq.d + 2 * i};
    }
  }
  // the large-resource chain: its partials, the speculative form's state, the
  // heterogeneous form's buffers (dm_large_chain.h)
  LargeChain chain;
  // worklist of resources for k_general (heterogeneous-subclient FairShare)
  DBuf<int32_t> glist, gcount;
  // Some non-small resource may need k_general.  A store update can make a store "maybe
  // general" (a NaN wants, subclients other than one) after its plan chose stream parts,
  // which plan_parts leaves out for a store that is general when planned.  The parts stay
  // (ADVICE r5 asked which): a tick that may run k_general joins every class stream before
  // it (dm_apportion: no deferred join), so k_general sees both parts' worklist appends,
  // and the parts' own kernels leave a heterogeneous resource untouched for it
  // (tests/test_parts_gpu.py::test_parts_store_turning_general_keeps_its_parts).
  bool maybe_general = false;
  bool all_sub_one = true;  // every loaded row had subclients == 1
  int64_t n_nonsmall = 0;
  // the staging of the store updates and the device-resolving reads (dm_update_stage.h):
  // set 0 for every call that is synchronous on return, the rest for dm_store_apply_async
  UpdateStage stage[1 + kAsyncSets];
  RowBitmap row_bits;
  int64_t async_seq = 0;  // asynchronous batches enqueued
  // a tick enqueued while an asynchronous batch that may make the store general is in flight
  bool async_may_general() const {
    for (int i = 1; i <= kAsyncSets; ++i)
      if (stage[i].pending && stage[i].may_general) return true;
    return false;
  }
  // dm_store_relayout: the rejection flags and the first rejected resource, compact mode's
  // block counts / prefix and per-resource bases, the row map's device staging
  DBuf<uint32_t> rl_flags;
  DBuf<unsigned long long> rl_bad;
  DBuf<int64_t> rl_blk_pre, rl_map;
  DBuf<int32_t> rl_seg_local;
  // dm_store_clean: the scan blocks' counts / prefix and minima, and the last clean's list
  // of released rows (sized from its count, never from N), kept for dm_read_cleaned until
  // the next clean, load or re-layout
  DBuf<int64_t> cl_blk_pre, cl_blk_min, cl_list;
  bool cl_valid = false;
  int64_t cl_n = 0;
  // dm_store_load_device: the flags its kernels raise (dm_launch.h kLdBadSub, kLdNotOne, kLdGeneral)
  DBuf<uint32_t> ld_flags;
  // dm_decide: a round's device buffers and the fast path's switch (dm_decide_round.h; the
  // round's plan and every buffer's count: dm_decide_plan.h)
  DecideRound round;
  // dm_publish_totals: the workgroups' validation flags and their arrival counter
  // (k_publish; both return to zero after each launch)
  DBuf<uint32_t> pub_sync;
  // dm_publish_ring: writeback tick k publishes into pub_ring[k % n]
  std::vector<double2*> pub_ring;
  int64_t pub_k = 0;
  // root side of the hierarchy: the exchange's layout (dm_hier_layout) and the
  // last round's per-server flags
  int hier_G = 0;                    // 0: not configured (replicated, G from each call)
  bool hier_sharded = false;
  std::vector<int64_t> h_hier_lo;    // [G + 1] sharded bounds
  DBuf<int64_t> hier_lo;
  int64_t hier_stride = 0;
  DBuf<uint32_t> hier_status;
  int hier_servers = 0;
  // dm_hier_attach / dm_hier_step (root side): the leaf it serves, its ring and gathered
  // buffer, its server index; the exchange's RCCL communicator (dm_hier_comm_init)
  dm_ctx* hs_leaf = nullptr;
  int hs_server = 0;
  std::vector<void*> hs_ring;
  void* hs_gathered = nullptr;
  ncclComm_t nccl_comm = nullptr;
  bool hs_ordered = false;  // dm_hier_step already ordered the exchange stream after the tick
  // The carried round (dm_carry_rule.h).  Root side: the launch arguments dm_hier_step kept
  // instead of launching (everything else the round does on the host is done: the slot is
  // staged, the epochs moved), and whether dm_hier_step holds it for its own tick.  The raw
  // pointers in it survive commit_templates' swaps (a DBuf swap moves ownership, not memory)
  // and every call that could free or replace a buffer flushes first.  Leaf side: the root
  // that may hold a round for this leaf (dm_hier_attach).  DM_CARRY_ROUND=0: never carried.
  // rounds_in_tick (both sides, dm_plan_info slot 29): the rounds that ran inside a leaf
  // launch since the store was loaded.
  int carry_ok = 1;
  bool carried = false, carry_held = false;
  RootRound carried_round{};
  dm_ctx* carry_root = nullptr;
  int64_t rounds_in_tick = 0;
  // Root side: the round stores a word of the root's rows and sums only where its bits differ
  // from what the lane loaded there (dm_hier_round.h; HierArgs::store_all is its negation).
  // DM_ROUND_STORES=0: every word, as before.
  int round_stores = 1;
  // a stream part's auxiliary stream (part 0: the bin's class stream).  Part 1 beside
  // bins 4-6's stream 1: stream 2 or 0 run C1 at 40.6-40.8 us per tick, stream 3 at
  // 61.6-64.2 us (which hardware queues pair well: take_aux; profiles/r05_parts_ab.txt)
  int part_stream(int b, int j) const {
    if (j == 0) return class_stream[b];
    return class_stream[b] != 2 ? 2 : 0;
  }
  // profiling
  bool profiling = false;
  std::vector<ProfEvent> pending;
  std::vector<hipEvent_t> event_pool;
  int64_t prof_launches[KC_COUNT] = {};
  double prof_ms[KC_COUNT] = {};

  int fail(int code, const std::string& msg) {
    err = msg;
    set_last_error(msg);
    return code;
  }
  int hip_fail(hipError_t e, const char* what) {
    return fail(DM_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  // The device's failure words (host-mapped, written by kernels of earlier ticks):
  // once one is set the store is lost (store_lost).  Called at the entry of every call
  // that touches the store and after every host wait that may have completed a tick.
  int check_device() {
    if (!store_lost) {
      for (const SplitSlot& s : split)
        if (s.guard.h && __atomic_load_n(s.guard.h, __ATOMIC_RELAXED)) {
          store_lost = true;
          lost_msg = "a dense kernel queued an item on a tick that skipped its rest kernel";
        }
      if (!store_lost && chain.gave_up()) {
        store_lost = true;
        lost_msg = "a redo workgroup of the speculative chain gave up waiting for its resource";
      }
    }
    if (!store_lost || reading) return DM_OK;  // (a reader of a lost store: dm_store_lost says so)
    return fail(DM_E_INTERNAL, "internal failure on the device: " + lost_msg +
                                   "; the store's leases and sums may be wrong, reload it (dm_store_load)");
  }
  bool reading = false;  // a read call in progress (DM_STORE_READABLE): a lost store may be read
  // wait for the context stream, then report a device failure the wait completed
  int synced(const char* what) {
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, what);
    return check_device();
  }
  hipEvent_t take_event() {
    if (!event_pool.empty()) {
      hipEvent_t e = event_pool.back();
      event_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  // HIP events around one launch on its stream while profiling is on (dm_kernel_times)
  template <typename F>
  hipError_t timed(int cls, hipStream_t s, F&& fn) {
    if (!profiling) return fn();
    ProfEvent pe{cls, take_event(), take_event()};
    (void)hipEventRecord(pe.a, s);
    hipError_t e = fn();
    (void)hipEventRecord(pe.b, s);
    pending.push_back(pe);
    return e;
  }
  void collect_profile() {
    for (auto& pe : pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
        prof_ms[pe.cls] += ms;
        prof_launches[pe.cls] += 1;
      }
      event_pool.push_back(pe.a);
      event_pool.push_back(pe.b);
    }
    pending.clear();
  }
};

namespace dm {
// dm_hier_host.cpp: the carried root round (dm_carry_rule.h) of c or of its attached peer,
// launched now unless dm_hier_step holds it; and the launch itself
int flush_carried(dm_ctx* c);
int launch_carried(dm_ctx* root);
}

#define DM_HIP(ctx, expr, what)                  \
  do {                                           \
    hipError_t _e = (expr);                      \
    if (_e != hipSuccess) return (ctx)->hip_fail(_e, what); \
  } while (0)

#define DM_CHECK_CTX_KEEP(ctx)                              \
  do {                                                      \
    if (!(ctx)) {                                           \
      dm::set_last_error("null context");                   \
      return DM_E_INVAL;                                    \
    }                                                       \
    DM_HIP(ctx, hipSetDevice((ctx)->device), "hipSetDevice"); \
  } while (0)

// Entry of every exported call that takes a context: a root round carried for the context
// or for its attached peer is launched first (dm_carry_rule.h flush_round; dm_hier_step
// alone enters with DM_CHECK_CTX_KEEP and holds the round for its own tick).
#define DM_CHECK_CTX(ctx)                                     \
  do {                                                        \
    DM_CHECK_CTX_KEEP(ctx);                                   \
    if (int _fl = dm::flush_carried(ctx)) return _fl;         \
  } while (0)

// Entry of every call that puts work on the context stream: join the auxiliary
// streams' deferred tick work first (DM_DEFER_JOIN), and remember that the
// context stream now holds work the next fork must order.
#define DM_ENTER(ctx)                                         \
  do {                                                        \
    DM_CHECK_CTX(ctx);                                        \
    DM_HIP(ctx, (ctx)->order.join(), "join auxiliary streams"); \
    (ctx)->order.main_has_work();                             \
  } while (0)

// Entry of every call that reads or updates the store: refuse a lost store
// (dm_ctx::store_lost) with the device's message.
#define DM_STORE_OK(ctx)                             \
  do {                                               \
    if (int _rc = (ctx)->check_device()) return _rc; \
  } while (0)
// The read calls work on a lost store too (for diagnosis): the failure is
// still recorded, and dm_store_lost reports it.  Ticks and updates keep refusing it.
struct ReadScope {
  dm_ctx* c;
  explicit ReadScope(dm_ctx* x) : c(x) { c->reading = true; }
  ~ReadScope() { c->reading = false; }
};
#define DM_STORE_READABLE(ctx)  \
  ReadScope _read_scope(ctx); \
  (void)(ctx)->check_device()

template <typename T>
static hipError_t upload(DBuf<T>& b, const T* src, size_t n, hipStream_t st) {
  hipError_t e = b.ensure(n);
  if (e != hipSuccess || n == 0) return e;
  return hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}

// (kind: into host memory, or hipMemcpyDeviceToDevice into a caller's device column)
template <typename T>
static hipError_t download(T* dst, const T* src, int64_t off, int64_t n, hipStream_t st,
                           hipMemcpyKind kind = hipMemcpyDeviceToHost) {
  if (!dst || n == 0) return hipSuccess;
  return hipMemcpyAsync(dst, src + off, (size_t)n * sizeof(T), kind, st);
}

static inline int check_range(dm_ctx* c, int64_t off, int64_t n, int64_t total) {
  if (off < 0 || n < 0 || off + n > total) return c->fail(DM_E_RANGE, "range out of bounds");
  return DM_OK;
}

static_assert(!std::is_copy_constructible<dm_ctx>::value, "a context owns its buffers and events: never copied");

// What one host unit defines and another calls.  Like the launchers (dm_launch.h) these
// live in namespace dm and never get a dm_-prefixed C name.
namespace dm {
// dm_plan.cpp
int64_t uniform_rows(const int64_t* seg_off, int64_t R);  // rows per resource when all have the same count, else 0
void build_plan(dm_ctx* c);
int upload_plan(dm_ctx* c);
int update_bin4_shape(dm_ctx* c, hipStream_t st);
int set_parts_ok(dm_ctx* c, bool ok);
// dm_tick.cpp
int ready(dm_ctx* c);
// dm_store.cpp
int check_device_ptr(dm_ctx* c, const void* p, size_t bytes, const char* what);
// A caller's device column of `bytes` bytes, when given: check_device_ptr, before any kernel or
// copy is given it.
#define DM_DEVICE_PTR(ctx, p, bytes, what)                                           \
  do {                                                                               \
    if (p)                                                                           \
      if (int _rc = dm::check_device_ptr(ctx, p, (size_t)(bytes), what)) return _rc; \
  } while (0)
// dm_store_update.cpp (its callers: the loads, dm_config_load, dm_store_layout.cpp)
void async_drain(dm_ctx* c);
int async_retire_all(dm_ctx* c);
// dm_store_update.cpp (its caller: dm_decide_assign): the upsert of device columns as the end
// of a call that has more on the context stream.  enqueue: what the call's one wait also
// covers, put on the stream behind the upsert's kernels; landed: called once that wait is
// over, before the upsert's flags word is judged (a rejected upsert still calls it).
struct UpsertTail {
  std::function<int()> enqueue;
  std::function<void()> landed;
};
int upsert_round(dm_ctx* c, int64_t n, const int64_t* rows, const double* has, const double* wants, const int64_t* sub,
                 const int64_t* exp, const UpsertTail& tail);
// dm_hier_host.cpp
struct RcclApi;
const RcclApi* rccl_api();
void rccl_destroy(const RcclApi* r, ncclComm_t comm);
}  // namespace dm
