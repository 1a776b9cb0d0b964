// dm_runtime.cpp — host runtime behind include/doorman_hip.h: the life of a context.
//
// A context (dm_ctx.h) owns the device-resident columnar lease store of one GPU.  This
// unit creates and destroys it, keeps the process's pool of stream sets, and holds the
// stream, synchronisation, pinned-memory, profiling and introspection calls.  The plan
// is built in dm_plan.cpp, a tick launched in dm_tick.cpp, a round of requests in
// dm_decide.cpp; the store is loaded and read in dm_store.cpp, updated in
// dm_store_update.cpp, re-laid out and cleaned in dm_store_layout.cpp; the hierarchy's host side is dm_hier_host.cpp.  See DESIGN.md §3-§5.
#include <mutex>

#include "dm_ctx.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

void dm::set_last_error(const std::string& msg) { g_last_error = msg; }

const char* dm_version(void) { return "doorman-hip 0.7 (gfx950, abi 7)"; }

int dm_device_count(int* out) {
  if (!out) return DM_E_INVAL;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
    *out = 0;
    return DM_E_HIP;
  }
  *out = n;
  return DM_OK;
}

// The context's cross-stream order (StreamOrder::xs_signal): one event per hop kind.
static hipError_t xs_setup(dm_ctx* c) {
  for (int i = 0; i < StreamOrder::XS_N; ++i) {
    hipError_t e = c->order.xs_ev[i].create(hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The context's streams (its own stream, the four auxiliary streams, the copy stream),
// kept for the life of the process and reused by later contexts on the same device
// (dm_destroy returns a context's set; take_aux hands out the earliest-created free
// set).  The hardware queues behind the streams are not interchangeable: measured on
// C2 (round 5, tools/archive/gpu_r5_perm.sh, profiles/r05_queues.txt), which of the four
// masked queues carries which work class moved the tick from 111 us to 157 us, and the
// best assignment is a property of the queue's position in the process's creation
// order (period 4, consistent with queues spread over four hardware pipes): the small
// tiles on the last-created queue, every other assignment with the tiles elsewhere
// 123-157 us.  Stream priority does not change it.  So the creation order below is
// part of the tuning (own stream, the four masked streams, then the copy stream:
// 110-112 us; the copy stream first 137 us; the masked streams first 125 us), and a
// set is reused rather than destroyed and created again: new queues take other
// positions (bench.py's default run measured configs[2] at 124-154 us after earlier
// contexts were destroyed, 111-113 us with the pool).
struct AuxSet {
  int device;
  uint64_t seq;  // creation order: the earliest set first (its queues' positions, below)
  hipStream_t s[dm_ctx::kAux];
  hipStream_t own, cpy;  // the context's own stream and its copy stream, pooled with them
  bool own_queue;  // every stream got its own hardware queue (CU mask)
};
static std::mutex g_aux_mu;
static std::vector<AuxSet> g_aux_free;
static uint64_t g_aux_seq = 0;

// The pooled streams are destroyed at exit, before the HIP runtime's own teardown (an
// atexit handler registered after the runtime came up runs first): streams left to
// that teardown crashed the process at exit under rocprofv3.
static void release_aux_pool() {
  std::lock_guard<std::mutex> lk(g_aux_mu);
  for (AuxSet& a : g_aux_free) {
    (void)hipSetDevice(a.device);
    for (hipStream_t s : a.s) (void)hipStreamDestroy(s);
    (void)hipStreamDestroy(a.own);
    (void)hipStreamDestroy(a.cpy);
  }
  g_aux_free.clear();
}

static hipError_t take_aux(dm_ctx* c, int ncu) {
  {
    std::lock_guard<std::mutex> lk(g_aux_mu);
    size_t best = g_aux_free.size();
    for (size_t i = 0; i < g_aux_free.size(); ++i)
      if (g_aux_free[i].device == c->device && (best == g_aux_free.size() || g_aux_free[i].seq < g_aux_free[best].seq))
        best = i;
    if (best < g_aux_free.size()) {
      const AuxSet& a = g_aux_free[best];
      for (int k = 0; k < dm_ctx::kAux; ++k) c->order.aux[k] = a.s[k];
      c->own_stream = a.own;
      c->cpy = a.cpy;
      c->order.aux_own_queue = a.own_queue;
      c->order.aux_seq = a.seq;
      g_aux_free.erase(g_aux_free.begin() + (ptrdiff_t)best);
      return hipSuccess;
    }
    c->order.aux_seq = g_aux_seq++;
    static bool registered = false;
    if (!registered) registered = std::atexit(release_aux_pool) == 0;
  }
  const size_t mwords = (size_t)std::max(1, (ncu + 31) / 32);
  std::vector<uint32_t> mask(mwords, 0u);
  for (int b = 0; b < ncu; ++b) mask[(size_t)(b / 32)] |= 1u << (b % 32);
  c->order.aux_own_queue = true;
  // the creation order is measured (above)
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  for (int i = 0; i < dm_ctx::kAux && e == hipSuccess; ++i) {
    hipStream_t* slot = &c->order.aux[i];
    e = ncu > 0 ? hipExtStreamCreateWithCUMask(slot, (uint32_t)mwords, mask.data()) : hipErrorNotSupported;
    if (e != hipSuccess) {  // no CU masks here: a plain stream (correct, queue sharing as above)
      (void)hipGetLastError();
      c->order.aux_own_queue = false;
      e = hipStreamCreateWithFlags(slot, hipStreamNonBlocking);
    }
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->cpy, hipStreamNonBlocking);
  return e;
}

static void give_aux(dm_ctx* c) {
  if (!c->order.aux[0] || !c->own_stream || !c->cpy) return;
  (void)hipStreamSynchronize(c->own_stream);
  (void)hipStreamSynchronize(c->cpy);
  AuxSet a{c->device, c->order.aux_seq, {}, c->own_stream, c->cpy, c->order.aux_own_queue};
  c->own_stream = c->cpy = nullptr;
  for (int k = 0; k < dm_ctx::kAux; ++k) {
    (void)hipStreamSynchronize(c->order.aux[k]);
    a.s[k] = c->order.aux[k];
    c->order.aux[k] = nullptr;
  }
  std::lock_guard<std::mutex> lk(g_aux_mu);
  g_aux_free.push_back(a);
}

int dm_create(int device, dm_ctx** out) {
  if (!out) return DM_E_INVAL;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_last_error = std::string("no HIP device: ") + hipGetErrorString(e);
    return DM_E_HIP;
  }
  if (device < 0 || device >= n) {
    g_last_error = "device index out of range";
    return DM_E_RANGE;
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    g_last_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return DM_E_HIP;
  }
  dm_ctx* c = new dm_ctx();
  c->device = device;
  // Test hooks: each forces one of two product paths that the
  // library chooses between by itself, so that a test can compare the two on the same
  // ticks.  No other environment switch exists (round 5 retired the A/B probes).
  if (const char* df = getenv("DM_DECIDE_FAST")) c->round.fast = atoi(df) != 0;
  if (const char* sc = getenv("DM_SPEC_CHAIN")) c->chain.spec_chain = atoi(sc) != 0;
  if (const char* rl = getenv("DM_REDO_LIGHT")) c->chain.redo_light = atoi(rl);
  if (const char* qc = getenv("DM_QUEUE_CALIB")) {  // 0: keep the creation-order queue assignment; 2: log
    if (atoi(qc) == 0) c->qcal.cal.phase = QueueCalib::Phase::Done;
    c->qcal.cal.log = atoi(qc) == 2;
  }
  if (const char* ds = getenv("DM_DENSE_SPLIT")) {
    const int v = (int)strtol(ds, nullptr, 0);
    c->dense_split = v == 1 ? 0xF : (v & 0xF);
  }
  if (const char* sd = getenv("DM_STEADY")) c->steady_ok = atoi(sd);
  if (const char* fx = getenv("DM_FIXED")) c->fixed_ok = atoi(fx) != 0;
  if (const char* sw = getenv("DM_SWEEP")) c->sweep_ok = atoi(sw) != 0;
  if (const char* cy = getenv("DM_CYCLE")) c->cycle_ok = atoi(cy) != 0;
  if (const char* fu = getenv("DM_FUSED")) c->fused_ok = atoi(fu);
  if (const char* cb = getenv("DM_CYCLE_BYTES")) c->cycle_bytes = atoll(cb);
  if (const char* cr = getenv("DM_CARRY_ROUND")) c->carry_ok = atoi(cr) != 0;
  if (const char* rs = getenv("DM_ROUND_STORES")) c->round_stores = atoi(rs) != 0;
  e = hipSuccess;
  // The auxiliary streams are created with a full CU mask, which gives each its own
  // hardware queue.  Plain streams share the process's GPU_MAX_HW_QUEUES (4) queues
  // round robin with every other stream of the process (torch's included), so which
  // work classes ended up serialised behind one queue depended on how many streams
  // existed before: C2 tick 147-179 us by creation order, 147-151 us with the masks
  // (tools/host_cost.py, one process per run).  Static CU partitions (round 3-4 A/Bs:
  // 139-491 us against 136-140 us) and a high-priority chain stream (a queue shared
  // again) lost, and were retired in round 5.
  int ncu = 0;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
  // a quarter of headroom: the other classes' streams hold slots too, and run ahead
  // (DM_DEFER_JOIN)
  c->chain.redo_cap = (int64_t)std::max(ncu, 1) * redo_blocks_per_cu() * 3 / 4;
  if (e == hipSuccess) e = take_aux(c, ncu);
  c->stream = c->own_stream;
  if (e == hipSuccess) e = xs_setup(c);
  for (UpdateStage& s : c->stage)
    if (e == hipSuccess) e = s.create_events();
  for (int j = 0; j < dm_ctx::kParts; ++j)
    for (int i = 0; i < kTickEv && e == hipSuccess; ++i) e = c->done.ev[j][i].create(hipEventDefault);
  if (e != hipSuccess) {
    g_last_error = std::string("stream/event setup: ") + hipGetErrorString(e);
    dm_destroy(c);
    return DM_E_HIP;
  }
  *out = c;
  return DM_OK;
}

void dm_destroy(dm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // a carried round (dm_carry_rule.h) is launched before either context of the pair goes: the
  // root store holds it, and the leaf's template slots it writes outlive it (the drain below)
  (void)flush_carried(c);
  if (c->carry_root && c->carry_root->hs_leaf == c) c->carry_root->hs_leaf = nullptr;
  if (c->hs_leaf && c->hs_leaf->carry_root == c) c->hs_leaf->carry_root = nullptr;
  if (c->nccl_comm) {
    rccl_destroy(rccl_api(), c->nccl_comm);
    c->nccl_comm = nullptr;
  }
  // deferred tick work (DM_DEFER_JOIN) and update copies may still run on the
  // auxiliary streams: drain every stream before any buffer is freed
  for (int i = 0; i < dm_ctx::kAux; ++i)
    if (c->order.aux[i]) (void)hipStreamSynchronize(c->order.aux[i]);
  if (c->cpy) (void)hipStreamSynchronize(c->cpy);
  (void)hipStreamSynchronize(c->stream);
  c->collect_profile();
  for (auto e : c->event_pool) (void)hipEventDestroy(e);
  c->qcal.free();
  give_aux(c);  // kept for the next context on this device (take_aux)
  for (int i = 0; i < dm_ctx::kAux; ++i)  // (a set not returned whole)
    if (c->order.aux[i]) (void)hipStreamDestroy(c->order.aux[i]);
  if (c->cpy) {
    (void)hipStreamSynchronize(c->cpy);
    (void)hipStreamDestroy(c->cpy);
  }
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // every buffer, pinned word and event goes with its owner (dm_ctx.h)
}

const char* dm_last_error(dm_ctx* c) { return c ? c->err.c_str() : g_last_error.c_str(); }

int dm_set_stream(dm_ctx* c, void* s) {
  DM_ENTER(c);
  DM_HIP(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  // the template slots' lazy signals on the old stream are complete now, and that
  // stream may not outlive this call: never record on it again
  c->tpl.forget_stream(c->stream);
  c->stream = s ? (hipStream_t)s : c->own_stream;
  c->order.main_has_work();
  return DM_OK;
}

void* dm_get_stream(dm_ctx* c) { return c ? (void*)c->stream : nullptr; }

int dm_join(dm_ctx* c) {
  DM_ENTER(c);
  return DM_OK;
}

int dm_stream_wait(dm_ctx* c, void* s) {
  DM_ENTER(c);
  if (!s) return c->fail(DM_E_INVAL, "null stream");
  DM_HIP(c, c->order.xs_order(StreamOrder::XS_EXT, c->stream, (hipStream_t)s), "stream order");
  return DM_OK;
}

int dm_sync(dm_ctx* c) {
  DM_ENTER(c);
  const int rc = c->synced("hipStreamSynchronize");
  c->collect_profile();
  return rc;
}

int dm_host_alloc(dm_ctx* c, size_t bytes, void** out) {
  DM_CHECK_CTX(c);
  if (!out) return c->fail(DM_E_INVAL, "null out");
  *out = nullptr;
  if (bytes == 0) return DM_OK;
  DM_HIP(c, hipHostMalloc(out, bytes, hipHostMallocDefault), "pinned host buffer");
  return DM_OK;
}

int dm_host_free(dm_ctx* c, void* p) {
  DM_CHECK_CTX(c);
  if (p) DM_HIP(c, hipHostFree(p), "pinned host buffer");
  return DM_OK;
}

int dm_set_profiling(dm_ctx* c, int on) {
  DM_CHECK_CTX(c);
  c->profiling = on != 0;
  return DM_OK;
}

int dm_keep_keys(dm_ctx* c, int on) {
  DM_CHECK_CTX(c);
  c->keep_mode = on;  // a bit set (DM_KEEP_REFRESH, DM_KEEP_UPDATES, DM_KEEP_FREE_SLOTS); any non-zero value keeps refreshes
  return DM_OK;
}

int dm_keep_stats(dm_ctx* c, int64_t* out, int max) {
  if (!c || !out) return DM_E_INVAL;
  const int64_t v[6] = {c->keep_mode,    c->kept_refreshes, c->kept_releases,
                        c->kept_upserts, c->kept_batches,   c->kept_upd_rows};
  for (int i = 0; i < 6 && i < max; ++i) out[i] = v[i];
  return 6;
}

int dm_kernel_class_names(const char** names, int max) {
  if (!names && max > 0) return DM_E_INVAL;
  for (int i = 0; i < KC_COUNT && i < max; ++i) names[i] = kClassNames[i];
  return KC_COUNT;
}

int dm_kernel_times(dm_ctx* c, dm_kernel_time* out, int max) {
  DM_ENTER(c);
  DM_HIP(c, hipStreamSynchronize(c->stream), "sync");
  c->collect_profile();
  for (int i = 0; i < KC_COUNT && i < max; ++i) {
    out[i].name = kClassNames[i];
    out[i].launches = c->prof_launches[i];
    out[i].total_ms = c->prof_ms[i];
  }
  return KC_COUNT;
}

int dm_reset_kernel_times(dm_ctx* c) {
  DM_ENTER(c);
  DM_HIP(c, hipStreamSynchronize(c->stream), "sync");
  c->collect_profile();
  for (int i = 0; i < KC_COUNT; ++i) {
    c->prof_ms[i] = 0.0;
    c->prof_launches[i] = 0;
  }
  return DM_OK;
}

int dm_plan_info(dm_ctx* c, int64_t* out, int max) {
  if (!c || !out) return DM_E_INVAL;
  int64_t v[21 + kNumBins];
  v[0] = (int64_t)c->h_tiles.size();
  for (int b = 0; b < kNumBins; ++b) v[1 + b] = (int64_t)c->h_bins[b].size();
  v[1 + kNumBins] = (int64_t)c->h_large.size();
  v[2 + kNumBins] = (int64_t)c->h_chunks.size();
  v[3 + kNumBins] = c->N;
  v[4 + kNumBins] = (c->bin6_wide ? 1 : 0) | (c->bin4_wave ? 2 : 0);  // bit 0: bin 6 on 512 x 8 (else 256 x 16); bit 1: bin 4 on 64 x 16
  v[5 + kNumBins] = c->chain.redo_cap;  // 3/4 of the redo's full-build workgroups the GPU holds at once
  v[6 + kNumBins] = 1;            // every store may speculate (the redo by teams has no bound)
  v[7 + kNumBins] = c->order.aux_own_queue ? 1 : 0;  // the work classes' streams each have a hardware queue
  int64_t parts = 1;  // the stream parts of the store's one workgroup bin (dm_ctx::kParts), else 1
  for (int b = 0; b < kNumBins; ++b) parts = std::max<int64_t>(parts, c->bin_parts[b]);
  v[8 + kNumBins] = parts;
  // the class streams' queue assignment the calibration chose (QueueCalib): perm[0] +
  // 4 perm[1] + 16 perm[2] + 64 perm[3], or -1 before it has finished (or with shared queues)
  v[9 + kNumBins] = c->qcal.cal.best;
  // the column the last writeback tick wrote: 1 the has column (in place), 0 the alternate
  // column, -1 before any writeback tick
  v[10 + kNumBins] = c->wb_inplace;
  v[11 + kNumBins] = v[12 + kNumBins] = v[13 + kNumBins] = 0;
  for (const SplitSlot& s : c->split) {
    v[11 + kNumBins] += s.last.steady;    // bin parts whose last tick ran a steady build
    v[12 + kNumBins] += s.last.use_keys;  // ... and ran it with the fixed-point keys in use
    v[13 + kNumBins] += s.last.sweep;     // ... as the sweep and the row kernel over its worklist
  }
  v[14 + kNumBins] = c->kept_refreshes;  // wants refreshes kept under dm_keep_keys since dm_create
  v[15 + kNumBins] = 0;  // bin parts whose last tick ran the cycle form with the keys in use
  for (const SplitSlot& s : c->split) v[15 + kNumBins] += s.last.cycle && s.last.use_keys;
  v[16 + kNumBins] = 0;  // bin parts whose last tick ran a masked build (DM_KEEP_FREE_SLOTS)
  for (const SplitSlot& s : c->split) v[16 + kNumBins] += s.last.masked;
  v[17 + kNumBins] = 0;  // bin parts whose last tick ran fused (one launch: k_block_fused)
  for (const SplitSlot& s : c->split) v[17 + kNumBins] += s.last.fused;
  // what the device last told the host of the workgroup-bin parts, summed: the listed items
  // (the sweep record's count, from the row kernel or a fused launch) and the rest items (the
  // rest kernel's queue, or a fused launch's ring: SplitSlot::read_queued)
  v[18 + kNumBins] = v[19 + kNumBins] = 0;
  for (const SplitSlot& s : c->split) {
    if (!s.sweep.h || !s.lo || s.items() <= 0) continue;
    v[18 + kNumBins] += (int64_t)(uint32_t)__atomic_load_n(s.sweep.h, __ATOMIC_RELAXED);
    v[19 + kNumBins] += s.read_queued();
  }
  v[20 + kNumBins] = c->rounds_in_tick;  // root rounds that ran inside a leaf launch since the store was loaded
  const int n = 21 + kNumBins;
  for (int i = 0; i < n && i < max; ++i) out[i] = v[i];
  return n;
}

int dm_store_lost(dm_ctx* c, int* lost) {
  DM_ENTER(c);
  if (!lost) return c->fail(DM_E_INVAL, "null output");
  (void)c->check_device();  // (records a failure the last sync completed)
  *lost = c->store_lost ? 1 : 0;
  if (c->store_lost) c->err = "internal failure on the device: " + c->lost_msg;
  return DM_OK;
}

int dm_store_stats(dm_ctx* c, int64_t* out, int max) {
  DM_ENTER(c);
  if (!out || max < 0) return c->fail(DM_E_INVAL, "bad output buffer");
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  std::vector<uint8_t> ex((size_t)c->R);
  DM_HIP(c, download(ex.data(), (const uint8_t*)c->expl.p, 0, c->R, c->stream), "read row states");
  DM_HIP(c, hipStreamSynchronize(c->stream), "read row states");
  int64_t v[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t r = 0; r < c->R; ++r) {
    if (ex[(size_t)r] >= 2) {
      v[0] += 1;
      v[1] += c->h_seg_off[r + 1] - c->h_seg_off[r];
    } else if (ex[(size_t)r] == 1) {
      v[2] += 1;
    }
  }
  v[3] = c->R;
  // the valid fixed-point keys of the parts whose keys are in use (SplitSlot::fix_live),
  // counted here on demand, never by the tick
  for (const SplitSlot& s : c->split) {
    // (a part in the cycle form: its keys in state 2, and in v[5] those of them whose prev_has
    // differs from the record's sum_has: a cycle that is no fixed point)
    if (max > 4 && s.cyc_live == c->row_epoch && s.items() > 0 && s.bin_keys->p && s.bin_aux->p) {
      int32_t cnt[2] = {0, 0};
      DM_HIP(c, launch_count_cycle(s.keys(), s.aux(), c->bins[s.b].p + s.lo[0], c->agg.p, (int)s.items(), c->fix_count.p,
                                   c->stream),
             "count keys");
      DM_HIP(c, download(cnt, (const int32_t*)c->fix_count.p, 0, 2, c->stream), "count keys");
      DM_HIP(c, hipStreamSynchronize(c->stream), "count keys");
      v[4] += cnt[0];
      v[5] += cnt[1];
      continue;
    }
    if (max <= 4 || s.fix_live != c->row_epoch || s.items() <= 0 || !s.bin_keys->p) continue;
    int32_t cnt = 0;
    DM_HIP(c, launch_count_keys(s.keys(), (int)s.items(), c->fix_count.p, c->stream), "count keys");
    DM_HIP(c, download(&cnt, (const int32_t*)c->fix_count.p, 0, 1, c->stream), "count keys");
    DM_HIP(c, hipStreamSynchronize(c->stream), "count keys");
    v[4] += cnt;
  }
  for (int i = 0; i < 6 && i < max; ++i) out[i] = v[i];
  return 6;
}
