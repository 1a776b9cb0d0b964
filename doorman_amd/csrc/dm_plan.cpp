// dm_plan.cpp — the dispatch plan of a store: resources binned by size into work items,
// tiles and chunks (build_plan), each work class's auxiliary stream and the stream parts
// (plan_streams, plan_parts), and the plan's device side with the state every new plan
// resets (upload_plan).  See DESIGN.md §4.
#include "dm_ctx.h"

int64_t dm::uniform_rows(const int64_t* seg_off, int64_t R) {
  if (R <= 0) return 0;
  const int64_t g = seg_off[1] - seg_off[0];
  bool same = g > 0;
  for (int64_t r = 1; r < R && same; ++r) same = seg_off[r + 1] - seg_off[r] == g;
  return same ? g : 0;
}

// ---------------------------------------------------------------------------
// plan: size-binned dispatch
// ---------------------------------------------------------------------------
static int bin_of(int64_t n) {
  if (n <= 16) return 7;
  if (n <= 32) return 8;
  if (n <= 64) return 0;
  if (n <= 128) return 1;
  if (n <= 256) return 2;
  if (n <= 512) return 3;
  if (n <= 1024) return 4;
  if (n <= 2048) return 5;
  return 6;
}

void dm::build_plan(dm_ctx* c) {
  c->h_tiles.clear();
  for (auto& b : c->h_bins) b.clear();
  c->h_chunks.clear();
  c->h_large.clear();
  const std::vector<int64_t>& off = c->h_seg_off;
  std::vector<int64_t> large;
  c->h_tile_list.clear();
  // runs of at least kTileMinRun consecutive small resources: tiles of at most kTileRes
  // resources and kTileRows rows; the small resources of shorter runs: list tiles
  std::vector<int32_t> scattered;
  auto run_tiles = [&](int64_t r0, int64_t r1) {
    if (r1 - r0 < kTileMinRun) {
      for (int64_t r = r0; r < r1; ++r) scattered.push_back((int32_t)r);
      return;
    }
    Tile tc{};
    bool topen = false;
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t n = off[r + 1] - off[r];
      if (topen && (tc.nrows + n > kTileRows || tc.nseg >= kTileRes)) {
        c->h_tiles.push_back(tc);
        topen = false;
      }
      if (!topen) {
        tc = Tile{(int32_t)r, 0, off[r], 0, 0};
        topen = true;
      }
      tc.nseg += 1;
      tc.nrows += (int32_t)n;
    }
    if (topen) c->h_tiles.push_back(tc);
  };
  int64_t run0 = -1;
  for (int64_t r = 0; r < c->R; ++r) {
    const int64_t n = off[r + 1] - off[r];
    if (n <= kSmallMax) {
      if (run0 < 0) run0 = r;
      continue;
    }
    if (run0 >= 0) run_tiles(run0, r);
    run0 = -1;
    if (n <= kLargeMin) {
      c->h_bins[bin_of(n)].push_back(WorkItem{(int32_t)r, (int32_t)n, off[r]});
    } else {
      large.push_back(r);
    }
  }
  if (run0 >= 0) run_tiles(run0, c->R);
  static_assert(kTileRes * kSmallMax <= kTileRows, "a list tile of kTileRes resources fits its LDS rows");
  for (size_t i = 0; i < scattered.size(); i += kTileRes) {
    const size_t e = std::min(scattered.size(), i + (size_t)kTileRes);
    Tile tc{(int32_t)c->h_tile_list.size(), (int32_t)(e - i), 0, 0, 1};
    for (size_t j = i; j < e; ++j) {
      const int32_t r = scattered[j];
      c->h_tile_list.push_back(TileEntry{r, tc.nrows});
      tc.nrows += (int32_t)(off[(size_t)r + 1] - off[(size_t)r]);
    }
    c->h_tiles.push_back(tc);
  }
  // the sub-wave bins: items ordered by shape (the narrowest kSubShapeG x kSubShapeR
  // that holds the resource, dm_device.h), each shape's items in resource order
  for (int k = 0; k < kSubShapes; ++k) {
    const int b = kSubShapeBin[k];
    const bool first = k == 0 || kSubShapeBin[k - 1] != b;
    const int64_t lo = first ? 0 : c->h_shape_lo[k - 1] + c->h_shape_n[k - 1];
    std::vector<WorkItem>& v = c->h_bins[b];
    const int cap = kSubShapeG[k] * kSubShapeR[k];
    auto mid = std::stable_partition(v.begin() + lo, v.end(), [&](const WorkItem& w) { return (w.n & 0xFFFF) <= cap; });
    c->h_shape_lo[k] = lo;
    c->h_shape_n[k] = (int64_t)(mid - v.begin()) - lo;
  }
  // Large resources largest first: a resource is verified by its last-arriving chunk,
  // and the largest's verification (the longest canonical trees) then overlaps the
  // other chunks instead of trailing the launch.  Each resource's chunks stay
  // consecutive and in row order (the canonical trees' order).
  std::stable_sort(large.begin(), large.end(),
                   [&](int64_t a, int64_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
  for (const int64_t r : large) {
    LargeSeg L{(int32_t)r, (int32_t)c->h_chunks.size(), 0, 0};
    for (int64_t o = off[r]; o < off[r + 1]; o += kChunkRows) {
      Chunk ch{(int32_t)r, (int32_t)c->h_large.size(), o, (int32_t)std::min<int64_t>(kChunkRows, off[r + 1] - o), 0};
      c->h_chunks.push_back(ch);
    }
    L.chunk_end = (int32_t)c->h_chunks.size();
    c->h_large.push_back(L);
  }
}

// The auxiliary stream of each launch unit of a tick (the sub-wave launch of bins 7, 8,
// 0, 1, 2; the workgroup bins 3-6, each a launch; the small tiles; the large chain).
// dm_ctx::kClassStream is the measured assignment for a store holding every class
// (configs[2]: bins 3-6 share stream 1 with bin 3 beside the sub-wave launch on stream 2,
// all hidden behind the large chain's critical path).  A store holding only some classes
// (a resource-id shard of a Zipf population: the head shards hold the large and
// workgroup classes, the tail shards the small ones) would then run classes one after
// another on a shared stream while another stream idles: the N = 8 shard of bins 3-6
// ran 36.6 us against 24-26 for its neighbours (profiles/r06_c2_shard8_ranks_contiguous_before_stream_plan.json).
// So, while some stream holds no unit of this store, the largest unit (by rows and
// records) of a stream holding several moves to it.
static void plan_streams(dm_ctx* c) {
  for (int i = 0; i < kNumBins + 2; ++i) c->class_stream[i] = dm_ctx::kClassStream[i];
  for (int b = 0; b < kNumBins; ++b)
    if (c->bin_parts[b] > 1) return;  // one bin in stream parts: its own two streams
  constexpr int kUnits = 7;  // 0 sub-wave launch, 1-4 bins 3-6, 5 tiles, 6 large chain
  auto unit_of_bin = [](int b) { return (b >= 3 && b <= 6) ? b - 2 : 0; };
  double bytes[kUnits] = {};
  bool present[kUnits] = {};
  const std::vector<int64_t>& off = c->h_seg_off;
  for (int b = 0; b < kNumBins; ++b)
    for (const WorkItem& w : c->h_bins[b]) {
      present[unit_of_bin(b)] = true;
      bytes[unit_of_bin(b)] += 28.0 * (double)(off[(size_t)w.seg + 1] - off[(size_t)w.seg]) + 97.0;
    }
  for (const Tile& t : c->h_tiles) {
    present[5] = true;
    bytes[5] += 28.0 * t.nrows + 97.0 * t.nseg;
  }
  for (const LargeSeg& L : c->h_large) {
    present[6] = true;
    bytes[6] += 28.0 * (double)(off[(size_t)L.seg + 1] - off[(size_t)L.seg]) + 97.0;
  }
  int us[kUnits];
  for (int u = 0; u < kUnits; ++u) us[u] = dm_ctx::kClassStream[u == 0 ? 0 : u <= 4 ? u + 2 : u == 5 ? kNumBins : kNumBins + 1];
  for (;;) {
    int load[dm_ctx::kAux] = {};
    for (int u = 0; u < kUnits; ++u) load[us[u]] += present[u] ? 1 : 0;
    int idle = -1, mover = -1;
    for (int k = 0; k < dm_ctx::kAux && idle < 0; ++k)
      if (load[k] == 0) idle = k;
    for (int u = 0; u < kUnits; ++u)
      if (present[u] && load[us[u]] > 1 && (mover < 0 || bytes[u] > bytes[mover])) mover = u;
    if (idle < 0 || mover < 0) break;
    us[mover] = idle;
  }
  for (int b = 0; b < kNumBins; ++b) c->class_stream[b] = us[unit_of_bin(b)];
  c->class_stream[kNumBins] = us[5];
  c->class_stream[kNumBins + 1] = us[6];
}

// Stream parts (dm_ctx::kParts): a workgroup bin holding every resource of the store
// (no other bin, tile or chunk, no heterogeneous subclients) and at most kPartBytes of
// rows, with enough items that each half still fills the GPU.
constexpr int64_t kPartBytes = int64_t(1) << 30;
constexpr int64_t kPartMinItems = 4096;
static void plan_parts(dm_ctx* c) {
  int nonempty = 0, only = -1;
  for (int b = 0; b < kNumBins; ++b)
    if (!c->h_bins[b].empty()) {
      ++nonempty;
      only = b;
    }
  for (int b = 0; b < kNumBins; ++b) {
    const int64_t n = (int64_t)c->h_bins[b].size();
    const bool split = c->parts_ok && nonempty == 1 && only == b && dm_ctx::is_split_bin(b) && c->h_tiles.empty() &&
                       c->h_chunks.empty() && !c->maybe_general && n >= kPartMinItems && c->N * 28 <= kPartBytes;
    c->bin_parts[b] = split ? dm_ctx::kParts : 1;
    for (int j = 0; j <= dm_ctx::kParts; ++j)
      c->part_lo[b][j] = split ? n * j / dm_ctx::kParts : (j == 0 ? 0 : n);
  }
  plan_streams(c);
}

// kBin4Wave (dm_device.h): bin 4 in stream parts and most of its resources FairShare
// by the loaded kinds.  (Without parts the shape did not pay: configs[3]'s N = 8 shard
// and the whole configs[3] unchanged, its N = 4 shard +3 %, profiles/r05_ab/b4_one_wave.txt.)
static bool bin4_prefers_wave(const dm_ctx* c) {
  const std::vector<WorkItem>& items = c->h_bins[4];
  if (items.empty() || c->bin_parts[4] < 2 || (int64_t)c->h_kind.size() != c->R) return false;
  int64_t fs = 0;
  for (const WorkItem& w : items) fs += c->h_kind[(size_t)w.seg] == DM_FAIR_SHARE ? 1 : 0;
  return 2 * fs > (int64_t)items.size();
}

// Bin 4's shape after a new plan, new kinds or parts turned off: a change re-uploads the
// bin's items without their hints (the dense hints and released-row masks are the
// shape's own; the next writeback tick sets them in the new shape).
int dm::update_bin4_shape(dm_ctx* c, hipStream_t st) {
  const bool wave = bin4_prefers_wave(c);
  if (wave == c->bin4_wave) return DM_OK;
  c->bin4_wave = wave;
  DM_HIP(c, upload(c->bins[4], c->h_bins[4].data(), c->h_bins[4].size(), st), "plan bins");
  DM_HIP(c, c->reset_keys(4, st), "fixed-point keys");
  return DM_OK;
}

// One split slot back to its start: the host-mapped words, the back-off, the rest queue
// sized for the part's items with its count ring, the epoch checks, and the sweep's ring
// where a tick has allocated it (dm_tick.cpp launch_dense_form).
int dm::SplitSlot::reset(dm_ctx* c, hipStream_t st) {
  __atomic_store_n(rec.h + 1, (uint64_t)0, __ATOMIC_RELAXED);
  __atomic_store_n(guard.h, 0, __ATOMIC_RELAXED);
  ver_epoch = 0;
  kept_epoch = 0;
  upd_rows = 0;
  recount = false;
  fix_live = cyc_live = 0;
  cyc = CycleAuto{};
  __atomic_store_n(queued.h, 0, __ATOMIC_RELAXED);
  skip = 0;
  wait = 64;
  DM_HIP(c, queue.ensure((size_t)std::max<int64_t>(items(), 1)), "dense split queue");
  DM_HIP(c, qcnt.ensure(3), "dense split queue");  // two-slot count + the last count told the host
  DM_HIP(c, hipMemsetAsync(qcnt.p, 0, 3 * sizeof(int32_t), st), "dense split queue");
  qpar = 0;
  __atomic_store_n(sweep.h, (uint64_t)0, __ATOMIC_RELAXED);
  __atomic_store_n(sweep.h + 1, (uint64_t)0, __ATOMIC_RELAXED);
  if (sw_cnt.p) DM_HIP(c, hipMemsetAsync(sw_cnt.p, 0, 4 * sizeof(int32_t), st), "sweep count");
  lpar = 0;
  if (fu_cnt.p) DM_HIP(c, hipMemsetAsync(fu_cnt.p, 0, 8 * sizeof(int32_t), st), "fused count");
  fpar = 0;
  ran_fused = false;
  __atomic_store_n(fused_queued.h, 0, __ATOMIC_RELAXED);
  __atomic_store_n(fused_queued.h + 1, 0, __ATOMIC_RELAXED);
  return DM_OK;
}

// The stream parts of the plan and every split slot's state (a new plan, or parts turned
// on or off).
static int init_split_slots(dm_ctx* c, hipStream_t st) {
  plan_parts(c);
  for (SplitSlot& s : c->split)
    if (int rc = s.reset(c, st)) return rc;
  return DM_OK;
}

// Stream parts allowed or not (dm_ctx::parts_ok): the plan's parts and the split slots
// are set up again after every stream has drained.
int dm::set_parts_ok(dm_ctx* c, bool ok) {
  if (c->parts_ok == ok) return DM_OK;
  c->parts_ok = ok;
  if (!c->h_dq.p) return DM_OK;  // no plan yet: upload_plan reads the flag
  DM_HIP(c, c->order.join(), "join");
  if (int rc = c->synced("stream parts")) return rc;
  c->order.main_has_work();
  if (int rc = init_split_slots(c, c->stream)) return rc;
  return update_bin4_shape(c, c->stream);
}

int dm::upload_plan(dm_ctx* c) {
  hipStream_t st = c->stream;
  // (first, as before the plan's own buffers: the store's allocations keep their order)
  DM_HIP(c, c->rmask.ensure((size_t)(c->N / 2 + 64)), "alloc released-row masks");  // zeroed below
  DM_HIP(c, upload(c->tiles, c->h_tiles.data(), c->h_tiles.size(), st), "plan tiles");
  DM_HIP(c, upload(c->tile_list, c->h_tile_list.data(), c->h_tile_list.size(), st), "plan tiles");
  for (int b = 0; b < kNumBins; ++b) DM_HIP(c, upload(c->bins[b], c->h_bins[b].data(), c->h_bins[b].size(), st), "plan bins");
  {  // every workgroup-bin resource's item (the update kernels keep its dense state, DenseUpd)
    std::vector<int32_t> io((size_t)std::max<int64_t>(c->R, 1), -1);
    for (int b = 3; b <= 6; ++b)
      for (size_t i = 0; i < c->h_bins[b].size(); ++i) io[(size_t)c->h_bins[b][i].seg] = (int32_t)(b << 24 | (int)i);
    DM_HIP(c, upload(c->item_of, io.data(), io.size(), st), "plan items");
    // the masks of a new plan start empty (the arrival masks are read only where an upsert
    // set a bit; the released-row masks are written whole when a tick sets the dense state)
    DM_HIP(c, hipMemsetAsync(c->rmask.p, 0, c->rmask.n, st), "plan masks");
  }
  DM_HIP(c, upload(c->chunks, c->h_chunks.data(), c->h_chunks.size(), st), "plan chunks");
  DM_HIP(c, upload(c->large, c->h_large.data(), c->h_large.size(), st), "plan large");
  if (!c->h_dq.p) {
    // fine-grained (coherent) host memory: a device store lands in host memory at once,
    // not in the GPU's L2 until a system-scope release (which a profiled dispatch under
    // rocprofv3 need not issue: the rest-skip check was never seen there)
    const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
    DM_HIP(c, c->h_dq.alloc(dm_ctx::kSplitSlots, mapped), "dense split word");
    DM_HIP(c, c->h_rec.alloc(dm_ctx::kSplitSlots * 3, mapped), "dense split check");
    DM_HIP(c, c->h_guard.alloc(dm_ctx::kSplitSlots, mapped), "dense split guard");
    DM_HIP(c, c->h_sw.alloc(dm_ctx::kSplitSlots * 2, mapped), "sweep count");
    DM_HIP(c, c->h_fq.alloc(dm_ctx::kSplitSlots * 2, mapped), "fused count");
    c->bind_split_slots();
  }
  c->rows_changed();  // new work items: no hints
  {
    int64_t rows6 = 0;
    for (const WorkItem& w : c->h_bins[6]) rows6 += w.n & 0xFFFF;
    c->bin6_wide = 2 * rows6 > c->N;
  }
  if (int rc = init_split_slots(c, st)) return rc;
  if (int rc = update_bin4_shape(c, st)) return rc;
  DM_HIP(c, c->chain.plan(c->h_large, c->h_chunks, st), "large-resource chain");
  c->n_nonsmall = 0;
  for (int64_t r = 0; r < c->R; ++r)
    if (c->h_seg_off[r + 1] - c->h_seg_off[r] > kSmallMax) ++c->n_nonsmall;
  DM_HIP(c, c->glist.ensure((size_t)std::max<int64_t>(c->n_nonsmall, 1)), "worklist");
  DM_HIP(c, c->gcount.ensure(1), "worklist");
  // (last: the allocations above keep their order)
  for (int b = 3; b < 3 + dm_ctx::kSplitBins; ++b)
    DM_HIP(c, c->reset_keys(b, st), "fixed-point keys");
  DM_HIP(c, c->fix_count.ensure(2), "fixed-point keys");
  return DM_OK;
}
