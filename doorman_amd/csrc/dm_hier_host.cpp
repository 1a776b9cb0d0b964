// dm_hier_host.cpp — the host side of the hierarchy (dm_hier.hip): a leaf's published
// totals and ring, the root's exchange round and its templates for the leaf, the
// attached pair's step, and librccl, loaded on first use.
#include <dlfcn.h>

#include "dm_ctx.h"

int dm_aggregate_bands(const double* wants, const int64_t* num_clients, int64_t n, double* wants_total,
                       int64_t* subclients_total) {
  if (n < 0 || (n > 0 && (!wants || !num_clients)) || !wants_total || !subclients_total) return DM_E_INVAL;
  double wt = 0.0;
  int64_t stot = 0;
  for (int64_t i = 0; i < n; ++i) {
    wt += wants[i];
    if (num_clients[i] < 1) {
      set_last_error("subclients should be > 0");
      return DM_E_ARGUMENT;
    }
    stot += num_clients[i];
  }
  *wants_total = wt;
  *subclients_total = stot;
  return DM_OK;
}

int dm_publish_totals(dm_ctx* c, void* dst) {
  DM_ENTER(c);
  DM_STORE_OK(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  if (!dst) return c->fail(DM_E_INVAL, "null destination");
  if (!c->pub_sync.p) {
    DM_HIP(c, c->pub_sync.ensure(2), "publish state");
    DM_HIP(c, hipMemsetAsync(c->pub_sync.p, 0, 2 * sizeof(uint32_t), c->stream), "publish state");
  }
  DM_HIP(c, c->timed(KC_PUBLISH, c->stream, [&] { return launch_publish(c->R, c->agg.p, dst, c->pub_sync.p, c->stream); }),
         "publish");
  return DM_OK;
}

int dm_publish_ring(dm_ctx* c, int n, void* const* bufs) {
  DM_ENTER(c);
  if (n < 0 || (n > 0 && !bufs)) return c->fail(DM_E_INVAL, "bad publish ring");
  if (n > 0 && n < 3) return c->fail(DM_E_INVAL, "a publish ring needs at least 3 buffers");
  for (int i = 0; i < n; ++i)
    if (!bufs[i]) return c->fail(DM_E_INVAL, "null publish buffer");
  c->pub_ring.clear();
  for (int i = 0; i < n; ++i) c->pub_ring.push_back((double2*)bufs[i]);
  c->pub_k = 0;
  // every buffer's record 0 starts clear: a tick clears only its own flags words of
  // the next buffer (DevParams::pub_word)
  for (int i = 0; i < n; ++i) DM_HIP(c, hipMemsetAsync(bufs[i], 0, sizeof(double2), c->stream), "publish ring");
  if (n > 0) c->main_dirty = true;
  return DM_OK;
}

int dm_hier_layout(dm_ctx* root, int n_servers, const int64_t* shard_lo, int64_t stride) {
  DM_ENTER(root);
  if (n_servers <= 0 || n_servers > kHierMaxServers) return root->fail(DM_E_INVAL, "1..64 intermediate servers");
  if (!root->store_loaded) return root->fail(DM_E_STATE, "load the root store first");
  int64_t widest = root->R;
  if (shard_lo) {
    if (shard_lo[0] != 0 || shard_lo[n_servers] != root->R)
      return root->fail(DM_E_INVAL, "shard bounds must run from 0 to the root's resource count");
    widest = 0;
    for (int g = 0; g < n_servers; ++g) {
      if (shard_lo[g + 1] < shard_lo[g]) return root->fail(DM_E_INVAL, "shard bounds must be non-decreasing");
      widest = std::max(widest, shard_lo[g + 1] - shard_lo[g]);
    }
  }
  if (stride == 0) stride = 1 + widest;
  if (stride < 1 + widest) return root->fail(DM_E_INVAL, "record stride below 1 + the largest shard");
  root->hier_G = n_servers;
  root->hier_sharded = shard_lo != nullptr;
  root->hier_stride = stride;
  if (shard_lo) {
    root->h_hier_lo.assign(shard_lo, shard_lo + n_servers + 1);
    DM_HIP(root, upload(root->hier_lo, root->h_hier_lo.data(), root->h_hier_lo.size(), root->stream), "shard bounds");
  } else {
    root->h_hier_lo.clear();
  }
  return DM_OK;
}

int dm_hier_pipeline(dm_ctx* leaf, int on) {
  DM_ENTER(leaf);
  if (!leaf->cfg_loaded) return leaf->fail(DM_E_STATE, "load the leaf's configuration first");
  if (on < 0 || on > dm_ctx::kTplSlots - 1) return leaf->fail(DM_E_INVAL, "pipeline lag must be 0..3");
  if (!on && leaf->tpl_pipe && !leaf->tpl_pending.empty()) {  // take the newest staged templates now
    const int take = leaf->tpl_pending.back().slot;
    DM_HIP(leaf, leaf->xs_wait(leaf->tpl_ready[take], leaf->stream), "staged templates");
    std::swap(leaf->cfg, leaf->tpl_cfg[take]);
    std::swap(leaf->cold, leaf->tpl_cold[take]);
  }
  leaf->tpl_pending.clear();
  leaf->tpl_free_slots.clear();
  for (int i = 0; i < dm_ctx::kTplSlots; ++i) {
    leaf->tpl_free_slots.push_back(i);
    leaf->tpl_free_rec[i] = false;
  }
  if (on) DM_HIP(leaf, hipStreamSynchronize(leaf->stream), "template slots");  // no tick still reads a slot
  leaf->tpl_pipe = on != 0;
  leaf->tpl_lag = on > 1 ? on : 1;
  return DM_OK;
}

// One exchange round of the hierarchy (server.go:227-323 -> :822-901): decide the
// round on the root store from every server's published block (the request and
// its validation flags, dm_publish_totals) and write this server's templates into
// its leaf -- in place, or into a staged slot the leaf takes one tick later
// (dm_hier_pipeline).  Stream-ordered: the all-gather that produced `gathered`
// must precede it on the root's stream.
// The exchange's stream after leaf tick `seq`: its parts' events (dm_ctx::tick_ev).
static hipError_t wait_tick(dm_ctx* leaf, uint64_t seq, hipStream_t s) {
  const int k = (int)(seq % dm_ctx::kTickEv);
  for (int j = 0; j < std::max(leaf->tick_nev[k], 1); ++j) {
    hipError_t e = hipStreamWaitEvent(s, leaf->tick_ev[j][k], 0);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int dm_hier_root_tick(dm_ctx* root, const void* gathered, int n_servers, int64_t now_ns, dm_ctx* leaf, int server) {
  DM_ENTER(root);
  DM_STORE_OK(root);
  if (!root->store_loaded || !root->cfg_loaded) return root->fail(DM_E_STATE, "root store / config not loaded");
  if (!gathered || !leaf) return root->fail(DM_E_INVAL, "null gathered buffer or leaf context");
  if (n_servers <= 0 || n_servers > kHierMaxServers)
    return root->fail(DM_E_INVAL, "1..64 intermediate servers per root store");
  if (root->hier_G != 0 && root->hier_G != n_servers)
    return root->fail(DM_E_INVAL, "n_servers differs from the root's dm_hier_layout");
  const bool sharded = root->hier_G != 0 && root->hier_sharded;
  const int K = sharded ? 1 : n_servers;
  root->expl_rows = true;  // the root's rows take the exchange's explicit expiries
  root->rows_changed();
  // checked at load (seg_uniform), not per round
  if (root->R <= 0 || root->N != root->R * (int64_t)K || root->seg_uniform != K)
    return root->fail(DM_E_STATE, sharded ? "sharded root store must hold one row per resource"
                                          : "root store must hold R resources x n_servers rows (resource r: rows "
                                            "r*G..r*G+G-1)");
  if (server < 0 || server >= n_servers) return root->fail(DM_E_RANGE, "server index out of range");
  if (leaf->device != root->device) return root->fail(DM_E_INVAL, "root and leaf contexts must share a device");
  const int64_t leaf_lo = sharded ? root->h_hier_lo[server] : 0;
  const int64_t leaf_R = sharded ? root->h_hier_lo[server + 1] - leaf_lo : root->R;
  if (!leaf->cfg_loaded || leaf->R != leaf_R)
    return root->fail(DM_E_STATE, "the leaf must hold exactly this server's resources");
  const int64_t stride = root->hier_G != 0 ? root->hier_stride : 1 + root->R;
  const bool same = root->stream == leaf->stream;
  // A pipelined leaf whose last tick's events cover its streams stays unjoined (the
  // round writes a free template slot, and waits on those events); otherwise the leaf's
  // streams join first.
  const bool cover = !same && leaf->tpl_pipe && leaf->tick_covers();
  if (!cover) {
    DM_HIP(root, leaf->join_aux(), "join leaf streams");
    leaf->main_dirty = true;
  }
  DM_HIP(root, root->hier_status.ensure((size_t)kHierMaxServers), "hierarchy status");
  root->hier_servers = n_servers;
  if (!same && !root->hs_ordered) {  // the root round after the leaf's prior work (its publish)
    if (cover) DM_HIP(root, wait_tick(leaf, leaf->tick_seq, root->stream), "leaf->root order");
    else DM_HIP(root, leaf->xs_order(dm_ctx::XS_LEAF, leaf->stream, root->stream), "leaf->root order");
  }
  ResCfg* tcfg = leaf->cfg.p;
  ResCold* tcold = leaf->cold.p;
  const ResCfg* pcfg = leaf->cfg.p;
  const ResCold* pcold = leaf->cold.p;
  int slot = -1;
  if (leaf->tpl_pipe) {
    if (leaf->tpl_free_slots.empty())
      return root->fail(DM_E_STATE, "too many staged exchanges: tick the leaf between exchanges");
    slot = leaf->tpl_free_slots.front();
    DM_HIP(root, leaf->tpl_cfg[slot].ensure((size_t)leaf->R), "template slot");
    DM_HIP(root, leaf->tpl_cold[slot].ensure((size_t)leaf->R), "template slot");
    if (leaf->stream != root->stream) leaf->tick_signal_wanted = true;
    if (leaf->stream == root->stream) {
      // stream order: the ticks that read the slot's old templates precede this round
    } else if (leaf->tpl_free_rec[slot] && leaf->tpl_free_seq[slot] > 0) {  // the ticks that read the slot's old
      if (cover && root->hs_ordered && leaf->tpl_free_seq[slot] <= leaf->tick_seq) {  // templates are done
        // this round already waits for the leaf's last tick, whose events cover every
        // earlier tick on the same streams
      } else if (leaf->tick_seq - leaf->tpl_free_seq[slot] < (uint64_t)dm_ctx::kTickEv - 1) {
        DM_HIP(root, wait_tick(leaf, leaf->tpl_free_seq[slot], root->stream), "template slot");
      } else {  // that tick's events were recorded again since: everything the leaf holds
        DM_HIP(root, leaf->join_aux(), "join leaf streams");
        leaf->main_dirty = true;
        DM_HIP(root, leaf->xs_order(dm_ctx::XS_LEAF, leaf->stream, root->stream), "template slot");
      }
    }
    else if (leaf->tpl_free_rec[slot])
      DM_HIP(root, leaf->xs_wait(leaf->tpl_free[slot], root->stream), "template slot");
    tcfg = leaf->tpl_cfg[slot].p;
    tcold = leaf->tpl_cold[slot].p;
    if (!leaf->tpl_pending.empty()) {  // a rejected round keeps the newest staged templates
      pcfg = leaf->tpl_cfg[leaf->tpl_pending.back().slot].p;
      pcold = leaf->tpl_cold[leaf->tpl_pending.back().slot].p;
    }
  }
  DevParams p{};
  p.seg_off = root->seg_off.p;
  p.wants = root->wants.p;
  p.has = root->has.p;
  p.sub = root->sub.p;
  p.expiry = root->expiry.p;
  p.cfg = root->cfg.p;
  p.agg = root->agg.p;
  p.expl = root->expl.p;
  p.out_gets = root->has.p;
  p.out_expiry = root->expiry.p;
  p.out_wants = root->wants.p;
  p.out_sub = root->sub.p;
  p.res = root->agg.p;
  p.now = now_ns;
  p.recompute = 0;  // the root's running sums, updated as the reference's Clean + Assigns
  HierArgs ha{};
  ha.gathered = (const double2*)gathered;
  ha.stride = stride;
  ha.shard_lo = sharded ? root->hier_lo.p : nullptr;
  ha.status_out = root->hier_status.p;
  ha.leaf_cfg = tcfg;
  ha.leaf_cold = tcold;
  ha.leaf_prev_cfg = pcfg;
  ha.leaf_prev_cold = pcold;
  ha.root_cold = root->cold.p;
  ha.R = root->R;
  ha.leaf_lo = leaf_lo;
  // Sharded: only this server ever requests its resources (server.go:234-255), and its
  // leaf reads only their templates, so the round is decided over its own range; the
  // root copy's other rows are the other ranks' (each decides its own range).
  ha.r_lo = sharded ? leaf_lo : 0;
  ha.r_hi = sharded ? leaf_lo + leaf_R : root->R;
  ha.G = n_servers;
  ha.K = K;
  ha.server = server;
  DM_HIP(root, root->timed(KC_HIER_ROOT, root->stream, [&] { return launch_hier_tick(p, ha, root->stream); }),
         "hierarchy root tick");
  if (slot >= 0) {
    leaf->tpl_free_slots.erase(leaf->tpl_free_slots.begin());
    if (same)  // the leaf's ticks follow in stream order
      leaf->xs_signal_lazy(dm_ctx::XS_READY0 + slot, root->stream, &leaf->tpl_ready[slot]);
    else
      DM_HIP(root,
             leaf->xs_signal(dm_ctx::XS_READY0 + slot, root->stream, &leaf->tpl_ready[slot]),
             "staged templates");
    leaf->tpl_pending.push_back(dm_ctx::Staged{slot, leaf->ticks_issued});
  } else if (!same) {  // the leaf's next tick after its new templates
    DM_HIP(root, leaf->xs_order(dm_ctx::XS_ROOT, root->stream, leaf->stream), "root->leaf order");
  }
  root->maybe_general = true;  // rows carry heterogeneous subclient counts
  root->all_sub_one = false;
  root->last_writeback = true;
  root->have_result = true;
  return DM_OK;
}

// librccl, loaded on first use: the copy torch already mapped if there is one (one
// RCCL per process), else ROCm's
struct dm::RcclApi {
  void* h = nullptr;
  ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
  ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*comm_count)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*comm_user_rank)(const ncclComm_t, int*) = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
};
const RcclApi* dm::rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (!tried) {
    tried = true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names)
      if ((api.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
    for (int i = 0; !api.h && i < 3; ++i) api.h = dlopen(names[i], RTLD_NOW);
    if (api.h) {
      api.get_unique_id = (decltype(api.get_unique_id))dlsym(api.h, "ncclGetUniqueId");
      api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(api.h, "ncclCommInitRank");
      api.all_gather = (decltype(api.all_gather))dlsym(api.h, "ncclAllGather");
      api.comm_destroy = (decltype(api.comm_destroy))dlsym(api.h, "ncclCommDestroy");
      api.error_string = (decltype(api.error_string))dlsym(api.h, "ncclGetErrorString");
      api.comm_count = (decltype(api.comm_count))dlsym(api.h, "ncclCommCount");
      api.comm_user_rank = (decltype(api.comm_user_rank))dlsym(api.h, "ncclCommUserRank");
      if (!api.get_unique_id || !api.comm_init_rank || !api.all_gather || !api.comm_destroy || !api.error_string ||
          !api.comm_count || !api.comm_user_rank)
        api.h = nullptr;
    }
  }
  return api.h ? &api : nullptr;
}
void dm::rccl_destroy(const RcclApi* r, ncclComm_t comm) {
  if (r && comm) (void)r->comm_destroy(comm);
}

int dm_rccl_unique_id(void* id_out) {
  if (!id_out) return DM_E_INVAL;
  const RcclApi* r = rccl_api();
  if (!r) {
    set_last_error("librccl not found");
    return DM_E_STATE;
  }
  ncclUniqueId id;
  const ncclResult_t e = r->get_unique_id(&id);
  if (e != ncclSuccess) {
    set_last_error(std::string("ncclGetUniqueId: ") + r->error_string(e));
    return DM_E_HIP;
  }
  memcpy(id_out, &id, sizeof id);
  return DM_OK;
}

int dm_hier_comm_init(dm_ctx* root, const void* id, int nranks, int rank) {
  DM_ENTER(root);
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) return root->fail(DM_E_INVAL, "bad communicator arguments");
  if (root->nccl_comm) return root->fail(DM_E_STATE, "the exchange already has a communicator");
  const RcclApi* r = rccl_api();
  if (!r) return root->fail(DM_E_STATE, "librccl not found");
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  const ncclResult_t e = r->comm_init_rank(&root->nccl_comm, nranks, uid, rank);
  if (e != ncclSuccess) {
    root->nccl_comm = nullptr;
    return root->fail(DM_E_HIP, std::string("ncclCommInitRank: ") + r->error_string(e));
  }
  return DM_OK;
}

int dm_hier_comm_info(dm_ctx* root, int* nranks, int* rank) {
  DM_CHECK_CTX(root);
  if (!nranks || !rank) return root->fail(DM_E_INVAL, "null output");
  if (!root->nccl_comm) return root->fail(DM_E_STATE, "the exchange has no RCCL communicator");
  const RcclApi* r = rccl_api();
  ncclResult_t e = r->comm_count(root->nccl_comm, nranks);
  if (e == ncclSuccess) e = r->comm_user_rank(root->nccl_comm, rank);
  if (e != ncclSuccess) return root->fail(DM_E_HIP, std::string("ncclCommCount/UserRank: ") + r->error_string(e));
  return DM_OK;
}

int dm_hier_attach(dm_ctx* leaf, dm_ctx* root, int server, void* const* ring, int nring, void* gathered,
                   void* exchange_stream) {
  DM_ENTER(root);
  if (!leaf || leaf->device != root->device) return root->fail(DM_E_INVAL, "the leaf must share the root's device");
  if (root->hier_G == 0) return root->fail(DM_E_STATE, "set the exchange's layout first (dm_hier_layout)");
  if (server < 0 || server >= root->hier_G) return root->fail(DM_E_RANGE, "server index out of range");
  if (nring < 3 || !ring) return root->fail(DM_E_INVAL, "the publish ring needs at least 3 blocks");
  if (root->hier_G > 1 && !gathered) return root->fail(DM_E_INVAL, "several servers need a gathered buffer");
  int rc = dm_publish_ring(leaf, nring, ring);
  if (rc) return rc;
  if ((rc = dm_hier_pipeline(leaf, leaf->tpl_pipe ? leaf->tpl_lag : 1))) return rc;
  if ((rc = dm_set_stream(root, exchange_stream ? exchange_stream : leaf->stream))) return rc;
  // an exchange on a stream of its own waits for every leaf tick: no stream parts
  if ((rc = set_parts_ok(leaf, root->stream == leaf->stream))) return rc;
  root->hs_leaf = leaf;
  root->hs_server = server;
  root->hs_ring.assign(ring, ring + nring);
  root->hs_gathered = gathered;
  return DM_OK;
}

int dm_hier_step(dm_ctx* leaf, dm_ctx* root, int64_t now_ns) {
  DM_CHECK_CTX(root);
  if (!leaf || root->hs_leaf != leaf) return root->fail(DM_E_STATE, "dm_hier_attach this leaf to the root first");
  int rc = dm_apportion(leaf, now_ns, DM_WRITEBACK | DM_ASYNC | DM_DEFER_JOIN);
  if (rc) return root->fail(rc, "leaf tick: " + leaf->err);  // callers read the root's message
  const int64_t n = (int64_t)root->hs_ring.size();
  void* block = root->hs_ring[(size_t)((leaf->pub_k - 1) % n)];  // what this tick published
  const int G = root->hier_G;
  const void* gathered = block;
  if (G > 1) {
    // the exchange stream after the tick that wrote the block: on the tick's events when
    // its last kernels complete them (no marker on the leaf's queues; the leaf's stream
    // parts stay unjoined), else after a join, on an event
    const bool cover = leaf->stream != root->stream && leaf->tick_covers();
    if (!cover) DM_HIP(root, leaf->join_aux(), "join leaf streams");
    if (leaf->stream != root->stream) leaf->tick_signal_wanted = true;
    if (leaf->stream == root->stream) {
      // stream order
    } else if (cover || (leaf->tick_flagged && leaf->tick_part_mask == 0))
      DM_HIP(root, wait_tick(leaf, leaf->tick_seq, root->stream), "leaf->exchange order");
    else
      DM_HIP(root, leaf->xs_order(dm_ctx::XS_LEAF, leaf->stream, root->stream), "leaf->exchange order");
    const size_t bytes = (size_t)root->hier_stride * 16;
    // (timed as one class on the exchange stream while profiling: bench.py's exchange_us)
    if (root->nccl_comm) {  // every server's block, in server order, over xGMI
      const RcclApi* r = rccl_api();
      ncclResult_t e = ncclSuccess;
      DM_HIP(root, root->timed(KC_HIER_GATHER, root->stream, [&] {
               e = r->all_gather(block, root->hs_gathered, (size_t)root->hier_stride * 2, ncclFloat64,
                                 root->nccl_comm, root->stream);
               return hipSuccess;
             }),
             "gather");
      if (e != ncclSuccess) return root->fail(DM_E_HIP, std::string("ncclAllGather: ") + r->error_string(e));
    } else {  // a rehearsal: this server's slot only
      DM_HIP(root, root->timed(KC_HIER_GATHER, root->stream, [&] {
               return hipMemcpyAsync((char*)root->hs_gathered + (size_t)root->hs_server * bytes, block, bytes,
                                     hipMemcpyDeviceToDevice, root->stream);
             }),
             "gather (local)");
    }
    gathered = root->hs_gathered;
  }
  root->hs_ordered = G > 1;
  rc = dm_hier_root_tick(root, gathered, G, now_ns, leaf, root->hs_server);
  root->hs_ordered = false;
  return rc;
}

int dm_hier_status(dm_ctx* root, uint32_t* status, int n) {
  DM_ENTER(root);
  if (!status || n < 0) return root->fail(DM_E_INVAL, "bad status buffer");
  if (root->hier_servers == 0) return root->fail(DM_E_STATE, "no dm_hier_root_tick yet");
  if (n != root->hier_servers) return root->fail(DM_E_INVAL, "status buffer must hold one word per server");
  DM_HIP(root, download(status, (const uint32_t*)root->hier_status.p, 0, n, root->stream), "hierarchy status");
  DM_HIP(root, hipStreamSynchronize(root->stream), "hierarchy status");
  int bad = 0;
  for (int g = 0; g < n; ++g) bad += status[g] != 0;
  return bad;
}
