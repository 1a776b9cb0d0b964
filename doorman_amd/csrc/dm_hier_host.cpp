// dm_hier_host.cpp — the host side of the hierarchy (dm_hier.hip): a leaf's published
// totals and ring, the root's exchange round and its templates for the leaf, the
// attached pair's step, and librccl, loaded on first use.  How the root's stream gets behind
// the leaf's ticks is asked of dm_tick_order.h (root_round_order, slot_reuse,
// follow_last_tick) and carried out here.
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
  if (n > 0) c->order.main_has_work();
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
  if (on < 0 || on > kTplSlots - 1) return leaf->fail(DM_E_INVAL, "pipeline lag must be 0..3");
  TemplatePipe& tp = leaf->tpl;
  if (!on && tp.on && tp.q.newest() >= 0) {  // take the newest staged templates now
    const int take = tp.q.newest();
    DM_HIP(leaf, leaf->order.xs_wait(tp.ready[take], leaf->stream), "staged templates");
    std::swap(leaf->cfg, tp.cfg[take]);
    std::swap(leaf->cold, tp.cold[take]);
  }
  tp.reset();
  if (on) DM_HIP(leaf, hipStreamSynchronize(leaf->stream), "template slots");  // no tick still reads a slot
  tp.on = on != 0;
  tp.q.lag = on > 1 ? on : 1;
  return DM_OK;
}

// Stream s behind the leaf's last tick, as dm_tick_order.h decided: on the tick's events,
// or on an event recorded on the leaf's context stream.
static hipError_t wait_leaf(dm_ctx* leaf, TickWait how, hipStream_t s) {
  if (how == TickWait::tick_events) return leaf->done.wait(leaf->done.sig.seq, s);
  if (how == TickWait::event) return leaf->order.xs_order(StreamOrder::XS_LEAF, leaf->stream, s);
  return hipSuccess;
}

// One exchange round of the hierarchy (server.go:227-323 -> :822-901): decide the
// round on the root store from every server's published block (the request and
// its validation flags, dm_publish_totals) and write this server's templates into
// its leaf -- in place, or into a staged slot the leaf takes one tick later
// (dm_hier_pipeline).  Stream-ordered: the all-gather that produced `gathered`
// must precede it on the root's stream.
// carry (dm_hier_step, dm_carry_rule.h carry_round): everything but the launch, whose arguments
// the root keeps as its carried round; errors found up to there are this call's.
static int root_round(dm_ctx* root, const void* gathered, int n_servers, int64_t now_ns, dm_ctx* leaf, int server,
                      bool carry) {
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
  TemplatePipe& tp = leaf->tpl;
  const RoundOrder ro = root_round_order(leaf->done.sig, same, tp.on, root->hs_ordered);
  if (ro.join) {
    DM_HIP(root, leaf->order.join(), "join leaf streams");
    leaf->order.main_has_work();
  }
  DM_HIP(root, root->hier_status.ensure((size_t)kHierMaxServers), "hierarchy status");
  root->hier_servers = n_servers;
  DM_HIP(root, wait_leaf(leaf, ro.wait, root->stream), "leaf->root order");
  ResCfg* tcfg = leaf->cfg.p;
  ResCold* tcold = leaf->cold.p;
  const ResCfg* pcfg = leaf->cfg.p;
  const ResCold* pcold = leaf->cold.p;
  int slot = -1;
  if (tp.on) {
    if ((slot = tp.q.next_free()) < 0)
      return root->fail(DM_E_STATE, "too many staged exchanges: tick the leaf between exchanges");
    DM_HIP(root, tp.cfg[slot].ensure((size_t)leaf->R), "template slot");
    DM_HIP(root, tp.cold[slot].ensure((size_t)leaf->R), "template slot");
    if (!same) leaf->done.sig.want();
    // the ticks that read the slot's old templates are done before the round writes it
    switch (slot_reuse(leaf->done.sig, same, tp.free_rec[slot], tp.free_seq[slot], ro.cover, root->hs_ordered)) {
      case SlotReuse::stream_order:
      case SlotReuse::covered:
      case SlotReuse::none: break;
      case SlotReuse::tick_events:
        DM_HIP(root, leaf->done.wait(tp.free_seq[slot], root->stream), "template slot");
        break;
      case SlotReuse::join_then_event:
        DM_HIP(root, leaf->order.join(), "join leaf streams");
        leaf->order.main_has_work();
        DM_HIP(root, wait_leaf(leaf, TickWait::event, root->stream), "template slot");
        break;
      case SlotReuse::lazy_token:
        DM_HIP(root, leaf->order.xs_wait(tp.free[slot], root->stream), "template slot");
        break;
    }
    tcfg = tp.cfg[slot].p;
    tcold = tp.cold[slot].p;
    if (tp.q.newest() >= 0) {  // a rejected round keeps the newest staged templates
      pcfg = tp.cfg[tp.q.newest()].p;
      pcold = tp.cold[tp.q.newest()].p;
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
  ha.store_all = root->round_stores ? 0 : 1;
  if (carry) {
    root->carried_round = RootRound{p, ha};
    root->carried = true;
  } else {
    DM_HIP(root, root->timed(KC_HIER_ROOT, root->stream, [&] { return launch_hier_tick(p, ha, root->stream); }),
           "hierarchy root tick");
  }
  if (slot >= 0) {
    if (same)  // the leaf's ticks follow in stream order
      leaf->order.xs_signal_lazy(StreamOrder::XS_READY0 + slot, root->stream, &tp.ready[slot]);
    else
      DM_HIP(root, leaf->order.xs_signal(StreamOrder::XS_READY0 + slot, root->stream, &tp.ready[slot]),
             "staged templates");
    tp.q.stage(slot);
  } else if (!same) {  // the leaf's next tick after its new templates
    DM_HIP(root, leaf->order.xs_order(StreamOrder::XS_ROOT, root->stream, leaf->stream), "root->leaf order");
  }
  root->maybe_general = true;  // rows carry heterogeneous subclient counts
  root->all_sub_one = false;
  root->last_writeback = true;
  root->have_result = true;
  return DM_OK;
}

int dm_hier_root_tick(dm_ctx* root, const void* gathered, int n_servers, int64_t now_ns, dm_ctx* leaf, int server) {
  return root_round(root, gathered, n_servers, now_ns, leaf, server, false);
}

// The carried round as a launch of its own on the root's stream: what the round would have
// been without the carry, at a later place of the same stream.
int dm::launch_carried(dm_ctx* root) {
  root->carried = false;
  const RootRound& r = root->carried_round;
  DM_HIP(root, root->timed(KC_HIER_ROOT, root->stream, [&] { return launch_hier_tick(r.p, r.ha, root->stream); }),
         "hierarchy root tick");
  return DM_OK;
}

int dm::flush_carried(dm_ctx* c) {
  dm_ctx* root = c->carried ? c : c->carry_root;
  if (!root || !flush_round(root->carried, root->carry_held)) return DM_OK;
  const int rc = launch_carried(root);
  if (rc && root != c) c->fail(rc, "carried root round: " + root->err);
  return rc;
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
  int rc = flush_carried(leaf);  // (a round another root carries for this leaf)
  if (rc) return root->fail(rc, "leaf: " + leaf->err);
  if ((rc = dm_publish_ring(leaf, nring, ring))) return rc;
  if ((rc = dm_hier_pipeline(leaf, leaf->tpl.on ? leaf->tpl.q.lag : 1))) return rc;
  if ((rc = dm_set_stream(root, exchange_stream ? exchange_stream : leaf->stream))) return rc;
  // an exchange on a stream of its own waits for every leaf tick: no stream parts
  if ((rc = set_parts_ok(leaf, root->stream == leaf->stream))) return rc;
  // the pair's back-pointers: the leaf reaches a round its root carries (dm_carry_rule.h)
  if (root->hs_leaf && root->hs_leaf != leaf && root->hs_leaf->carry_root == root) root->hs_leaf->carry_root = nullptr;
  if (leaf->carry_root && leaf->carry_root != root && leaf->carry_root->hs_leaf == leaf)
    leaf->carry_root->hs_leaf = nullptr;
  leaf->carry_root = root;
  root->hs_leaf = leaf;
  root->hs_server = server;
  root->hs_ring.assign(ring, ring + nring);
  root->hs_gathered = gathered;
  return DM_OK;
}

namespace {
// dm_hier_step holds a carried round for its own leaf tick: the calls it makes do not flush it.
struct CarryHold {
  dm_ctx* root;
  explicit CarryHold(dm_ctx* r) : root(r) { root->carry_held = true; }
  ~CarryHold() { root->carry_held = false; }
};
}  // namespace

int dm_hier_step(dm_ctx* leaf, dm_ctx* root, int64_t now_ns) {
  DM_CHECK_CTX_KEEP(root);
  if (!leaf || root->hs_leaf != leaf) {
    if (int rc = flush_carried(root)) return rc;
    return root->fail(DM_E_STATE, "dm_hier_attach this leaf to the root first");
  }
  // The last step's round, when carried, rides in this step's leaf tick or is launched ahead
  // of its launches (dm_tick.cpp, by dm_carry_rule.h place_round); this step's is carried in
  // its turn when the rule allows.
  CarryHold hold(root);
  int rc = dm_apportion(leaf, now_ns, DM_WRITEBACK | DM_ASYNC | DM_DEFER_JOIN);
  if (rc) return root->fail(rc, "leaf tick: " + leaf->err);  // callers read the root's message
  if (root->carried && (rc = launch_carried(root))) return rc;  // (never: the tick placed it)
  const int64_t n = (int64_t)root->hs_ring.size();
  void* block = root->hs_ring[(size_t)((leaf->pub_k - 1) % n)];  // what this tick published
  const int G = root->hier_G;
  const void* gathered = block;
  if (G > 1) {
    // the exchange stream after the tick that wrote the block: on the tick's events when
    // its last kernels complete them (no marker on the leaf's queues; the leaf's stream
    // parts stay unjoined), else after a join, on an event
    const bool same = leaf->stream == root->stream;
    const FollowOrder fo = follow_last_tick(leaf->done.sig, same);
    if (fo.join) DM_HIP(root, leaf->order.join(), "join leaf streams");
    if (!same) leaf->done.sig.want();
    DM_HIP(root, wait_leaf(leaf, fo.wait, root->stream), "leaf->exchange order");
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
  CarryInputs ci;
  ci.carry_ok = root->carry_ok != 0;
  ci.servers = G;
  ci.same_stream = root->stream == leaf->stream;
  ci.pipelined = leaf->tpl.on;
  rc = root_round(root, gathered, G, now_ns, leaf, root->hs_server, carry_round(ci));
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
