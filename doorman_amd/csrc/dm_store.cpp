// dm_store.cpp — a store and its configuration onto the device (dm_store_load,
// dm_store_load_device, dm_config_load) and the calls that read them back (dm_read_*, into
// host memory or, dm_read_*_device, into device memory).
#include "dm_ctx.h"

// Could some non-small resource need k_general (heterogeneous subclients or NaN
// wants among its rows)?  Conservative: expiry is ignored.
// Could any FairShare resource need k_general (live subclients not all equal, or NaN
// wants)?  Released rows (DM_RELEASED) are never live, so they do not count.
static bool scan_maybe_general(const int64_t* off, int64_t R, const int64_t* sub, const double* wants,
                               const int64_t* exp) {
  for (int64_t r = 0; r < R; ++r) {
    if (off[r + 1] - off[r] <= kSmallMax) continue;
    int64_t s0 = -1;
    for (int64_t i = off[r]; i < off[r + 1]; ++i) {
      if (exp[i] == DM_RELEASED) continue;
      if (std::isnan(wants[i])) return true;
      if (s0 < 0) s0 = sub[i];
      if (sub[i] != s0) return true;
    }
  }
  return false;
}

// A store was just loaded: the four columns, the running sums and the explicit flags are
// on the device (enqueued on the context stream).  What both loads do from there, so that
// they cannot drift apart: the layout on host and device, the row index, the plan, and the
// host's flags and state.  seg_off: the layout in host memory; dev_seg_off: the same in device
// memory where the caller has it there (copied in HBM), else null (uploaded).
static int store_loaded(dm_ctx* c, int64_t R, int64_t N, const int64_t* seg_off, const int64_t* dev_seg_off,
                        bool maybe_general, bool all_sub_one) {
  c->R = R;
  c->N = N;
  c->h_seg_off.assign(seg_off, seg_off + R + 1);
  c->seg_uniform = uniform_rows(seg_off, R);  // every resource the same number of rows (a hierarchy root store: G)
  hipStream_t st = c->stream;
  if (dev_seg_off) {
    DM_HIP(c, c->seg_off.ensure((size_t)R + 1), "copy seg_off");
    DM_HIP(c, hipMemcpyAsync(c->seg_off.p, dev_seg_off, ((size_t)R + 1) * 8, hipMemcpyDeviceToDevice, st),
           "copy seg_off");
  } else {
    DM_HIP(c, upload(c->seg_off, seg_off, (size_t)R + 1, st), "upload seg_off");
  }
  {  // RowIndex: resource of the first row of every 2^kRowBlkShift-row block
    const int64_t nb = (N >> kRowBlkShift) + 2;
    std::vector<int32_t> blk((size_t)nb, 0);
    int64_t sg = 0;
    for (int64_t b = 0; b < nb && R > 0; ++b) {
      const int64_t row = std::min<int64_t>(b << kRowBlkShift, std::max<int64_t>(N - 1, 0));
      while (sg + 1 < R && seg_off[sg + 1] <= row) ++sg;
      blk[(size_t)b] = (int32_t)sg;
    }
    DM_HIP(c, upload(c->blk_seg, blk.data(), blk.size(), st), "upload row index");
    DM_HIP(c, hipStreamSynchronize(st), "upload row index");  // blk leaves scope
  }
  build_plan(c);
  int rc = upload_plan(c);
  if (rc) return rc;
  c->maybe_general = maybe_general;
  c->all_sub_one = all_sub_one;
  DM_HIP(c, hipStreamSynchronize(st), "store load");
  c->store_loaded = true;
  c->rounds_in_tick = 0;
  c->cl_valid = false;  // the last clean's list named rows of the store this one replaced
  c->store_lost = false;  // upload_plan cleared the device's failure words
  c->expl_rows = true;
  c->rows_changed();
  c->have_result = false;
  c->wb_inplace = -1;
  c->hints_set = false;
  if (c->cfg_loaded && (int64_t)c->h_refresh_s.size() != R) c->cfg_loaded = false;
  return DM_OK;
}

int dm_store_load(dm_ctx* c, const dm_snapshot* s) {
  DM_ENTER(c);
  async_drain(c);
  if (!s || s->n_resources < 0 || s->n_leases < 0 || !s->seg_off) return c->fail(DM_E_INVAL, "bad snapshot");
  const int64_t R = s->n_resources, N = s->n_leases;
  if (R > INT32_MAX - 1) return c->fail(DM_E_INVAL, "too many resources for one context (max 2^31-2)");
  if (N > 0 && (!s->wants || !s->has || !s->subclients || !s->expiry_ns))
    return c->fail(DM_E_INVAL, "snapshot columns missing");
  if (s->seg_off[0] != 0 || s->seg_off[R] != N) return c->fail(DM_E_INVAL, "seg_off must run from 0 to n_leases");
  for (int64_t r = 0; r < R; ++r)
    if (s->seg_off[r + 1] < s->seg_off[r]) return c->fail(DM_E_INVAL, "seg_off must be non-decreasing");
  for (int64_t i = 0; i < N; ++i)
    if (s->subclients[i] < 0 || s->subclients[i] > kSubMax)
      return c->fail(DM_E_INVAL, "subclients must be in [0, 2^31-2]");
  const bool have_agg = s->agg_count && s->agg_sum_has && s->agg_sum_wants;
  if ((s->agg_count || s->agg_sum_has || s->agg_sum_wants) && !have_agg)
    return c->fail(DM_E_INVAL, "give all three running sums or none");
  DM_HIP(c, hipStreamSynchronize(c->stream), "sync");
  hipStream_t st = c->stream;
  DM_HIP(c, upload(c->wants, s->wants, (size_t)N, st), "upload wants");
  DM_HIP(c, upload(c->has, s->has, (size_t)N, st), "upload has");
  {
    std::vector<int32_t> sub32((size_t)N);
    // every loaded row keeps its own expiry (explicit, dm_device.h); a writeback tick
    // turns the live ones into followers of their resource's expiry
    for (int64_t i = 0; i < N; ++i) sub32[i] = (int32_t)((uint32_t)s->subclients[i] | kSubExplicit);
    DM_HIP(c, upload(c->sub, sub32.data(), (size_t)N, st), "upload subclients");
    DM_HIP(c, hipStreamSynchronize(st), "upload subclients");  // sub32 leaves scope
  }
  DM_HIP(c, upload(c->expiry, s->expiry_ns, (size_t)N, st), "upload expiry");
  std::vector<int64_t> cnt;
  std::vector<double> sh, sw;
  const int64_t* ac = s->agg_count;
  const double* ah = s->agg_sum_has;
  const double* aw = s->agg_sum_wants;
  if (!have_agg) {  // one Assign per row, in row order (store.go:156-158)
    cnt.assign(R, 0);
    sh.assign(R, 0.0);
    sw.assign(R, 0.0);
    for (int64_t r = 0; r < R; ++r)
      for (int64_t i = s->seg_off[r]; i < s->seg_off[r + 1]; ++i) {
        sh[r] += s->has[i] - 0.0;
        sw[r] += s->wants[i] - 0.0;
        cnt[r] += s->subclients[i];
      }
    ac = cnt.data();
    ah = sh.data();
    aw = sw.data();
  }
  std::vector<ResAgg> agg(R);
  for (int64_t r = 0; r < R; ++r) agg[r] = ResAgg{ac[r], ah[r], aw[r], 0};
  DM_HIP(c, upload(c->agg, agg.data(), (size_t)R, st), "upload running sums");
  const std::vector<uint8_t> expl((size_t)std::max<int64_t>(R, 1), 1);  // loaded rows carry explicit expiries
  DM_HIP(c, upload(c->expl, expl.data(), expl.size(), st), "upload explicit flags");
  const bool maybe_general = scan_maybe_general(s->seg_off, R, s->subclients, s->wants, s->expiry_ns);
  // released rows never take part in a tick, so they do not count against this
  bool all_sub_one = true;
  for (int64_t i = 0; i < N && all_sub_one; ++i)
    all_sub_one = s->subclients[i] == 1 || s->expiry_ns[i] == DM_RELEASED;
  return store_loaded(c, R, N, s->seg_off, nullptr, maybe_general, all_sub_one);
}

int dm_config_load(dm_ctx* c, int64_t R, const dm_resource_cfg* cfg) {
  DM_ENTER(c);
  // In-flight batches finish first (their arrivals take the lease lengths they were sent
  // under).  The store stays, so their outcome counts: every set is retired through
  // apply_check, which keeps maybe_general / all_sub_one true to the rows (a drained NaN
  // wants or other subclient count would otherwise leave later ticks on the non-general
  // path: tests/test_general_transitions_gpu.py), and a rejected batch's error is
  // returned instead of loading the configuration -- the caller calls again.
  if (int ra = async_retire_all(c)) return ra;
  c->rows_changed();
  if (!cfg || R < 0 || !cfg->kind || !cfg->capacity || !cfg->lease_length_s || !cfg->refresh_interval_s ||
      !cfg->learning_end_ns || !cfg->parent_expiry_ns || !cfg->safe_capacity)
    return c->fail(DM_E_INVAL, "bad config");
  for (int64_t r = 0; r < R; ++r) {
    if (cfg->lease_length_s[r] < 0 || cfg->refresh_interval_s[r] < 0)
      return c->fail(DM_E_INVAL, "lease_length and refresh_interval must be >= 0 (server.go:384-434)");
    if (cfg->refresh_interval_s[r] > INT32_MAX || cfg->lease_length_s[r] > INT32_MAX)
      return c->fail(DM_E_INVAL, "refresh_interval and lease_length must be < 2^31 s");
  }
  for (int64_t r = 0; r < R; ++r)
    if (cfg->kind[r] < DM_NO_ALGORITHM || cfg->kind[r] > DM_FAIR_SHARE) {
      char buf[96];
      snprintf(buf, sizeof buf, "unknown algorithm kind %d for resource %lld", cfg->kind[r], (long long)r);
      return c->fail(DM_E_KIND, buf);
    }
  DM_HIP(c, hipStreamSynchronize(c->stream), "sync");
  hipStream_t st = c->stream;
  std::vector<ResCfg> rc(R);
  std::vector<ResCold> rcold(R);
  for (int64_t r = 0; r < R; ++r) {
    rc[r] = ResCfg{cfg->capacity[r], cfg->learning_end_ns[r], cfg->parent_expiry_ns[r],
                   (int32_t)cfg->lease_length_s[r], cfg->kind[r]};
    rcold[r] = ResCold{cfg->safe_capacity[r], (int32_t)cfg->refresh_interval_s[r], 0};
  }
  c->tpl.q.drop_pending();  // staged exchanges were computed for the old configuration
  DM_HIP(c, upload(c->cfg, rc.data(), (size_t)R, st), "upload config");
  DM_HIP(c, upload(c->cold, rcold.data(), (size_t)R, st), "upload config");
  c->h_refresh_s.assign(cfg->refresh_interval_s, cfg->refresh_interval_s + R);
  c->h_kind.assign(cfg->kind, cfg->kind + R);
  if (c->store_loaded && R == c->R) {  // bin 4's shape by the new kinds
    if (int rc2 = update_bin4_shape(c, st)) return rc2;
  }
  DM_HIP(c, hipStreamSynchronize(st), "config load");
  c->cfg_loaded = true;
  return DM_OK;
}

// The two range reads, each one body for both destinations.  Host memory (device false): the
// plain columns are downloaded straight from the store or the tick's outputs, the resolved ones
// go through set 0's exp / sub and are downloaded from there.  The caller's device columns
// (checked by check_device_ptr, below): the same columns copied in HBM, the resolved ones
// written by the kernel where the caller wants them.
static int read_leases(dm_ctx* c, bool device, int64_t off, int64_t n, double* gets, int64_t* expiry_ns) {
  DM_ENTER(c);
  UpdateStage& S = c->stage[0];  // synchronous on return: set 0 (dm_update_stage.h)
  DM_STORE_READABLE(c);
  if (!c->have_result) return c->fail(DM_E_STATE, "no dm_apportion result");
  int rc = check_range(c, off, n, c->N);
  if (rc) return rc;
  if (device) {
    DM_DEVICE_PTR(c, gets, n * 8, "gets");
    DM_DEVICE_PTR(c, expiry_ns, n * 8, "expiry_ns");
  }
  hipStream_t st = c->stream;
  const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  DM_HIP(c, download(gets, c->last_writeback ? c->has.p : c->out_gets.p, off, n, st, kind), "read gets");
  if (expiry_ns && c->last_writeback) {  // the store's encoding, resolved on the device
    if (!device) DM_HIP(c, S.exp.ensure((size_t)std::max<int64_t>(n, 1)), "stage expiry");
    DM_HIP(c, launch_resolve_rows(n, nullptr, off, c->sub.p, c->expiry.p, c->row_index(), c->agg.p,
                                  device ? expiry_ns : S.exp.p, nullptr, st),
           "resolve expiry");
    if (!device) DM_HIP(c, download(expiry_ns, (const int64_t*)S.exp.p, 0, n, st), "read expiry");
  } else {
    DM_HIP(c, download(expiry_ns, (const int64_t*)c->out_expiry.p, off, n, st, kind), "read expiry");
  }
  return c->synced("read leases");
}

int dm_read_leases(dm_ctx* c, int64_t off, int64_t n, double* gets, int64_t* expiry_ns) {
  return read_leases(c, false, off, n, gets, expiry_ns);
}
int dm_read_leases_device(dm_ctx* c, int64_t off, int64_t n, double* gets, int64_t* expiry_ns) {
  return read_leases(c, true, off, n, gets, expiry_ns);
}

int dm_read_leases_rows(dm_ctx* c, int64_t n, const int64_t* rows, double* gets, int64_t* expiry_ns) {
  DM_ENTER(c);
  UpdateStage& S = c->stage[0];  // synchronous on return: set 0 (dm_update_stage.h)
  DM_STORE_READABLE(c);
  if (!c->have_result) return c->fail(DM_E_STATE, "no dm_apportion result");
  if (n < 0 || (n > 0 && !rows)) return c->fail(DM_E_INVAL, "bad rows");
  if (n == 0) return DM_OK;
  for (int64_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= c->N) return c->fail(DM_E_RANGE, "row out of range");
  const double* g = c->last_writeback ? c->has.p : c->out_gets.p;
  const int64_t* e = c->last_writeback ? nullptr : c->out_expiry.p;  // the store's encoding: resolved below
  DM_HIP(c, S.rows.ensure((size_t)n), "stage rows");
  DM_HIP(c, S.has.ensure((size_t)n), "stage gets");
  DM_HIP(c, S.exp.ensure((size_t)n), "stage expiry");
  DM_HIP(c, hipMemcpyAsync(S.rows.p, rows, (size_t)n * 8, hipMemcpyHostToDevice, c->stream), "stage rows");
  DM_HIP(c, launch_gather_leases(n, S.rows.p, g, e, S.has.p, S.exp.p, c->stream), "gather leases");
  if (!e)
    DM_HIP(c, launch_resolve_rows(n, S.rows.p, 0, c->sub.p, c->expiry.p, c->row_index(), c->agg.p, S.exp.p,
                                  nullptr, c->stream),
           "resolve expiry");
  DM_HIP(c, download(gets, (const double*)S.has.p, 0, n, c->stream), "read gets");
  DM_HIP(c, download(expiry_ns, (const int64_t*)S.exp.p, 0, n, c->stream), "read expiry");
  return c->synced("read leases");
}

int dm_read_leases_proto(dm_ctx* c, int64_t off, int64_t n, double* capacity, int64_t* expiry_time_s,
                         int64_t* refresh_interval_s) {
  std::vector<int64_t> e(n > 0 ? n : 0);
  int rc = dm_read_leases(c, off, n, capacity, e.data());
  if (rc) return rc;
  if (expiry_time_s)
    for (int64_t i = 0; i < n; ++i) {
      // time.Time.Unix(): floor division by 1e9 (server.go:789)
      int64_t v = e[i];
      if (v == DM_RELEASED) {
        expiry_time_s[i] = DM_RELEASED;
        continue;
      }
      int64_t q = v / kNs;
      if (v % kNs != 0 && v < 0) --q;
      expiry_time_s[i] = q;
    }
  if (refresh_interval_s && n > 0) {
    // the device config: a hierarchy exchange rewrites a leaf's algorithm (dm_hier_root_tick)
    const auto& so = c->h_seg_off;
    const int64_t r0 = std::upper_bound(so.begin(), so.end(), off) - so.begin() - 1;
    const int64_t r1 = std::upper_bound(so.begin(), so.end(), off + n - 1) - so.begin() - 1;
    std::vector<ResCold> cf((size_t)(r1 - r0 + 1));
    DM_HIP(c, download(cf.data(), (const ResCold*)c->cold.p, r0, r1 - r0 + 1, c->stream), "read config");
    DM_HIP(c, hipStreamSynchronize(c->stream), "read config");
    int64_t r = r0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t row = off + i;
      while (r + 1 < (int64_t)so.size() && so[r + 1] <= row) ++r;
      refresh_interval_s[i] = e[i] == DM_RELEASED ? 0 : cf[(size_t)(r - r0)].refresh_s;
    }
  }
  return DM_OK;
}

int dm_read_resources(dm_ctx* c, int64_t r0, int64_t n, int64_t* count, double* sum_has, double* sum_wants,
                      double* safe) {
  DM_ENTER(c);
  DM_STORE_READABLE(c);
  int rc = check_range(c, r0, n, c->R);
  if (rc) return rc;
  if (safe && !c->have_result) return c->fail(DM_E_STATE, "safe capacity needs a dm_apportion result");
  const bool wb = !c->have_result || c->last_writeback;
  std::vector<ResAgg> v(n > 0 ? n : 0);
  std::vector<ResCfg> cf(safe && n > 0 ? n : 0);
  std::vector<ResCold> cc(safe && n > 0 ? n : 0);
  DM_HIP(c, download(v.data(), (const ResAgg*)(wb ? c->agg.p : c->res.p), r0, n, c->stream), "read resources");
  // the device config: a hierarchy exchange rewrites a leaf's templates (dm_hier_root_tick)
  if (safe) DM_HIP(c, download(cf.data(), (const ResCfg*)c->cfg.p, r0, n, c->stream), "read config");
  if (safe) DM_HIP(c, download(cc.data(), (const ResCold*)c->cold.p, r0, n, c->stream), "read config");
  if (int rs = c->synced("read resources")) return rs;
  for (int64_t i = 0; i < n; ++i) {
    if (count) count[i] = v[i].count;
    if (sum_has) sum_has[i] = v[i].sum_has;
    if (sum_wants) sum_wants[i] = v[i].sum_wants;
    // SetSafeCapacity (resource.go:81-96) after the tick's Clean: configured, or capacity / Count
    if (safe) safe[i] = safe_capacity_of(cf[i].capacity, cc[i].safe_capacity, v[i].count);
  }
  return DM_OK;
}

int dm_read_config(dm_ctx* c, int64_t r0, int64_t n, int32_t* kind, double* capacity, int64_t* lease_length_s,
                   int64_t* refresh_interval_s, int64_t* learning_end_ns, int64_t* parent_expiry_ns,
                   double* safe_capacity) {
  DM_ENTER(c);
  if (!c->cfg_loaded) return c->fail(DM_E_STATE, "no configuration loaded");
  int rc = check_range(c, r0, n, c->R);
  if (rc) return rc;
  std::vector<ResCfg> v(n > 0 ? (size_t)n : 0);
  std::vector<ResCold> vc(n > 0 ? (size_t)n : 0);
  DM_HIP(c, download(v.data(), (const ResCfg*)c->cfg.p, r0, n, c->stream), "read config");
  DM_HIP(c, download(vc.data(), (const ResCold*)c->cold.p, r0, n, c->stream), "read config");
  DM_HIP(c, hipStreamSynchronize(c->stream), "read config");
  for (int64_t i = 0; i < n; ++i) {
    if (kind) kind[i] = v[i].kind;
    if (capacity) capacity[i] = v[i].capacity;
    if (lease_length_s) lease_length_s[i] = v[i].lease_len_s;
    if (refresh_interval_s) refresh_interval_s[i] = vc[i].refresh_s;
    if (learning_end_ns) learning_end_ns[i] = v[i].learning_end_ns;
    if (parent_expiry_ns) parent_expiry_ns[i] = v[i].parent_expiry_ns;
    if (safe_capacity) safe_capacity[i] = vc[i].safe_capacity;
  }
  return DM_OK;
}

static int read_store(dm_ctx* c, bool device, int64_t off, int64_t n, double* has, double* wants, int64_t* sub,
                      int64_t* exp) {
  DM_ENTER(c);
  UpdateStage& S = c->stage[0];  // synchronous on return: set 0 (dm_update_stage.h)
  DM_STORE_READABLE(c);
  if (!c->store_loaded) return c->fail(DM_E_STATE, "no store loaded");
  int rc = check_range(c, off, n, c->N);
  if (rc) return rc;
  if (device) {
    DM_DEVICE_PTR(c, has, n * 8, "has");
    DM_DEVICE_PTR(c, wants, n * 8, "wants");
    DM_DEVICE_PTR(c, sub, n * 8, "subclients");
    DM_DEVICE_PTR(c, exp, n * 8, "expiry_ns");
  }
  hipStream_t st = c->stream;
  const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  DM_HIP(c, download(has, (const double*)c->has.p, off, n, st, kind), "read has");
  DM_HIP(c, download(wants, (const double*)c->wants.p, off, n, st, kind), "read wants");
  if ((sub || exp) && n > 0) {  // subclients and expiry from the column encoding (dm_device.h)
    if (!device) {
      DM_HIP(c, S.exp.ensure((size_t)n), "stage expiry");
      DM_HIP(c, S.sub.ensure((size_t)n), "stage subclients");
    }
    DM_HIP(c, launch_resolve_rows(n, nullptr, off, c->sub.p, c->expiry.p, c->row_index(), c->agg.p,
                                  device || !exp ? exp : S.exp.p, device || !sub ? sub : S.sub.p, st),
           "resolve rows");
    if (!device) {
      DM_HIP(c, download(exp, (const int64_t*)S.exp.p, 0, n, st), "read expiry");
      DM_HIP(c, download(sub, (const int64_t*)S.sub.p, 0, n, st), "read subclients");
    }
  }
  return c->synced("read store");
}

int dm_read_store(dm_ctx* c, int64_t off, int64_t n, double* has, double* wants, int64_t* sub, int64_t* exp) {
  return read_store(c, false, off, n, has, wants, sub, exp);
}
int dm_read_store_device(dm_ctx* c, int64_t off, int64_t n, double* has, double* wants, int64_t* sub, int64_t* exp) {
  return read_store(c, true, off, n, has, wants, sub, exp);
}

// ---- the store from and into device memory (dm_load.hip) ----

// A caller's device column (dm_ctx.h DM_DEVICE_PTR), for the device calls of this unit and the
// device twins of the update calls (dm_store_update.cpp): p must be device memory of the
// context's device, and where the runtime knows p's allocation, that allocation must hold
// `bytes` bytes from p.  Asked of the runtime before any kernel or copy is given p.
int dm::check_device_ptr(dm_ctx* c, const void* p, size_t bytes, const char* what) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // (a pointer the runtime does not know: plain host memory on older runtimes)
    return c->fail(DM_E_INVAL, std::string(what) + " is not device memory");
  }
  if (at.type != hipMemoryTypeDevice) return c->fail(DM_E_INVAL, std::string(what) + " is not device memory");
  if (at.device != c->device) return c->fail(DM_E_INVAL, std::string(what) + " is memory of another device");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();  // no allocation reported: the attributes are what there is
    return DM_OK;
  }
  const char *b = (const char*)base, *q = (const char*)p;
  if (q < b || (size_t)(q - b) > size || bytes > size - (size_t)(q - b))
    return c->fail(DM_E_INVAL, std::string(what) + ": its allocation does not hold the column");
  return DM_OK;
}

int dm_store_load_device(dm_ctx* c, const dm_snapshot* s) {
  DM_ENTER(c);
  async_drain(c);
  if (!s || s->n_resources < 0 || s->n_leases < 0 || !s->seg_off) return c->fail(DM_E_INVAL, "bad snapshot");
  const int64_t R = s->n_resources, N = s->n_leases;
  if (R > INT32_MAX - 1) return c->fail(DM_E_INVAL, "too many resources for one context (max 2^31-2)");
  if (N > 0 && (!s->wants || !s->has || !s->subclients || !s->expiry_ns))
    return c->fail(DM_E_INVAL, "snapshot columns missing");
  const bool have_agg = s->agg_count && s->agg_sum_has && s->agg_sum_wants;
  if ((s->agg_count || s->agg_sum_has || s->agg_sum_wants) && !have_agg)
    return c->fail(DM_E_INVAL, "give all three running sums or none");
  DM_DEVICE_PTR(c, s->seg_off, (R + 1) * 8, "seg_off");
  DM_DEVICE_PTR(c, s->wants, N * 8, "wants");
  DM_DEVICE_PTR(c, s->has, N * 8, "has");
  DM_DEVICE_PTR(c, s->subclients, N * 8, "subclients");
  DM_DEVICE_PTR(c, s->expiry_ns, N * 8, "expiry_ns");
  DM_DEVICE_PTR(c, s->agg_count, R * 8, "agg_count");
  DM_DEVICE_PTR(c, s->agg_sum_has, R * 8, "agg_sum_has");
  DM_DEVICE_PTR(c, s->agg_sum_wants, R * 8, "agg_sum_wants");
  hipStream_t st = c->stream;
  DM_HIP(c, hipStreamSynchronize(st), "sync");
  // Validation reads the caller's columns only: the layout on the host (the plan is built
  // from it anyway), the rows by k_ld_check.  A rejection leaves the store as it was.
  std::vector<int64_t> off((size_t)R + 1);
  DM_HIP(c, hipMemcpyAsync(off.data(), s->seg_off, off.size() * 8, hipMemcpyDeviceToHost, st), "read seg_off");
  DM_HIP(c, hipStreamSynchronize(st), "read seg_off");
  if (off[0] != 0 || off[(size_t)R] != N) return c->fail(DM_E_INVAL, "seg_off must run from 0 to n_leases");
  for (int64_t r = 0; r < R; ++r)
    if (off[(size_t)r + 1] < off[(size_t)r]) return c->fail(DM_E_INVAL, "seg_off must be non-decreasing");
  DM_HIP(c, c->ld_flags.ensure(1), "load flags");
  const LoadArgs a{R,           N,           s->wants,         s->has,        s->subclients, s->expiry_ns,
                   s->agg_count, s->agg_sum_has, s->agg_sum_wants, c->ld_flags.p};
  uint32_t f = 0;
  DM_HIP(c, launch_load_check(a, st), "check rows");
  DM_HIP(c, hipMemcpyAsync(&f, c->ld_flags.p, sizeof f, hipMemcpyDeviceToHost, st), "read load flags");
  DM_HIP(c, hipStreamSynchronize(st), "check rows");
  if (f & kLdBadSub) return c->fail(DM_E_INVAL, "subclients must be in [0, 2^31-2]");
  // from here on the context's own columns are written
  const size_t n = (size_t)N;
  DM_HIP(c, c->wants.ensure(n), "store columns");
  DM_HIP(c, c->has.ensure(n), "store columns");
  DM_HIP(c, c->sub.ensure(n), "store columns");
  DM_HIP(c, c->expiry.ensure(n), "store columns");
  DM_HIP(c, c->agg.ensure((size_t)R), "running sums");
  DM_HIP(c, c->expl.ensure((size_t)std::max<int64_t>(R, 1)), "explicit flags");
  if (N > 0) {
    DM_HIP(c, hipMemcpyAsync(c->wants.p, s->wants, n * 8, hipMemcpyDeviceToDevice, st), "copy wants");
    DM_HIP(c, hipMemcpyAsync(c->has.p, s->has, n * 8, hipMemcpyDeviceToDevice, st), "copy has");
    DM_HIP(c, hipMemcpyAsync(c->expiry.p, s->expiry_ns, n * 8, hipMemcpyDeviceToDevice, st), "copy expiry");
  }
  DM_HIP(c, launch_load_sub(a, c->sub.p, st), "load subclients");
  DM_HIP(c, launch_load_resources(a, s->seg_off, c->agg.p, st), "load running sums");
  DM_HIP(c, hipMemsetAsync(c->expl.p, 1, c->expl.n, st), "explicit flags");  // loaded rows carry explicit expiries
  DM_HIP(c, hipMemcpyAsync(&f, c->ld_flags.p, sizeof f, hipMemcpyDeviceToHost, st), "read load flags");
  DM_HIP(c, hipStreamSynchronize(st), "load rows");
  return store_loaded(c, R, N, off.data(), s->seg_off, (f & kLdGeneral) != 0, !(f & kLdNotOne));
}

int dm_read_store_sums_device(dm_ctx* c, int64_t r0, int64_t n, int64_t* count, double* sum_has, double* sum_wants) {
  DM_ENTER(c);
  DM_STORE_READABLE(c);
  int rc = check_range(c, r0, n, c->R);
  if (rc) return rc;
  DM_DEVICE_PTR(c, count, n * 8, "count");
  DM_DEVICE_PTR(c, sum_has, n * 8, "sum_has");
  DM_DEVICE_PTR(c, sum_wants, n * 8, "sum_wants");
  // always the store's running sums (agg), never a non-writeback tick's view (res)
  if (n > 0) DM_HIP(c, launch_unpack_sums(c->agg.p + r0, n, count, sum_has, sum_wants, c->stream), "read sums");
  return c->synced("read sums");
}
