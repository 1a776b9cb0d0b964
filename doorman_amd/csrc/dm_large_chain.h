// dm_large_chain.h — the host half of the large-resource chain (the device half: the unit
// dm_tick_large.hip, its forms in dm_tick_large.h, _spec.h and _het.h): the one
// owner of what the chain keeps from tick to tick.  dm_large_form.h decides the form of a
// tick's launches (plain C++, tested on the CPU); LargeChain holds the buffers and the words
// the device tells the host, and Tick::large_chain (dm_tick.cpp) asks, then launches.
// Part of dm_ctx.h, which includes it below the buffer types and the kernel classes it uses.
#pragma once

namespace dm {

// A phase's profiling class and grid: per chunk, per large resource, pass B's (per large
// resource under Partials::b_first, else per chunk), k_large_e's 2-D grid of a resource's
// buckets by fours, the redo's team grid of its build.
enum class LargeGrid : uint8_t { chunk, resource, pass_b, buckets, redo };
struct LargePhaseRow {
  int cls;
  LargeGrid grid;
};
constexpr LargePhaseRow kLargePhaseRows[kLargePhases] = {  // by LargePhase
    {KC_LARGE_A, LargeGrid::chunk},     {KC_LARGE_B, LargeGrid::pass_b},  {KC_LARGE_T, LargeGrid::resource},
    {KC_LARGE_C, LargeGrid::chunk},     {KC_LARGE_CH, LargeGrid::chunk},  {KC_LARGE_E, LargeGrid::buckets},
    {KC_LARGE_MAP, LargeGrid::chunk},   {KC_LARGE_MH, LargeGrid::chunk},  {KC_LARGE_FIN, LargeGrid::resource},
    {KC_LARGE_SPEC, LargeGrid::chunk},  {KC_LARGE_REDO, LargeGrid::redo}, {KC_LARGE_REDO, LargeGrid::redo}};
static_assert(kLargePhaseRows[(int)LargePhase::T].cls == KC_LARGE_T &&
                  kLargePhaseRows[(int)LargePhase::MAP].cls == KC_LARGE_MAP &&
                  kLargePhaseRows[(int)LargePhase::FIN].cls == KC_LARGE_FIN &&
                  kLargePhaseRows[(int)LargePhase::SPEC].cls == KC_LARGE_SPEC,
              "the rows follow LargePhase's order");

struct LargeChain {
  // the chunks' partials of each pass (Partials), the per-resource totals and the map's counts
  DBuf<int64_t> a_cnt, a_cnt_all, a_smin, a_smax, b_w, c_sgt;
  DBuf<double> a_has, a_wants, a_has_all, a_wants_all, b_x, b_y, c_ee, d_delta;
  DBuf<int32_t> a_nan;
  DBuf<uint32_t> a_live;
  DBuf<uint8_t> tot;
  DBuf<int32_t> uni;
  // the last call that changed the store was a writeback tick through the chain
  // (Partials::s_live): taken and cleared at the start of every tick, cleared by every call
  // that writes a subclients word or releases a row (rows_written)
  bool live_ok = false;
  void rows_written() { live_ok = false; }
  // The speculative form (k_large_spec + k_large_redo_team; DM_SPEC_CHAIN=0: the chain): per
  // large resource its SpecTot, the redo's launch count, the host-mapped words
  bool spec_chain = true;
  DBuf<SpecTot> spec;
  DBuf<uint32_t> spec_ring;  // SpecArgs::ring
  uint64_t spec_seq = 0;
  HBuf<int32_t> h_serr;  // [0] the give-up flag, [1] SpecArgs::seen
  // 3/4 of the redo workgroups (full build) the GPU holds at once (dm_create): the full
  // build's grid when the store has that many team slots; dm_plan_info slot 5 + kNumBins
  int64_t redo_cap = 0;
  // the redo by teams: team slots and the two builds' grids (only a team waits for itself,
  // so kTeamMax co-resident workgroups finish any resource)
  DBuf<int32_t> team;
  int nslots = 0, team_grid_full = 1, team_grid_light = 1;
  // the redo's light build (dm_large_form.h LargeForm::ask_seen has the rule)
  int redo_light = 1;        // DM_REDO_LIGHT
  uint64_t redo_epoch = 0;   // dm_ctx::write_epoch at the last speculative tick
  // heterogeneous FairShare on the chain (allocated by the first tick that may need it)
  DBuf<uint32_t> h_set;  // per large resource: distinct subclient counts (all ones between ticks)
  DBuf<int32_t> h_n, h_bkc;
  size_t h_set_ready = 0;  // large resources whose set slots are initialised
  DBuf<uint8_t> h_res;
  DBuf<double> h_bkw;
  DBuf<int64_t> h_bks;

  template <typename... B>
  static hipError_t ensure_each(size_t n, B&... b) {  // in argument order
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? b.ensure(n) : e), ...);
    return e;
  }

  // A new plan (upload_plan): buffers sized for its chunks and large resources, no resource
  // with totals to speculate on (SpecTot::valid 0), the team slots, the words at their start.
  // The allocations keep this order.
  hipError_t plan(const std::vector<LargeSeg>& h_large, const std::vector<Chunk>& h_chunks, hipStream_t st) {
    const size_t nc = std::max<size_t>(h_chunks.size(), 1), nl = std::max<size_t>(h_large.size(), 1);
    hipError_t e = ensure_each(nc, a_cnt, a_cnt_all, a_has_all, a_wants_all, a_smin, a_smax, b_w, c_sgt, a_has,
                               a_wants, b_x, b_y, c_ee, d_delta, a_nan);
    if (e == hipSuccess) e = a_live.ensure(nc * 256);
    if (e == hipSuccess) e = uni.ensure(nc);
    if (e == hipSuccess) e = tot.ensure(nl * kSegTotBytes);
    if (e == hipSuccess) e = spec.ensure(nl);
    if (e == hipSuccess) e = hipMemsetAsync(spec.p, 0, nl * sizeof(SpecTot), st);
    if (e == hipSuccess) e = spec_ring.ensure(4);
    if (e == hipSuccess) e = hipMemsetAsync(spec_ring.p, 0, 4 * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    std::vector<int32_t> slots;
    for (size_t l = 0; l < h_large.size(); ++l) {
      const int nch_l = h_large[l].chunk_end - h_large[l].chunk_begin;
      for (int m = 0; m < std::min(nch_l, kTeamMax); ++m) slots.push_back((int32_t)(l << 8 | (size_t)m));
    }
    nslots = (int)slots.size();
    e = team.ensure(slots.size());
    if (e == hipSuccess && nslots > 0)
      e = hipMemcpyAsync(team.p, slots.data(), slots.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    // every team's members can be resident at once: >= kTeamMax workgroups (the full
    // build: up to what the GPU holds; the light one: a steady tick's launch is all it costs)
    team_grid_full = std::max(1, (int)std::min<int64_t>(nslots, std::max<int64_t>(kTeamMax, redo_cap)));
    team_grid_light = std::max(1, std::min(nslots, kTeamMax));
    spec_seq = 0;
    if (e == hipSuccess && !h_serr.p) e = h_serr.alloc(2, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    __atomic_store_n(h_serr.p, 0, __ATOMIC_RELAXED);
    __atomic_store_n(h_serr.p + 1, 1, __ATOMIC_RELAXED);  // no redo seen yet: the full build first
    return hipMemsetAsync(tot.p, 0, nl * kSegTotBytes, st);  // SegTot::rel starts clear
  }

  // (without the heterogeneous buffers: with_het; b_first and s_live are the form's)
  Partials partials() const {
    return Partials{a_cnt.p, a_has.p, a_wants.p, a_cnt_all.p, a_has_all.p, a_wants_all.p, a_smin.p, a_smax.p,
                    a_nan.p, b_x.p,   b_y.p,     b_w.p,       c_ee.p,      c_sgt.p,       d_delta.p, a_live.p,
                    tot.p,   nullptr, nullptr,   nullptr,     nullptr,     nullptr,       nullptr,   0,
                    0,       uni.p};
  }

  // The heterogeneous form's buffers into P: allocated by the first tick that needs them, the
  // resources' sets initialised once (k_large_t leaves them empty for the next tick).
  hipError_t with_het(Partials& P, int nls, int nch, hipStream_t st) {
    const size_t nc = (size_t)nch, nl = (size_t)std::max(nls, 1);
    hipError_t e = hipSuccess;
    if (h_set_ready < nl || h_set.n < nl * 2 * kHetMaxS) {
      e = h_set.ensure(nl * 2 * kHetMaxS);
      if (e == hipSuccess) e = h_n.ensure(nl);
      if (e == hipSuccess) e = hipMemsetAsync(h_set.p, 0xFF, nl * 2 * kHetMaxS * sizeof(uint32_t), st);
      if (e == hipSuccess) e = hipMemsetAsync(h_n.p, 0, nl * sizeof(int32_t), st);
      if (e != hipSuccess) return e;
      h_set_ready = nl;
    }
    e = h_res.ensure(nl * sizeof(HetRes));
    if (e == hipSuccess) e = ensure_each(nc * kHetBuckets, h_bkw, h_bks, h_bkc);
    P.s_set = h_set.p;
    P.s_n = h_n.p;
    P.het = h_res.p;
    P.bk_w = h_bkw.p;
    P.bk_s = h_bks.p;
    P.bk_c = h_bkc.p;
    return e;
  }

  // A speculative tick's arguments: its launch number and parity, then the next tick's.
  SpecArgs spec_args(int nch) {
    const SpecArgs S{spec.p, spec_seq, h_serr.d, spec_ring.p, (int)(spec_seq & 1), nch,
                     reinterpret_cast<uint32_t*>(h_serr.d + 1), team.p, nslots};
    spec_seq += 1;
    return S;
  }
  // The redo's word (SpecArgs::seen): whether a redo since the last reading found a resource
  // marked.  Reading clears it, so only a tick whose form asks reads it (LargeForm::ask_seen).
  bool take_seen() { return __atomic_exchange_n(h_serr.p + 1, 0, __ATOMIC_RELAXED) != 0; }
  // a redo workgroup gave up waiting for its resource's others (dm_ctx::check_device)
  bool gave_up() const { return h_serr.p && __atomic_load_n(h_serr.p, __ATOMIC_RELAXED); }

  dim3 grid(LargePhase ph, int nch, int nls, bool b_first) const {
    switch (kLargePhaseRows[(int)ph].grid) {
      case LargeGrid::chunk: return dim3(nch);
      case LargeGrid::resource: return dim3(nls);
      case LargeGrid::pass_b: return dim3(b_first ? nls : nch);
      case LargeGrid::buckets: return dim3(nls, (kHetBuckets + 3) / 4);
      case LargeGrid::redo: break;
    }
    return dim3(ph == LargePhase::REDO_LIGHT ? team_grid_light : team_grid_full);
  }
};
static_assert(!std::is_copy_constructible<LargeChain>::value, "the chain's buffers have one owner");

}  // namespace dm
