// dm_tick_large.hip — the large-resource chain of a tick: k_large_a/b/c/map/fin, its
// speculative form (k_large_spec, k_large_redo_team) and its heterogeneous-subclient
// form (k_large_t, k_large_c_het, k_large_e, k_large_map_het).  The algorithms' mapping
// and the float semantics: dm_tick_group.hip.
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_threshold_util.h"

namespace dm {

// the chain's gets stores are non-temporal (see kGroupNT, dm_tick_group.h)
constexpr bool kSpecNT = true;

// --------------------------------------------------------------------------
// Large resources (n > kLargeMin): kChunkRows-row chunks, one workgroup each.
// Per-resource totals are re-derived in every workgroup from the chunk partials
// with the same fixed reduction tree, so all chunks of a resource agree exactly.
// --------------------------------------------------------------------------
struct SegTot {
  AggA a;
  AggB b;
  uint32_t pad[7];  // pad[0]: the map's arrival counter (k_large_map finishes the resource; its
                    // last arriver resets it)
  // nonzero when some chunk's Clean released subclients this tick (pass A, atomicOr),
  // i.e. round 1 must be recomputed; cleared by k_large_fin for the next tick.  With
  // it zero, pass B's other chunks return at once and its first chunk leaves the
  // speculative round-1 totals for C and the map (no O(chunks) re-reduction there)
  uint32_t rel;
};
static_assert(sizeof(SegTot) <= kSegTotBytes, "SegTot slot");
__device__ __forceinline__ SegTot* seg_tot(const Partials& P, int lseg) {
  return reinterpret_cast<SegTot*>(P.tot + (size_t)lseg * kSegTotBytes);
}

template <int G>
__device__ __forceinline__ SegState seg_state(const DevParams& p, const Partials& P, const LargeSeg& L,
                                              Lds<G>& lds) {
  AggA a = zeroA();
  for (int c = L.chunk_begin + (int)threadIdx.x; c < L.chunk_end; c += G) {
    AggA x;
    x.cnt = P.a_cnt[c];
    x.h = P.a_has[c];
    x.w = P.a_wants[c];
    x.all = AggR{P.a_cnt_all[c], P.a_has_all[c], P.a_wants_all[c]};
    x.smin = (int)P.a_smin[c];
    x.smax = (int)P.a_smax[c];
    x.nan = P.a_nan[c];
    x.nlive = 0;
    const AggR all = OpR()(a.all, x.all);  // OpA carries `all` through unchanged
    a = OpA()(a, x);
    a.all = all;
  }
  {
    const AggR all_part = a.all;
    a = group_reduce<G>(a, OpA(), lds.a);
    if (p.recompute) a.all = group_reduce<G>(all_part, OpR(), lds.r);
  }
  return seg_state_of(p, L.seg, a);
}

template <int G>
__device__ __forceinline__ AggB seg_b(const Partials& P, const LargeSeg& L, Lds<G>& lds) {
  AggB b{0.0, 0.0, 0};
  for (int c = L.chunk_begin + (int)threadIdx.x; c < L.chunk_end; c += G) b = OpB()(b, AggB{P.b_x[c], P.b_y[c], P.b_w[c]});
  return group_reduce<G>(b, OpB(), lds.b);
}

template <int G>
__device__ __forceinline__ AggC seg_c(const Partials& P, const LargeSeg& L, Lds<G>& lds) {
  AggC c{0.0, 0};
  for (int q = L.chunk_begin + (int)threadIdx.x; q < L.chunk_end; q += G) c = OpC()(c, AggC{P.c_ee[q], P.c_sgt[q]});
  return group_reduce<G>(c, OpC(), lds.c);
}

// kChunkRows rows of one chunk, kLR per thread, loaded in one batch (all loads in
// flight before the first use).
constexpr int kLR = kChunkRows / 256;
struct ChunkRows {
  double w[kLR], h[kLR];
  int s[kLR];
  unsigned valid, live;
  unsigned expl, rel;  // rows whose expiry is explicit / already marked released (dm_device.h)
};
// Pass A: wants and subclients of the chunk's rows (loads issued before any is
// consumed, see group_segment), liveness from the expiry encoding, then has for
// the rows Clean releases only (every row in recompute mode): the steady state
// reads 12 of a lease's 20 bytes here (C2: 122 -> 73 MB per tick).
// uni >= 0: the subclients words are not read -- a row whose bit in prev_live (the
// last writeback tick's live bits, Partials::s_live) is set holds uni, any other row is
// marked released
template <bool ALLH = false>  // ALLH: has of every row, loaded beside wants (the speculative chain)
__device__ __forceinline__ void load_chunk(const DevParams& p, const Chunk& ch, ChunkRows& r, const Res& rs,
                                           int uni = -1, uint32_t prev_live = 0) {
  const double* __restrict__ wb = p.wants + ch.row0;
  const double* __restrict__ hb = p.has + ch.row0;
  const int32_t* __restrict__ sb = p.sub + ch.row0;
  const int64_t* __restrict__ eb = p.expiry + ch.row0;
  r.valid = r.live = r.expl = r.rel = 0;
  int sr[kLR];
  // the wants loads leave first, whichever form follows: they wait only for the chunk
  // record, not for the per-chunk count (uni) that picks the form (one memory latency
  // less per workgroup in the steady state)
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    const int i = k * 256 + threadIdx.x;
    r.w[k] = wb[(unsigned)(i < ch.nrows ? i : ch.nrows - 1)];
    r.h[k] = ALLH ? hb[(unsigned)(i < ch.nrows ? i : ch.nrows - 1)] : 0.0;
  }
  if (uni >= 0) {
#pragma unroll
    for (int k = 0; k < kLR; ++k) sr[k] = (prev_live >> k & 1) ? uni : (int32_t)kSubReleased;
  } else {
#pragma unroll
    for (int k = 0; k < kLR; ++k) {
      const int i = k * 256 + threadIdx.x;
      sr[k] = sb[(unsigned)(i < ch.nrows ? i : ch.nrows - 1)];
    }
  }
  int64_t e[kLR];
#pragma unroll
  for (int k = 0; k < kLR; ++k) e[k] = rs.follow_exp;
  if (any_explicit(rs)) {  // the resource's flag (see group_segment)
#pragma unroll
    for (int k = 0; k < kLR; ++k) {
      const int i = k * 256 + threadIdx.x;
      const int64_t x = eb[(unsigned)(i < ch.nrows ? i : ch.nrows - 1)];
      if (sub_explicit(sr[k])) e[k] = x;
    }
  }
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    const unsigned vk = (k * 256 + (int)threadIdx.x < ch.nrows) ? 1u : 0u;
    r.valid |= vk << k;
    if (sub_released(sr[k])) e[k] = kReleased;
    r.live |= (vk & (p.now > e[k] ? 0u : 1u)) << k;
    r.expl |= (sub_explicit(sr[k]) ? 1u : 0u) << k;
    r.rel |= (sub_released(sr[k]) ? 1u : 0u) << k;
    r.s[k] = sub_value(sr[k]);
  }
  // a row already marked released holds has 0 (every path that marks one zeroes it)
  const unsigned need_h = ALLH ? 0u : p.recompute ? r.valid : (r.valid & ~r.live & ~r.rel);
  if (__any(need_h != 0)) {
#pragma unroll
    for (int k = 0; k < kLR; ++k)
      if (need_h >> k & 1) r.h[k] = hb[(unsigned)(k * 256 + threadIdx.x)];
  }
}

// Passes B, C and the map: wants (plus has / subclients where the pass uses them)
// of the chunk's rows and the live mask pass A left instead of re-reading expiry.
__device__ __forceinline__ void load_chunk_w(const DevParams& p, const Partials& P, const Chunk& ch,
                                             ChunkRows& r, bool with_sub, bool with_has = false) {
  const double* __restrict__ wb = p.wants + ch.row0;
  const double* __restrict__ hb = p.has + ch.row0;
  const int32_t* __restrict__ sb = p.sub + ch.row0;
  r.valid = 0;
  const uint32_t m = P.live[(size_t)blockIdx.x * 256 + threadIdx.x];
  r.live = m & 0xFFu;
  r.expl = (m >> 8) & 0xFFu;
  r.rel = (m >> 16) & 0xFFu;
  // every load issued before any is consumed (lanes past the chunk re-read its last
  // row, see group_segment): loads inside a per-lane branch made the compiler wait
  // for each row-block before issuing the next, eight memory latencies per chunk
  const int n = ch.nrows;
  int sr[kLR];
  // wants / has first, subclients after: with_sub comes from the resource's config
  // (ProportionalShare), which need not have arrived for the first loads to leave
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    const int i = k * 256 + threadIdx.x;
    const unsigned u = (unsigned)(i < n ? i : n - 1);
    r.w[k] = *col_at(wb, u);
    r.h[k] = with_has ? *col_at(hb, u) : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    const int i = k * 256 + threadIdx.x;
    sr[k] = with_sub ? *col_at(sb, (unsigned)(i < n ? i : n - 1)) : 0;
  }
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    const bool v = k * 256 + (int)threadIdx.x < n;
    r.valid |= (v ? 1u : 0u) << k;
    r.s[k] = v ? sub_value(sr[k]) : 0;
    if (!v) {
      r.w[k] = 0.0;
      r.h[k] = 0.0;
    }
  }
}

__device__ __forceinline__ HetRes* het_of(const Partials& P, int lseg) {
  return reinterpret_cast<HetRes*>(P.het + (size_t)lseg * sizeof(HetRes));
}
constexpr uint32_t kHetEmpty = 0xFFFFFFFFu;  // never a subclient count (<= kSubMax)

__device__ __forceinline__ bool het_insert(uint32_t* set, int* n, uint32_t key) {  // true when new
  uint32_t slot = (key * 0x9E3779B1u >> 23) & (2 * kHetMaxS - 1);
  for (int probe = 0; probe < 2 * kHetMaxS; ++probe, slot = (slot + 1) & (2 * kHetMaxS - 1)) {
    uint32_t cur = set[slot];
    if (cur == key) return false;
    if (cur == kHetEmpty) {
      cur = atomicCAS(&set[slot], kHetEmpty, key);
      if (cur == kHetEmpty) {
        atomicAdd(n, 1);
        return true;
      }
      if (cur == key) return false;
    }
  }
  atomicAdd(n, kHetMaxS + 1);  // table full: overflow
  return false;
}

// the same on the resource's set in global memory (agent-scope atomics; the
// chunks of a resource insert concurrently)
__device__ __forceinline__ void het_insert_global(uint32_t* set, int32_t* n, uint32_t key) {
  uint32_t slot = (key * 0x9E3779B1u >> 23) & (2 * kHetMaxS - 1);
  for (int probe = 0; probe < 2 * kHetMaxS; ++probe, slot = (slot + 1) & (2 * kHetMaxS - 1)) {
    uint32_t cur = __hip_atomic_load((gu32*)(set + slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return;
    if (cur == kHetEmpty) {
      cur = atomicCAS(set + slot, kHetEmpty, key);
      if (cur == kHetEmpty) {
        atomicAdd(n, 1);
        return;
      }
      if (cur == key) return;
    }
  }
  atomicAdd(n, kHetMaxS + 1);  // table full: overflow
}

// pass A (k_large_a, when P.s_set): the chunk's distinct subclient counts of live
// rows into its resource's set -- one insert for a chunk whose live rows share one
// count, else the chunk's own LDS set first, one global insert per distinct count
__device__ void chunk_s_insert(const Partials& P, int lseg, const ChunkRows& rw, const AggA& a) {
  __shared__ uint32_t set[2 * kHetMaxS];
  __shared__ int n;
  const int t = threadIdx.x;
  uint32_t* gset = P.s_set + (size_t)lseg * 2 * kHetMaxS;
  int32_t* gn = P.s_n + lseg;
  if (a.smin > a.smax) return;  // no live rows
  if (a.smin == a.smax) {
    if (t == 0) het_insert_global(gset, gn, (uint32_t)a.smin);
    return;
  }
  for (int i = t; i < 2 * kHetMaxS; i += 256) set[i] = kHetEmpty;
  if (t == 0) n = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLR; ++k)
    if (rw.live >> k & 1) het_insert(set, &n, (uint32_t)rw.s[k]);
  __syncthreads();
  if (n > kHetMaxS) {
    if (t == 0) atomicAdd(gn, kHetMaxS + 1);
    return;
  }
  for (int i = t; i < 2 * kHetMaxS; i += 256)
    if (set[i] != kHetEmpty) het_insert_global(gset, gn, set[i]);
}

// A chunk's sums over its rows in registers, stated once for the chain (k_large_a/b/c), the
// speculative launch and the redo (k ascending in every thread: one order, the same bits).
// Pass A (Clean sums of the rows it releases, the live rows' count range, NaN wants) and
// round 1 with equalShare eq
__device__ __forceinline__ AggA chunk_a(const ChunkRows& rw) {
  AggA a = zeroA();
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    if (!(rw.valid >> k & 1)) continue;
    if (!(rw.live >> k & 1)) {
      a.cnt += rw.s[k];
      a.h += rw.h[k];
      a.w += rw.w[k];
    } else {
      a.smin = rw.s[k] < a.smin ? rw.s[k] : a.smin;
      a.smax = rw.s[k] > a.smax ? rw.s[k] : a.smax;
      a.nan |= __builtin_isnan(rw.w[k]) ? 1 : 0;
    }
  }
  return a;
}
__device__ __forceinline__ AggB chunk_b(const ChunkRows& rw, int kind, double eq) {
  AggB b{0.0, 0.0, 0};
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    if (!(rw.live >> k & 1)) continue;
    const double w = rw.w[k];
    const int sk = rw.s[k];
    if (kind == 2) {
      const double e = eq * (double)sk;  // algorithm.go:273
      if (w < e)
        b.x += e - w;
      else
        b.y += w - e;
    } else {
      const double d = (double)sk * eq;  // algorithm.go:160
      if (w < d)
        b.x += d - w;
      else if (w > d)
        b.i += sk;
    }
  }
  return b;
}
// round 2 at threshold Tu over the live rows, every one holding s0 (k_large_c)
__device__ __forceinline__ AggC chunk_c(const ChunkRows& rw, int s0, double eq, double Tu) {
  AggC x{0.0, 0};
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    if (!(rw.live >> k & 1)) continue;
    const double w = rw.w[k];
    if (!(w > (double)s0 * eq)) continue;
    if (w < Tu)
      x.ee += Tu - w;
    else if (w > Tu)
      x.sgt += s0;
  }
  return x;
}

__global__ __launch_bounds__(256) void k_large_a(DevParams p, const Chunk* __restrict__ chunks, Partials P) {
  __shared__ Lds<256> lds;
  const Chunk ch = chunks[blockIdx.x];
  const Res rs = load_res(p, ch.seg);
  ChunkRows rw;
  {
    const int uni = P.s_live ? __builtin_amdgcn_readfirstlane(P.uni[blockIdx.x]) : -1;
    const uint32_t prev_live = P.s_live ? P.live[(size_t)blockIdx.x * 256 + threadIdx.x] : 0u;
    load_chunk(p, ch, rw, rs, uni, prev_live);
  }
  AggA a = chunk_a(rw);
  if (p.recompute) {  // every row's sums
#pragma unroll
    for (int k = 0; k < kLR; ++k) {
      if (!(rw.valid >> k & 1)) continue;
      a.all.cnt += rw.s[k];
      a.all.h += rw.h[k];
      a.all.w += rw.w[k];
    }
  }
  P.live[(size_t)blockIdx.x * 256 + threadIdx.x] = rw.live | rw.expl << 8 | rw.rel << 16;
  // Speculative pass B (ProportionalShare / FairShare outside learning mode) with
  // equalShare from the store's running Count.  It is exactly pass B's result
  // whenever Clean releases no subclients of the resource (same eq, same live
  // rows, same per-chunk summation order); k_large_b checks that and recomputes
  // otherwise.  Saves pass B's row reads (12 B per lease) in the steady state.
  const bool spec = !p.recompute && !rs.learning && rs.kind >= 2;
  AggB b{0.0, 0.0, 0};
  if (spec) b = chunk_b(rw, rs.kind, rs.C / (double)rs.agg_count);
  {
    const AggR all_part = a.all;
    if (P.s_set)  // every thread reads the chunk's count range (chunk_s_insert)
      a = group_reduce<256>(a, OpA(), lds.a);
    else
      a = group_reduce_t0<256>(a, OpA(), lds.a);
    if (p.recompute) a.all = group_reduce_t0<256>(all_part, OpR(), lds.r);
    if (spec) b = group_reduce_t0<256>(b, OpB(), lds.b);
  }
  if (P.s_set && !rs.learning && rs.kind == 3) chunk_s_insert(P, ch.lseg, rw, a);  // heterogeneous FairShare
  if (threadIdx.x == 0) {
    const int c = blockIdx.x;
    if (a.cnt != 0) atomicOr(&seg_tot(P, ch.lseg)->rel, 1u);
    if (spec) {
      P.b_x[c] = b.x;
      P.b_y[c] = b.y;
      P.b_w[c] = b.i;
    }
    P.a_cnt[c] = a.cnt;
    P.a_cnt_all[c] = a.all.cnt;
    P.a_has_all[c] = a.all.h;
    P.a_wants_all[c] = a.all.w;
    P.a_has[c] = a.h;
    P.a_wants[c] = a.w;
    P.a_smin[c] = a.smin;
    P.a_smax[c] = a.smax;
    P.a_nan[c] = a.nan;
  }
}

__global__ __launch_bounds__(256) void k_large_b(DevParams p, const Chunk* __restrict__ chunks,
                                                 const LargeSeg* __restrict__ ls, Partials P) {
  __shared__ Lds<256> lds;
  // P.b_first: one workgroup per large resource, as its first chunk (pass A's
  // speculative round 1 is exact: the store holds no explicit-expiry rows, so Clean
  // releases none of the resource's live rows or all of them, and then round 1 sums
  // nothing either way)
  const int ci = P.b_first ? ls[blockIdx.x].chunk_begin : (int)blockIdx.x;
  const Chunk ch = chunks[ci];
  // most chunks leave here: their resource's round 1 is exact from pass A and they
  // are not its first chunk (no config load on that path)
  const LargeSeg L = ls[ch.lseg];
  const bool first = ci == L.chunk_begin;
  const bool spec_ok = P.b_first || (!p.recompute && seg_tot(P, ch.lseg)->rel == 0);  // pass A's partials are exact
  if (spec_ok && !first) return;
  bool ps;
  {  // only ProportionalShare / FairShare outside learning mode need this pass
    const ResCfg cf = p.cfg[ch.seg];
    if (cf.learning_end_ns > p.now || cf.kind < 2) return;
    ps = cf.kind == 2;
  }
  const SegState st = seg_state<256>(p, P, L, lds);
  if (threadIdx.x == 0 && first) seg_tot(P, ch.lseg)->a = st.a;
  const bool het = st.general && P.s_set;  // heterogeneous FairShare decided on the chain
  if ((st.general && !het) || st.rs.learning || st.rs.kind < 2) return;
  if (spec_ok) {  // the first chunk leaves the speculative round-1 totals (C and the map read them)
    const AggB b = seg_b<256>(P, L, lds);
    if (threadIdx.x == 0) seg_tot(P, ch.lseg)->b = b;
    return;
  }
  ChunkRows rw;
  load_chunk_w(p, P, ch, rw, ps || het);
  const double eq = st.rs.C / (double)st.cl.count;
  if (!ps && !het) {  // uniform FairShare: one count
#pragma unroll
    for (int k = 0; k < kLR; ++k) rw.s[k] = st.a.smin;
  }
  const AggB b = group_reduce_t0<256>(chunk_b(rw, st.rs.kind, eq), OpB(), lds.b);
  if (threadIdx.x == 0) {
    P.b_x[blockIdx.x] = b.x;
    P.b_y[blockIdx.x] = b.y;
    P.b_w[blockIdx.x] = b.i;
  }
}

__global__ __launch_bounds__(256) void k_large_c(DevParams p, const Chunk* __restrict__ chunks,
                                                 const LargeSeg* __restrict__ ls, Partials P) {
  __shared__ Lds<256> lds;
  const Chunk ch = chunks[blockIdx.x];
  {  // only FairShare outside learning mode has a round 2
    const ResCfg cf = p.cfg[ch.seg];
    if (cf.learning_end_ns > p.now || cf.kind != 3) return;
  }
  ChunkRows rw;
  load_chunk_w(p, P, ch, rw, false);  // rows in flight while the resource's partials are reduced
  const LargeSeg L = ls[ch.lseg];
  const SegState st = seg_state_of(p, L.seg, seg_tot(P, ch.lseg)->a);  // left by pass B
  if (st.general || st.rs.learning || st.rs.kind != 3) return;
  const bool spec_ok = !p.recompute && seg_tot(P, ch.lseg)->rel == 0;  // pass B's first chunk left b
  const AggB b = spec_ok ? seg_tot(P, ch.lseg)->b : seg_b<256>(P, L, lds);
  if (threadIdx.x == 0 && !spec_ok && (int)blockIdx.x == L.chunk_begin) seg_tot(P, ch.lseg)->b = b;
  const double eq = st.rs.C / (double)st.cl.count;
  const double s0 = (double)st.a.smin;  // uniform subclients here
  const double Tu = (b.x / (double)b.i) * s0 + eq * s0;
  const AggC c = group_reduce_t0<256>(chunk_c(rw, st.a.smin, eq, Tu), OpC(), lds.c);
  if (threadIdx.x == 0) {
    P.c_ee[blockIdx.x] = c.ee;
    P.c_sgt[blockIdx.x] = c.sgt;
  }
}

// The map of one chunk (store.go:153-167 Assign): decide and write every lease of its
// rows under the resource's totals; returns the chunk's sum of gets - has.  (k_large_map
// keeps its own copy of the loop: called, that kernel spilled 68 B per lane.)
__device__ __forceinline__ double map_chunk(const DevParams& p, const Chunk& ch, const ChunkRows& rw, const Res rs,
                                            const Clean cl, const AggB b, const FsU fu) {
  const double C = rs.C;
  const double eq = C / (double)cl.count;
  double delta = 0.0;
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    if (!(rw.valid >> k & 1)) continue;
    const unsigned u = (unsigned)(k * 256 + threadIdx.x);
    const double w = rw.w[k], h = rw.h[k];
    if (!(rw.live >> k & 1)) {  // released by Clean (the raw word for put_released: marked or not)
      put_released(p, ch.row0, u, (rw.rel >> k & 1) ? (int32_t)kSubReleased : 0);
      continue;
    }
    double g;
    if (rs.learning) {
      g = h;
    } else if (rs.kind == 0) {
      g = w;
    } else if (rs.kind == 1) {
      g = minF(C, w);
    } else if (rs.kind == 2) {
      const double epc = eq * (double)rw.s[k];
      const double unused = C - cl.sum_has + h;
      g = (cl.sum_wants <= C || w <= epc) ? minF(w, unused) : minF(epc + (w - epc) * (b.x / b.y), unused);
    } else {
      g = fs_uniform_row(w, h, C, cl.sum_has, fu);
    }
    // an explicit row becomes a follower (its subclients word without the flag)
    put_live(p, ch.row0, u, g, rs, (rw.expl >> k & 1) ? (p.sub[ch.row0 + u] | (int32_t)kSubExplicit) : 0);
    delta += g - h;
  }
  return delta;
}

__global__ __launch_bounds__(256) void k_large_map(DevParams p, const Chunk* __restrict__ chunks,
                                                   const LargeSeg* __restrict__ ls, Partials P, int32_t* glist,
                                                   int32_t* gcount) {
  __shared__ Lds<256> lds;
  const Chunk ch = chunks[blockIdx.x];
  bool ps, fs;
  {
    const ResCfg cf = p.cfg[ch.seg];
    const bool lrn = cf.learning_end_ns > p.now;
    ps = !lrn && cf.kind == 2;
    fs = !lrn && cf.kind == 3;
  }
  ChunkRows rw;
  load_chunk_w(p, P, ch, rw, ps, true);  // rows in flight while the resource's partials are reduced
  const LargeSeg L = ls[ch.lseg];
  // pass A totals: left by pass B for ProportionalShare / FairShare
  const SegState st =
      uniform((ps || fs) ? seg_state_of(p, L.seg, seg_tot(P, ch.lseg)->a) : seg_state<256>(p, P, L, lds));
  // Without the heterogeneous chain (P.s_set) the map also does k_large_fin's work: the
  // resource's last-arriving chunk sums the chunks' deltas and writes its record
  const bool finish = P.s_set == nullptr;
  if (st.general) {  // k_general decides it; its first chunk lists it (fin's job)
    if (threadIdx.x == 0) P.uni[blockIdx.x] = -1;
    if (finish && threadIdx.x == 0 && (int)blockIdx.x == L.chunk_begin) {
      glist[atomicAdd(gcount, 1)] = L.seg;
      seg_tot(P, ch.lseg)->rel = 0;
    }
    return;
  }
  const Res& rs = st.rs;
  const double C = rs.C;
  const double eq = C / (double)st.cl.count;
  AggB b{0.0, 0.0, 0};
  AggC c{0.0, 0};
  if (ps) b = (!p.recompute && seg_tot(P, ch.lseg)->rel == 0) ? seg_tot(P, ch.lseg)->b : seg_b<256>(P, L, lds);
  if (fs) {
    b = seg_tot(P, ch.lseg)->b;  // left by pass C
    c = seg_c<256>(P, L, lds);
  }
  b = uniform(b);  // the resource's totals stay in SGPRs through the map
  const FsU fu = uniform(make_fsu(eq, st.a.smin, b.x, b.i, c));  // SGPRs through the map
  SumD delta{0.0};
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    if (!(rw.valid >> k & 1)) continue;
    const unsigned u = (unsigned)(k * 256 + threadIdx.x);
    const double w = rw.w[k], h = rw.h[k];
    if (!(rw.live >> k & 1)) {  // released by Clean (the raw word for put_released: marked or not)
      put_released(p, ch.row0, u, (rw.rel >> k & 1) ? (int32_t)kSubReleased : 0);
      continue;
    }
    double g;
    if (rs.learning) {
      g = h;
    } else if (rs.kind == 0) {
      g = w;
    } else if (rs.kind == 1) {
      g = minF(C, w);
    } else if (rs.kind == 2) {
      const double epc = eq * (double)rw.s[k];
      const double unused = C - st.cl.sum_has + h;
      g = (st.cl.sum_wants <= C || w <= epc) ? minF(w, unused) : minF(epc + (w - epc) * (b.x / b.y), unused);
    } else {
      g = fs_uniform_row(w, h, C, st.cl.sum_has, fu);
    }
    // an explicit row becomes a follower (its subclients word without the flag)
    put_live(p, ch.row0, u, g, rs, (rw.expl >> k & 1) ? (p.sub[ch.row0 + u] | (int32_t)kSubExplicit) : 0);
    delta.v += g - h;
  }
  delta = group_reduce_t0<256>(delta, OpSumD(), lds.d);
  if (threadIdx.x == 0)  // after a writeback tick every row this left live holds it (Partials::s_live)
    P.uni[blockIdx.x] = st.a.smin == st.a.smax ? st.a.smin : -1;
  if (!finish) {
    if (threadIdx.x == 0) P.d_delta[blockIdx.x] = delta.v;
    return;
  }
  if (threadIdx.x >= 64) return;  // wave 0 hands off (dm_kernel_util.h: write-through, then arrive)
  if (threadIdx.x == 0) st_wt(P.d_delta + blockIdx.x, delta.v);
  SegTot* tt = seg_tot(P, ch.lseg);
  if (!arrive_last(&tt->pad[0], L.chunk_end - L.chunk_begin)) return;
  SumD d{0.0};
  for (int q = L.chunk_begin + (int)threadIdx.x; q < L.chunk_end; q += 64) d.v += ld_wt(P.d_delta + q);
  d = wave_reduce(d, OpSumD());
  if (threadIdx.x == 0) {
    tt->rel = 0;  // pass A of the next tick sets it again (every chunk has read it)
    write_resource(p, L.seg, rs, st.cl, d.v);
  }
}

// --------------------------------------------------------------------------
// The speculative chain (the steady state of P.b_first ticks, DM_SPEC_CHAIN).
// k_large_spec: one launch over every chunk.  Each chunk computes its exact pass-A
// partials and its round-1 partials (equalShare from the running Count, as pass A's
// speculative round 1), its round-2 partials at the threshold the resource's stored
// totals give (SpecTot: its last tick's), and writes its leases under those stored
// totals -- unless its own rows show a lapse, a NaN wants or another count, when it
// writes nothing.  The resource's last-arriving chunk (no waiting) reduces the
// partials with one fixed tree and compares them bit for bit with the stored totals:
// equal, the leases written are exactly the chain's (the same totals, the same rows)
// and it writes the resource's record; else it marks the resource for
// k_large_redo.  Per lease: wants and has read, gets written -- one pass instead of
// the chain's four launches and second read.
// k_large_redo_team: one launch, every workgroup leaves at once when nothing is
// marked.  A marked resource's chunks are shared by a team of at most kTeamMax
// workgroups that meet twice at most (round 1 again when Clean released rows, round
// 2), through write-through partials, the last arriver's write-through total and a
// ready flag (the launch number); they then rewrite their leases and the last arriver
// stores the totals as the next tick's speculation.  Only a team waits for itself, so
// any grid of >= kTeamMax co-resident workgroups finishes; a wait is still bounded
// (kSpecSpin polls: the host then reports DM_E_INTERNAL and refuses the store until it
// is reloaded).
// --------------------------------------------------------------------------
constexpr uint32_t kSpecSpin = 1u << 22;  // polls of ~0.1 us

__device__ __forceinline__ bool dbl_pos0(double x) { return __double_as_longlong(x) == 0; }

// wave 0's fixed reduction over a resource's chunk partials (lane l: chunks begin + l,
// begin + l + 64, ... in order, then the wave's DPP tree); every lane gets the total
template <typename T, typename Op, typename Ld>
__device__ __forceinline__ T canon_reduce(int begin, int end, T v, Op op, Ld ld) {
  for (int q = begin + (int)(threadIdx.x & 63); q < end; q += 64) v = op(v, ld(q));
  return wave_reduce(v, op);
}
__device__ __forceinline__ AggB canon_b(const Partials& P, const LargeSeg& L) {
  return canon_reduce(L.chunk_begin, L.chunk_end, AggB{0.0, 0.0, 0}, OpB(),
                      [&](int q) { return AggB{ld_wt(P.b_x + q), ld_wt(P.b_y + q), ld_wt(P.b_w + q)}; });
}
__device__ __forceinline__ AggC canon_c(const Partials& P, const LargeSeg& L) {
  return canon_reduce(L.chunk_begin, L.chunk_end, AggC{0.0, 0}, OpC(),
                      [&](int q) { return AggC{ld_wt(P.c_ee + q), ld_wt(P.c_sgt + q)}; });
}
__device__ __forceinline__ double canon_d(const Partials& P, const LargeSeg& L) {
  return canon_reduce(L.chunk_begin, L.chunk_end, SumD{0.0}, OpSumD(),
                      [&](int q) { return SumD{ld_wt(P.d_delta + q)}; }).v;
}
// pass A's totals, canon_b, canon_c and canon_d in one pass over the chunks (k_large_spec's
// verifier): every partial of a 64-chunk stripe loaded at once, one round trip per
// stripe instead of four; each quantity keeps its own order and tree (the same bits)
struct CanonAll {
  AggA a;
  AggB b;
  AggC c;
  double d;
};
__device__ __forceinline__ CanonAll canon_all(const Partials& P, const LargeSeg& L) {
  AggA a = zeroA();
  AggB b{0.0, 0.0, 0};
  AggC c{0.0, 0};
  SumD d{0.0};
  for (int q = L.chunk_begin + (int)(threadIdx.x & 63); q < L.chunk_end; q += 64) {
    AggA x = zeroA();
    x.cnt = ld_wt(P.a_cnt + q);
    x.h = ld_wt(P.a_has + q);
    x.w = ld_wt(P.a_wants + q);
    x.smin = (int)ld_wt(P.a_smin + q);
    x.smax = (int)ld_wt(P.a_smax + q);
    x.nan = ld_wt(P.a_nan + q);
    const AggB y{ld_wt(P.b_x + q), ld_wt(P.b_y + q), ld_wt(P.b_w + q)};
    const AggC z{ld_wt(P.c_ee + q), ld_wt(P.c_sgt + q)};
    const SumD u{ld_wt(P.d_delta + q)};
    a = OpA()(a, x);
    b = OpB()(b, y);
    c = OpC()(c, z);
    d = OpSumD()(d, u);
  }
  return CanonAll{wave_reduce(a, OpA()), wave_reduce(b, OpB()), wave_reduce(c, OpC()), wave_reduce(d, OpSumD()).v};
}

// (at 5 waves per SIMD -- amdgpu_waves_per_eu(5): 96 VGPRs, 2 spilled -- C2 lost 105.2 ->
// 108.7 us, both orders, round 6: the chain's workgroups are latency-bound per phase,
// and the spill sits on the map's path)
__global__ __launch_bounds__(256) void k_large_spec(DevParams p, const Chunk* __restrict__ chunks,
                                                    const LargeSeg* __restrict__ ls, Partials P, SpecArgs S) {
  __shared__ Lds<256> lds;
  __shared__ int s_ok;
  const int c = blockIdx.x;
  const int t = threadIdx.x;
  const Chunk ch = chunks[c];
  const Res rs = load_res(p, ch.seg);
  SpecTot* sp = S.tot + ch.lseg;
  ChunkRows rw;
  {
    const int uni = P.s_live ? __builtin_amdgcn_readfirstlane(P.uni[c]) : -1;
    const uint32_t prev_live = P.s_live ? P.live[(size_t)c * 256 + t] : 0u;
    load_chunk<true>(p, ch, rw, rs, uni, prev_live);
  }
  const int valid = sp->valid, s0 = sp->s0;  // the stored totals (written by earlier launches)
  const AggB bs{sp->bx, sp->by, sp->bi};
  const AggC cs{sp->cee, sp->csgt};
  AggA a = chunk_a(rw);
  P.live[(size_t)c * 256 + t] = rw.live | rw.expl << 8 | rw.rel << 16;
  const bool r1 = !rs.learning && rs.kind >= 2;
  const bool fs = !rs.learning && rs.kind == 3;
  const double eq = rs.C / (double)rs.agg_count;  // the running Count: exact when Clean releases nothing
  AggB b = r1 ? chunk_b(rw, rs.kind, eq) : AggB{0.0, 0.0, 0};
  a = group_reduce_t0<256>(a, OpA(), lds.a);
  if (r1) b = group_reduce_t0<256>(b, OpB(), lds.b);
  if (t == 0)  // this chunk's rows agree with the speculation: nothing released, one count s0, no NaN
    s_ok = (valid && a.cnt == 0 && dbl_pos0(a.h) && dbl_pos0(a.w) && !a.nan &&
            (a.smin > a.smax || (a.smin == s0 && a.smax == s0)))
               ? 1
               : 0;
  __syncthreads();
  const bool ok = s_ok != 0;
  AggC x{0.0, 0};
  SumD delta{0.0};
  if (ok) {
    AggA z = zeroA();
    z.smin = z.smax = s0;
    const Clean cl = clean_from(p, rs, z);  // the running sums: the Clean of a tick that releases nothing
    const FsU fu = uniform(make_fsu(eq, s0, bs.x, bs.i, cs));
    if (fs) x = group_reduce_t0<256>(chunk_c(rw, s0, eq, fu.T), OpC(), lds.c);
    delta.v = map_chunk(p, ch, rw, rs, cl, uniform(bs), fu);
    delta = group_reduce_t0<256>(delta, OpSumD(), lds.d);
  }
  if (t == 0) {
    st_wt(P.a_cnt + c, (int64_t)a.cnt);
    st_wt(P.a_has + c, a.h);
    st_wt(P.a_wants + c, a.w);
    st_wt(P.a_smin + c, (int64_t)a.smin);
    st_wt(P.a_smax + c, (int64_t)a.smax);
    st_wt(P.a_nan + c, a.nan);
    st_wt(P.b_x + c, b.x);
    st_wt(P.b_y + c, b.y);
    st_wt(P.b_w + c, (int64_t)b.i);
    st_wt(P.c_ee + c, x.ee);
    st_wt(P.c_sgt + c, (int64_t)x.sgt);
    st_wt(P.d_delta + c, delta.v);
    P.uni[c] = ok ? s0 : -1;  // the redo rewrites a marked resource's
    if (!ok) __hip_atomic_store((gu32*)&sp->redo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (t >= 64) return;  // wave 0 verifies (dm_kernel_util.h arrive_last)
  const LargeSeg L = ls[ch.lseg];
  if (!arrive_last(&sp->arrive[0], L.chunk_end - L.chunk_begin)) return;
  const CanonAll ca = canon_all(P, L);
  const AggA at = ca.a;
  const AggB bt = ca.b;
  const AggC ct = ca.c;
  const bool marked = __hip_atomic_load((gu32*)&sp->redo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  bool same = valid && !marked && at.cnt == 0 && dbl_pos0(at.h) && dbl_pos0(at.w) && !at.nan &&
              (at.smin > at.smax || (at.smin == s0 && at.smax == s0));
  if (rs.kind == 2 && !rs.learning)
    same = same && __double_as_longlong(bt.x) == __double_as_longlong(bs.x) &&
           __double_as_longlong(bt.y) == __double_as_longlong(bs.y);
  if (fs)
    same = same && __double_as_longlong(bt.x) == __double_as_longlong(bs.x) && bt.i == bs.i &&
           __double_as_longlong(ct.ee) == __double_as_longlong(cs.ee) && ct.sgt == cs.sgt;
  if (same) {
    const double d = ca.d;
    if (t == 0) {
      AggA z = zeroA();
      z.smin = z.smax = s0;
      write_resource(p, L.seg, rs, clean_from(p, rs, z), d);
    }
    return;
  }
  if (t == 0) {  // the redo's inputs: the actual pass-A totals and round 1 at the running Count
    sp->redo = 1;
    S.ring[S.par] = 1;  // (read by the next launch)
    sp->a_cnt = at.cnt;
    sp->a_h = at.h;
    sp->a_w = at.w;
    sp->a_smin = at.smin;
    sp->a_smax = at.smax;
    sp->a_nan = at.nan;
    sp->abx = bt.x;
    sp->aby = bt.y;
    sp->abi = bt.i;
  }
}

// every thread's write-through stores have landed, then one arrival; true (uniform)
// for the last arriver, which resets the counter
__device__ __forceinline__ bool spec_arrive(uint32_t* ctr, int nch, int* s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add((gu32*)ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == (uint32_t)nch - 1 ? 1 : 0;
    if (last) __hip_atomic_store((gu32*)ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = last;
  }
  __syncthreads();
  return *s_last != 0;
}
__device__ __forceinline__ void spec_ready(const SpecArgs& S, uint64_t* flag) {  // the last arriver's stores landed
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st_wt(flag, S.seq + 1);
  }
}
__device__ __forceinline__ void spec_wait(const SpecArgs& S, const uint64_t* flag) {
  if (threadIdx.x == 0) {
    for (uint32_t it = 0; ld_wt(flag) < S.seq + 1; ++it) {
      if (it >= kSpecSpin) {
        __hip_atomic_store(S.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
  }
  __syncthreads();
}

// The redo by teams: a marked resource's chunks are shared among W = min(chunks,
// kTeamMax) workgroups (its team slots, in ticket order), each taking every W-th chunk
// through each phase, its rows loaded again per phase.  Every chunk partial is one
// 256-thread reduction and every total one canonical tree (canon_*), so the bits are
// those the chain would write; only a team waits for itself, so any grid of >= kTeamMax
// co-resident workgroups finishes (no bound on a resource's chunks).  (Round 4's
// per-chunk redo, one workgroup per chunk with every chunk of a resource co-resident,
// was retired in round 5.)
// Two builds of the same code: the full one and a light one held to 64 VGPRs (8 waves;
// a chunk's rows spill to scratch).  A steady tick marks nothing, and there the launch
// is all the redo costs: the light build's workgroups find a free slot beside the
// other classes' waves much sooner (C2: 20 -> 10 us of event time, the tick -3.6 us),
// while a redo of every large resource takes it about 2x as long.  The host launches
// the light build while the last redo it saw found nothing marked and no row changed
// since (dm_tick.cpp); both leave the same bits.
__device__ __forceinline__ void redo_team(const DevParams& p, const Chunk* __restrict__ chunks,
                                          const LargeSeg* __restrict__ ls, const Partials& P, const SpecArgs& S,
                                          int32_t* glist, int32_t* gcount, int l, int m, Lds<256>& lds,
                                          int* s_last_p) {
  int& s_last = *s_last_p;
  const int t = threadIdx.x;
  SpecTot* sp = S.tot + l;
  const LargeSeg L = ls[l];
  const int nch = L.chunk_end - L.chunk_begin;
  const int W = nch < kTeamMax ? nch : kTeamMax;
  AggA at = zeroA();
  at.cnt = sp->a_cnt;
  at.h = sp->a_h;
  at.w = sp->a_w;
  at.smin = sp->a_smin;
  at.smax = sp->a_smax;
  at.nan = sp->a_nan;
  const SegState st = uniform(seg_state_of(p, L.seg, at));
  const Res rs = st.rs;
  if (st.general) {  // k_general decides it (its member 0 lists it)
    for (int c = L.chunk_begin + m; c < L.chunk_end; c += W)
      if (t == 0) P.uni[c] = -1;
    if (t == 0 && m == 0) {
      glist[atomicAdd(gcount, 1)] = L.seg;
      sp->redo = 0;
      sp->valid = 0;
    }
    return;
  }
  const bool r1 = !rs.learning && rs.kind >= 2;
  const bool fs = !rs.learning && rs.kind == 3;
  const double eq = rs.C / (double)st.cl.count;
  AggB bt{sp->abx, sp->aby, sp->abi};  // round 1 at the running Count: exact when Clean released nothing
  if (r1 && at.cnt != 0) {  // round 1 again at the Count after Clean
    for (int c = L.chunk_begin + m; c < L.chunk_end; c += W) {
      ChunkRows rw;
      load_chunk<true>(p, chunks[c], rw, rs);
      const AggB x = group_reduce_t0<256>(chunk_b(rw, rs.kind, eq), OpB(), lds.b);
      if (t == 0) {
        st_wt(P.b_x + c, x.x);
        st_wt(P.b_y + c, x.y);
        st_wt(P.b_w + c, (int64_t)x.i);
      }
      __syncthreads();
    }
    if (spec_arrive(&sp->arrive[1], W, &s_last)) {
      if (t < 64) {
        const AggB r = canon_b(P, L);
        if (t == 0) {
          st_wt(&sp->abx, r.x);
          st_wt(&sp->aby, r.y);
          st_wt(reinterpret_cast<int64_t*>(&sp->abi), (int64_t)r.i);
        }
      }
      spec_ready(S, &sp->ready[0]);
    }
    spec_wait(S, &sp->ready[0]);
    bt = AggB{ld_wt(&sp->abx), ld_wt(&sp->aby), ld_wt(reinterpret_cast<const int64_t*>(&sp->abi))};
  }
  const int s0 = st.a.smin;
  AggC ct{0.0, 0};
  FsU fu = make_fsu(eq, s0, bt.x, bt.i, ct);
  if (fs) {  // round 2 at the resource's threshold
    for (int c = L.chunk_begin + m; c < L.chunk_end; c += W) {
      ChunkRows rw;
      load_chunk<true>(p, chunks[c], rw, rs);
      const AggC x = group_reduce_t0<256>(chunk_c(rw, s0, eq, fu.T), OpC(), lds.c);
      if (t == 0) {
        st_wt(P.c_ee + c, x.ee);
        st_wt(P.c_sgt + c, (int64_t)x.sgt);
      }
      __syncthreads();
    }
    if (spec_arrive(&sp->arrive[2], W, &s_last)) {
      if (t < 64) {
        const AggC r = canon_c(P, L);
        if (t == 0) {
          st_wt(&sp->cee, r.ee);
          st_wt(reinterpret_cast<int64_t*>(&sp->csgt), (int64_t)r.sgt);
        }
      }
      spec_ready(S, &sp->ready[1]);
    }
    spec_wait(S, &sp->ready[1]);
    ct = AggC{ld_wt(&sp->cee), ld_wt(reinterpret_cast<const int64_t*>(&sp->csgt))};
    fu = make_fsu(eq, s0, bt.x, bt.i, ct);
  }
  for (int c = L.chunk_begin + m; c < L.chunk_end; c += W) {
    ChunkRows rw;
    const Chunk ch = chunks[c];
    load_chunk<true>(p, ch, rw, rs);
    SumD delta{map_chunk(p, ch, rw, rs, st.cl, uniform(bt), uniform(fu))};
    delta = group_reduce_t0<256>(delta, OpSumD(), lds.d);
    if (t == 0) {
      P.uni[c] = st.a.smin == st.a.smax ? st.a.smin : -1;
      st_wt(P.d_delta + c, delta.v);
    }
    __syncthreads();
  }
  if (!spec_arrive(&sp->arrive[0], W, &s_last)) return;
  if (t >= 64) return;
  const double d = canon_d(P, L);
  if (t == 0) {
    write_resource(p, L.seg, rs, st.cl, d);
    // the next tick's speculation: this tick's totals (round 1 and 2 as the chunks used
    // them; a resource whose live rows hold mixed counts is not speculated on)
    sp->bx = bt.x;
    sp->by = bt.y;
    sp->bi = bt.i;
    sp->cee = ct.ee;
    sp->csgt = ct.sgt;
    sp->s0 = s0;
    sp->valid = (st.a.smin >= st.a.smax) ? 1 : 0;  // one count, or no live row
    sp->redo = 0;
  }
}

// Team slots in ticket order (a resource's slots consecutive): with a grid of >=
// kTeamMax workgroups only the team at the ticket front can have members not yet taken
template <bool kLight>
__global__ __launch_bounds__(256, kLight ? 8 : 1) void k_large_redo_team(DevParams p, const Chunk* __restrict__ chunks,
                                                                          const LargeSeg* __restrict__ ls, Partials P,
                                                                          SpecArgs S, int32_t* glist, int32_t* gcount) {
  __shared__ Lds<256> lds;
  __shared__ int s_last, s_c;
  const int q = S.par ^ 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the next tick's slots (its k_large_spec runs after this)
    S.ring[q] = 0;
    S.ring[2 + q] = 0;
    // tell the host only that a redo ran (it clears the word when it reads it): a
    // system-scope store to host memory keeps an otherwise empty launch alive ~2 us
    // longer, and the steady tick's empty redo is on the large chain's critical path
    const uint32_t marked = S.ring[S.par];
    if (marked) __hip_atomic_store(S.seen, marked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (!S.ring[S.par]) return;  // nothing marked (k_large_spec: the previous launch)
  for (;;) {
    if (threadIdx.x == 0) s_c = (int)atomicAdd(S.ring + 2 + S.par, 1u);
    __syncthreads();
    const int k = s_c;
    if (k >= S.nslots) return;
    const int32_t tm = S.team[k];
    const int l = tm >> 8, m = tm & 0xFF;
    if (S.tot[l].redo) redo_team(p, chunks, ls, P, S, glist, gcount, l, m, lds, &s_last);
    __syncthreads();  // every wave back before the next ticket
  }
}

__global__ __launch_bounds__(256) void k_large_fin(DevParams p, const LargeSeg* __restrict__ ls, Partials P,
                                                   int32_t* general_list, int32_t* general_count) {
  __shared__ Lds<256> lds;
  const LargeSeg L = ls[blockIdx.x];
  if (threadIdx.x == 0) seg_tot(P, blockIdx.x)->rel = 0;  // pass A of the next tick sets it again
  const SegState st = seg_state<256>(p, P, L, lds);
  if (st.general) {
    if (!P.s_set) {  // no heterogeneous path on the chain this tick: k_general decides it
      if (threadIdx.x == 0) general_list[atomicAdd(general_count, 1)] = L.seg;
      return;
    }
    if (het_of(P, blockIdx.x)->mode != 1) return;  // k_large_t handed it to k_general
  }
  SumD d{0.0};
  for (int c = L.chunk_begin + (int)threadIdx.x; c < L.chunk_end; c += 256) d.v += P.d_delta[c];
  d = group_reduce<256>(d, OpSumD(), lds.d);
  if (threadIdx.x == 0) write_resource(p, L.seg, st.rs, st.cl, d.v);
}

// --------------------------------------------------------------------------
// Heterogeneous-subclient FairShare of large resources on the chain (instead of
// one workgroup per resource in k_general): launched only when the store may hold
// such resources.  After pass B (round 1 with each row's own count):
//   k_large_t      per resource: round-1 totals, the distinct subclient counts of
//                  the live rows (from pass A's per-chunk lists) and their round-2
//                  thresholds T(s) = (E / W) s + eq s -- a row reaching round 2 has
//                  w > deservedShare, so its wantExtra is W and its threshold
//                  depends on its count only (algorithm.go:148,175,197) -- sorted;
//   k_large_c_het  per chunk: (count, sum wants, sum subclients) of the wantExtra
//                  clients per bucket between / at the thresholds (as k_general);
//   k_large_e      per resource: the chunks' buckets in chunk order, prefix sums:
//                  extraExtra(T) = k T - sum(w < T), wantExtraExtra(T) = sum(s : w > T);
//   k_large_map_het per chunk: every row decided (fs_stage01 / fs_stage2).
// More than kHetMaxS counts or a non-finite threshold: k_general (HetRes.mode 2).
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_large_t(DevParams p, const LargeSeg* __restrict__ ls, Partials P,
                                                 int32_t* general_list, int32_t* general_count) {
  __shared__ Lds<256> lds;
  __shared__ uint32_t set[2 * kHetMaxS];
  __shared__ double T[kHetMaxS];
  __shared__ int n, fill;
  const int t = threadIdx.x;
  const LargeSeg L = ls[blockIdx.x];
  SegTot* tot = seg_tot(P, blockIdx.x);
  HetRes* H = het_of(P, blockIdx.x);
  uint32_t* gset = P.s_set + (size_t)blockIdx.x * 2 * kHetMaxS;
  // the resource's distinct counts (pass A), and the set emptied for the next tick
  for (int i = t; i < 2 * kHetMaxS; i += 256) {
    set[i] = gset[i];
    gset[i] = kHetEmpty;
  }
  if (t == 0) {
    n = P.s_n[blockIdx.x];
    P.s_n[blockIdx.x] = 0;
    fill = 0;
  }
  __syncthreads();
  const SegState st = seg_state_of(p, L.seg, tot->a);  // left by pass B's first chunk
  if (!st.general) {
    if (t == 0) H->mode = 0;
    return;
  }
  const AggB b = seg_b<256>(P, L, lds);  // round 1 with every row's own count: E = b.x, W = b.i
  if (t == 0) tot->b = b;
  const int K0 = n;
  // NaN wants: such a row's threshold has W + s in its wantExtra (its w > deservedShare
  // is false), not one of T(s) below -- k_general collects the rows' own thresholds
  bool bad = K0 > kHetMaxS || st.a.nan;
  if (!bad) {
    for (int i = t; i < 2 * kHetMaxS; i += 256)
      if (set[i] != kHetEmpty) {
        const double s = (double)set[i];
        const double eq = st.rs.C / (double)st.cl.count;  // as fs_stage01's arguments
        const double ds = eq * s;                          // :126
        const double dE = (b.x / (double)b.i) * s;         // :175 (wantExtra = W for a round-2 row)
        T[atomicAdd(&fill, 1)] = dE + ds;                  // :197
      }
    __syncthreads();
    if (t >= K0) T[t] = __builtin_inf();
    int nonfinite = 0;
    if (t < K0 && !__builtin_isfinite(T[t])) nonfinite = 1;
    bad = __syncthreads_or(nonfinite) != 0;
  }
  if (bad) {  // k_general decides the resource (per-threshold passes)
    if (t == 0) {
      H->mode = 2;
      general_list[atomicAdd(general_count, 1)] = L.seg;
    }
    return;
  }
  for (int k = 2; k <= kHetMaxS; k <<= 1)  // ascending bitonic sort of the thresholds
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const int q = t ^ j;
      if (q > t) {
        const double x = T[t], y = T[q];
        if ((x > y) == ((t & k) == 0)) {
          T[t] = y;
          T[q] = x;
        }
      }
    }
  __syncthreads();
  if (t == 0) {  // distinct values only (counts may share a threshold)
    int K = 0;
    for (int i = 0; i < K0; ++i)
      if (K == 0 || T[i] != H->T[K - 1]) H->T[K++] = T[i];
    H->K = K;
    H->mode = 1;
  }
}

// One 64-row tile of a wave into its bucket accumulators (k_general's method:
// sort the lanes by bucket, segmented scan, one writer per bucket; fixed order).
__device__ __forceinline__ void het_tile(const double* T, int K, double w, long long s, bool in, double* accw,
                                         long long* accs, int* accc) {
  const int lane = threadIdx.x & 63;
  const uint32_t bk = in ? (uint32_t)gen_bucket(T, K, w) : 0xFFFFu;
  const uint32_t key = wave_sort64(bk << 6 | (uint32_t)lane);
  const int src = (int)(key & 63);
  const int mb = (int)(key >> 6);
  double vw = shfl_d(in ? w : 0.0, src);
  long long vs = __shfl(in ? s : 0ll, src, 64);
  int vc = mb != 0xFFFF ? 1 : 0;
  const int prevb = __shfl_up(mb, 1, 64);
  int run = (lane == 0 || prevb != mb) ? 1 : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double ow = shfl_d(vw, lane >= off ? lane - off : lane);
    const long long os = __shfl(vs, lane >= off ? lane - off : lane, 64);
    const int oc = __shfl(vc, lane >= off ? lane - off : lane, 64);
    const int orun = __shfl(run, lane >= off ? lane - off : lane, 64);
    if (lane >= off && !run) {
      vw = ow + vw;
      vs = os + vs;
      vc = oc + vc;
      run = orun;
    }
  }
  const int nextb = __shfl_down(mb, 1, 64);
  if (mb != 0xFFFF && (lane == 63 || nextb != mb)) {
    accw[mb] += vw;
    accs[mb] += vs;
    accc[mb] += vc;
  }
}

__global__ __launch_bounds__(256) void k_large_c_het(DevParams p, const Chunk* __restrict__ chunks,
                                                     const LargeSeg* __restrict__ ls, Partials P) {
  __shared__ double T[kHetMaxS];
  __shared__ double accw[4][kHetBuckets];
  __shared__ long long accs[4][kHetBuckets];
  __shared__ int accc[4][kHetBuckets];
  const int t = threadIdx.x, wv = t >> 6;
  const Chunk ch = chunks[blockIdx.x];
  const HetRes* H = het_of(P, ch.lseg);
  if (H->mode != 1) return;
  ChunkRows rw;
  load_chunk_w(p, P, ch, rw, true);
  const SegState st = seg_state_of(p, ch.seg, seg_tot(P, ch.lseg)->a);
  const double eq = st.rs.C / (double)st.cl.count;
  const int K = H->K;
  for (int i = t; i < K; i += 256) T[i] = H->T[i];
  for (int i = t; i < 4 * kHetBuckets; i += 256) {
    (&accw[0][0])[i] = 0.0;
    (&accs[0][0])[i] = 0;
    (&accc[0][0])[i] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLR; ++k) {  // row k*256 + t: tile 4k + wv, in order per wave
    const double w = rw.w[k];
    const long long s = rw.s[k];
    const bool in = (rw.live >> k & 1) && w > (double)s * eq;  // wantExtraClients (:165-169)
    het_tile(T, K, w, s, in, accw[wv], accs[wv], accc[wv]);
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * kHetBuckets;
  for (int bb = t; bb < 2 * K + 1; bb += 256) {  // the waves combined in a fixed order
    P.bk_w[base + bb] = ((accw[0][bb] + accw[1][bb]) + accw[2][bb]) + accw[3][bb];
    P.bk_s[base + bb] = accs[0][bb] + accs[1][bb] + accs[2][bb] + accs[3][bb];
    P.bk_c[base + bb] = accc[0][bb] + accc[1][bb] + accc[2][bb] + accc[3][bb];
  }
}

// one wave per (resource, bucket): the bucket's chunk partials, lanes striding the
// chunks, combined by the fixed DPP tree of wave_reduce
__global__ __launch_bounds__(256) void k_large_e(DevParams p, const LargeSeg* __restrict__ ls, Partials P) {
  const int lane = threadIdx.x & 63;
  const LargeSeg L = ls[blockIdx.x];
  HetRes* H = het_of(P, blockIdx.x);
  if (H->mode != 1) return;
  const int bb = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (bb >= 2 * H->K + 1) return;  // whole waves
  AggR v{0, 0.0, 0.0};  // cnt: clients, h: subclients (exact below 2^53), w: wants
  for (int q = L.chunk_begin + lane; q < L.chunk_end; q += 64) {
    const size_t i = (size_t)q * kHetBuckets + bb;
    v.w += P.bk_w[i];
    v.h += (double)P.bk_s[i];
    v.cnt += P.bk_c[i];
  }
  v = wave_reduce(v, OpR());
  if (lane == 0) {
    H->bw[bb] = v.w;
    H->bs[bb] = (int64_t)v.h;
    H->bc[bb] = v.cnt;
  }
}

__global__ __launch_bounds__(256) void k_large_map_het(DevParams p, const Chunk* __restrict__ chunks,
                                                       const LargeSeg* __restrict__ ls, Partials P) {
  __shared__ Lds<256> lds;
  __shared__ double T[kHetMaxS], ee[kHetMaxS];
  __shared__ long long sgt[kHetMaxS];
  const int t = threadIdx.x;
  const Chunk ch = chunks[blockIdx.x];
  const HetRes* H = het_of(P, ch.lseg);
  if (H->mode != 1) return;
  ChunkRows rw;
  load_chunk_w(p, P, ch, rw, true, true);
  const SegTot* tot = seg_tot(P, ch.lseg);
  const SegState st = seg_state_of(p, ch.seg, tot->a);
  const AggB b = tot->b;
  const double C = st.rs.C;
  const double eq = C / (double)st.cl.count;
  const int K = H->K;
  __shared__ double bw[kHetBuckets];
  __shared__ long long bs[kHetBuckets], bc[kHetBuckets];
  for (int i = t; i < K; i += 256) T[i] = H->T[i];
  for (int i = t; i < 2 * K + 1; i += 256) {
    bw[i] = H->bw[i];
    bs[i] = H->bs[i];
    bc[i] = H->bc[i];
  }
  __syncthreads();
  if (t == 0) {  // prefix over the buckets (as k_general): every chunk the same, in LDS
    long long stot = 0;
    for (int bb = 0; bb < 2 * K + 1; ++bb) stot += bs[bb];
    long long cnt = 0, sle = 0;
    double sw = 0.0;
    for (int k = 0; k < K; ++k) {
      const int bl = 2 * k;  // below T_k; bl + 1: w == T_k
      cnt += bc[bl];
      sw = sw + bw[bl];
      sle += bs[bl];
      const long long seq = bs[bl + 1];
      ee[k] = cnt == 0 ? 0.0 : (double)cnt * T[k] - sw;  // :197-198
      sgt[k] = stot - sle - seq;                          // :199-200
      sle += seq;
      cnt += bc[bl + 1];
      sw = sw + bw[bl + 1];
    }
  }
  __syncthreads();
  SumD delta{0.0};
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    if (!(rw.valid >> k & 1)) continue;
    const unsigned u = (unsigned)(k * 256 + t);
    const double w = rw.w[k], h = rw.h[k];
    if (!(rw.live >> k & 1)) {
      put_released<kSpecNT>(p, ch.row0, u, (rw.rel >> k & 1) ? (int32_t)kSubReleased : 0);
      continue;
    }
    const long long s = rw.s[k];
    double g, Tr = 0.0;
    if (!fs_stage01(w, h, s, C, st.cl.sum_has, eq, b.x, b.i, &g, &Tr)) {
      AggC c{0.0, 0};
      if (!__builtin_isnan(Tr)) {
        const int q = gen_index(T, K, Tr);
        c = AggC{ee[q], sgt[q]};
      }
      g = fs_stage2(w, h, s, C, st.cl.sum_has, eq, b.x, b.i, Tr, c);
    }
    put_live<kSpecNT>(p, ch.row0, u, g, st.rs, (rw.expl >> k & 1) ? (p.sub[ch.row0 + u] | (int32_t)kSubExplicit) : 0);
    delta.v += g - h;
  }
  delta = group_reduce<256>(delta, OpSumD(), lds.d);
  if (t == 0) P.d_delta[blockIdx.x] = delta.v;
}

// --------------------------------------------------------------------------
// host-side launchers (called by dm_tick.cpp)
// --------------------------------------------------------------------------
hipError_t launch_large(LargePhase ph, dim3 grid, const DevParams& p, const LargeArgs& a, hipStream_t st) {
  if (grid.x == 0 || grid.y == 0) return hipSuccess;
  const Chunk* chunks = a.chunks;
  const LargeSeg* ls = a.ls;
  switch (ph) {
    case LargePhase::A: k_large_a<<<grid, 256, 0, st>>>(p, chunks, a.P); break;
    case LargePhase::B: k_large_b<<<grid, 256, 0, st>>>(p, chunks, ls, a.P); break;
    case LargePhase::T: k_large_t<<<grid, 256, 0, st>>>(p, ls, a.P, a.glist, a.gcount); break;
    case LargePhase::C: k_large_c<<<grid, 256, 0, st>>>(p, chunks, ls, a.P); break;
    case LargePhase::C_HET: k_large_c_het<<<grid, 256, 0, st>>>(p, chunks, ls, a.P); break;
    case LargePhase::E: k_large_e<<<grid, 256, 0, st>>>(p, ls, a.P); break;
    case LargePhase::MAP: k_large_map<<<grid, 256, 0, st>>>(p, chunks, ls, a.P, a.glist, a.gcount); break;
    case LargePhase::MAP_HET: k_large_map_het<<<grid, 256, 0, st>>>(p, chunks, ls, a.P); break;
    case LargePhase::FIN: k_large_fin<<<grid, 256, 0, st>>>(p, ls, a.P, a.glist, a.gcount); break;
    case LargePhase::SPEC: k_large_spec<<<grid, 256, 0, st>>>(p, chunks, ls, a.P, a.S); break;
    case LargePhase::REDO_FULL:
      k_large_redo_team<false><<<grid, 256, 0, st>>>(p, chunks, ls, a.P, a.S, a.glist, a.gcount);
      break;
    case LargePhase::REDO_LIGHT:
      k_large_redo_team<true><<<grid, 256, 0, st>>>(p, chunks, ls, a.P, a.S, a.glist, a.gcount);
      break;
  }
  return hipGetLastError();
}

// Workgroups of the redo's full build that one CU holds at once (the full build's grid:
// up to 3/4 of what the GPU holds, dm_create in dm_runtime.cpp).
int redo_blocks_per_cu() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_large_redo_team<false>, 256, 0) != hipSuccess) return 1;
  return n > 0 ? n : 1;
}

}  // namespace dm

// k_general is compiled as part of this unit, not as one of its own: alone in a unit
// its code comes out different (146 VGPRs for 144, other LDS addressing) from the same
// source: the optimizer's choices follow the unit's other kernels (any one chain kernel
// beside it is not enough, the chain is).  The file compiles on its own too; making it a
// unit is a change to measure first (profiles/split_isa.md).
#include "dm_tick_general.hip"
