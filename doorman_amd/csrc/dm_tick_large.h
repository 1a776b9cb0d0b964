// dm_tick_large.h — what every form of the large-resource chain shares (dm_tick_large.hip: the
// four-launch chain; dm_tick_large_spec.h: the speculative form; dm_tick_large_het.h: the
// heterogeneous-subclient form): a resource's totals record, the chunk partials' words and the
// reductions over them, a chunk's rows and its sums, the map's row.  Each step is stated once and
// called by every form: the chain's "the same order, the same bits" rests on that.
#pragma once
#include <hip/hip_runtime.h>

#include "dm_kernel_util.h"
#include "dm_launch.h"
#include "dm_threshold_util.h"

namespace dm {

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

// the resource's kind and whether it is in learning mode, from its config alone: a pass that
// only some kinds outside learning mode need leaves on this before any row is loaded
struct KindNow {
  bool learning;
  int kind;
};
__device__ __forceinline__ KindNow kind_now(const DevParams& p, int seg) {
  const ResCfg cf = p.cfg[seg];
  return KindNow{cf.learning_end_ns > p.now, (int)cf.kind};
}
// list the resource for k_general, which decides it after the chain
__device__ __forceinline__ void list_general(int32_t* list, int32_t* count, int seg) { list[atomicAdd(count, 1)] = seg; }

// The chunk partials' words (Partials, dm_device.h): one store and one load per partial.  WT:
// write-through (dm_kernel_util.h: the hand-off between workgroups of one launch), plain where the
// next launch reads.  The index keeps the caller's type (an int index costs a sign extension).
template <bool WT, typename T>
__device__ __forceinline__ void st_word(T* a, T v) {
  if (WT) st_wt(a, v);
  else *a = v;
}
template <bool WT, typename T>
__device__ __forceinline__ T ld_word(const T* a) { return WT ? ld_wt(a) : *a; }
// ALL: with the sums over every row (recompute mode; the four-launch chain alone carries them)
template <bool WT, bool ALL, typename I>
__device__ __forceinline__ void store_a(const Partials& P, I c, const AggA& a) {
  st_word<WT>(P.a_cnt + c, (int64_t)a.cnt);
  if constexpr (ALL) {
    st_word<WT>(P.a_cnt_all + c, (int64_t)a.all.cnt);
    st_word<WT>(P.a_has_all + c, a.all.h);
    st_word<WT>(P.a_wants_all + c, a.all.w);
  }
  st_word<WT>(P.a_has + c, a.h);
  st_word<WT>(P.a_wants + c, a.w);
  st_word<WT>(P.a_smin + c, (int64_t)a.smin);
  st_word<WT>(P.a_smax + c, (int64_t)a.smax);
  st_word<WT>(P.a_nan + c, (int32_t)a.nan);
}
template <bool WT, bool ALL, typename I>
__device__ __forceinline__ AggA load_a(const Partials& P, I c) {
  AggA x = zeroA();
  x.cnt = ld_word<WT>(P.a_cnt + c);
  x.h = ld_word<WT>(P.a_has + c);
  x.w = ld_word<WT>(P.a_wants + c);
  if constexpr (ALL)
    x.all = AggR{ld_word<WT>(P.a_cnt_all + c), ld_word<WT>(P.a_has_all + c), ld_word<WT>(P.a_wants_all + c)};
  x.smin = (int)ld_word<WT>(P.a_smin + c);
  x.smax = (int)ld_word<WT>(P.a_smax + c);
  x.nan = ld_word<WT>(P.a_nan + c);
  return x;
}
template <bool WT, typename I>
__device__ __forceinline__ void store_b(const Partials& P, I c, const AggB b) {  // (b, x by value: k_large_a keeps its text)
  st_word<WT>(P.b_x + c, b.x);
  st_word<WT>(P.b_y + c, b.y);
  st_word<WT>(P.b_w + c, (int64_t)b.i);
}
template <bool WT, typename I>
__device__ __forceinline__ AggB load_b(const Partials& P, I c) {
  return AggB{ld_word<WT>(P.b_x + c), ld_word<WT>(P.b_y + c), ld_word<WT>(P.b_w + c)};
}
template <bool WT, typename I>
__device__ __forceinline__ void store_c(const Partials& P, I c, const AggC x) {
  st_word<WT>(P.c_ee + c, x.ee);
  st_word<WT>(P.c_sgt + c, (int64_t)x.sgt);
}
template <bool WT, typename I>
__device__ __forceinline__ AggC load_c(const Partials& P, I c) {
  return AggC{ld_word<WT>(P.c_ee + c), ld_word<WT>(P.c_sgt + c)};
}
template <bool WT, typename I>
__device__ __forceinline__ void store_d(const Partials& P, I c, double delta) { st_word<WT>(P.d_delta + c, delta); }
template <bool WT, typename I>
__device__ __forceinline__ double load_d(const Partials& P, I c) { return ld_word<WT>(P.d_delta + c); }

template <int G>
__device__ __forceinline__ SegState seg_state(const DevParams& p, const Partials& P, const LargeSeg& L,
                                              Lds<G>& lds) {
  AggA a = zeroA();
  for (int c = L.chunk_begin + (int)threadIdx.x; c < L.chunk_end; c += G) {
    const AggA x = load_a<false, true>(P, c);
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
  for (int c = L.chunk_begin + (int)threadIdx.x; c < L.chunk_end; c += G) b = OpB()(b, load_b<false>(P, c));
  return group_reduce<G>(b, OpB(), lds.b);
}

template <int G>
__device__ __forceinline__ AggC seg_c(const Partials& P, const LargeSeg& L, Lds<G>& lds) {
  AggC c{0.0, 0};
  for (int q = L.chunk_begin + (int)threadIdx.x; q < L.chunk_end; q += G) c = OpC()(c, load_c<false>(P, q));
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
// lanes past the chunk re-read its last row (see group_segment)
__device__ __forceinline__ unsigned row_clamp(int i, int n) { return (unsigned)(i < n ? i : n - 1); }

// the live word pass A leaves per thread of chunk c (Partials::live): its rows' live, explicit
// and released bits
template <typename I>
__device__ __forceinline__ void store_live(const Partials& P, I c, const ChunkRows& r) {
  P.live[(size_t)c * 256 + threadIdx.x] = r.live | r.expl << 8 | r.rel << 16;
}
template <typename I>
__device__ __forceinline__ void load_live(const Partials& P, I c, ChunkRows& r) {
  const uint32_t m = P.live[(size_t)c * 256 + threadIdx.x];
  r.live = m & 0xFFu;
  r.expl = (m >> 8) & 0xFFu;
  r.rel = (m >> 16) & 0xFFu;
}

// What the last writeback tick through the chain left of chunk c (Partials::s_live): the count
// every row it left live holds (-1: none, or no such tick) and this thread's live word; pass A
// proper (k_large_a, k_large_spec) hands both to load_chunk
template <typename I>
__device__ __forceinline__ int prev_uni(const Partials& P, I c) {
  return P.s_live ? __builtin_amdgcn_readfirstlane(P.uni[c]) : -1;
}
template <typename I>
__device__ __forceinline__ uint32_t prev_live(const Partials& P, I c) {
  return P.s_live ? P.live[(size_t)c * 256 + threadIdx.x] : 0u;
}
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
    r.w[k] = wb[row_clamp(i, ch.nrows)];
    r.h[k] = ALLH ? hb[row_clamp(i, ch.nrows)] : 0.0;
  }
  if (uni >= 0) {
#pragma unroll
    for (int k = 0; k < kLR; ++k) sr[k] = (prev_live >> k & 1) ? uni : (int32_t)kSubReleased;
  } else {
#pragma unroll
    for (int k = 0; k < kLR; ++k) {
      const int i = k * 256 + threadIdx.x;
      sr[k] = sb[row_clamp(i, ch.nrows)];
    }
  }
  int64_t e[kLR];
#pragma unroll
  for (int k = 0; k < kLR; ++k) e[k] = rs.follow_exp;
  if (any_explicit(rs)) {  // the resource's flag (see group_segment)
#pragma unroll
    for (int k = 0; k < kLR; ++k) {
      const int i = k * 256 + threadIdx.x;
      const int64_t x = eb[row_clamp(i, ch.nrows)];
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
  load_live(P, blockIdx.x, r);
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
    const unsigned u = row_clamp(i, n);
    r.w[k] = *col_at(wb, u);
    r.h[k] = with_has ? *col_at(hb, u) : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kLR; ++k) {
    const int i = k * 256 + threadIdx.x;
    sr[k] = with_sub ? *col_at(sb, row_clamp(i, n)) : 0;
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

// The map (store.go:153-167 Assign), per row: a row Clean released is written released, a live
// row gets grant(k) and becomes a follower; delta gathers the thread's sum of gets - has.  Every
// map of the chain is a loop over k of this row (the gets stores are non-temporal: put_live's
// default, see kGroupNT in dm_tick_group.h).  The loop stays with the caller: inside this
// function it moved every map's code (k_large_map's text grew by 6%, k_large_spec's by 16%).
template <typename Grant>
__device__ __forceinline__ void map_row(const DevParams& p, const Chunk& ch, const ChunkRows& rw, const Res& rs,
                                        int k, double& delta, Grant grant) {
  if (!(rw.valid >> k & 1)) return;
  const unsigned u = (unsigned)(k * 256 + threadIdx.x);
  if (!(rw.live >> k & 1)) {  // released by Clean (the raw word for put_released: marked or not)
    put_released(p, ch.row0, u, (rw.rel >> k & 1) ? (int32_t)kSubReleased : 0);
    return;
  }
  const double g = grant(k);
  // an explicit row becomes a follower (its subclients word without the flag)
  put_live(p, ch.row0, u, g, rs, (rw.expl >> k & 1) ? (p.sub[ch.row0 + u] | (int32_t)kSubExplicit) : 0);
  delta += g - rw.h[k];
}
// the grant of a row under a resource's totals when its live rows hold one count (or the kind
// does not look at counts): learning mode, kinds 0 to 2, uniform FairShare
__device__ __forceinline__ double grant_uniform(const Res& rs, const Clean& cl, double eq, const AggB& b,
                                                const FsU& fu, double w, double h, int s) {
  const double C = rs.C;
  if (rs.learning) return h;
  if (rs.kind == 0) return w;
  if (rs.kind == 1) return minF(C, w);
  if (rs.kind == 2) {
    const double epc = eq * (double)s;
    const double unused = C - cl.sum_has + h;
    return (cl.sum_wants <= C || w <= epc) ? minF(w, unused) : minF(epc + (w - epc) * (b.x / b.y), unused);
  }
  return fs_uniform_row(w, h, C, cl.sum_has, fu);
}

}  // namespace dm
