// dm_tick_large.hip — the large-resource chain of a tick: the four-launch chain
// k_large_a/b/c/map/fin here, what every form shares in dm_tick_large.h, its speculative form
// (k_large_spec, k_large_redo_team) in dm_tick_large_spec.h and its heterogeneous-subclient
// form (k_large_t, k_large_c_het, k_large_e, k_large_map_het) in dm_tick_large_het.h: one
// translation unit.  The algorithms' mapping and the float semantics: dm_tick_group.hip.
#include "dm_tick_large.h"
#include "dm_tick_large_het.h"
#include "dm_tick_large_spec.h"

namespace dm {

__global__ __launch_bounds__(256) void k_large_a(DevParams p, const Chunk* __restrict__ chunks, Partials P) {
  __shared__ Lds<256> lds;
  const Chunk ch = chunks[blockIdx.x];
  const Res rs = load_res(p, ch.seg);
  ChunkRows rw;
  load_chunk(p, ch, rw, rs, prev_uni(P, blockIdx.x), prev_live(P, blockIdx.x));
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
  store_live(P, blockIdx.x, rw);
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
    if (spec) store_b<false>(P, c, b);
    store_a<false, true>(P, c, a);
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
  const KindNow kn = kind_now(p, ch.seg);
  if (kn.learning || kn.kind < 2) return;  // only ProportionalShare / FairShare outside learning mode need this pass
  const bool ps = kn.kind == 2;
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
  if (threadIdx.x == 0) store_b<false>(P, blockIdx.x, b);
}

__global__ __launch_bounds__(256) void k_large_c(DevParams p, const Chunk* __restrict__ chunks,
                                                 const LargeSeg* __restrict__ ls, Partials P) {
  __shared__ Lds<256> lds;
  const Chunk ch = chunks[blockIdx.x];
  {  // only FairShare outside learning mode has a round 2
    const KindNow kn = kind_now(p, ch.seg);
    if (kn.learning || kn.kind != 3) return;
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
  if (threadIdx.x == 0) store_c<false>(P, blockIdx.x, c);
}

__global__ __launch_bounds__(256) void k_large_map(DevParams p, const Chunk* __restrict__ chunks,
                                                   const LargeSeg* __restrict__ ls, Partials P, int32_t* glist,
                                                   int32_t* gcount) {
  __shared__ Lds<256> lds;
  const Chunk ch = chunks[blockIdx.x];
  const KindNow kn = kind_now(p, ch.seg);
  const bool ps = !kn.learning && kn.kind == 2, fs = !kn.learning && kn.kind == 3;
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
      list_general(glist, gcount, L.seg);
      seg_tot(P, ch.lseg)->rel = 0;
    }
    return;
  }
  const Res& rs = st.rs;
  const double eq = rs.C / (double)st.cl.count;
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
  for (int k = 0; k < kLR; ++k)
    map_row(p, ch, rw, rs, k, delta.v,
            [&](int i) { return grant_uniform(rs, st.cl, eq, b, fu, rw.w[i], rw.h[i], rw.s[i]); });
  delta = group_reduce_t0<256>(delta, OpSumD(), lds.d);
  if (threadIdx.x == 0)  // after a writeback tick every row this left live holds it (Partials::s_live)
    P.uni[blockIdx.x] = st.a.smin == st.a.smax ? st.a.smin : -1;
  if (!finish) {
    if (threadIdx.x == 0) store_d<false>(P, blockIdx.x, delta.v);
    return;
  }
  if (threadIdx.x >= 64) return;  // wave 0 hands off (dm_kernel_util.h: write-through, then arrive)
  if (threadIdx.x == 0) store_d<true>(P, blockIdx.x, delta.v);
  SegTot* tt = seg_tot(P, ch.lseg);
  if (!arrive_last(&tt->pad[0], L.chunk_end - L.chunk_begin)) return;
  SumD d{0.0};
  for (int q = L.chunk_begin + (int)threadIdx.x; q < L.chunk_end; q += 64) d.v += load_d<true>(P, q);
  d = wave_reduce(d, OpSumD());
  if (threadIdx.x == 0) {
    tt->rel = 0;  // pass A of the next tick sets it again (every chunk has read it)
    write_resource(p, L.seg, rs, st.cl, d.v);
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
      if (threadIdx.x == 0) list_general(general_list, general_count, L.seg);
      return;
    }
    if (het_of(P, blockIdx.x)->mode != 1) return;  // k_large_t handed it to k_general
  }
  SumD d{0.0};
  for (int c = L.chunk_begin + (int)threadIdx.x; c < L.chunk_end; c += 256) d.v += load_d<false>(P, c);
  d = group_reduce<256>(d, OpSumD(), lds.d);
  if (threadIdx.x == 0) write_resource(p, L.seg, st.rs, st.cl, d.v);
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
