// dm_tick_large_spec.h — the speculative form of the large-resource chain (the steady state of
// P.b_first ticks, DM_SPEC_CHAIN): k_large_spec and k_large_redo_team.  The chunk steps they
// share with the four-launch chain: dm_tick_large.h.
#pragma once
#include "dm_tick_large.h"

namespace dm {

// --------------------------------------------------------------------------
// The speculative chain.
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
__device__ __forceinline__ bool same_bits(double x, double y) {
  return __double_as_longlong(x) == __double_as_longlong(y);
}

// SpecTot's totals as the aggregates they hold (dm_device.h; its layout is the host's too).  The
// speculation: the last verified (or redone) tick's rounds 1 and 2.  WT: a team's hand-off.
__device__ __forceinline__ AggB spec_b(const SpecTot* sp) { return AggB{sp->bx, sp->by, sp->bi}; }
__device__ __forceinline__ void set_spec_b(SpecTot* sp, const AggB& b) {
  sp->bx = b.x;
  sp->by = b.y;
  sp->bi = b.i;
}
template <bool WT = false>
__device__ __forceinline__ AggC spec_c(const SpecTot* sp) { return AggC{ld_word<WT>(&sp->cee), ld_word<WT>(&sp->csgt)}; }
template <bool WT = false>
__device__ __forceinline__ void set_spec_c(SpecTot* sp, const AggC& c) {
  st_word<WT>(&sp->cee, c.ee);
  st_word<WT>(&sp->csgt, c.sgt);
}
// the redo's inputs: the resource's actual pass-A totals and round 1 at the running Count
__device__ __forceinline__ AggA redo_a(const SpecTot* sp) {
  AggA a = zeroA();
  a.cnt = sp->a_cnt;
  a.h = sp->a_h;
  a.w = sp->a_w;
  a.smin = sp->a_smin;
  a.smax = sp->a_smax;
  a.nan = sp->a_nan;
  return a;
}
__device__ __forceinline__ void set_redo_a(SpecTot* sp, const AggA& a) {
  sp->a_cnt = a.cnt;
  sp->a_h = a.h;
  sp->a_w = a.w;
  sp->a_smin = a.smin;
  sp->a_smax = a.smax;
  sp->a_nan = a.nan;
}
template <bool WT = false>
__device__ __forceinline__ AggB redo_b(const SpecTot* sp) {
  return AggB{ld_word<WT>(&sp->abx), ld_word<WT>(&sp->aby), ld_word<WT>(&sp->abi)};
}
template <bool WT = false>
__device__ __forceinline__ void set_redo_b(SpecTot* sp, const AggB& b) {
  st_word<WT>(&sp->abx, b.x);
  st_word<WT>(&sp->aby, b.y);
  st_word<WT>(&sp->abi, b.i);
}

// Rows (a chunk's, or all of the resource's) agree with the speculation, given that it is
// usable: nothing released, one count s0 (or no live row), no NaN wants
__device__ __forceinline__ bool spec_agrees(bool usable, const AggA& a, int s0) {
  return usable && a.cnt == 0 && dbl_pos0(a.h) && dbl_pos0(a.w) && !a.nan &&
         (a.smin > a.smax || (a.smin == s0 && a.smax == s0));
}
// the Clean of a tick that releases nothing: the running sums, every live row holding s0
__device__ __forceinline__ Clean clean_none(const DevParams& p, const Res& rs, int s0) {
  AggA z = zeroA();
  z.smin = z.smax = s0;
  return clean_from(p, rs, z);
}

// The map of one chunk under the resource's totals (its live rows hold one count); returns the
// thread's sum of gets - has
__device__ __forceinline__ double map_chunk(const DevParams& p, const Chunk& ch, const ChunkRows& rw, const Res rs,
                                            const Clean cl, const AggB b, const FsU fu) {
  const double eq = rs.C / (double)cl.count;
  double delta = 0.0;
#pragma unroll
  for (int k = 0; k < kLR; ++k)
    map_row(p, ch, rw, rs, k, delta,
            [&](int i) { return grant_uniform(rs, cl, eq, b, fu, rw.w[i], rw.h[i], rw.s[i]); });
  return delta;
}

// wave 0's fixed reduction over a resource's chunk partials (lane l: chunks begin + l,
// begin + l + 64, ... in order, then the wave's DPP tree); every lane gets the total
template <typename T, typename Op, typename Ld>
__device__ __forceinline__ T canon_reduce(int begin, int end, T v, Op op, Ld ld) {
  for (int q = begin + (int)(threadIdx.x & 63); q < end; q += 64) v = op(v, ld(q));
  return wave_reduce(v, op);
}
__device__ __forceinline__ AggB canon_b(const Partials& P, const LargeSeg& L) {
  return canon_reduce(L.chunk_begin, L.chunk_end, AggB{0.0, 0.0, 0}, OpB(), [&](int q) { return load_b<true>(P, q); });
}
__device__ __forceinline__ AggC canon_c(const Partials& P, const LargeSeg& L) {
  return canon_reduce(L.chunk_begin, L.chunk_end, AggC{0.0, 0}, OpC(), [&](int q) { return load_c<true>(P, q); });
}
__device__ __forceinline__ double canon_d(const Partials& P, const LargeSeg& L) {
  return canon_reduce(L.chunk_begin, L.chunk_end, SumD{0.0}, OpSumD(),
                      [&](int q) { return SumD{load_d<true>(P, q)}; }).v;
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
    const AggA x = load_a<true, false>(P, q);
    const AggB y = load_b<true>(P, q);
    const AggC z = load_c<true>(P, q);
    const SumD u{load_d<true>(P, q)};
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
  load_chunk<true>(p, ch, rw, rs, prev_uni(P, c), prev_live(P, c));
  const int valid = sp->valid, s0 = sp->s0;  // the stored totals (written by earlier launches)
  const AggB bs = spec_b(sp);
  const AggC cs = spec_c(sp);
  AggA a = chunk_a(rw);
  store_live(P, c, rw);
  const bool r1 = !rs.learning && rs.kind >= 2;
  const bool fs = !rs.learning && rs.kind == 3;
  const double eq = rs.C / (double)rs.agg_count;  // the running Count: exact when Clean releases nothing
  AggB b = r1 ? chunk_b(rw, rs.kind, eq) : AggB{0.0, 0.0, 0};
  a = group_reduce_t0<256>(a, OpA(), lds.a);
  if (r1) b = group_reduce_t0<256>(b, OpB(), lds.b);
  if (t == 0) s_ok = spec_agrees(valid, a, s0) ? 1 : 0;  // this chunk's rows
  __syncthreads();
  const bool ok = s_ok != 0;
  AggC x{0.0, 0};
  SumD delta{0.0};
  if (ok) {
    const Clean cl = clean_none(p, rs, s0);
    const FsU fu = uniform(make_fsu(eq, s0, bs.x, bs.i, cs));
    if (fs) x = group_reduce_t0<256>(chunk_c(rw, s0, eq, fu.T), OpC(), lds.c);
    delta.v = map_chunk(p, ch, rw, rs, cl, uniform(bs), fu);
    delta = group_reduce_t0<256>(delta, OpSumD(), lds.d);
  }
  if (t == 0) {
    store_a<true, false>(P, c, a);
    store_b<true>(P, c, b);
    store_c<true>(P, c, x);
    store_d<true>(P, c, delta.v);
    P.uni[c] = ok ? s0 : -1;  // the redo rewrites a marked resource's
    if (!ok) __hip_atomic_store((gu32*)&sp->redo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (t >= 64) return;  // wave 0 verifies (dm_kernel_util.h arrive_last)
  const LargeSeg L = ls[ch.lseg];
  if (!arrive_last(&sp->arrive[0], L.chunk_end - L.chunk_begin)) return;
  const CanonAll ca = canon_all(P, L);
  const AggB bt = ca.b;
  const AggC ct = ca.c;
  const bool marked = __hip_atomic_load((gu32*)&sp->redo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  bool same = spec_agrees(valid && !marked, ca.a, s0);  // the resource's rows, and the totals they give
  if (rs.kind == 2 && !rs.learning) same = same && same_bits(bt.x, bs.x) && same_bits(bt.y, bs.y);
  if (fs) same = same && same_bits(bt.x, bs.x) && bt.i == bs.i && same_bits(ct.ee, cs.ee) && ct.sgt == cs.sgt;
  if (same) {
    if (t == 0) write_resource(p, L.seg, rs, clean_none(p, rs, s0), ca.d);
    return;
  }
  if (t == 0) {  // the redo's inputs
    sp->redo = 1;
    S.ring[S.par] = 1;  // (read by the next launch)
    set_redo_a(sp, ca.a);
    set_redo_b(sp, bt);
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
// One meeting of a team (member m of W) over resource L: part(c) takes each of the member's
// chunks to its write-through partial, the members arrive, the last arriver's wave 0 runs
// total() (the canonical tree over the partials, stored write-through) and raises the round's
// ready flag, and every member waits for it; the caller then reloads the total.
template <typename Part, typename Total>
__device__ __forceinline__ void team_round(const SpecArgs& S, SpecTot* sp, const LargeSeg& L, int m, int W,
                                           int round, int* s_last, Part part, Total total) {
  for (int c = L.chunk_begin + m; c < L.chunk_end; c += W) {
    part(c);
    __syncthreads();
  }
  if (spec_arrive(&sp->arrive[round], W, s_last)) {
    if (threadIdx.x < 64) total();
    spec_ready(S, &sp->ready[round - 1]);
  }
  spec_wait(S, &sp->ready[round - 1]);
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
  const AggA at = redo_a(sp);
  const SegState st = uniform(seg_state_of(p, L.seg, at));
  const Res rs = st.rs;
  if (st.general) {  // k_general decides it (its member 0 lists it)
    for (int c = L.chunk_begin + m; c < L.chunk_end; c += W)
      if (t == 0) P.uni[c] = -1;
    if (t == 0 && m == 0) {
      list_general(glist, gcount, L.seg);
      sp->redo = 0;
      sp->valid = 0;
    }
    return;
  }
  const bool r1 = !rs.learning && rs.kind >= 2;
  const bool fs = !rs.learning && rs.kind == 3;
  const double eq = rs.C / (double)st.cl.count;
  AggB bt = redo_b(sp);  // round 1 at the running Count: exact when Clean released nothing
  if (r1 && at.cnt != 0) {  // round 1 again at the Count after Clean
    team_round(S, sp, L, m, W, 1, &s_last,
               [&](int c) {
                 ChunkRows rw;
                 load_chunk<true>(p, chunks[c], rw, rs);
                 const AggB x = group_reduce_t0<256>(chunk_b(rw, rs.kind, eq), OpB(), lds.b);
                 if (t == 0) store_b<true>(P, c, x);
               },
               [&] { const AggB r = canon_b(P, L); if (t == 0) set_redo_b<true>(sp, r); });
    bt = redo_b<true>(sp);
  }
  const int s0 = st.a.smin;
  AggC ct{0.0, 0};
  FsU fu = make_fsu(eq, s0, bt.x, bt.i, ct);
  if (fs) {  // round 2 at the resource's threshold
    team_round(S, sp, L, m, W, 2, &s_last,
               [&](int c) {
                 ChunkRows rw;
                 load_chunk<true>(p, chunks[c], rw, rs);
                 const AggC x = group_reduce_t0<256>(chunk_c(rw, s0, eq, fu.T), OpC(), lds.c);
                 if (t == 0) store_c<true>(P, c, x);
               },
               [&] { const AggC r = canon_c(P, L); if (t == 0) set_spec_c<true>(sp, r); });
    ct = spec_c<true>(sp);
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
      store_d<true>(P, c, delta.v);
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
    set_spec_b(sp, bt);
    set_spec_c(sp, ct);
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

}  // namespace dm
