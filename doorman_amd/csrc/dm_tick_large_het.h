// dm_tick_large_het.h — the heterogeneous-subclient form of the large-resource chain: pass A's
// set of distinct counts (chunk_s_insert, called by k_large_a) and k_large_t, k_large_c_het,
// k_large_e, k_large_map_het.  The chunk steps they share with the four-launch chain:
// dm_tick_large.h.
#pragma once
#include "dm_tick_large.h"

namespace dm {

__device__ __forceinline__ HetRes* het_of(const Partials& P, int lseg) {
  return reinterpret_cast<HetRes*>(P.het + (size_t)lseg * sizeof(HetRes));
}
constexpr uint32_t kHetEmpty = 0xFFFFFFFFu;  // never a subclient count (<= kSubMax)

// Insert a count into an open-addressing set of 2 * kHetMaxS slots, *n counting its keys (past
// kHetMaxS: overflow); true when the key is new.  GLOBAL: the resource's set in global memory
// (agent-scope atomics; the chunks of a resource insert concurrently), else a workgroup's in LDS
template <bool GLOBAL>
__device__ __forceinline__ bool het_insert(uint32_t* set, int32_t* n, uint32_t key) {
  uint32_t slot = (key * 0x9E3779B1u >> 23) & (2 * kHetMaxS - 1);
  for (int probe = 0; probe < 2 * kHetMaxS; ++probe, slot = (slot + 1) & (2 * kHetMaxS - 1)) {
    uint32_t cur;
    if constexpr (GLOBAL) cur = __hip_atomic_load((gu32*)(set + slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else cur = set[slot];
    if (cur == key) return false;
    if (cur == kHetEmpty) {
      cur = atomicCAS(set + slot, kHetEmpty, key);
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

// pass A (k_large_a, when P.s_set): the chunk's distinct subclient counts of live
// rows into its resource's set -- one insert for a chunk whose live rows share one
// count, else the chunk's own LDS set first, one global insert per distinct count
__device__ inline void chunk_s_insert(const Partials& P, int lseg, const ChunkRows& rw, const AggA& a) {
  __shared__ uint32_t set[2 * kHetMaxS];
  __shared__ int n;
  const int t = threadIdx.x;
  uint32_t* gset = P.s_set + (size_t)lseg * 2 * kHetMaxS;
  int32_t* gn = P.s_n + lseg;
  if (a.smin > a.smax) return;  // no live rows
  if (a.smin == a.smax) {
    if (t == 0) het_insert<true>(gset, gn, (uint32_t)a.smin);
    return;
  }
  for (int i = t; i < 2 * kHetMaxS; i += 256) set[i] = kHetEmpty;
  if (t == 0) n = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kLR; ++k)
    if (rw.live >> k & 1) het_insert<false>(set, &n, (uint32_t)rw.s[k]);
  __syncthreads();
  if (n > kHetMaxS) {
    if (t == 0) atomicAdd(gn, kHetMaxS + 1);
    return;
  }
  for (int i = t; i < 2 * kHetMaxS; i += 256)
    if (set[i] != kHetEmpty) het_insert<true>(gset, gn, set[i]);
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
      list_general(general_list, general_count, L.seg);
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
  for (int k = 0; k < kLR; ++k)
    map_row(p, ch, rw, st.rs, k, delta.v, [&](int i) {  // the row's own count and threshold
      const double w = rw.w[i], h = rw.h[i];
      const long long s = rw.s[i];
      double g, Tr = 0.0;
      if (!fs_stage01(w, h, s, C, st.cl.sum_has, eq, b.x, b.i, &g, &Tr)) {
        AggC c{0.0, 0};
        if (!__builtin_isnan(Tr)) {
          const int q = gen_index(T, K, Tr);
          c = AggC{ee[q], sgt[q]};
        }
        g = fs_stage2(w, h, s, C, st.cl.sum_has, eq, b.x, b.i, Tr, c);
      }
      return g;
    });
  delta = group_reduce<256>(delta, OpSumD(), lds.d);
  if (t == 0) store_d<false>(P, blockIdx.x, delta.v);
}

}  // namespace dm
