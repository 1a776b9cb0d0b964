// dm_tick_group.hip — gfx950 kernels for one apportionment tick: the resource-per-group
// kernels (workgroup bins, sub-wave groups, packed tiles).  The other work classes of a
// tick: dm_tick_large.hip (the large-resource chain), dm_tick_general.hip (k_general).
// group_segment, the body of the workgroup and sub-wave kernels, is in dm_tick_group.h; the
// split form's dense-side kernels are in dm_tick_steady.h (this unit: their unmasked builds).
//
// Every lease row is decided against the same frozen store (include/doorman_hip.h).
// Per resource the reference's per-request loops (go/server/doorman/algorithm.go)
// collapse to segmented reductions:
//   Clean          store.go:169-181   pass A: expired-row sums (parity) or live sums
//   ProportionalShare algorithm.go:213-293  pass B: extraCapacity / extraNeed, then map
//   FairShare      algorithm.go:95-206    pass B: extra / wantExtra (round 1),
//                                         pass C: extraExtra / wantExtraExtra at T (round 2), then map
//   NoAlgorithm / Static / Learn  algorithm.go:66-84,297-302  map only
// No MFMA: the arithmetic is binary64 compares, adds and a few divisions per row, and
// the segmented reductions.  Rows are read once from HBM into VGPRs and every pass runs
// from registers; the large-resource path re-reads from L2 / Infinity Cache.  Bytes set
// the floor (24-48 B per lease), but the dense tick that skips unchanged stores is bound
// by vector issue, not HBM: ~160 VALU instructions per row slot keep every SIMD's VALU
// busy for the kernel's whole duration (profiles/steady_pmc.md), hence the steady builds
// below, which leave out the pass whose result is known.
//
// Float semantics follow Go on amd64: binary64, no FMA contraction (built with
// -ffp-contract=off), minF = `l > r ? r : l`, IEEE division by zero.
#include "dm_tick_steady.h"

namespace dm {

// One G-thread workgroup per resource (G = 128..512, R = 4 or 8 rows per thread).
// 257-1024 rows run on 128 threads (2 waves) with 8 rows each, held to 5 waves per
// SIMD (<= 96 VGPRs): 5 x 4 SIMDs x 64 lanes x 8 rows = 10240 rows in flight per CU
// against 7168 for 256 threads x 4 rows at 7 waves per SIMD (65 VGPRs).  The tick is
// bound by bytes in flight: C3 560-590 -> 490-500 us, C1 61 -> 55 us
// (tools/ab.py, one box); 6 waves per SIMD spills (80 VGPRs + scratch: 2x slower).
// 1025-2048 / 2049-4096 rows likewise on 256 x 8 (5 waves) / 512 x 8 (106 VGPRs, 4
// waves) instead of 512 x 4 / 1024 x 4: C2's kernel time -5%, its tick -2%.
template <int G, int R>
__global__ __launch_bounds__(G, (G <= 256 && R == 8) ? 5 : 1) void k_block(DevParams p, WorkItem* __restrict__ items, int nitems,
                                             int32_t* general_list, int32_t* general_count) {
  __shared__ Lds<G> lds;
  if ((int)blockIdx.x >= nitems) return;
  group_segment<G, R>(p, items[blockIdx.x], items + blockIdx.x, threadIdx.x, lds, general_list, general_count);
}

// The split form's dense side -- k_block_dense, k_sweep, k_block_list -- is dm_tick_steady.h.
template <int G, int R>
__global__ __launch_bounds__(G) void k_block_rest(DevParams p, WorkItem* __restrict__ items,
                                                  const int32_t* __restrict__ queue, int32_t* qcnt, int par,
                                                  int32_t* host_count, int32_t* general_list, int32_t* general_count) {
  __shared__ Lds<G> lds;
  const int count = qcnt[par];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    qcnt[par ^ 1] = 0;
    if (host_count && qcnt[2] != count) {
      __hip_atomic_store(host_count, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      qcnt[2] = count;
    }
  }
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    const int idx = queue[q];
    group_segment<G, R, kRest>(p, items[idx], items + idx, threadIdx.x, lds, general_list, general_count);
    __syncthreads();  // the next item reuses the single-use LDS slots
  }
}

// One workgroup: how many items of a workgroup bin are not dense after a writeback
// tick, published to host-mapped memory as {count, epoch} (count first, the epoch
// with release order) -- the host's once-per-epoch check before it skips the bin's
// k_block_rest (dm_tick.cpp).  The count word's high half counts the dense items
// whose hint word carries released rows or arrivals (bits 8, 9): with both halves zero
// the host may launch the steady builds.  rec[2], stored before the epoch as the counts are:
// the items whose hint word carries an arrival bit (bit 9), which the host reads only under
// DM_KEEP_FREE_SLOTS (the items the masked builds still hand to the rest kernel).
__global__ __launch_bounds__(1024) void k_count_undense(const WorkItem* __restrict__ items, int n,
                                                        unsigned long long* rec, unsigned long long epoch) {
  __shared__ int part[16], part_f[16], part_a[16];
  int c = 0, f = 0, a = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int hw = items[i].n >> 16;
    c += hw == 0 ? 1 : 0;
    f += (hw >> 8 & 3) != 0 ? 1 : 0;
    a += (hw >> 9 & 1) != 0 ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_down(c, o, 64);
    f += __shfl_down(f, o, 64);
    a += __shfl_down(a, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6] = c;
    part_f[threadIdx.x >> 6] = f;
    part_a[threadIdx.x >> 6] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0, arr = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      tot += (unsigned long long)(unsigned)part[w] | (unsigned long long)(unsigned)part_f[w] << 32;
      arr += (unsigned long long)(unsigned)part_a[w];
    }
    __hip_atomic_store(rec, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(rec + 2, arr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(rec + 1, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Sub-wave groups: G = 8, 16 or 32 lanes own one resource of up to G*R rows (R rows
// per lane), so a wave decides 64 / G resources with one set of reduction chains
// (DPP inside each 16-lane row, plus one readlane combine for G = 32); G = 64 is one
// wave per resource (wave reductions only, no barriers).  Small resources are
// VALU-bound on their per-resource reductions (~28 reduced dwords per pass set, 4 DPP
// steps each): narrow groups with several rows per lane share every DPP step among
// 64 / G resources.
// The sub-wave bins in one launch (k_subs): the workgroups of each bin follow one
// another in blockIdx order, so the class stream runs them without a kernel boundary
// (drain + ramp) between bins.  Register use is the largest bin's.
template <int G, int R>
__device__ __forceinline__ void sub_part(const DevParams& p, WorkItem* __restrict__ items, int nitems, int blk,
                                         int32_t* general_list, int32_t* general_count) {
  Lds<G> lds;  // unused by sub-wave and wave reductions
  const int i = blk * (256 / G) + (int)(threadIdx.x / G);
  if (i >= nitems) return;
  group_segment<G, R>(p, items[i], items + i, threadIdx.x & (G - 1), lds, general_list, general_count);
}

template <int K>
__device__ __forceinline__ void sub_shape(const DevParams& p, const SubBins& sb, int b, int32_t* general_list,
                                          int32_t* general_count) {
  if constexpr (K < kSubShapes) {
    if (b < sb.blocks[K])
      return sub_part<kSubShapeG[K], kSubShapeR[K]>(p, sb.items[K], sb.n[K], b, general_list, general_count);
    sub_shape<K + 1>(p, sb, b - sb.blocks[K], general_list, general_count);
  }
}

__global__ __launch_bounds__(256, 5) void k_subs(DevParams p, SubBins sb, int32_t* general_list,
                                              int32_t* general_count) {
  sub_shape<0>(p, sb, (int)blockIdx.x, general_list, general_count);
}

// --------------------------------------------------------------------------
// Tiles of small resources (n <= kSmallMax), one 256-thread workgroup per tile
// (dm_device.h Tile): the workgroup stages the tile's rows in LDS with lane-strided
// (coalesced) loads while thread k loads resource k's offsets and record (consecutive
// records: coalesced as well) -- one memory round trip, where the packed kernel waits
// for its pack, then for the records its rows' resources name.  Thread k then decides
// resource k literally, in row order (sums in the oracle's order: bit-exact), from LDS;
// the gets go back to global memory row-parallel (coalesced), and each resource's
// record from its thread (coalesced).
// --------------------------------------------------------------------------
struct TileLds {
  double w[kTileRows];
  double h[kTileRows];  // a row's has, then its gets (only the row's own resource thread reads either)
  int32_t sr[kTileRows];
  uint8_t lv[kTileRows];
};

__global__ __launch_bounds__(256) void k_tile_small(DevParams p, const Tile* __restrict__ tiles,
                                                    const TileEntry* __restrict__ list) {
  __shared__ TileLds L;
  const Tile tl = tiles[blockIdx.x];
  const int t = threadIdx.x;
  const bool lst = tl.list != 0;  // (uniform)
  const int nrows = tl.nrows, nseg = tl.nseg;
  constexpr int K = kTileRows / 256;
  // the records first, then the rows: every load of the tile is in flight before the
  // first is consumed (the LDS stores below)
  const bool own = t < nseg;
  int seg, ldo = 0;
  if (lst) {
    const TileEntry e = list[tl.first_seg + (own ? t : 0)];
    seg = e.seg;
    ldo = e.lds;
  } else {
    seg = tl.first_seg + (own ? t : 0);
  }
  const int64_t lo64 = p.seg_off[seg], hi64 = p.seg_off[seg + 1];
  // a row's global index is base + its LDS index (a list tile: per resource)
  const int64_t row0 = lst ? lo64 - ldo : tl.row0;
  const Res rs = load_res(p, seg);
  if (lst) {  // each thread its own resource's rows (n <= kSmallMax)
    const int n = own ? (int)(hi64 - lo64) : 0;
    double wv[kSmallMax], hv[kSmallMax];
    int sv[kSmallMax];
#pragma unroll
    for (int j = 0; j < kSmallMax; ++j)
      if (j < n) {
        wv[j] = p.wants[lo64 + j];
        hv[j] = p.has[lo64 + j];
        sv[j] = p.sub[lo64 + j];
      }
#pragma unroll
    for (int j = 0; j < kSmallMax; ++j)
      if (j < n) {
        L.w[ldo + j] = wv[j];
        L.h[ldo + j] = hv[j];
        L.sr[ldo + j] = sv[j];
      }
  } else {
    double wv[K], hv[K];
    int sv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k * 256 < nrows) {  // uniform
        const int i = k * 256 + t;
        const unsigned u = (unsigned)(i < nrows ? i : nrows - 1);
        wv[k] = *col_at(p.wants + row0, u);
        hv[k] = *col_at(p.has + row0, u);
        sv[k] = *col_at(p.sub + row0, u);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = k * 256 + t;
      if (k * 256 < nrows && i < nrows) {
        L.w[i] = wv[k];
        L.h[i] = hv[k];
        L.sr[i] = sv[k];
      }
    }
  }
  __syncthreads();
  if (own) {
    const int lo = (int)(lo64 - row0), hi = (int)(hi64 - row0);
    // Clean (store.go:169-181): the store's running sums (or rebuilt from every row in
    // row order, recompute mode) less the rows that expired, in row order
    long long count;
    double sh, sw;
    if (p.recompute) {
      count = 0;
      sh = 0.0;
      sw = 0.0;
      for (int q = lo; q < hi; ++q) {
        sh += L.h[q] - 0.0;
        sw += L.w[q] - 0.0;
        count += sub_value(L.sr[q]);
      }
    } else {
      count = rs.agg_count;
      sh = rs.agg_has;
      sw = rs.agg_wants;
    }
    const bool expl_rows = any_explicit(rs);
    unsigned live = 0;  // bit q - lo (n <= kSmallMax)
    for (int q = lo; q < hi; ++q) {
      const int32_t raw = L.sr[q];
      int64_t e = rs.follow_exp;
      if (expl_rows && sub_explicit(raw)) e = p.expiry[row0 + q];
      if (sub_released(raw)) e = kReleased;
      const bool lv = !(p.now > e);  // store.go:174
      live |= (lv ? 1u : 0u) << (q - lo);
      if (!lv && !sub_released(raw)) {  // expired: Clean releases it (a released row holds zeros)
        sw -= L.w[q];
        sh -= L.h[q];
        count -= sub_value(raw);
      }
    }
    const double C = rs.C;
    const double eq = C / (double)count;
    const bool ps = !rs.learning && rs.kind == 2, fs = !rs.learning && rs.kind == 3;
    double x = 0.0, y = 0.0;
    long long wi = 0;
    if (ps || fs) {
      for (int q = lo; q < hi; ++q) {
        if (!(live >> (q - lo) & 1)) continue;
        const double wj = L.w[q];
        const int sj = sub_value(L.sr[q]);
        if (ps) {
          const double e2 = eq * (double)sj;  // algorithm.go:273
          if (wj < e2)
            x += e2 - wj;
          else
            y += wj - e2;
        } else {
          const double d = (double)sj * eq;  // algorithm.go:160
          if (wj < d)
            x += d - wj;
          else if (wj > d)
            wi += sj;
        }
      }
    }
    double osh = sh;  // Assign: sumHas += gets - has (store.go:156), row order
    double Tc = 0.0;  // round 2 at the last threshold asked for (uniform subclients: one per resource)
    AggC cc{0.0, 0};
    bool have_c = false;
    for (int q = lo; q < hi; ++q) {
      const bool lv = live >> (q - lo) & 1;
      L.lv[q] = lv ? 1 : 0;
      if (!p.writeback) __builtin_nontemporal_store(lv ? (int64_t)rs.exp_out : (int64_t)kReleased,
                                                    col_at(p.out_expiry + row0, (uint32_t)q));
      if (!lv) {
        L.h[q] = 0.0;
        continue;
      }
      const double w = L.w[q], h = L.h[q];
      const int s = sub_value(L.sr[q]);
      double g;
      if (rs.learning) {
        g = h;  // Learn (algorithm.go:297-302)
      } else if (rs.kind == 0) {
        g = w;  // NoAlgorithm
      } else if (rs.kind == 1) {
        g = minF(C, w);  // Static
      } else if (ps) {
        const double epc = eq * (double)s;  // :233
        const double unused = C - sh + h;   // :239
        g = (sw <= C || w <= epc) ? minF(w, unused) : minF(epc + (w - epc) * (x / y), unused);
      } else {
        double T = 0.0;
        if (!fs_stage01(w, h, s, C, sh, eq, x, wi, &g, &T)) {
          if (!have_c || __double_as_longlong(T) != __double_as_longlong(Tc)) {
            cc = AggC{0.0, 0};
            for (int j = lo; j < hi; ++j) {  // round 2 at this row's threshold (algorithm.go:189-204)
              if (!(live >> (j - lo) & 1)) continue;
              const double wj = L.w[j];
              const int sj = sub_value(L.sr[j]);
              if (!(wj > (double)sj * eq)) continue;
              if (wj < T)
                cc.ee += T - wj;
              else if (wj > T)
                cc.sgt += sj;
            }
            Tc = T;
            have_c = true;
          }
          g = fs_stage2(w, h, s, C, sh, eq, x, wi, T, cc);
        }
      }
      L.h[q] = g;
      osh += g - h;
    }
    write_resource(p, seg, rs, Clean{count, osh, sw}, 0.0);
  }
  if (lst) {  // a list tile: each thread its own resource's leases
    if (own) {
      for (int i = (int)(lo64 - row0); i < (int)(hi64 - row0); ++i) {
        const int32_t raw = L.sr[i];
        if (L.lv[i]) {
          __builtin_nontemporal_store(L.h[i], col_at(p.out_gets + row0, (uint32_t)i));
          if (p.writeback && raw < 0) *col_at(p.out_sub + row0, (uint32_t)i) = raw & 0x7FFFFFFF;
        } else {
          __builtin_nontemporal_store(0.0, col_at(p.out_gets + row0, (uint32_t)i));
          if (p.writeback && !sub_released(raw)) {
            *col_at(p.out_wants + row0, (uint32_t)i) = 0.0;
            *col_at(p.out_sub + row0, (uint32_t)i) = (int32_t)kSubReleased;
          }
        }
      }
    }
    return;
  }
  __syncthreads();
  // the leases, row-parallel (put_live / put_released of the packed kernel)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = k * 256 + t;
    if (k * 256 < nrows && i < nrows) {
      const int32_t raw = L.sr[i];
      if (L.lv[i]) {
        __builtin_nontemporal_store(L.h[i], col_at(p.out_gets + row0, (uint32_t)i));
        if (p.writeback && raw < 0) *col_at(p.out_sub + row0, (uint32_t)i) = raw & 0x7FFFFFFF;
      } else {
        __builtin_nontemporal_store(0.0, col_at(p.out_gets + row0, (uint32_t)i));
        if (p.writeback && !sub_released(raw)) {
          *col_at(p.out_wants + row0, (uint32_t)i) = 0.0;
          *col_at(p.out_sub + row0, (uint32_t)i) = (int32_t)kSubReleased;
        }
      }
    }
  }
}

// --------------------------------------------------------------------------
// host-side launchers (called by dm_tick.cpp)
// --------------------------------------------------------------------------
hipError_t launch_tile_small(const DevParams& p, const Tile* tiles, const TileEntry* list, int n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  k_tile_small<<<n, 256, 0, st>>>(p, tiles, list);
  return hipGetLastError();
}

// the workgroup bins (3-6) in their one-kernel form; the sub-wave bins run in k_subs
hipError_t launch_bin(const BinItems& w, const DevParams& p, int32_t* glist, int32_t* gcount, hipStream_t st) {
  if (w.n <= 0) return hipSuccess;
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    k_block<G, R><<<w.n, G, 0, st>>>(p, w.items, w.n, glist, gcount);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_subs(const DevParams& p, const SubBins& sb, int32_t* glist, int32_t* gcount, hipStream_t st) {
  unsigned blocks = 0;
  for (int k = 0; k < kSubShapes; ++k) blocks += (unsigned)sb.blocks[k];
  if (blocks == 0) return hipSuccess;
  k_subs<<<blocks, 256, 0, st>>>(p, sb, glist, gcount);
  return hipGetLastError();
}

// The bins split by the dense hint: the dense kernel over every item, then the rest kernel over
// what it queued (two launches, timed separately).  dm_launch.h has the three launchers'
// arguments; a masked launch goes to dm_tick_masked.hip's half.
hipError_t launch_bin_dense(const BinItems& w, const DevParams& p, const SplitArgs& a, hipEvent_t done, bool steady,
                            bool masked, FixKey* keys, bool use_keys, hipStream_t st) {
  if (masked && !steady) return hipErrorInvalidValue;  // masked implies steady
  if (masked) return launch_dense_masked(w, p, a, done, keys, use_keys, st);
  return launch_dense_build<false>(w, p, a, done, steady, keys, use_keys, st);
}

hipError_t launch_bin_sweep(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw, bool masked,
                            hipStream_t st) {
  if (masked) return launch_list_masked(false, w, p, a, sw, nullptr, true, 0u, false, st);
  return launch_list_build<false, false>(w, p, a, sw, nullptr, true, 0u, false, st);
}

hipError_t launch_bin_cycle(const BinItems& w, const DevParams& p, const SplitArgs& a, const SweepArgs& sw, bool masked,
                            CycAux* aux, bool use_keys, unsigned stamp, bool tell, hipStream_t st) {
  if (masked) return launch_list_masked(true, w, p, a, sw, aux, use_keys, stamp, tell, st);
  return launch_list_build<true, false>(w, p, a, sw, aux, use_keys, stamp, tell, st);
}

// dm_store_stats for a part in the cycle form: out[0] the keys in state 2, out[1] those of
// them whose prev_has differs from the record's sum_has (the items in a cycle that is no
// fixed point)
__global__ __launch_bounds__(1024) void k_count_cycle(const FixKey* __restrict__ keys, const CycAux* __restrict__ aux,
                                                      const WorkItem* __restrict__ items, const ResAgg* __restrict__ agg,
                                                      int n, int32_t* out) {
  __shared__ int part[16], part_c[16];
  int c = 0, y = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const bool v = keys[i].valid == 2;
    c += v ? 1 : 0;
    y += v && aux[i].prev_has != (uint64_t)__double_as_longlong(agg[items[i].seg].sum_has) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_down(c, o, 64);
    y += __shfl_down(y, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6] = c;
    part_c[threadIdx.x >> 6] = y;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0, tot_c = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      tot += part[w];
      tot_c += part_c[w];
    }
    out[0] = tot;
    out[1] = tot_c;
  }
}
hipError_t launch_count_cycle(const FixKey* keys, const CycAux* aux, const WorkItem* items, const ResAgg* agg, int n,
                              int32_t* out, hipStream_t st) {
  k_count_cycle<<<1, 1024, 0, st>>>(keys, aux, items, agg, n, out);
  return hipGetLastError();
}

// dm_store_stats: the valid keys among n (one workgroup, on demand; never on the tick)
__global__ __launch_bounds__(1024) void k_count_keys(const FixKey* __restrict__ keys, int n, int32_t* out) {
  __shared__ int part[16];
  int c = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) c += keys[i].valid ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += part[w];
    *out = tot;
  }
}
hipError_t launch_count_keys(const FixKey* keys, int n, int32_t* out, hipStream_t st) {
  k_count_keys<<<1, 1024, 0, st>>>(keys, n, out);
  return hipGetLastError();
}

hipError_t launch_count_undense(const WorkItem* items, int n, unsigned long long* rec, unsigned long long epoch,
                                hipStream_t st) {
  k_count_undense<<<1, 1024, 0, st>>>(items, n, rec, epoch);
  return hipGetLastError();
}

hipError_t launch_bin_rest(const BinItems& w, const DevParams& p, const SplitArgs& a, int32_t* host_count,
                           int rest_grid, hipEvent_t done, hipStream_t st) {
  if (w.n <= 0) return hipSuccess;
  const dim3 rg((unsigned)std::max(1, std::min(w.n, rest_grid)));
  const bool known = with_bin_shape(w.bin, [&](auto g, auto r) {
    constexpr int G = decltype(g)::value, R = decltype(r)::value;
    hipExtLaunchKernelGGL((k_block_rest<G, R>), rg, dim3(G), 0, st, nullptr, done, 0, p, w.items, a.queue, a.qcnt, a.par,
                          host_count, a.glist, a.gcount);
  });
  return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace dm
