// dm_refresh_dense.inc -- the body of k_refresh_dense and of k_refresh_dense_keys (dm_update.hip
// has the account of both), included once in each.  The including kernel defines kKeys (the
// key-clearing build) and `kc` (its KeyClear argument; unused and empty in the plain kernel).
// One text and two kernels, as dm_mask_apply.inc: the plain kernel's code does not depend on
// the other build (profiles/device_update_isa.md).
  __shared__ uint32_t wg_cnt[4], wg_nan[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nruns = (n + 63) >> 6;  // 64-row runs of the range (the last may be partial)
  const int64_t w0 = ((int64_t)blockIdx.x * 4 + wave) * kMaskWords;
  // (a wave past the range has nw = 0 and falls through to the workgroup's reduction)
  const int nw = w0 >= nruns ? 0 : nruns - w0 < kMaskWords ? (int)(nruns - w0) : kMaskWords;
  int my_seg = 0;
  int64_t my_end = 0;
  if (lane < nw) {
    my_seg = seg_of_row(ix, first_row + 64 * (w0 + lane));
    my_end = ix.seg_off[my_seg + 1];  // the run lies in one resource iff its last changed row < my_end
  }
  // Every load in flight before the first use.  The loads are unconditional: a lane past the
  // range (the last run's tail, an idle wave) reads entry 0 of the range instead and drops it
  // (`inr`), so the values are plain registers and no branch carries them.
  double v[kMaskWords], old[kMaskWords];
  uint32_t inr = 0;  // bit q: this lane's row of run q is in the range
#pragma unroll
  for (int q = 0; q < kMaskWords; ++q) {
    const int64_t i = 64 * (w0 + q) + lane;
    const bool in = q < nw && i < n;
    const int64_t ic = in ? i : 0;
    inr |= (in ? 1u : 0u) << q;
    v[q] = wants[ic];
    old[q] = s_wants[first_row + ic];
  }
  uint32_t dif = 0;  // bit q: ... and its bits differ
#pragma unroll
  for (int q = 0; q < kMaskWords; ++q)
    dif |= (__double_as_longlong(v[q]) != __double_as_longlong(old[q]) ? 1u : 0u) << q;
  dif &= inr;
  // Released (a free slot: left alone): the mark a tick or a release leaves in the subclients
  // word, or a row that was loaded or upserted as released -- explicit, its expiry DM_RELEASED --
  // and that no tick has marked yet (dm_read_store reports both as DM_RELEASED).  The
  // subclients word is loaded only where the bits differ, the expiry only for an explicit row
  // among those: none after a writeback tick, which leaves followers and marked rows.
  uint32_t freed = 0;  // bit q: ... and the row is released
#pragma unroll
  for (int q = 0; q < kMaskWords; ++q)
    if (dif >> q & 1u) {
      const int64_t r = first_row + 64 * (w0 + q) + lane;
      const int32_t raw = s_sub[r];
      const bool rel = sub_released(raw) || (raw < 0 && s_exp[r] == kReleased);
      freed |= (rel ? 1u : 0u) << q;
    }
  const uint32_t chg = dif & ~freed;  // bit q: this lane's row of run q is written
  int cur = -1;      // resource whose deltas `acc` holds (uniform)
  double acc = 0.0;  // this lane's share of them
  bool nan = false;
  uint32_t cnt = 0;  // rows this wave wrote (uniform)
#pragma unroll
  for (int q = 0; q < kMaskWords; ++q) {
    const bool act = chg >> q & 1u;
    const uint64_t m = __ballot(act);  // the run's changed mask: no count pass, no packed index
    if (m != 0ull) {  // uniform; a run without a changed row does nothing more
      const int64_t row0 = first_row + 64 * (w0 + q);
      cnt += (uint32_t)__popcll(m);
      const int s0 = __builtin_amdgcn_readlane(my_seg, q);
      const bool single = readlane_any(my_end, q) > row0 + 63 - __builtin_clzll(m);
      double d = 0.0;
      int seg = s0;
      if (act) {
        const int64_t r = row0 + lane;
        nan |= __builtin_isnan(v[q]);
        if (!single)
          while (ix.seg_off[seg + 1] <= r) ++seg;
        d = v[q] - old[q];
        s_wants[r] = v[q];
      }
      if (single && s0 == cur) {
        acc += d;
      } else {
        if (cur >= 0) {  // flush the previous resource: some row of it changed
          const double t = wave_reduce(acc, [](double a, double b) { return a + b; });
          if (lane == 0) atomicAdd(&agg[cur].sum_wants, t);
          if constexpr (kKeys) {
            if (lane == 0) clear_key(kc, cur);
          }
        }
        if (single) {
          cur = s0;
          acc = d;
        } else {
          cur = -1;
          acc = 0.0;
          wave_seg_add<kKeys>(agg, act, seg, 0.0, d, 0, false, false, act, kc);
        }
      }
    }
  }
  if (cur >= 0) {
    const double t = wave_reduce(acc, [](double a, double b) { return a + b; });
    if (lane == 0) atomicAdd(&agg[cur].sum_wants, t);
    if constexpr (kKeys) {
      if (lane == 0) clear_key(kc, cur);
    }
  }
  // the NaN flag and the count: per wave, then per workgroup, one atomic a word at most
  const bool wnan = __ballot(nan) != 0ull;
  if (lane == 0) {
    wg_cnt[wave] = cnt;
    wg_nan[wave] = wnan ? 1u : 0u;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = wg_cnt[0] + wg_cnt[1] + wg_cnt[2] + wg_cnt[3];
    if (total) atomicAdd(count, (unsigned long long)total);
    if (wg_nan[0] | wg_nan[1] | wg_nan[2] | wg_nan[3]) atomicOr(flags, kUpdNaN);
  }
