// dm_mask_apply.inc -- the body of k_mask_apply and of k_mask_apply_keys (dm_update.hip has
// the account of both), included once in each.  The including kernel defines kKeys (the
// key-clearing build) and `kc` (its KeyClear argument; unused and empty in the plain kernel).
// One text and two kernels, not two instances of one inlined function: the plain kernel's
// code then does not depend on the other build (profiles/keep_keys_isa.md).
  if (*flags & kUpdReject) return;  // uniform over the grid
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kMaskWords;
  if (w0 >= nwords) return;  // whole waves
  const int nw = nwords - w0 < kMaskWords ? (int)(nwords - w0) : kMaskWords;
  uint64_t my_m = 0ull;
  int64_t my_off = 0, my_end = 0;
  if (lane < nw) {
    const int64_t w = w0 + lane;
    my_m = mask[w];
    my_off = block_offs[w >> 8] + word_pre[w];
  }
  // only the values [vlo, vhi) have landed (dm_store_apply copies them in chunks): a
  // wave whose words' values all lie outside is done
  {
    const int64_t first = readlane_any(my_off, 0);
    const int64_t last = readlane_any(my_off, nw - 1) + __popcll(readlane_any(my_m, nw - 1));  // one past
    if (last <= vlo || first >= vhi) return;
  }
  int my_seg = 0;
  if (lane < nw) {
    my_seg = seg_of_row(ix, first_row + 64 * (w0 + lane));
    my_end = ix.seg_off[my_seg + 1];  // the word lies in one resource iff its last row < my_end
  }
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t inr = 0;  // bit q: this lane's row of word q is set and its value in [vlo, vhi)
  double v[kMaskWords], old[kMaskWords];
  uint32_t freed = 0;  // bit q: this lane's row of word q is released (k_update_wants: left alone)
#pragma unroll
  for (int q = 0; q < kMaskWords; ++q) {  // every load in flight before the first use
    v[q] = 0.0;
    old[q] = 0.0;
    if (q < nw) {
      const uint64_t m = readlane_any(my_m, q);
      const int64_t vi = readlane_any(my_off, q) + __popcll(m & below);
      if (((m >> lane) & 1ull) && vi >= vlo && vi < vhi) {
        inr |= 1u << q;
        v[q] = wants[vi];
        old[q] = s_wants[first_row + 64 * (w0 + q) + lane];
        freed |= (sub_released(s_sub[first_row + 64 * (w0 + q) + lane]) ? 1u : 0u) << q;
      }
    }
  }
  int cur = -1;      // resource whose deltas `acc` holds (uniform)
  double acc = 0.0;  // this lane's share of them
  bool chg = false;  // (kKeys) ... and whether a row of this lane's changed its wants bits in it
  bool nan = false;
#pragma unroll
  for (int q = 0; q < kMaskWords; ++q) {
    const uint64_t m = q < nw ? readlane_any(my_m, q) : 0ull;
    if (m != 0ull) {  // uniform
      const int64_t row0 = first_row + 64 * (w0 + q);
      const bool act = (inr >> q & 1u) && !(freed >> q & 1u);
      const int s0 = __builtin_amdgcn_readlane(my_seg, q);
      const bool single = readlane_any(my_end, q) > row0 + 63 - __builtin_clzll(m);
      double d = 0.0;
      int seg = s0;
      bool changed = false;  // (kKeys) this lane's row of the word changed its wants bits
      if (act) {
        const int64_t r = row0 + lane;
        nan |= __builtin_isnan(v[q]);
        if (!single)
          while (ix.seg_off[seg + 1] <= r) ++seg;
        d = v[q] - old[q];
        s_wants[r] = v[q];
        if constexpr (kKeys) changed = __double_as_longlong(v[q]) != __double_as_longlong(old[q]);
      }
      if (single && s0 == cur) {
        acc += d;
        if constexpr (kKeys) chg |= changed;
      } else {
        if (cur >= 0) {  // flush the previous resource
          const double t = wave_reduce(acc, [](double a, double b) { return a + b; });
          if (lane == 0) atomicAdd(&agg[cur].sum_wants, t);
          if constexpr (kKeys) {
            if (__ballot(chg) != 0ull && lane == 0) clear_key(kc, cur);
          }
        }
        if (single) {
          cur = s0;
          acc = d;
          if constexpr (kKeys) chg = changed;
        } else {
          cur = -1;
          acc = 0.0;
          if constexpr (kKeys) chg = false;
          wave_seg_add<kKeys>(agg, act, seg, 0.0, d, 0, false, false, changed, kc);
        }
      }
    }
  }
  if (cur >= 0) {
    const double t = wave_reduce(acc, [](double a, double b) { return a + b; });
    if (lane == 0) atomicAdd(&agg[cur].sum_wants, t);
    if constexpr (kKeys) {
      if (__ballot(chg) != 0ull && lane == 0) clear_key(kc, cur);
    }
  }
  if (__ballot(nan) && lane == 0) atomicOr(flags, kUpdNaN);
