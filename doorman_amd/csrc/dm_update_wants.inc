// dm_update_wants.inc -- the body of k_update_wants and of k_update_wants_keys (dm_update.hip
// has the account of both), included once in each.  The including kernel defines kKeys (the
// key-clearing build) and `kc` (its KeyClear argument; unused and empty in the plain kernel).
// One text and two kernels, not two instances of one inlined function: the plain kernel's
// code then does not depend on the other build (profiles/keep_keys_isa.md).
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (*flags & kUpdReject) return;  // uniform over the grid
  const bool active = i < n;
  int seg = 0;
  double d = 0.0;
  bool changed = false;  // (kKeys) the row changed its wants bits
  if (active) {
    const int64_t r = rows[i];
    seg = seg_of_row(ix, r);
    if (!sub_released(s_sub[r])) {
      d = wants[i] - s_wants[r];
      if constexpr (kKeys) changed = __double_as_longlong(wants[i]) != __double_as_longlong(s_wants[r]);
      s_wants[r] = wants[i];
    }
  }
  wave_seg_add<kKeys>(agg, active, seg, 0.0, d, 0, false, false, changed, kc);
