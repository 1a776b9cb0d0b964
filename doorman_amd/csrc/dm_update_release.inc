// dm_update_release.inc -- the body of k_release and of k_release_keys (dm_update.hip has the account
// of both), included once in each.  The including kernel defines kKeys (the key-clearing build)
// and `kc` (its KeyClear argument; unused and empty in the plain kernel).  One text and two
// kernels, as dm_update_wants.inc: the plain kernel's code does not depend on the other build
// (profiles/keep_updates_isa.md).  Every active row counts as changed: the key of each
// workgroup-bin resource of which the call writes a row is cleared, once per run of the
// resource within the wave (wave_seg_add<true>).
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (*flags & kUpdReject) return;  // uniform over the grid
  const bool active = i < n;
  int seg = 0;
  double dh = 0.0, dw = 0.0;
  long long ds = 0;
  if (active) {
    const int64_t r = rows[i];
    seg = seg_of_row(ix, r);
    (void)s_exp;
    release_row(ix, seg, r, s_has, s_wants, s_sub, expl, du, &dh, &dw, &ds);
  }
  wave_seg_add<kKeys>(agg, active, seg, dh, dw, ds, true, true, active, kc);
