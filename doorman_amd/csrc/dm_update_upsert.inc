// dm_update_upsert.inc -- the body of k_upsert and of k_upsert_keys (dm_update.hip has the account
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
    const double hv = has ? has[i] : 0.0;
    const int64_t sv = sub32 ? (int64_t)sub32[i] : sub[i];
    dh = hv - s_has[r];
    dw = wants[i] - s_wants[r];
    ds = sv - sub_value(s_sub[r]);
    s_has[r] = hv;
    s_wants[r] = wants[i];
    s_sub[r] = (int32_t)((uint32_t)sv | kSubExplicit);  // in [0, kSubMax] (k_check_rows); expiry explicit
    const int64_t ex = expiry ? expiry[i] : now + (int64_t)cfg[seg].lease_len_s * kNs;
    s_exp[r] = ex;
    // an arrival with the dense resource's count and the Assign's expiry, not before the
    // followers': the resource stays dense, the row goes into its arrival mask
    MaskPos mp;
    WorkItem* it;
    const uint8_t st = expl[seg];
    if (!expiry && dense_row(du, ix, seg, r, st, &mp, &it) && sv == (int64_t)st - 1 && ex >= agg[seg].follow_exp) {
      mask_bit(du.rmask + rel_mask_offset(ix.seg_off[seg]), mp.roff, mp.rbit, false);
      mask_bit(du.rmask + rel_mask_offset(ix.seg_off[seg]), mp.aoff, mp.abit, true);
      atomicOr(&it->n, 1 << 25);
    } else {
      expl[seg] = 1;  // the tick reads this resource's expiry column again
    }
  }
  wave_seg_add<kKeys>(agg, active, seg, dh, dw, ds, true, true, active, kc);
