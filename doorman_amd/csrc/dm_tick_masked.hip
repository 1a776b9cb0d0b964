// dm_tick_masked.hip — the masked builds of the split form's dense-side kernels (dm_keep_keys'
// DM_KEEP_FREE_SLOTS, dm_split_form.h PartForm::masked): dm_tick_steady.h's kernels instantiated
// with kMasked, and the masked half of their launchers.  A unit, and so a code object, of their
// own: dm_tick_group.hip's is what it is without them, the order and placement of its kernels
// included.
#include "dm_tick_steady.h"

namespace dm {

hipError_t launch_dense_masked(const BinItems& w, const DevParams& p, const SplitArgs& a, hipEvent_t done,
                               FixKey* keys, bool use_keys, hipStream_t st) {
  return launch_dense_build<true>(w, p, a, done, true, keys, use_keys, st);
}

hipError_t launch_list_masked(bool cycle, const BinItems& w, const DevParams& p, const SplitArgs& a,
                              const SweepArgs& sw, CycAux* aux, bool use_keys, unsigned stamp, bool tell,
                              hipStream_t st) {
  if (cycle) return launch_list_build<true, true>(w, p, a, sw, aux, use_keys, stamp, tell, st);
  return launch_list_build<false, true>(w, p, a, sw, aux, use_keys, stamp, tell, st);
}

}  // namespace dm
