// dm_tick_fused_root.hip — the ROOT builds of k_block_fused (dm_tick_fused.hip: the fused tick
// that also carries the root's round of the previous step) and their launcher, as a unit of
// their own: dm_tick_fused.hip's device code is what it is without them.
#define DM_FUSED_ROOT_UNIT 1
#include "dm_tick_fused.hip"
