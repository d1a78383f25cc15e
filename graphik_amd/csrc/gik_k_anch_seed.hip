// graphik_amd/csrc/gik_k_anch_seed.hip -- device code of the seeded fixed-anchor glue and the clearance, link-clearance and sweep kernels
// (gik_anch_seed.hip.h)
#define GIK_DEFINE_ANCH_SEED_KERNELS 1
#include "gik_anch_seed.hip.h"
