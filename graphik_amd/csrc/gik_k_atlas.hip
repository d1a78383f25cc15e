// graphik_amd/csrc/gik_k_atlas.hip -- device code of the atlas kernels (gik_atlas.hip.h)
#define GIK_DEFINE_ATLAS_KERNELS 1
#include "gik_atlas.hip.h"
