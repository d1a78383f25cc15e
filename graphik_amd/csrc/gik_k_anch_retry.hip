// graphik_amd/csrc/gik_k_anch_retry.hip -- device code of the fixed-anchor restart kernels (gik_anch_retry.hip.h)
#define GIK_DEFINE_ANCH_RETRY_KERNELS 1
#include "gik_anch_retry.hip.h"
