// graphik_amd/csrc/gik_k_retry.hip -- device code of the restart kernels (gik_retry.hip.h)
#define GIK_DEFINE_RETRY_KERNELS 1
#include "gik_retry.hip.h"
