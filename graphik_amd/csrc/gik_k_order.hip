// graphik_amd/csrc/gik_k_order.hip -- device code of the claim-order kernels (gik_order.hip.h)
#define GIK_DEFINE_ORDER_KERNELS 1
#include "gik_order.hip.h"
