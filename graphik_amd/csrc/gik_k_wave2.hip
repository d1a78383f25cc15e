// graphik_amd/csrc/gik_k_wave2.hip -- device code of the GIK_KERNELS_WAVE2 group (gik_instances.h)
#include "gik_wave_kernels.hip.h"
#include "gik_instances.h"

namespace gik {
GIK_KERNELS_WAVE2(GIK_INSTANTIATE)
}  // namespace gik
