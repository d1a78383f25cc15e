// graphik_amd/csrc/gik_k_anch_self.hip -- the fixed-anchor kernels with self hinges (WaveCtx<.., SELF>), without and with link hinges
#include "gik_wave_kernels.hip.h"
#include "gik_instances.h"
namespace gik {
GIK_KERNELS_ANCH_SELF(GIK_INSTANTIATE)
}
