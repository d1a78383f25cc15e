// graphik_amd/csrc/gik_k_anch_half.hip -- the fixed-anchor kernels with half-space obstacles (WaveCtx<.., HALF>), without and with link hinges
#include "gik_wave_kernels.hip.h"
#include "gik_instances.h"
namespace gik {
GIK_KERNELS_ANCH_HALF(GIK_INSTANTIATE)
}
