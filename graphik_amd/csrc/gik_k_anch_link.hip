// graphik_amd/csrc/gik_k_anch_link.hip -- the fixed-anchor kernels with link hinges (WaveCtx<.., LINKS>)
#include "gik_wave_kernels.hip.h"
#include "gik_instances.h"
namespace gik {
GIK_KERNELS_ANCH_LINK(GIK_INSTANTIATE)
}
