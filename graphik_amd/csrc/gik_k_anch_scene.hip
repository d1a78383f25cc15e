// graphik_amd/csrc/gik_k_anch_scene.hip -- the fixed-anchor solve kernels with per-goal obstacle scenes (rtr_wave_run<.., SCENES>)
#include "gik_wave_kernels.hip.h"
#include "gik_instances.h"
namespace gik {
GIK_KERNELS_ANCH_SCENE(GIK_INSTANTIATE)
}
