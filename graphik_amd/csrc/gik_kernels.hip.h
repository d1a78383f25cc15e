// graphik_amd/csrc/gik_kernels.hip.h -- every kernel family header at once, for gik_host.hip alone: it takes every
// kernel's address and calls the contexts' lds_bytes.  A gik_k_*.hip unit includes its own family's header instead.
#pragma once

#include "gik_wave_kernels.hip.h"
#include "gik_block_kernels.hip.h"
#include "gik_npt_kernels.hip.h"
#include "gik_quad_kernels.hip.h"
#include "gik_prep.hip.h"
#include "gik_prep_quad.hip.h"
#include "gik_recover_seed.hip.h"
#include "gik_anch_glue.hip.h"

// The groups that stand beside GIK_ALL_KERNELS (gik_instances.h), the fixed-anchor kernels with self hinges and those with
// half-space obstacles, declared here for the same reason gik_host.hip declares the others: their addresses refer to
// gik_k_anch_self.hip's and gik_k_anch_half.hip's symbols.
#include "gik_instances.h"
namespace gik {
GIK_KERNELS_ANCH_SELF(GIK_EXTERN_TEMPLATE)
GIK_KERNELS_ANCH_HALF(GIK_EXTERN_TEMPLATE)
}
