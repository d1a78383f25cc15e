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
