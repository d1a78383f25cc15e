// graphik_amd/csrc/gik_instances.h -- the list of compiled kernel instantiations, by translation unit.
//
// GIK_KERNELS_<GROUP>(X) calls X(<function signature>) for every instantiation of the group; gik_k_<group>.hip expands
// it with GIK_INSTANTIATE, gik_host.hip expands all groups with GIK_EXTERN_TEMPLATE (so that taking a kernel's address
// there -- the variant tables, hipLaunchKernelGGL -- refers to the other file's symbol instead of compiling the kernel
// a second time).  The five non-template kernels (prep_wave_kernel of gik_prep.hip.h; recover_kernel, seed_kernel of
// gik_recover_seed.hip.h; anch_init_kernel, anch_gather_kernel of gik_anch_glue.hip.h) are defined where
// GIK_DEFINE_PLAIN_KERNELS is set, gik_k_prep.hip; every other unit that includes one of those headers -- both host units
// do -- sees their prototypes.  This header names kernels and argument types only: include the family's header first.
#pragma once

#define GIK_INSTANTIATE(...) template __global__ __VA_ARGS__;
#define GIK_EXTERN_TEMPLATE(...) extern template __global__ __VA_ARGS__;

// one unknown per lane (rtr_wave_kernel<K, slots, flag word>, WaveBuild of gik_wave_kernels.hip.h), k = 3: column-form
// product (+ ConjugateGradient, known answers, tail spreading)
#define GIK_KERNELS_WAVE3(X)                                   \
  X(void rtr_wave_kernel<3, 9, W_THETA1>(SolveArgs))           \
  X(void rtr_wave_kernel<3, 9, 0>(SolveArgs))                  \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_SPREAD>(SolveArgs)) \
  X(void rcg_wave_kernel<3, 9>(SolveArgs))                     \
  X(void kat_wave_kernel<3, 9>(KatArgs))                       \
  X(void rtr_wave_kernel<3, 10, W_THETA1>(SolveArgs))          \
  X(void rtr_wave_kernel<3, 10, 0>(SolveArgs))                 \
  X(void rcg_wave_kernel<3, 10>(SolveArgs))                    \
  X(void kat_wave_kernel<3, 10>(KatArgs))
// ... per-edge product form (gik_wave_strict.hip.h)
#define GIK_KERNELS_WAVE3_STRICT(X)                                         \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_PER_EDGE>(SolveArgs))           \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_SPREAD | W_PER_EDGE>(SolveArgs)) \
  X(void rtr_wave_kernel<3, 9, W_PER_EDGE>(SolveArgs))                      \
  X(void kat_wave_kernel<3, 9, W_PER_EDGE>(KatArgs))                        \
  X(void rtr_wave_kernel<3, 10, W_THETA1 | W_PER_EDGE>(SolveArgs))          \
  X(void rtr_wave_kernel<3, 10, W_THETA1 | W_SPREAD | W_PER_EDGE>(SolveArgs)) \
  X(void rtr_wave_kernel<3, 10, W_PER_EDGE>(SolveArgs))                     \
  X(void kat_wave_kernel<3, 10, W_PER_EDGE>(KatArgs))
// ... fixed-anchor formulation
#define GIK_KERNELS_ANCH(X)                                    \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH>(SolveArgs))  \
  X(void kat_wave_kernel<3, 9, W_ANCH>(KatArgs))               \
  X(void rtr_wave_kernel<3, 20, W_THETA1 | W_ANCH>(SolveArgs)) \
  X(void kat_wave_kernel<3, 20, W_ANCH>(KatArgs))
// ... with link hinges (gik_anchored_attach_links, hinges = 1)
#define GIK_KERNELS_ANCH_LINK(X)                                        \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS>(SolveArgs)) \
  X(void kat_wave_kernel<3, 9, W_ANCH | W_LINKS>(KatArgs))
// ... with per-goal obstacle scenes (gik_solve_batch_scenes): the scene builds of the three solve kernels above
#define GIK_KERNELS_ANCH_SCENE(X)                                                        \
  X(void rtr_wave_scene_kernel<3, 9, W_THETA1 | W_ANCH>(SolveArgs, SceneArgs))           \
  X(void rtr_wave_scene_kernel<3, 20, W_THETA1 | W_ANCH>(SolveArgs, SceneArgs))          \
  X(void rtr_wave_scene_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS>(SolveArgs, SceneArgs))
// ... with self hinges (gik_anchored_attach_self_hinges), without and with link hinges: solve, known answers, scenes
// (gik_k_anch_self.hip)
#define GIK_KERNELS_ANCH_SELF(X)                                                                  \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH | W_SELF>(SolveArgs))                            \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS | W_SELF>(SolveArgs))                  \
  X(void kat_wave_kernel<3, 9, W_ANCH | W_SELF>(KatArgs))                                         \
  X(void kat_wave_kernel<3, 9, W_ANCH | W_LINKS | W_SELF>(KatArgs))                               \
  X(void rtr_wave_scene_kernel<3, 9, W_THETA1 | W_ANCH | W_SELF>(SolveArgs, SceneArgs))           \
  X(void rtr_wave_scene_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS | W_SELF>(SolveArgs, SceneArgs))
// ... with half-space obstacles (gik_anchored_attach_halfspaces), without and with link hinges: solve, known answers, scenes
// (gik_k_anch_half.hip)
#define GIK_KERNELS_ANCH_HALF(X)                                                                  \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH | W_HALF>(SolveArgs))                            \
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS | W_HALF>(SolveArgs))                  \
  X(void kat_wave_kernel<3, 9, W_ANCH | W_HALF>(KatArgs))                                         \
  X(void kat_wave_kernel<3, 9, W_ANCH | W_LINKS | W_HALF>(KatArgs))                               \
  X(void rtr_wave_scene_kernel<3, 9, W_THETA1 | W_ANCH | W_HALF>(SolveArgs, SceneArgs))           \
  X(void rtr_wave_scene_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS | W_HALF>(SolveArgs, SceneArgs))
// one unknown per lane, k = 2
#define GIK_KERNELS_WAVE2(X)                          \
  X(void rtr_wave_kernel<2, 6, W_THETA1>(SolveArgs))  \
  X(void rtr_wave_kernel<2, 6, 0>(SolveArgs))         \
  X(void rcg_wave_kernel<2, 6>(SolveArgs))            \
  X(void kat_wave_kernel<2, 6>(KatArgs))              \
  X(void rtr_wave_kernel<2, 16, W_THETA1>(SolveArgs)) \
  X(void rtr_wave_kernel<2, 16, 0>(SolveArgs))        \
  X(void rcg_wave_kernel<2, 16>(SolveArgs))           \
  X(void kat_wave_kernel<2, 16>(KatArgs))             \
  X(void rtr_wave_kernel<2, 31, W_THETA1>(SolveArgs)) \
  X(void rtr_wave_kernel<2, 31, 0>(SolveArgs))        \
  X(void rcg_wave_kernel<2, 31>(SolveArgs))           \
  X(void kat_wave_kernel<2, 31>(KatArgs))
// workgroup per problem
#define GIK_KERNELS_BLOCK(X)                    \
  X(void rtr_block_kernel<2>(SolveArgs, int))   \
  X(void rtr_block_kernel<3>(SolveArgs, int))   \
  X(void rcg_block_kernel<2>(SolveArgs, int))   \
  X(void rcg_block_kernel<3>(SolveArgs, int))   \
  X(void kat_block_kernel<2>(KatArgs, int))     \
  X(void kat_block_kernel<3>(KatArgs, int))
// node per lane
#define GIK_KERNELS_NPT(X)                              \
  X(void rtr_npt_kernel<1, 1, 2, false>(SolveArgs))     \
  X(void kat_npt_kernel<1, 1, 2, false>(KatArgs))       \
  X(void rtr_npt_kernel<4, 1, 2, false>(SolveArgs))     \
  X(void kat_npt_kernel<4, 1, 2, false>(KatArgs))       \
  X(void rtr_npt_kernel<1, 2, 1, false>(SolveArgs))     \
  X(void kat_npt_kernel<1, 2, 1, false>(KatArgs))       \
  X(void rtr_npt_kernel<4, 2, 1, false>(SolveArgs))     \
  X(void kat_npt_kernel<4, 2, 1, false>(KatArgs))
#define GIK_KERNELS_NPT4(X)                             \
  X(void rtr_npt_kernel<1, 1, 4, true>(SolveArgs))      \
  X(void kat_npt_kernel<1, 1, 4, true>(KatArgs))        \
  X(void rtr_npt_kernel<4, 1, 4, true>(SolveArgs))      \
  X(void kat_npt_kernel<4, 1, 4, true>(KatArgs))
// four planar problems / goals per wavefront
#define GIK_KERNELS_QUAD(X)                 \
  X(void rtr_quad_kernel<6>(SolveArgs))     \
  X(void kat_quad_kernel<6>(KatArgs))       \
  X(void prep_quad_kernel<13>(PrepArgs))    \
  X(void prep_quad_kernel<0>(PrepArgs))
// prepare (workgroup per goal); the five plain kernels are defined next to these
#define GIK_KERNELS_PREP(X)                            \
  X(void prep_block_kernel<true>(PrepArgs, double *))  \
  X(void prep_block_kernel<false>(PrepArgs, double *)) \
  X(void prep_block_kernel<false, PREP_BIGN>(PrepArgs, double *))

#define GIK_ALL_KERNELS(X)                                                                                      \
  GIK_KERNELS_WAVE3(X) GIK_KERNELS_WAVE3_STRICT(X) GIK_KERNELS_ANCH(X) GIK_KERNELS_ANCH_LINK(X) GIK_KERNELS_ANCH_SCENE(X) \
  GIK_KERNELS_ANCH_SELF(X) GIK_KERNELS_ANCH_HALF(X)                                                             \
  GIK_KERNELS_WAVE2(X) GIK_KERNELS_BLOCK(X) GIK_KERNELS_NPT(X) GIK_KERNELS_NPT4(X) GIK_KERNELS_QUAD(X) GIK_KERNELS_PREP(X)
