// graphik_amd/csrc/gik_order.hip.h -- claim order of a batch: which problem each ticket of the solve kernels' work
// counter stands for (SolveArgs::claim_order, NOTEBOOK 21).
//
//   claim_key_kernel  : one thread per problem: key[b] = sum_i w_i targets[b][term_i] over the template's short term
//                       list (gik_template_set_claim_key), in double, stored as float.
//   claim_rank_kernel : the permutation that sorts the keys ascending, by counting: problem i goes to position
//                       #{j : (key_j, j) < (key_i, i)}.  The pairs are distinct, so the positions are a permutation
//                       whatever the keys hold; ties come out in index order and NaN keys last (they map to the
//                       largest code).  Deterministic: no atomics, every position is written by exactly one thread.
//                       B^2 comparisons on LDS broadcasts -- 64 problems x 4 quarters of the key array per workgroup,
//                       ~10 us at 4096 problems, a few hundred at PLAN_CLAIM_ORDER_MAX_BATCH, beyond which the plan
//                       keeps index order (gik_plan.h).
// Plain kernels, defined where GIK_DEFINE_ORDER_KERNELS is set (gik_k_order.hip); the host units see prototypes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gik_args.h"

namespace gik {

constexpr int ORDER_ROWS = 64;                      // problems per workgroup of claim_rank_kernel
constexpr int ORDER_PARTS = 4;                      // ... each against a quarter of the keys per wavefront
constexpr int ORDER_NT = ORDER_ROWS * ORDER_PARTS;
constexpr int ORDER_TILE = 1024;                    // key codes staged in LDS at a time

struct ClaimKey {
  int n = 0;                            // 0: index order
  int term[CLAIM_KEY_MAX_TERMS] = {};   // each within [0, T)
  double w[CLAIM_KEY_MAX_TERMS] = {};
};

// float -> unsigned code with the same order; every NaN -> the largest code
__host__ __device__ inline uint32_t claim_key_code(float k) {
  if (k != k) return 0xffffffffu;
  union { float f; uint32_t u; } v;
  v.f = k == 0.0f ? 0.0f : k;      // (-0 -> +0: equal keys, equal codes)
  return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}

#ifdef GIK_DEFINE_ORDER_KERNELS
__global__ void __launch_bounds__(256) claim_key_kernel(const double *targets, int T, int B, ClaimKey k, float *key) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < k.n; ++i) s += k.w[i] * targets[(size_t)b * T + k.term[i]];
  key[b] = (float)s;
}

__global__ void __launch_bounds__(ORDER_NT) claim_rank_kernel(const float *key, int B, int *order) {
  __shared__ uint32_t sh_code[ORDER_TILE];
  __shared__ int sh_cnt[ORDER_PARTS][ORDER_ROWS];
  const int row = (int)threadIdx.x % ORDER_ROWS, part = (int)threadIdx.x / ORDER_ROWS;
  const int i = (int)blockIdx.x * ORDER_ROWS + row;
  const uint64_t mine = i < B ? ((uint64_t)claim_key_code(key[i]) << 32) | (uint32_t)i : 0;
  int cnt = 0;
  for (int j0 = 0; j0 < B; j0 += ORDER_TILE) {
    const int n = min(ORDER_TILE, B - j0);
    __syncthreads();      // (the previous tile has been read)
    for (int j = (int)threadIdx.x; j < n; j += ORDER_NT) sh_code[j] = claim_key_code(key[j0 + j]);
    __syncthreads();
    // this wavefront's quarter of the tile; every lane reads the same word: an LDS broadcast
    const int q = (n + ORDER_PARTS - 1) / ORDER_PARTS, lo = part * q, hi = min(n, lo + q);
    for (int j = lo; j < hi; ++j) cnt += ((((uint64_t)sh_code[j] << 32) | (uint32_t)(j0 + j)) < mine) ? 1 : 0;
  }
  sh_cnt[part][row] = cnt;
  __syncthreads();
  if (part == 0 && i < B) {
    int pos = 0;
    for (int p = 0; p < ORDER_PARTS; ++p) pos += sh_cnt[p][row];
    order[pos] = i;       // pos < B: at most B - 1 pairs are smaller than this one
  }
}
#else
__global__ void claim_key_kernel(const double *targets, int T, int B, ClaimKey k, float *key);
__global__ void claim_rank_kernel(const float *key, int B, int *order);
#endif

}  // namespace gik
