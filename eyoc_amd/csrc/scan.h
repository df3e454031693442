// The flag scan shared by the coordinate maps, the voxeliser (coordmap.hip) and the batch drop (isolate.hip): per-tile sums of 0 / 1
// flags (k_scan_partials), their exclusive scan by one workgroup (k_scan_top); the compaction kernels add the in-tile part themselves.
// The kernels sit in an unnamed namespace: every translation unit that includes this header gets its own copies.
#pragma once

#include "common.h"

namespace {

constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_TILE = SCAN_ITEMS * SCAN_BLOCK;  // 2048 flags per block

__device__ inline int block_exclusive_scan(int v, int* total) {
  __shared__ int wave_sum[SCAN_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
    int s = wave_sum[w];
    if (w < wave) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_partials(const int* __restrict__ flag, int n, int* __restrict__ partial) {
  const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  int s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) s += (base + j < n) ? flag[base + j] : 0;
  int tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// single block: exclusive scan of partial[0..nb) in place, total -> *total
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_top(int* __restrict__ partial, int nb, int* __restrict__ total) {
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += SCAN_BLOCK) {
    int i = b0 + threadIdx.x;
    int v = i < nb ? partial[i] : 0;
    int tot;
    int ex = block_exclusive_scan(v, &tot);
    if (i < nb) partial[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

}  // namespace
