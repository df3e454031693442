// The metrics of the reference's validation loop (lib/trainer.py:362-378 of `_valid_epoch`) for every pair of a batch at once:
// corr_dist (lib/metrics.py:13-19, weight None) over the pair's full source cloud, the hit ratio of its correspondences
// (evaluate_hit_ratio, lib/trainer.py:421-424), RTE and RRE (:365-368, no clamp: a cosine outside [-1, 1] is a NaN the loop skips).
// One workgroup per pair, VM_CHUNK pairs per launch, one 64-byte eyoc_valid_record per pair; nothing is read back.  All arithmetic is
// fp64 on the fp32 inputs without contraction, and every sum is reduced lane -> wave -> workgroup in a fixed order: a pair's record has
// the same bytes alone, in any batch and on every run.  The poses are read where eyoc_irls_quad_batched wrote them.
#include "pose_math.h"

using namespace eyoc;

namespace {

constexpr int VM_THREADS = 1024;
constexpr int VM_CHUNK = 64;

struct ValidSegs {
  int n_seg;
  int r0[VM_CHUNK], n0[VM_CHUNK];   // first row and row count of the pair's correspondences (p0, idx1)
  int r1[VM_CHUNK], n1[VM_CHUNK];   // ... of its p1 segment
  int rx[VM_CHUNK], nx[VM_CHUNK];   // ... of its full source cloud
};

__device__ inline int wave_sum_int(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // valid in lane 0
}

__global__ __launch_bounds__(VM_THREADS) void valid_metrics_kernel(ValidSegs s, const float* __restrict__ p0, const float* __restrict__ p1,
                                                                   const long long* __restrict__ idx1, const float* __restrict__ x0,
                                                                   const float* __restrict__ T_est, const float* __restrict__ T_gt,
                                                                   double hit_thresh, double max_dist,
                                                                   eyoc_valid_record* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red_d[VM_THREADS / 64];
  __shared__ int red_i[VM_THREADS / 64];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = s.n0[b], n1 = s.n1[b], nx = s.nx[b];
  double E[12], G[12];
  bool finite = true;
  for (int k = 0; k < 16; ++k) {
    const float e = T_est[16 * (size_t)b + k];
    finite = finite && isfinite(e);
    if (k < 12) { E[k] = e; G[k] = T_gt[16 * (size_t)b + k]; }
  }
  // hits: sqrt(|R_gt p0 + t_gt - p1[idx1]|^2 + 1e-6) < hit_thresh.  An index outside the pair's p1 segment is clamped into it BEFORE it
  // becomes an address (a pair with correspondences and no p1 rows reads nothing) and marks the pair.
  int hits = 0, bad = (n > 0 && n1 == 0);
  if (n1 > 0) {
    const float* a = p0 + 3 * (size_t)s.r0[b];
    const float* q1 = p1 + 3 * (size_t)s.r1[b];
    const long long* ix = idx1 ? idx1 + s.r0[b] : nullptr;
    for (int i = threadIdx.x; i < n; i += VM_THREADS) {
      long long j = ix ? ix[i] : (long long)i;
      if (j < 0 || j >= (long long)n1) {
        bad = 1;
        j = j < 0 ? 0 : (long long)n1 - 1;
      }
      const double ox = a[3 * i], oy = a[3 * i + 1], oz = a[3 * i + 2];
      const float* q = q1 + 3 * (size_t)j;
      const double gx = (G[0] * ox + G[1] * oy + G[2] * oz + G[3]) - (double)q[0];
      const double gy = (G[4] * ox + G[5] * oy + G[6] * oz + G[7]) - (double)q[1];
      const double gz = (G[8] * ox + G[9] * oy + G[10] * oz + G[11]) - (double)q[2];
      hits += sqrt(gx * gx + gy * gy + gz * gz + 1e-6) < hit_thresh ? 1 : 0;
    }
  }
  // loss: mean over the full cloud of min(|T_est x - T_gt x|, max_dist)
  double acc = 0.0;
  if (finite) {
    const float* x = x0 + 3 * (size_t)s.rx[b];
    for (int i = threadIdx.x; i < nx; i += VM_THREADS) {
      const double ox = x[3 * i], oy = x[3 * i + 1], oz = x[3 * i + 2];
      const double ex = (E[0] * ox + E[1] * oy + E[2] * oz + E[3]) - (G[0] * ox + G[1] * oy + G[2] * oz + G[3]);
      const double ey = (E[4] * ox + E[5] * oy + E[6] * oz + E[7]) - (G[4] * ox + G[5] * oy + G[6] * oz + G[7]);
      const double ez = (E[8] * ox + E[9] * oy + E[10] * oz + E[11]) - (G[8] * ox + G[9] * oy + G[10] * oz + G[11]);
      const double d = sqrt(ex * ex + ey * ey + ez * ez);
      acc += d < max_dist ? d : max_dist;
    }
  }
  acc = wave_sum(acc);
  hits = wave_sum_int(hits);
  if (lane == 0) { red_d[wave] = acc; red_i[wave] = hits; }
  const int any_bad = __syncthreads_or(bad);   // (also the barrier between the writes above and thread 0's reads)
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  int cnt = 0;
  for (int w = 0; w < VM_THREADS / 64; ++w) { sum += red_d[w]; cnt += red_i[w]; }
  const double nan = __builtin_nan("");
  eyoc_valid_record r;
  r.status = (n == 0 ? EYOC_VALID_EMPTY : 0u) | (any_bad ? EYOC_VALID_BAD_INDEX : 0u) | (finite ? 0u : EYOC_VALID_POSE_NONFINITE);
  r.n_corr = n;
  r.n_points = nx;
  r.hits = any_bad ? 0 : cnt;
  r.hit_ratio = (n == 0 || any_bad) ? nan : (double)cnt / (double)n;
  r.loss = (finite && nx > 0 && n > 0) ? sum / (double)nx : nan;
  const double dx = E[3] - G[3], dy = E[7] - G[7], dz = E[11] - G[11];
  r.rte = finite ? sqrt(dx * dx + dy * dy + dz * dz) : nan;
  double tr = 0.0;   // trace(R_est^T R_gt) = sum_ij R_est[i][j] R_gt[i][j], row by row
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) tr += E[4 * i + j] * G[4 * i + j];
  r.cos_rre = (tr - 1.0) / 2.0;
  r.rre = (finite && r.cos_rre >= -1.0 && r.cos_rre <= 1.0) ? acos(r.cos_rre) : nan;
  r.reserved = 0.0;
  out[b] = r;
}

}  // namespace

extern "C" {

int eyoc_valid_metrics_batched(eyoc_ctx* ctx, const float* p0_dev, const float* p1_dev, const int64_t* idx1_dev,
                               const int32_t* seg0_host, const int32_t* seg1_host, const float* x0_dev, const int32_t* segx_host, int nseg,
                               const float* T_est_dev, const float* T_gt_dev, double hit_thresh, double max_dist,
                               eyoc_valid_record* records_dev, void* stream) {
  static_assert(sizeof(eyoc_valid_record) == 64, "eyoc_valid_record is 64 bytes");
  EYOC_REQUIRE(ctx && seg0_host && seg1_host && segx_host && T_est_dev && T_gt_dev && records_dev, EYOC_ERR_INVALID,
               "eyoc_valid_metrics_batched: NULL argument");
  EYOC_REQUIRE(nseg >= 1 && nseg <= 1024, EYOC_ERR_INVALID, "eyoc_valid_metrics_batched: nseg = %d is outside [1, 1024]", nseg);
  EYOC_REQUIRE(seg0_host[0] == 0 && seg1_host[0] == 0 && segx_host[0] == 0, EYOC_ERR_INVALID,
               "eyoc_valid_metrics_batched: segments must start at 0");
  for (int b = 0; b < nseg; ++b) {
    EYOC_REQUIRE(seg0_host[b + 1] >= seg0_host[b] && seg1_host[b + 1] >= seg1_host[b] && segx_host[b + 1] >= segx_host[b],
                 EYOC_ERR_INVALID, "eyoc_valid_metrics_batched: segment offsets must not decrease (pair %d)", b);
    EYOC_REQUIRE(idx1_dev || seg1_host[b + 1] == seg0_host[b + 1], EYOC_ERR_INVALID,
                 "eyoc_valid_metrics_batched: without idx1 row i pairs with row i, and the segments of pair %d differ", b);
  }
  if (seg0_host[nseg] > 0) EYOC_REQUIRE(p0_dev && p1_dev, EYOC_ERR_INVALID, "eyoc_valid_metrics_batched: NULL argument");
  if (segx_host[nseg] > 0) EYOC_REQUIRE(x0_dev, EYOC_ERR_INVALID, "eyoc_valid_metrics_batched: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  ValidSegs s;
  for (int b0 = 0; b0 < nseg; b0 += VM_CHUNK) {
    s.n_seg = nseg - b0 < VM_CHUNK ? nseg - b0 : VM_CHUNK;
    for (int b = 0; b < VM_CHUNK; ++b) {
      const int k = b < s.n_seg ? b0 + b : -1;
      s.r0[b] = k < 0 ? 0 : seg0_host[k]; s.n0[b] = k < 0 ? 0 : seg0_host[k + 1] - seg0_host[k];
      s.r1[b] = k < 0 ? 0 : seg1_host[k]; s.n1[b] = k < 0 ? 0 : seg1_host[k + 1] - seg1_host[k];
      s.rx[b] = k < 0 ? 0 : segx_host[k]; s.nx[b] = k < 0 ? 0 : segx_host[k + 1] - segx_host[k];
    }
    hipLaunchKernelGGL(valid_metrics_kernel, dim3(s.n_seg), dim3(VM_THREADS), 0, st, s, p0_dev, p1_dev, (const long long*)idx1_dev, x0_dev,
                       T_est_dev + 16 * (size_t)b0, T_gt_dev + 16 * (size_t)b0, hit_thresh, max_dist, records_dev + b0);
  }
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"
