// The augmentation of the reference's training loader for a whole batch of raw scans, in front of the posed voxeliser
// (coordmap.hip, eyoc_voxelize_batched_posed):
//   eyoc_cloud_centroids  the np.mean(pcd, axis=0) of sample_random_trans (lib/data_loaders.py:99), here an fp64 mean
//   eyoc_augment_poses    T_c = [R_c | R_c (-mean_c)] (:93-100) for both clouds of every pair and the pair's pose
//                         T_1 M2 inv(T_0) with its translation scaled (:917, :933)
// All arithmetic is fp64, every operation rounded on its own (no contraction).  Sums are reduced lane -> wave -> workgroup -> cloud in
// an order that depends on nothing but the cloud's own size: a cloud's record has the same bytes alone, anywhere in a batch and on
// every run.  No atomics, no read-back, no allocation: the clouds' offsets travel as kernel arguments, CEN_CLOUDS clouds per launch.
#include "pose_math.h"

using namespace eyoc;

namespace {

constexpr int CEN_BLOCK = 256;
constexpr int CEN_ITEMS = 16;
constexpr int CEN_TILE = CEN_BLOCK * CEN_ITEMS;   // points of one cloud summed by one workgroup
constexpr int CEN_CLOUDS = 64;                    // clouds per pair of launches

struct CloudSegs {
  int n_clouds;
  int pt[CEN_CLOUDS + 1];     // the clouds' first points, counted from the launch's first point
  int tile[CEN_CLOUDS + 1];   // the clouds' first tiles (cdiv(points, CEN_TILE) each), counted from the launch's first tile
};

inline int tiles_of(long long points) { return (int)((points + CEN_TILE - 1) / CEN_TILE); }

// partial[g][3]: the sums of x, y, z over tile g.  Thread t adds points t, t + 256, ... of the tile in that order, lanes fold by
// wave_sum's tree, thread 0 adds the four waves in order.
__global__ __launch_bounds__(CEN_BLOCK) void k_centroid_tiles(CloudSegs s, const float* __restrict__ xyz, int stride,
                                                              double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[CEN_BLOCK / 64][3];
  const int g = blockIdx.x;
  int b = 0;
  while (s.tile[b + 1] <= g) ++b;   // g < tile[n_clouds]; clouds without tiles are stepped over
  const int n = s.pt[b + 1] - s.pt[b];
  const int first = (g - s.tile[b]) * CEN_TILE;
  const float* p = xyz + (size_t)(s.pt[b] + first) * stride;
  const int m = min(CEN_TILE, n - first);
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (int i = threadIdx.x; i < m; i += CEN_BLOCK) {
    ax += (double)p[(size_t)i * stride];
    ay += (double)p[(size_t)i * stride + 1];
    az += (double)p[(size_t)i * stride + 2];
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  az = wave_sum(az);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = ax; red[wave][1] = ay; red[wave][2] = az; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < CEN_BLOCK / 64; ++w) v += red[w][threadIdx.x];
    partial[3 * (size_t)g + threadIdx.x] = v;
  }
}

// one thread per cloud: its tiles in order, then the division
__global__ __launch_bounds__(CEN_CLOUDS) void k_centroid_final(CloudSegs s, const double* __restrict__ partial, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int b = threadIdx.x;
  if (b >= s.n_clouds) return;
  const int n = s.pt[b + 1] - s.pt[b];
  double v[3] = {0.0, 0.0, 0.0};
  for (int g = s.tile[b]; g < s.tile[b + 1]; ++g)
    for (int k = 0; k < 3; ++k) v[k] += partial[3 * (size_t)g + k];
  const double cnt = (double)n;
  for (int k = 0; k < 3; ++k) out[4 * (size_t)b + k] = n > 0 ? v[k] / cnt : 0.0;
  out[4 * (size_t)b + 3] = cnt;
}

// T_c of one cloud (the header's expression): rotation R, translation t_k = (R[k][0] (-m_0) + R[k][1] (-m_1)) + R[k][2] (-m_2)
__device__ inline void cloud_pose(const double* __restrict__ R, const double* __restrict__ c, double T[12]) {
#pragma clang fp contract(off)
  const double m0 = -c[0], m1 = -c[1], m2 = -c[2];
  for (int k = 0; k < 3; ++k) {
    T[4 * k] = R[3 * k];
    T[4 * k + 1] = R[3 * k + 1];
    T[4 * k + 2] = R[3 * k + 2];
    T[4 * k + 3] = (R[3 * k] * m0 + R[3 * k + 1] * m1) + R[3 * k + 2] * m2;
  }
}

__device__ inline void store_pose(double* __restrict__ out, const double T[12]) {
  for (int k = 0; k < 12; ++k) out[k] = T[k];
  out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
}

// one thread per pair
__global__ void k_augment_poses(const double* __restrict__ rot, const double* __restrict__ cen, const double* __restrict__ scale,
                                const double* __restrict__ M2, int n_pairs, double* __restrict__ pose, double* __restrict__ T_gt) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_pairs) return;
  double T0[12], T1[12];
  cloud_pose(rot + 18 * (size_t)b, cen + 8 * (size_t)b, T0);
  cloud_pose(rot + 18 * (size_t)b + 9, cen + 8 * (size_t)b + 4, T1);
  store_pose(pose + 32 * (size_t)b, T0);
  store_pose(pose + 32 * (size_t)b + 16, T1);
  const double* M = M2 + 16 * (size_t)b;
  double A[12], G[12], ti[3];
  for (int i = 0; i < 3; ++i) {   // A = T_1 M2
    for (int j = 0; j < 3; ++j) A[4 * i + j] = (T1[4 * i] * M[j] + T1[4 * i + 1] * M[4 + j]) + T1[4 * i + 2] * M[8 + j];
    A[4 * i + 3] = ((T1[4 * i] * M[3] + T1[4 * i + 1] * M[7]) + T1[4 * i + 2] * M[11]) + T1[4 * i + 3];
  }
  for (int k = 0; k < 3; ++k) ti[k] = -((T0[k] * T0[3] + T0[4 + k] * T0[7]) + T0[8 + k] * T0[11]);   // -R_0^T t_0
  for (int i = 0; i < 3; ++i) {   // G = A [R_0^T | ti]
    for (int j = 0; j < 3; ++j) G[4 * i + j] = (A[4 * i] * T0[4 * j] + A[4 * i + 1] * T0[4 * j + 1]) + A[4 * i + 2] * T0[4 * j + 2];
    G[4 * i + 3] = ((A[4 * i] * ti[0] + A[4 * i + 1] * ti[1]) + A[4 * i + 2] * ti[2]) + A[4 * i + 3];
  }
  if (scale) {
    const double sc = scale[b];
    for (int i = 0; i < 3; ++i) G[4 * i + 3] = sc * G[4 * i + 3];
  }
  store_pose(T_gt + 16 * (size_t)b, G);
}

}  // namespace

extern "C" {

size_t eyoc_cloud_centroids_workspace_bytes(int n_points_total, int n_clouds) {
  if (n_points_total < 0 || n_clouds < 1) return 0;
  return align_up(((size_t)n_points_total / CEN_TILE + (size_t)n_clouds + 1) * 3 * sizeof(double));
}

int eyoc_cloud_centroids(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds, int n_points,
                         double* centroid_dev, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "eyoc_cloud_centroids";
  EYOC_REQUIRE(ctx && point_offsets && centroid_dev, EYOC_ERR_INVALID, "%s: NULL argument", who);
  EYOC_REQUIRE(n_clouds >= 1 && n_clouds <= 1024, EYOC_ERR_INVALID, "%s: %d clouds (1 .. 1024)", who, n_clouds);
  EYOC_REQUIRE(n_points >= 0 && n_points <= (1 << 30) && stride >= 3, EYOC_ERR_INVALID, "%s: %d points in all (0 .. 2^30), stride %d", who,
               n_points, stride);
  EYOC_REQUIRE(point_offsets[0] == 0, EYOC_ERR_INVALID, "%s: point_offsets[0] = %lld", who, (long long)point_offsets[0]);
  for (int b = 0; b < n_clouds; ++b)
    EYOC_REQUIRE(point_offsets[b + 1] >= point_offsets[b], EYOC_ERR_INVALID, "%s: point offsets decrease at cloud %d (%lld -> %lld)", who, b,
                 (long long)point_offsets[b], (long long)point_offsets[b + 1]);
  EYOC_REQUIRE(point_offsets[n_clouds] == n_points, EYOC_ERR_INVALID, "%s: point_offsets[%d] = %lld, not the total %d", who, n_clouds,
               (long long)point_offsets[n_clouds], n_points);
  EYOC_REQUIRE(n_points == 0 || (xyz_dev && ws), EYOC_ERR_INVALID, "%s: NULL argument", who);
  const size_t need = eyoc_cloud_centroids_workspace_bytes(n_points, n_clouds);
  EYOC_REQUIRE(n_points == 0 || (((uintptr_t)ws & 255) == 0 && ws_bytes >= need), EYOC_ERR_WORKSPACE,
               "%s: workspace %zu < required %zu bytes (256-byte aligned)", who, ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  for (int b0 = 0; b0 < n_clouds; b0 += CEN_CLOUDS) {
    CloudSegs s;
    s.n_clouds = n_clouds - b0 < CEN_CLOUDS ? n_clouds - b0 : CEN_CLOUDS;
    s.pt[0] = s.tile[0] = 0;
    for (int b = 0; b < CEN_CLOUDS; ++b) {
      const long long pts = b < s.n_clouds ? point_offsets[b0 + b + 1] - point_offsets[b0 + b] : 0;
      s.pt[b + 1] = s.pt[b] + (int)pts;
      s.tile[b + 1] = s.tile[b] + tiles_of(pts);
    }
    const int tiles = s.tile[s.n_clouds];
    if (tiles > 0)
      hipLaunchKernelGGL(k_centroid_tiles, dim3(tiles), dim3(CEN_BLOCK), 0, st, s, xyz_dev + (size_t)point_offsets[b0] * stride, stride,
                         partial);
    hipLaunchKernelGGL(k_centroid_final, dim3(1), dim3(CEN_CLOUDS), 0, st, s, (const double*)partial, centroid_dev + 4 * (size_t)b0);
    partial += 3 * (size_t)tiles;
  }
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_augment_poses(eyoc_ctx* ctx, const double* rot_dev, const double* centroid_dev, const double* scale_dev, const double* M2_dev,
                       int n_pairs, double* pose_dev, double* T_gt_dev, void* stream) {
  EYOC_REQUIRE(ctx && rot_dev && centroid_dev && M2_dev && pose_dev && T_gt_dev, EYOC_ERR_INVALID, "eyoc_augment_poses: NULL argument");
  EYOC_REQUIRE(n_pairs >= 1 && n_pairs <= 512, EYOC_ERR_INVALID, "eyoc_augment_poses: %d pairs (1 .. 512)", n_pairs);
  hipLaunchKernelGGL(k_augment_poses, dim3(cdiv(n_pairs, 64)), dim3(64), 0, (hipStream_t)stream, rot_dev, centroid_dev, scale_dev, M2_dev,
                     n_pairs, pose_dev, T_gt_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"
