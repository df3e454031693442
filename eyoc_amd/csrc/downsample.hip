// Centroid voxel down-sampling for a batch of clouds: Open3D's PointCloud::VoxelDownSample as the reference calls it
// (util/pointcloud.py:38,43-44), restated as the contract of include/eyoc_hip.h (eyoc_voxel_downsample_batched).
//
// Passes: per-cloud bounds (integer atomics on order-preserving encodings of the floats: min and max commute, so the bytes do not
// depend on the order), grid origin and status per cloud, one 64-bit key per point (cloud | cx | cy | cz), ONE stable radix sort of
// (key, point index), run heads scattered back to point order, the flag scan of scan.h for the row numbers, and the sum pass over the
// runs, which the stable sort left in ascending point order - the contract's sequential fp64 sum (ds_sum_kernel has the two forms).
// No floating-point atomics; nothing of a cloud depends on its neighbours in the batch.
#include "common.h"
#include "scan.h"

namespace eyoc {

constexpr int DS_THREADS = 256;
constexpr int DS_CELL_BITS = 17;                       // a cloud spans at most 2^17 cells on an axis
constexpr int DS_CLOUD_SHIFT = 3 * DS_CELL_BITS;       // key = cloud << 51 | cx << 34 | cy << 17 | cz
constexpr int DS_MAX_ATTR = 8;
constexpr int DS_TILE = 8 * DS_THREADS;                // points per workgroup of the bounds pass
constexpr int DS_SHORT = 16;                           // runs up to this length are summed by their head's lane, longer ones by the wave
constexpr int DS_STAGES = 7;                           // bounds+status, keys, sort, heads, scan, rows+offsets, sums

struct DsWs {
  int64_t* pt_off;              // [B + 1]
  unsigned int *lo, *hi;        // [B][3] encoded minima / maxima
  int* bad;                     // [B] non-finite flag, then the cloud's status
  double* vmin;                 // [B][3]
  int* voff;                    // [B + 1] + the total behind it
  unsigned long long *key, *key_s;
  int *idx, *idx_s, *flag, *excl, *partial;
  void* sort_tmp;
  size_t sort_bytes, total;
};

static DsWs ds_carve(void* base, size_t bytes, int n, int B) {
  DsWs w;
  Carver cv(base, bytes);
  const size_t np = (size_t)n, nb = (size_t)B;
  w.pt_off = cv.take<int64_t>(nb + 1);
  w.lo = cv.take<unsigned int>(nb * 3);
  w.hi = cv.take<unsigned int>(nb * 3);
  w.bad = cv.take<int>(nb);
  w.vmin = cv.take<double>(nb * 3);
  w.voff = cv.take<int>(nb + 2);
  w.key = cv.take<unsigned long long>(np);
  w.key_s = cv.take<unsigned long long>(np);
  w.idx = cv.take<int>(np);
  w.idx_s = cv.take<int>(np);
  w.flag = cv.take<int>(np);
  w.excl = cv.take<int>(np);
  w.partial = cv.take<int>(np / SCAN_TILE + 2);
  w.sort_bytes = align_up(sort_rows64_tmp_bytes(n));
  w.sort_tmp = cv.take<char>(w.sort_bytes);
  w.total = align_up(cv.off);
  return w;
}

// the cloud that owns point i: the last b with pt_off[b] <= i (empty clouds own nothing)
__device__ inline int ds_cloud_of(const int64_t* __restrict__ pt_off, int B, int i) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pt_off[mid] <= (int64_t)i) lo = mid; else hi = mid;
  }
  return lo;
}

// finite floats -> unsigned integers in the same order (-0 and +0 share one code: they give the same origin and the same cells)
__device__ inline unsigned int ds_encode(float v) {
  const unsigned int u = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float ds_decode(unsigned int e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }

__global__ __launch_bounds__(DS_THREADS) void ds_init_kernel(int B, unsigned int* __restrict__ lo, unsigned int* __restrict__ hi,
                                                             int* __restrict__ bad) {
  const int t = blockIdx.x * DS_THREADS + threadIdx.x;
  if (t < 3 * B) {
    lo[t] = 0xFFFFFFFFu;
    hi[t] = 0u;
  }
  if (t < B) bad[t] = 0;
}

// one wave's step over 64 consecutive points: a wave inside one cloud reduces first and issues one set of atomics
__device__ inline void ds_bounds_step(const float* __restrict__ xyz, int n, int stride, const int64_t* __restrict__ pt_off, int B, int i,
                                      unsigned int* __restrict__ lo, unsigned int* __restrict__ hi, int* __restrict__ bad) {
  const bool live = i < n;
  const int b = live ? ds_cloud_of(pt_off, B, i) : -1;
  unsigned int mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  bool finite = true;
  if (live) {
    const float* p = xyz + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    finite = isfinite(x) && isfinite(y) && isfinite(z);
    if (finite) {
      mn[0] = mx[0] = ds_encode(x);
      mn[1] = mx[1] = ds_encode(y);
      mn[2] = mx[2] = ds_encode(z);
    }
  }
  if (live && !finite) atomicOr(bad + b, 1);
  const int b0 = __shfl(b, 0, 64);
  if (__all(b == b0)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        mn[k] = min(mn[k], (unsigned int)__shfl_xor((int)mn[k], d, 64));
        mx[k] = max(mx[k], (unsigned int)__shfl_xor((int)mx[k], d, 64));
      }
    }
    if ((threadIdx.x & 63) == 0 && b0 >= 0 && mn[0] <= mx[0]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        atomicMin(lo + 3 * b0 + k, mn[k]);
        atomicMax(hi + 3 * b0 + k, mx[k]);
      }
    }
  } else if (live && finite) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(lo + 3 * b + k, mn[k]);
      atomicMax(hi + 3 * b + k, mx[k]);
    }
  }
}

// A workgroup owns DS_TILE consecutive points.  A tile inside one cloud (all but a cloud's first and last, at LiDAR sizes) is reduced
// on chip and costs six atomics; one atomic set per wave, the first form of this kernel, spent half the call waiting on a cloud's six
// addresses.  A tile that straddles clouds goes through ds_bounds_step, 64 points at a time.
__global__ __launch_bounds__(DS_THREADS) void ds_bounds_kernel(const float* __restrict__ xyz, int n, int stride,
                                                               const int64_t* __restrict__ pt_off, int B, unsigned int* __restrict__ lo,
                                                               unsigned int* __restrict__ hi, int* __restrict__ bad) {
  __shared__ unsigned int red[DS_THREADS / 64][6];
  const int base = blockIdx.x * DS_TILE, end = min(base + DS_TILE, n);          // base < n by the grid
  const int b_first = ds_cloud_of(pt_off, B, base), b_last = ds_cloud_of(pt_off, B, end - 1);
  if (b_first != b_last) {                                 // block-uniform branch
    for (int j = 0; j < DS_TILE / DS_THREADS; ++j) ds_bounds_step(xyz, n, stride, pt_off, B, base + j * DS_THREADS + threadIdx.x, lo, hi, bad);
    return;
  }
  unsigned int mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  bool all_finite = true;
#pragma unroll
  for (int j = 0; j < DS_TILE / DS_THREADS; ++j) {
    const int i = base + j * DS_THREADS + threadIdx.x;
    if (i < end) {
      const float* p = xyz + (size_t)i * stride;
      const float x = p[0], y = p[1], z = p[2];
      if (isfinite(x) && isfinite(y) && isfinite(z)) {
        const unsigned int e[3] = {ds_encode(x), ds_encode(y), ds_encode(z)};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          mn[k] = min(mn[k], e[k]);
          mx[k] = max(mx[k], e[k]);
        }
      } else {
        all_finite = false;
      }
    }
  }
  if (!all_finite) atomicOr(bad + b_first, 1);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      mn[k] = min(mn[k], (unsigned int)__shfl_xor((int)mn[k], d, 64));
      mx[k] = max(mx[k], (unsigned int)__shfl_xor((int)mx[k], d, 64));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      red[threadIdx.x >> 6][k] = mn[k];
      red[threadIdx.x >> 6][3 + k] = mx[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    unsigned int v = red[0][k];
#pragma unroll
    for (int w = 1; w < DS_THREADS / 64; ++w) v = k < 3 ? min(v, red[w][k]) : max(v, red[w][k]);
    if (k < 3) {
      if (v != 0xFFFFFFFFu) atomicMin(lo + 3 * b_first + k, v);             // (no finite point in the tile: nothing to add)
    } else if (v != 0u) {
      atomicMax(hi + 3 * b_first + (k - 3), v);
    }
  }
}

// grid origin and status of every cloud; bad[b] becomes the status
__global__ __launch_bounds__(DS_THREADS) void ds_status_kernel(const int64_t* __restrict__ pt_off, int B, double voxel,
                                                               const unsigned int* __restrict__ lo, const unsigned int* __restrict__ hi,
                                                               int* __restrict__ bad, double* __restrict__ vmin,
                                                               int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * DS_THREADS + threadIdx.x;
  if (b >= B) return;
  int st = 0;
  double vm[3] = {0.0, 0.0, 0.0};
  if (pt_off[b + 1] > pt_off[b]) {
    if (bad[b]) {
      st = EYOC_ICP_RANGE;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double half = 0.5 * voxel;
        vm[k] = (double)ds_decode(lo[3 * b + k]) - half;
        const double d = (double)ds_decode(hi[3 * b + k]) - vm[k];
        const double q = floor(d / voxel);
        if (!(q < (double)(1 << DS_CELL_BITS))) st = EYOC_ICP_RANGE;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) vmin[3 * b + k] = vm[k];
  bad[b] = st;
  status[b] = st;
}

__global__ __launch_bounds__(DS_THREADS) void ds_keys_kernel(const float* __restrict__ xyz, int n, int stride,
                                                             const int64_t* __restrict__ pt_off, int B, double voxel,
                                                             const int* __restrict__ bad, const double* __restrict__ vmin,
                                                             unsigned long long* __restrict__ key, int* __restrict__ idx) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * DS_THREADS + threadIdx.x;
  if (i >= n) return;
  const int b = ds_cloud_of(pt_off, B, i);
  unsigned long long k = (unsigned long long)b << DS_CLOUD_SHIFT;
  if (!bad[b]) {
    const float* p = xyz + (size_t)i * stride;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double d = (double)p[a] - vmin[3 * b + a];
      const double q = floor(d / voxel);                  // 0 <= q < 2^17: the status pass checked the cloud's largest point
      k |= ((unsigned long long)(long long)q & ((1ull << DS_CELL_BITS) - 1)) << ((2 - a) * DS_CELL_BITS);
    }
  }
  key[i] = k;
  idx[i] = i;
}

__device__ inline bool ds_is_head(const unsigned long long* __restrict__ key_s, int j, unsigned long long k) {
  return j == 0 || key_s[j - 1] != k;
}

// run heads back to point order (idx_s is a permutation: every flag is written); a refused cloud has no heads and inverse -1
__global__ __launch_bounds__(DS_THREADS) void ds_heads_kernel(const unsigned long long* __restrict__ key_s, const int* __restrict__ idx_s,
                                                              int n, const int* __restrict__ bad, int* __restrict__ flag,
                                                              int32_t* __restrict__ inverse) {
  const int j = blockIdx.x * DS_THREADS + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = key_s[j];
  const int i = idx_s[j];
  const bool refused = bad[(int)(k >> DS_CLOUD_SHIFT)] != 0;
  flag[i] = (!refused && ds_is_head(key_s, j, k)) ? 1 : 0;
  if (refused && inverse) inverse[i] = -1;
}

// excl[i] = flags before point i (global row of a head); first[row] = the head's index within its cloud
__global__ __launch_bounds__(SCAN_BLOCK) void ds_rows_kernel(const int* __restrict__ flag, const int* __restrict__ partial, int n,
                                                             const int64_t* __restrict__ pt_off, int B, int* __restrict__ excl,
                                                             int32_t* __restrict__ first) {
  const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  int f[SCAN_ITEMS];
  int s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    f[j] = (base + j < n) ? flag[base + j] : 0;
    s += f[j];
  }
  int tot;
  int pos = partial[blockIdx.x] + block_exclusive_scan(s, &tot);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const int i = base + j;
    if (i >= n) break;
    excl[i] = pos;
    if (f[j]) {
      if (first) first[pos] = i - (int)pt_off[ds_cloud_of(pt_off, B, i)];
      ++pos;
    }
  }
}

__global__ __launch_bounds__(DS_THREADS) void ds_offsets_kernel(const int64_t* __restrict__ pt_off, int B, int n,
                                                                const int* __restrict__ excl, int* __restrict__ voff) {
  const int b = blockIdx.x * DS_THREADS + threadIdx.x;
  if (b > B) return;
  const int64_t p = pt_off[b];
  voff[b] = p < (int64_t)n ? excl[p] : voff[B + 1];       // voff[B + 1]: the scan's total
}

// Sums.  The lane at a run's head owns the run; the stable sort left it in ascending point order, the contract's order.
//   runs of at most DS_SHORT points   the lane walks its run: the loads of a step do not depend on the step before, only the adds do
//   longer runs                       one after the other, by the whole wave: 64 points are gathered at once, one per lane, and every
//                                     lane then adds them in order from the others' registers (the same fp64 adds, in the same order,
//                                     sixty-four times over: what is saved is the chain of dependent gathers - at 0.3 m a KITTI-shaped
//                                     scan has runs of ~1000 points next to the sensor, and one lane walking them was the whole pass)
struct DsSumArgs {
  const unsigned long long* key_s;
  const int *idx_s, *bad, *excl, *voff;
  const float *xyz, *attr;
  float *xyz_out, *attr_out;
  int32_t *count, *inverse;
  int n, stride, n_attr;
};

__device__ inline void ds_write_row(const DsSumArgs& a, int row, int cnt, const double* s, const double* sa) {
  const double m = (double)cnt;
  a.xyz_out[3 * (size_t)row] = (float)(s[0] / m);
  a.xyz_out[3 * (size_t)row + 1] = (float)(s[1] / m);
  a.xyz_out[3 * (size_t)row + 2] = (float)(s[2] / m);
  if (a.attr) {
#pragma unroll
    for (int c = 0; c < DS_MAX_ATTR; ++c)
      if (c < a.n_attr) a.attr_out[(size_t)row * a.n_attr + c] = (float)(sa[c] / m);
  }
  if (a.count) a.count[row] = cnt;
}

__global__ __launch_bounds__(DS_THREADS) void ds_sum_kernel(const DsSumArgs a) {
  const int j = blockIdx.x * DS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  const int n = a.n;
  unsigned long long k = 0;
  bool head = false;
  if (j < n) {
    k = a.key_s[j];
    head = !a.bad[(int)(k >> DS_CLOUD_SHIFT)] && ds_is_head(a.key_s, j, k);
  }
  // the run's length, up to DS_SHORT + 1: independent loads
  int len = 0;
  if (head) {
    unsigned int same = 1;
#pragma unroll
    for (int q = 1; q <= DS_SHORT; ++q) same |= (unsigned int)(j + q < n && a.key_s[min(j + q, n - 1)] == k) << q;
    len = __ffs((int)~same) - 1;                           // the first q that left the run; DS_SHORT + 1: a long run
  }
  int row = 0, local = 0;
  if (head) {
    row = a.excl[a.idx_s[j]];
    local = row - a.voff[(int)(k >> DS_CLOUD_SHIFT)];
  }
  if (head && len <= DS_SHORT) {
    double s[3] = {0.0, 0.0, 0.0}, sa[DS_MAX_ATTR] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int q = 0; q < len; ++q) {
      const int i = a.idx_s[j + q];
      const float* p = a.xyz + (size_t)i * a.stride;
      s[0] += (double)p[0];
      s[1] += (double)p[1];
      s[2] += (double)p[2];
      if (a.attr) {
        const float* at = a.attr + (size_t)i * a.n_attr;
#pragma unroll
        for (int c = 0; c < DS_MAX_ATTR; ++c)
          if (c < a.n_attr) sa[c] += (double)at[c];
      }
      if (a.inverse) a.inverse[i] = local;
    }
    ds_write_row(a, row, len, s, sa);
  }
  // long runs: every lane of the wave arrives here
  unsigned long long todo = __ballot(head && len > DS_SHORT);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int j0 = __shfl(j, src, 64), row0 = __shfl(row, src, 64), local0 = __shfl(local, src, 64);
    const unsigned long long k0 = ((unsigned long long)(unsigned int)__shfl((int)(k >> 32), src, 64) << 32) |
                                  (unsigned int)__shfl((int)(unsigned int)k, src, 64);
    double s[3] = {0.0, 0.0, 0.0}, sa[DS_MAX_ATTR] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cnt = 0;
    for (int t0 = j0;; t0 += 64) {
      const int t = t0 + lane;
      const bool in = t < n && a.key_s[min(t, n - 1)] == k0;          // a prefix of the lanes: the run is contiguous
      float v[3] = {0.0f, 0.0f, 0.0f}, va[DS_MAX_ATTR] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (in) {
        const int i = a.idx_s[t];
        const float* p = a.xyz + (size_t)i * a.stride;
        v[0] = p[0];
        v[1] = p[1];
        v[2] = p[2];
        if (a.attr) {
          const float* at = a.attr + (size_t)i * a.n_attr;
#pragma unroll
          for (int c = 0; c < DS_MAX_ATTR; ++c)
            if (c < a.n_attr) va[c] = at[c];
        }
        if (a.inverse) a.inverse[i] = local0;
      }
      const int m = __popcll(__ballot(in));
      for (int l = 0; l < m; ++l) {                        // l is wave-uniform: the reads below are lane broadcasts
        s[0] += (double)__shfl(v[0], l, 64);
        s[1] += (double)__shfl(v[1], l, 64);
        s[2] += (double)__shfl(v[2], l, 64);
        if (a.attr) {
#pragma unroll
          for (int c = 0; c < DS_MAX_ATTR; ++c)
            if (c < a.n_attr) sa[c] += (double)__shfl(va[c], l, 64);
        }
      }
      cnt += m;
      if (m < 64) break;
    }
    if (lane == 0) ds_write_row(a, row0, cnt, s, sa);
  }
}

static int ds_run(eyoc_ctx* ctx, const float* xyz, int stride, const int64_t* point_offsets, int B, int n, double voxel, const float* attr,
                  int n_attr, float* xyz_out, float* attr_out, int32_t* first, int32_t* count, int32_t* inverse, int32_t* status,
                  int64_t* voxel_offsets, void* ws, size_t ws_bytes, hipStream_t st, float* stage_ms) {
  const DsWs w = ds_carve(ws, ws_bytes, n, B);
  const size_t up_bytes = align_up((size_t)(B + 1) * 8);
  EYOC_REQUIRE(up_bytes + (size_t)(B + 1) * 4 <= ctx->pinned_bytes, EYOC_ERR_INVALID,
               "eyoc_voxel_downsample_batched: %d clouds exceed the pinned staging", B);
  int64_t* up = (int64_t*)ctx->pinned;
  int* host = (int*)((char*)ctx->pinned + up_bytes);
  hipEvent_t ev[DS_STAGES + 1] = {};
  int n_ev = 0;
  auto mark = [&]() {                                     // stage boundaries of the timed call only
    if (stage_ms && n_ev <= DS_STAGES && hipEventCreate(&ev[n_ev]) == hipSuccess) (void)hipEventRecord(ev[n_ev++], st);
  };
  memcpy(up, point_offsets, (size_t)(B + 1) * 8);
  EYOC_CHECK_HIP(hipMemcpyAsync(w.pt_off, up, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
  const dim3 pg(cdiv(n, DS_THREADS)), cg(cdiv(B + 1, DS_THREADS)), tb(DS_THREADS);
  mark();
  hipLaunchKernelGGL(ds_init_kernel, dim3(cdiv(3 * B, DS_THREADS)), tb, 0, st, B, w.lo, w.hi, w.bad);
  hipLaunchKernelGGL(ds_bounds_kernel, dim3(cdiv(n, DS_TILE)), tb, 0, st, xyz, n, stride, (const int64_t*)w.pt_off, B, w.lo, w.hi, w.bad);
  hipLaunchKernelGGL(ds_status_kernel, cg, tb, 0, st, (const int64_t*)w.pt_off, B, voxel, (const unsigned int*)w.lo,
                     (const unsigned int*)w.hi, w.bad, w.vmin, status);
  mark();
  hipLaunchKernelGGL(ds_keys_kernel, pg, tb, 0, st, xyz, n, stride, (const int64_t*)w.pt_off, B, voxel, (const int*)w.bad,
                     (const double*)w.vmin, w.key, w.idx);
  mark();
  int cloud_bits = 0;
  while ((1 << cloud_bits) < B) ++cloud_bits;
  // equal keys keep their input order: inside a run the point indices ascend, and its head is the voxel's lowest point
  if (int rc = sort_rows_by_key64(w.sort_tmp, w.sort_bytes, w.key, w.key_s, w.idx, w.idx_s, n, DS_CLOUD_SHIFT + cloud_bits, st)) return rc;
  mark();
  hipLaunchKernelGGL(ds_heads_kernel, pg, tb, 0, st, (const unsigned long long*)w.key_s, (const int*)w.idx_s, n, (const int*)w.bad, w.flag,
                     inverse);
  mark();
  const int nb = cdiv(n, SCAN_TILE);
  hipLaunchKernelGGL(k_scan_partials, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const int*)w.flag, n, w.partial);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_BLOCK), 0, st, w.partial, nb, w.voff + B + 1);
  mark();
  hipLaunchKernelGGL(ds_rows_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const int*)w.flag, (const int*)w.partial, n,
                     (const int64_t*)w.pt_off, B, w.excl, first);
  hipLaunchKernelGGL(ds_offsets_kernel, cg, tb, 0, st, (const int64_t*)w.pt_off, B, n, (const int*)w.excl, w.voff);
  mark();
  const DsSumArgs sum_args{w.key_s, w.idx_s, w.bad, w.excl, w.voff, xyz, attr, xyz_out, attr_out, count, inverse, n, stride, n_attr};
  hipLaunchKernelGGL(ds_sum_kernel, pg, tb, 0, st, sum_args);
  mark();
  EYOC_CHECK_HIP(hipGetLastError());
  EYOC_CHECK_HIP(hipMemcpyAsync(host, w.voff, (size_t)(B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
  EYOC_CHECK_HIP(hipStreamSynchronize(st));
  for (int b = 0; b <= B; ++b) voxel_offsets[b] = host[b];
  if (stage_ms) {
    for (int s = 0; s < DS_STAGES; ++s) {
      stage_ms[s] = -1.0f;
      if (s + 1 < n_ev) (void)hipEventElapsedTime(&stage_ms[s], ev[s], ev[s + 1]);
    }
    for (int s = 0; s < n_ev; ++s) (void)hipEventDestroy(ev[s]);
  }
  return EYOC_OK;
}

static int ds_call(eyoc_ctx* ctx, const float* xyz, int stride, const int64_t* point_offsets, int B, int n, double voxel, const float* attr,
                   int n_attr, float* xyz_out, float* attr_out, int32_t* first, int32_t* count, int32_t* inverse, int32_t* status,
                   int64_t* voxel_offsets, void* ws, size_t ws_bytes, void* stream, float* stage_ms) {
  const char* who = "eyoc_voxel_downsample_batched";
  EYOC_REQUIRE(ctx && point_offsets && voxel_offsets, EYOC_ERR_INVALID, "%s: NULL argument", who);
  EYOC_REQUIRE(B >= 1 && B <= 1024, EYOC_ERR_INVALID, "%s: %d clouds (1 .. 1024)", who, B);
  EYOC_REQUIRE(n >= 0 && n <= (1 << 30), EYOC_ERR_INVALID, "%s: %d points in all (0 .. 2^30)", who, n);
  EYOC_REQUIRE((stride == 3 || stride == 4) && voxel > 0.0 && voxel <= 1.7976931348623157e308, EYOC_ERR_INVALID,
               "%s: stride %d voxel %g", who, stride, voxel);
  EYOC_REQUIRE(n_attr >= 0 && n_attr <= DS_MAX_ATTR, EYOC_ERR_INVALID, "%s: %d attribute columns (0 .. %d)", who, n_attr, DS_MAX_ATTR);
  EYOC_REQUIRE(point_offsets[0] == 0, EYOC_ERR_INVALID, "%s: point_offsets[0] = %lld", who, (long long)point_offsets[0]);
  for (int b = 0; b < B; ++b)
    EYOC_REQUIRE(point_offsets[b + 1] >= point_offsets[b], EYOC_ERR_INVALID, "%s: point offsets decrease at cloud %d (%lld -> %lld)", who, b,
                 (long long)point_offsets[b], (long long)point_offsets[b + 1]);
  EYOC_REQUIRE(point_offsets[B] == n, EYOC_ERR_INVALID, "%s: point_offsets[%d] = %lld, not the total %d", who, B,
               (long long)point_offsets[B], n);
  if (n == 0) {                                           // every cloud empty: nothing to launch, nothing written on the device
    for (int b = 0; b <= B; ++b) voxel_offsets[b] = 0;
    if (stage_ms) for (int s = 0; s < DS_STAGES; ++s) stage_ms[s] = 0.0f;
    return EYOC_OK;
  }
  if (n_attr == 0) attr = nullptr;
  EYOC_REQUIRE(xyz && xyz_out && status && ws && (!attr || attr_out), EYOC_ERR_INVALID, "%s: NULL argument", who);
  const size_t need = eyoc_voxel_downsample_workspace_bytes(n, B, n_attr);
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0 && ws_bytes >= need, EYOC_ERR_WORKSPACE,
               "%s: workspace %zu < required %zu bytes (256-byte aligned)", who, ws_bytes, need);
  return ds_run(ctx, xyz, stride, point_offsets, B, n, voxel, attr, n_attr, xyz_out, attr_out, first, count, inverse, status, voxel_offsets,
                ws, ws_bytes, (hipStream_t)stream, stage_ms);
}

}  // namespace eyoc

using namespace eyoc;

extern "C" {

size_t eyoc_voxel_downsample_workspace_bytes(int n_points_total, int n_clouds, int n_attr) {
  if (n_points_total <= 0 || n_clouds < 1 || n_attr < 0) return 0;
  return ds_carve(nullptr, 0, n_points_total, n_clouds).total;      // the attributes are summed in registers: n_attr adds nothing
}

int eyoc_voxel_downsample_batched(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds, int n_points,
                                  double voxel_size, const float* attr_dev, int n_attr, float* xyz_out_dev, float* attr_out_dev,
                                  int32_t* first_dev, int32_t* count_dev, int32_t* inverse_dev, int32_t* status_dev,
                                  int64_t* voxel_offsets, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return ds_call(ctx, xyz_dev, stride, point_offsets, n_clouds, n_points, voxel_size, attr_dev, n_attr, xyz_out_dev, attr_out_dev,
                 first_dev, count_dev, inverse_dev, status_dev, voxel_offsets, workspace_dev, workspace_bytes, stream, nullptr);
}

int eyoc_voxel_downsample_batched_timed(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds,
                                        int n_points, double voxel_size, const float* attr_dev, int n_attr, float* xyz_out_dev,
                                        float* attr_out_dev, int32_t* first_dev, int32_t* count_dev, int32_t* inverse_dev,
                                        int32_t* status_dev, int64_t* voxel_offsets, void* workspace_dev, size_t workspace_bytes,
                                        void* stream, float* stage_ms) {
  EYOC_REQUIRE(stage_ms, EYOC_ERR_INVALID, "eyoc_voxel_downsample_batched_timed: NULL stage_ms");
  return ds_call(ctx, xyz_dev, stride, point_offsets, n_clouds, n_points, voxel_size, attr_dev, n_attr, xyz_out_dev, attr_out_dev,
                 first_dev, count_dev, inverse_dev, status_dev, voxel_offsets, workspace_dev, workspace_bytes, stream, stage_ms);
}

}  // extern "C"
