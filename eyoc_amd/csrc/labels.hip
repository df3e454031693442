// Label-generation kernels: the EYOC-specific matching filters of lib/trainer.py:993-1151
// (Lowe ratio weights on the two nearest feature neighbours, top-k by weight, spherical filter) and the
// pose-consistency filter of lib/trainer.py:1199-1218.  The nearest neighbours themselves come from
// eyoc_knn2 / eyoc_knn1 (knn.hip).
#include "common.h"

using namespace eyoc;

namespace {

// lib/trainer.py:993-1010 + :1066-1070 in the reference's own order of fp32 operations:
//   cosine = 1 - 0.5 * dist;  x = clamp(1 - cosine, min = 1e-9);  ratio = x0 / x1;  weight = 1 - ratio.
// The sort key orders floats descending (radix sort ascending on the key), ties keep the input order.
__global__ void k_lowe_weight(const float* __restrict__ d1, const float* __restrict__ d2, int n, float* __restrict__ w,
                              unsigned int* __restrict__ key, int* __restrict__ row) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float c1 = 1.0f - 0.5f * d1[i], c2 = 1.0f - 0.5f * d2[i];
  const float x1 = fmaxf(1.0f - c1, 1e-9f), x2 = fmaxf(1.0f - c2, 1e-9f);
  const float wt = 1.0f - x1 / x2;
  w[i] = wt;
  unsigned int u = __float_as_uint(wt);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending float order
  key[i] = ~u;                                        // descending
  row[i] = i;
}

__global__ void k_take_topk(const int* __restrict__ sorted_row, const float* __restrict__ w, int k, long long* __restrict__ idx_out,
                            float* __restrict__ w_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int r = sorted_row[i];
  idx_out[i] = r;
  if (w_out) w_out[i] = w[r];
}

__device__ inline float norm3(float x, float y, float z) {
#pragma clang fp contract(off)
  return sqrtf((x * x + y * y) + z * z);
}

// mode 0 (lib/trainer.py:1107-1110): keep pair i iff |P0[i0]| > radius and |P1[i1]| > radius.
// mode 1 (lib/trainer.py:1203-1206): keep iff |R P0[i0] + t - P1[i1]| < radius, T row-major 4x4.
// mode 2 (lib/trainer.py:1118-1149, "Similarity"): d0 = |P0[i0]|, d1 = |P1[i1]|; look the pair up in the
//         distance-similarity table at [min(int(|d0 - d1| / g1), xlim - 1)][min(int(min(d0, d1) / g0), ylim - 1)] and keep it
//         iff the entry exceeds the threshold (fp64 table and compare, like the reference's float64 tensor).
// One workgroup, order-preserving compaction (m is a few thousand).
struct SimTable { const double* t; int xlim, ylim; float g0, g1; double thresh; };

__global__ __launch_bounds__(1024) void k_pair_filter(int mode, const float* __restrict__ P0, const float* __restrict__ P1,
                                                     const long long* __restrict__ i0, const long long* __restrict__ i1, int m,
                                                     const float* __restrict__ T, float radius, long long* __restrict__ out,
                                                     int* __restrict__ n_out, SimTable sim) {
#pragma clang fp contract(off)
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  for (int start = 0; start < m; start += 1024) {
    const int i = start + threadIdx.x;
    bool keep = false;
    long long a = 0, b = 0;
    if (i < m) {
      a = i0[i]; b = i1[i];
      const float* p = P0 + 3 * a;
      const float* q = P1 + 3 * b;
      if (mode == 0) {
        keep = norm3(p[0], p[1], p[2]) > radius && norm3(q[0], q[1], q[2]) > radius;
      } else if (mode == 2) {
        const float d0 = norm3(p[0], p[1], p[2]), d1 = norm3(q[0], q[1], q[2]);
        long long c0 = (long long)(fminf(d0, d1) / sim.g0), c1 = (long long)(fabsf(d0 - d1) / sim.g1);   // .long(): towards zero
        c0 = c0 < 0 ? 0 : (c0 >= sim.ylim ? sim.ylim - 1 : c0);
        c1 = c1 < 0 ? 0 : (c1 >= sim.xlim ? sim.xlim - 1 : c1);
        keep = sim.t[c1 * sim.ylim + c0] > sim.thresh;
      } else {
        const float x = ((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3];
        const float y = ((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7];
        const float z = ((T[8] * p[0] + T[9] * p[1]) + T[10] * p[2]) + T[11];
        keep = norm3(x - q[0], y - q[1], z - q[2]) < radius;
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (keep) {
      const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
      out[2 * (size_t)pos] = a;
      out[2 * (size_t)pos + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < 16; ++w) tot += wave_cnt[w];
      base_s += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_out = base_s;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same three stages for every pair of a batch at once (eyoc_lowe_topk_segmented, eyoc_pair_filter_batched).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LBL_CHUNK = 64;     // segments per launch: their offsets travel as kernel arguments

struct TopkSegs { int n_seg, first_seg; int seg[LBL_CHUNK + 1]; };

// mode 0: k_lowe_weight's expressions, unchanged.  mode 1: weight = d1 (feature_filter = "None"; the order is that of a stable
// descending fp64 argsort: -0 = +0, NaN last).  The 64-bit key holds the segment above the descending float key, so one stable sort orders
// every segment on its own.
__global__ void k_lowe_weight_seg(TopkSegs s, int mode, const float* __restrict__ d1, const float* __restrict__ d2, float* __restrict__ w,
                                  unsigned long long* __restrict__ key, int* __restrict__ row) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int i = s.seg[b] + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.seg[b + 1]) return;
  float wt;
  unsigned int k32;
  if (mode == 0) {
    const float c1 = 1.0f - 0.5f * d1[i], c2 = 1.0f - 0.5f * d2[i];
    const float x1 = fmaxf(1.0f - c1, 1e-9f), x2 = fmaxf(1.0f - c2, 1e-9f);
    wt = 1.0f - x1 / x2;
    unsigned int u = __float_as_uint(wt);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending float order
    k32 = ~u;                                           // descending
  } else {
    wt = d1[i];
    unsigned int u = __float_as_uint(wt + 0.0f);        // -0 -> +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    k32 = wt != wt ? 0xFFFFFFFFu : ~u;
  }
  w[i] = wt;
  key[i] = ((unsigned long long)(unsigned)(s.first_seg + b) << 32) | k32;
  row[i] = i;
}

__global__ void k_take_topk_seg(TopkSegs s, const int* __restrict__ sorted_row, const float* __restrict__ w, int k,
                                long long* __restrict__ idx_out, float* __restrict__ w_out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const int r = sorted_row[s.seg[b] + i];               // k <= the segment's length
  const size_t o = (size_t)(s.first_seg + b) * k + i;
  idx_out[o] = r - s.seg[b];
  if (w_out) w_out[o] = w[r];
}

struct FilterSegs {
  int n_seg;
  int p0[LBL_CHUNK], p1[LBL_CHUNK], n0[LBL_CHUNK], n1[LBL_CHUNK];   // first row and row count of the pair's two clouds
  int m[LBL_CHUNK + 1];                                             // index lists / output rows
  long long tab[LBL_CHUNK];                                         // mode 2: the pair's table slice (offset in doubles)
  int xlim[LBL_CHUNK], ylim[LBL_CHUNK];
  float g1[LBL_CHUNK];
};

// k_pair_filter for pair blockIdx.x of the chunk: the same expressions, the same order-preserving compaction, one workgroup per pair.
// An index outside its cloud (the grid search's -1 included) drops the row; mode 1 with a non-finite pose keeps nothing.
__global__ __launch_bounds__(1024) void k_pair_filter_batched(FilterSegs s, int mode, const float* __restrict__ P0, const float* __restrict__ P1,
                                                             const long long* __restrict__ i0, const long long* __restrict__ i1,
                                                             const float* __restrict__ Ts, float radius, float g0, double thresh,
                                                             const double* __restrict__ tables, long long* __restrict__ out,
                                                             int* __restrict__ n_out) {
#pragma clang fp contract(off)
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  const int pb = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = s.m[pb], m = s.m[pb + 1] - m0;
  const float* T = Ts ? Ts + 16 * (size_t)pb : nullptr;
  bool pose_ok = true;
  if (mode == 1)
    for (int k = 0; k < 16; ++k) pose_ok = pose_ok && isfinite(T[k]);
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  for (int start = 0; start < m; start += 1024) {
    const int i = start + threadIdx.x;
    bool keep = false;
    long long a = 0, b = 0;
    if (i < m) {
      a = i0[m0 + i]; b = i1[m0 + i];
      if (a >= 0 && a < s.n0[pb] && b >= 0 && b < s.n1[pb] && pose_ok) {
        const float* p = P0 + 3 * ((size_t)s.p0[pb] + a);
        const float* q = P1 + 3 * ((size_t)s.p1[pb] + b);
        if (mode == 0) {
          keep = norm3(p[0], p[1], p[2]) > radius && norm3(q[0], q[1], q[2]) > radius;
        } else if (mode == 2) {
          const float d0 = norm3(p[0], p[1], p[2]), d1 = norm3(q[0], q[1], q[2]);
          const int xl = s.xlim[pb], yl = s.ylim[pb];
          long long c0 = (long long)(fminf(d0, d1) / g0), c1 = (long long)(fabsf(d0 - d1) / s.g1[pb]);   // .long(): towards zero
          c0 = c0 < 0 ? 0 : (c0 >= yl ? yl - 1 : c0);
          c1 = c1 < 0 ? 0 : (c1 >= xl ? xl - 1 : c1);
          keep = tables[s.tab[pb] + c1 * yl + c0] > thresh;
        } else {
          const float x = ((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3];
          const float y = ((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7];
          const float z = ((T[8] * p[0] + T[9] * p[1]) + T[10] * p[2]) + T[11];
          keep = norm3(x - q[0], y - q[1], z - q[2]) < radius;
        }
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; ++w) off += wave_cnt[w];
    if (keep) {
      const size_t pos = (size_t)m0 + off + __popcll(mask & ((1ull << lane) - 1ull));
      out[2 * pos] = a;
      out[2 * pos + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < 16; ++w) tot += wave_cnt[w];
      base_s += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) n_out[pb] = base_s;
}

// the ctx-scratch arrays of a top-k call over n rows with sort keys of type K; on a null base `bytes` alone means anything
template <typename K>
struct TopkWs { float* w; K *k0, *k1; int *r0, *r1; void* tmp; size_t bytes; };
template <typename K>
TopkWs<K> topk_layout(void* base, int n, size_t tmp_bytes) {
  Carver c(base, 0);
  TopkWs<K> t;
  t.w = c.take<float>(n);
  t.k0 = c.take<K>(n); t.k1 = c.take<K>(n);
  t.r0 = c.take<int>(n); t.r1 = c.take<int>(n);
  t.tmp = c.take<char>(tmp_bytes);
  t.bytes = align_up(c.off);
  return t;
}

}  // namespace

extern "C" {

// weights of n queries from their two nearest squared feature distances, and the k best (largest weight first,
// ties in query order): idx_out int64 [k] query indices, w_out f32 [k] or NULL.  k <= n.
int eyoc_lowe_topk(eyoc_ctx* ctx, const float* d1_dev, const float* d2_dev, int n, int k, int64_t* idx_out_dev,
                   float* w_out_dev, void* stream) {
  EYOC_REQUIRE(ctx && d1_dev && d2_dev && idx_out_dev, EYOC_ERR_INVALID, "eyoc_lowe_topk: NULL argument");
  EYOC_REQUIRE(n >= 0 && k >= 0 && k <= n, EYOC_ERR_INVALID, "eyoc_lowe_topk: k %d not in [0, n = %d]", k, n);
  if (k == 0) return EYOC_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t tmp = align_up(sort_rows_tmp_bytes(n, 32));
  int rc = ctx->ensure_scratch(topk_layout<unsigned int>(nullptr, n, tmp).bytes, st);
  if (rc) return rc;
  const TopkWs<unsigned int> t = topk_layout<unsigned int>(ctx->scratch, n, tmp);
  hipLaunchKernelGGL(k_lowe_weight, dim3(cdiv(n, 256)), dim3(256), 0, st, d1_dev, d2_dev, n, t.w, t.k0, t.r0);
  rc = sort_rows_by_key(t.tmp, tmp, t.k0, t.k1, t.r0, t.r1, n, 32, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_take_topk, dim3(cdiv(k, 256)), dim3(256), 0, st, t.r1, t.w, k, (long long*)idx_out_dev, w_out_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_pair_filter(eyoc_ctx* ctx, int mode, const float* P0_dev, const float* P1_dev, const int64_t* idx0_dev,
                     const int64_t* idx1_dev, int m, const float* T_dev, float radius, int64_t* pairs_out_dev, int32_t* n_out_dev,
                     void* stream) {
  EYOC_REQUIRE(ctx && P0_dev && P1_dev && idx0_dev && idx1_dev && pairs_out_dev && n_out_dev, EYOC_ERR_INVALID,
               "eyoc_pair_filter: NULL argument");
  EYOC_REQUIRE(mode == 0 || (mode == 1 && T_dev), EYOC_ERR_INVALID, "eyoc_pair_filter: mode %d (1 needs a pose)", mode);
  EYOC_REQUIRE(m >= 0, EYOC_ERR_INVALID, "eyoc_pair_filter: m %d", m);
  hipLaunchKernelGGL(k_pair_filter, dim3(1), dim3(1024), 0, (hipStream_t)stream, mode, P0_dev, P1_dev, (const long long*)idx0_dev,
                     (const long long*)idx1_dev, m, T_dev, radius, (long long*)pairs_out_dev, n_out_dev, SimTable{});
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_pair_filter_similarity(eyoc_ctx* ctx, const float* P0_dev, const float* P1_dev, const int64_t* idx0_dev,
                                const int64_t* idx1_dev, int m, const double* table_dev, int xlim, int ylim, float grid0,
                                float grid1, double thresh, int64_t* pairs_out_dev, int32_t* n_out_dev, void* stream) {
  EYOC_REQUIRE(ctx && P0_dev && P1_dev && idx0_dev && idx1_dev && table_dev && pairs_out_dev && n_out_dev, EYOC_ERR_INVALID,
               "eyoc_pair_filter_similarity: NULL argument");
  EYOC_REQUIRE(m >= 0 && xlim >= 1 && ylim >= 1 && grid0 > 0.f && grid1 > 0.f, EYOC_ERR_INVALID,
               "eyoc_pair_filter_similarity: m %d table %d x %d grid %g %g", m, xlim, ylim, grid0, grid1);
  SimTable sim{table_dev, xlim, ylim, grid0, grid1, thresh};
  hipLaunchKernelGGL(k_pair_filter, dim3(1), dim3(1024), 0, (hipStream_t)stream, 2, P0_dev, P1_dev, (const long long*)idx0_dev,
                     (const long long*)idx1_dev, m, (const float*)nullptr, 0.0f, (long long*)pairs_out_dev, n_out_dev, sim);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// eyoc_lowe_topk on every segment of a batch: one weight kernel, one stable 64-bit sort and one take kernel per LBL_CHUNK segments'
// worth of kernel arguments (the sort is always one).  Segment s of the output is byte for byte eyoc_lowe_topk on it alone.
int eyoc_lowe_topk_segmented(eyoc_ctx* ctx, const float* d1_dev, const float* d2_dev, const int32_t* seg_host, int nseg, int k, int mode,
                             int64_t* idx_out_dev, float* w_out_dev, void* stream) {
  EYOC_REQUIRE(ctx && d1_dev && seg_host && idx_out_dev, EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: NULL argument");
  EYOC_REQUIRE(mode == 0 || mode == 1, EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: mode %d", mode);
  EYOC_REQUIRE(mode == 1 || d2_dev, EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: mode 0 needs d2");
  EYOC_REQUIRE(nseg >= 1 && nseg <= (1 << 20) && k >= 0, EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: nseg %d, k %d", nseg, k);
  EYOC_REQUIRE(seg_host[0] == 0, EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: segments must start at 0");
  int max_len = 0;
  for (int s = 0; s < nseg; ++s) {
    EYOC_REQUIRE(seg_host[s + 1] >= seg_host[s], EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: segment offsets must not decrease (segment %d)", s);
    const int len = seg_host[s + 1] - seg_host[s];
    EYOC_REQUIRE(k <= len, EYOC_ERR_INVALID, "eyoc_lowe_topk_segmented: k %d above the %d rows of segment %d", k, len, s);
    max_len = len > max_len ? len : max_len;
  }
  if (k == 0) return EYOC_OK;
  const int n = seg_host[nseg];
  hipStream_t st = (hipStream_t)stream;
  const size_t tmp = sort_rows64_tmp_bytes(n);
  int rc = ctx->ensure_scratch(topk_layout<unsigned long long>(nullptr, n, tmp).bytes, st);
  if (rc) return rc;
  const TopkWs<unsigned long long> t = topk_layout<unsigned long long>(ctx->scratch, n, tmp);
  int seg_bits = 1;
  while ((1 << seg_bits) < nseg) ++seg_bits;
  TopkSegs ts;
  for (int s0 = 0; s0 < nseg; s0 += LBL_CHUNK) {
    ts.n_seg = nseg - s0 < LBL_CHUNK ? nseg - s0 : LBL_CHUNK;
    ts.first_seg = s0;
    for (int b = 0; b <= ts.n_seg; ++b) ts.seg[b] = seg_host[s0 + b];
    hipLaunchKernelGGL(k_lowe_weight_seg, dim3(cdiv(max_len, 256), ts.n_seg), dim3(256), 0, st, ts, mode, d1_dev, d2_dev, t.w, t.k0, t.r0);
  }
  rc = sort_rows_by_key64(t.tmp, tmp, t.k0, t.k1, t.r0, t.r1, n, 32 + seg_bits, st);
  if (rc) return rc;
  for (int s0 = 0; s0 < nseg; s0 += LBL_CHUNK) {
    ts.n_seg = nseg - s0 < LBL_CHUNK ? nseg - s0 : LBL_CHUNK;
    ts.first_seg = s0;
    for (int b = 0; b <= ts.n_seg; ++b) ts.seg[b] = seg_host[s0 + b];
    hipLaunchKernelGGL(k_take_topk_seg, dim3(cdiv(k, 256), ts.n_seg), dim3(256), 0, st, ts, t.r1, t.w, k, (long long*)idx_out_dev, w_out_dev);
  }
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_pair_filter_batched(eyoc_ctx* ctx, int mode, const float* P0_dev, const float* P1_dev, const int64_t* idx0_dev,
                             const int64_t* idx1_dev, const int32_t* seg_p0_host, const int32_t* seg_p1_host, const int32_t* seg_m_host,
                             int nseg, const float* T_dev, float radius, const double* tables_dev, const eyoc_sim_slice* slices_host,
                             float grid0, double thresh, int64_t* pairs_out_dev, int32_t* count_dev, void* stream) {
  EYOC_REQUIRE(ctx && seg_p0_host && seg_p1_host && seg_m_host && count_dev, EYOC_ERR_INVALID, "eyoc_pair_filter_batched: NULL argument");
  EYOC_REQUIRE(mode >= 0 && mode <= 2, EYOC_ERR_INVALID, "eyoc_pair_filter_batched: mode %d", mode);
  EYOC_REQUIRE(mode != 1 || T_dev, EYOC_ERR_INVALID, "eyoc_pair_filter_batched: mode 1 needs the poses");
  EYOC_REQUIRE(mode != 2 || (tables_dev && slices_host && grid0 > 0.f), EYOC_ERR_INVALID, "eyoc_pair_filter_batched: mode 2 needs the tables and grid0 > 0");
  EYOC_REQUIRE(nseg >= 1 && nseg <= 1024, EYOC_ERR_INVALID, "eyoc_pair_filter_batched: nseg = %d is outside [1, 1024]", nseg);
  EYOC_REQUIRE(seg_p0_host[0] == 0 && seg_p1_host[0] == 0 && seg_m_host[0] == 0, EYOC_ERR_INVALID, "eyoc_pair_filter_batched: segments must start at 0");
  for (int b = 0; b < nseg; ++b) {
    EYOC_REQUIRE(seg_p0_host[b + 1] >= seg_p0_host[b] && seg_p1_host[b + 1] >= seg_p1_host[b] && seg_m_host[b + 1] >= seg_m_host[b],
                 EYOC_ERR_INVALID, "eyoc_pair_filter_batched: segment offsets must not decrease (pair %d)", b);
    if (mode == 2)
      EYOC_REQUIRE(slices_host[b].table_offset >= 0 && slices_host[b].xlim >= 1 && slices_host[b].ylim >= 1 && slices_host[b].grid1 > 0.f,
                   EYOC_ERR_INVALID, "eyoc_pair_filter_batched: table slice of pair %d", b);
  }
  if (seg_m_host[nseg] > 0)
    EYOC_REQUIRE(P0_dev && P1_dev && idx0_dev && idx1_dev && pairs_out_dev, EYOC_ERR_INVALID, "eyoc_pair_filter_batched: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  FilterSegs fs;
  for (int b0 = 0; b0 < nseg; b0 += LBL_CHUNK) {
    fs.n_seg = nseg - b0 < LBL_CHUNK ? nseg - b0 : LBL_CHUNK;
    for (int b = 0; b < fs.n_seg; ++b) {
      fs.p0[b] = seg_p0_host[b0 + b]; fs.n0[b] = seg_p0_host[b0 + b + 1] - seg_p0_host[b0 + b];
      fs.p1[b] = seg_p1_host[b0 + b]; fs.n1[b] = seg_p1_host[b0 + b + 1] - seg_p1_host[b0 + b];
      fs.tab[b] = mode == 2 ? slices_host[b0 + b].table_offset : 0;
      fs.xlim[b] = mode == 2 ? slices_host[b0 + b].xlim : 1;
      fs.ylim[b] = mode == 2 ? slices_host[b0 + b].ylim : 1;
      fs.g1[b] = mode == 2 ? slices_host[b0 + b].grid1 : 1.0f;
    }
    for (int b = 0; b <= fs.n_seg; ++b) fs.m[b] = seg_m_host[b0 + b];
    hipLaunchKernelGGL(k_pair_filter_batched, dim3(fs.n_seg), dim3(1024), 0, st, fs, mode, P0_dev, P1_dev, (const long long*)idx0_dev,
                       (const long long*)idx1_dev, T_dev ? T_dev + 16 * (size_t)b0 : nullptr, radius, grid0, thresh, tables_dev,
                       (long long*)pairs_out_dev, count_dev + b0);
  }
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"
