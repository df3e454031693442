// Per-pair failure isolation, device side: removing the clouds of faulty pairs from a collated batch.
//
//  * eyoc_batch_drop: rows whose batch index has its bit in a 1024-bit mask are dropped, the others keep their order and their batch
//    index.  One flag pass (which also counts the kept rows per batch index), the flag scan the coordinate maps use (scan.h), one
//    compaction pass that moves coordinates, features and the old -> new row map together.  Plain bandwidth kernels: a wave owns 512
//    consecutive rows and walks them 64 at a time, so every load is one contiguous segment per wave-instruction (16-byte coordinate
//    rows as int4, feature rows in the widest vector their width and alignment allow) and every store goes to the contiguous run of
//    kept rows.  A row's new position is its tile's scanned partial sum + the kept rows of the waves before it + the kept lanes below
//    it (ballot + popcount): no atomics on the data path, the output is the same bytes on every run.
//  * eyoc_remap_rows: an int64 index array through the row map (the sample indices of the batch).
#include "scan.h"

using namespace eyoc;

namespace {

constexpr int DROP_WAVES = SCAN_BLOCK / 64, DROP_PER_WAVE = SCAN_TILE / DROP_WAVES, DROP_STEPS = DROP_PER_WAVE / 64;
constexpr int MAX_BATCH = 1024;

__device__ inline bool dropped(const unsigned int* __restrict__ mask, int b) {
  return b >= 0 && b < MAX_BATCH && ((mask[b >> 5] >> (b & 31)) & 1u);
}

// flag[i] = 1 iff row i stays; kept[b] += the rows of batch index b that stay (b in [0, 1024): per-workgroup histogram in LDS, a wave
// whose 64 rows share their batch index - the usual case, clouds are contiguous - adds once; integer sums, so the order does not matter)
__global__ __launch_bounds__(SCAN_BLOCK) void k_drop_flag(const int32_t* __restrict__ coords, int n,
                                                          const unsigned int* __restrict__ mask, int* __restrict__ flag,
                                                          int* __restrict__ kept) {
  __shared__ int hist[MAX_BATCH];
  __shared__ unsigned int m[32];
  for (int k = threadIdx.x; k < MAX_BATCH; k += SCAN_BLOCK) hist[k] = 0;
  if (threadIdx.x < 32) m[threadIdx.x] = mask[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int base = blockIdx.x * SCAN_TILE + (threadIdx.x >> 6) * DROP_PER_WAVE + lane;
#pragma unroll
  for (int s = 0; s < DROP_STEPS; ++s) {
    const int i = base + s * 64;
    const int b = i < n ? coords[4 * (size_t)i] : -1;
    const bool keep = i < n && !dropped(m, b);
    if (i < n) flag[i] = keep;
    const bool counted = keep && b >= 0 && b < MAX_BATCH;
    const int b0 = __shfl(b, 0, 64);
    if (__all(b == b0)) {
      const unsigned long long bal = __ballot(counted);
      if (lane == 0 && bal) atomicAdd(&hist[b0], __popcll(bal));
    } else if (counted) {
      atomicAdd(&hist[b], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < MAX_BATCH; k += SCAN_BLOCK)
    if (hist[k]) atomicAdd(&kept[k], hist[k]);
}

template <int V> struct FeatVec;
template <> struct FeatVec<1> { using type = float; };
template <> struct FeatVec<2> { using type = float2; };
template <> struct FeatVec<4> { using type = float4; };

// partial: the exclusive scan of the tiles' kept rows (k_scan_partials + k_scan_top).  cv: vectors of V floats per feature row
// (feats == NULL: none), cv_shift: log2(cv) when cv is a power of two, else -1.
template <int V>
__global__ __launch_bounds__(SCAN_BLOCK) void k_drop_compact(const int* __restrict__ flag, const int* __restrict__ partial,
                                                             const int32_t* __restrict__ coords, const float* __restrict__ feats,
                                                             int n, int cv, int cv_shift, int32_t* __restrict__ coords_out,
                                                             float* __restrict__ feats_out, int32_t* __restrict__ row_map) {
  using vec = typename FeatVec<V>::type;
  __shared__ int wave_sum[DROP_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int first = blockIdx.x * SCAN_TILE + wave * DROP_PER_WAVE;
  unsigned long long bal[DROP_STEPS];
  int tot = 0;
#pragma unroll
  for (int s = 0; s < DROP_STEPS; ++s) {
    const int i = first + s * 64 + lane;
    bal[s] = __ballot(i < n && flag[i] != 0);
    tot += __popcll(bal[s]);
  }
  if (lane == 0) wave_sum[wave] = tot;
  __syncthreads();
  int pos = partial[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos += wave_sum[w];
  const vec* __restrict__ fin = reinterpret_cast<const vec*>(feats);
  vec* __restrict__ fout = reinterpret_cast<vec*>(feats_out);
#pragma unroll
  for (int s = 0; s < DROP_STEPS; ++s) {
    const int i0 = first + s * 64, i = i0 + lane;
    const unsigned long long b = bal[s];
    if (i < n) {
      const bool keep = (b >> lane) & 1ull;
      const int to = pos + __popcll(b & ((1ull << lane) - 1ull));
      row_map[i] = keep ? to : -1;
      if (keep) reinterpret_cast<int4*>(coords_out)[to] = reinterpret_cast<const int4*>(coords)[i];
    }
    if (feats && b) {
      // the step's 64 * cv feature vectors, lane after lane: a set bit r of the ballot is a row of this step that is < n
      for (int e = lane; e < 64 * cv; e += 64) {
        const int r = cv_shift >= 0 ? e >> cv_shift : e / cv;
        if ((b >> r) & 1ull) {
          const int to = pos + __popcll(b & ((1ull << r) - 1ull));
          fout[(size_t)to * cv + (e - r * cv)] = fin[(size_t)i0 * cv + e];
        }
      }
    }
    pos += __popcll(b);
  }
}

__global__ void k_remap_rows(const long long* __restrict__ idx, int m, const int32_t* __restrict__ row_map, int n,
                             long long* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const long long v = idx[k];
  out[k] = v >= 0 && v < n ? (long long)row_map[v] : -1;
}

}  // namespace

extern "C" {

size_t eyoc_batch_drop_workspace_bytes(int n_rows) {
  if (n_rows < 0) return 0;
  const size_t n = (size_t)n_rows;
  return align_up(32 * 4) + align_up((1 + MAX_BATCH) * 4) + align_up(n * 4) + align_up((n / SCAN_TILE + 2) * 4);
}

int eyoc_batch_drop(eyoc_ctx* ctx, const int32_t* coords_dev, const float* feats_dev, int n, int c, const uint32_t* drop_mask,
                    int32_t* coords_out_dev, float* feats_out_dev, int32_t* row_map_dev, int* n_kept, int32_t* kept_per_batch,
                    void* ws, size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx && drop_mask && n_kept, EYOC_ERR_INVALID, "eyoc_batch_drop: NULL argument");
  EYOC_REQUIRE(n >= 0 && c >= 0 && (long long)n * (c > 1 ? c : 1) <= (1ll << 40), EYOC_ERR_INVALID, "eyoc_batch_drop: n %d c %d", n, c);
  *n_kept = 0;
  if (kept_per_batch) memset(kept_per_batch, 0, MAX_BATCH * sizeof(int32_t));
  if (n == 0) return EYOC_OK;
  EYOC_REQUIRE(coords_dev && coords_out_dev && row_map_dev && ws && coords_dev != coords_out_dev, EYOC_ERR_INVALID,
               "eyoc_batch_drop: NULL argument (or coords_out == coords: not in place)");
  EYOC_REQUIRE((feats_dev == nullptr) == (feats_out_dev == nullptr) && (feats_dev == nullptr || (c >= 1 && feats_dev != feats_out_dev)),
               EYOC_ERR_INVALID, "eyoc_batch_drop: feats and feats_out go together, c >= 1, not in place");
  EYOC_REQUIRE((((uintptr_t)coords_dev | (uintptr_t)coords_out_dev) & 15) == 0, EYOC_ERR_INVALID,
               "eyoc_batch_drop: coordinate arrays must be 16-byte aligned");
  const size_t need = eyoc_batch_drop_workspace_bytes(n);
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0 && ws_bytes >= need, EYOC_ERR_WORKSPACE,
               "eyoc_batch_drop: workspace %zu < required %zu bytes (256-byte aligned)", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  Carver cv(ws, ws_bytes);
  unsigned int* mask = cv.take<unsigned int>(32);
  int* counters = cv.take<int>(1 + MAX_BATCH);      // [0] kept rows, [1 ..] kept rows per batch index
  int* flag = cv.take<int>(n);
  int* partial = cv.take<int>(n / SCAN_TILE + 2);
  EYOC_REQUIRE(cv.ok(), EYOC_ERR_WORKSPACE, "eyoc_batch_drop: internal workspace accounting error (%zu > %zu)", cv.off, cv.cap);
  // pinned staging: the mask up at 0, the counts back behind it
  EYOC_REQUIRE(256 + (1 + MAX_BATCH) * sizeof(int) <= ctx->pinned_bytes, EYOC_ERR_INVALID, "eyoc_batch_drop: pinned staging too small");
  memcpy(ctx->pinned, drop_mask, 32 * sizeof(uint32_t));
  int* host = (int*)((char*)ctx->pinned + 256);
  EYOC_CHECK_HIP(hipMemcpyAsync(mask, ctx->pinned, 32 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  EYOC_CHECK_HIP(hipMemsetAsync(counters, 0, (1 + MAX_BATCH) * sizeof(int), st));
  const int nb = cdiv(n, SCAN_TILE);
  hipLaunchKernelGGL(k_drop_flag, dim3(nb), dim3(SCAN_BLOCK), 0, st, coords_dev, n, (const unsigned int*)mask, flag, counters + 1);
  hipLaunchKernelGGL(k_scan_partials, dim3(nb), dim3(SCAN_BLOCK), 0, st, (const int*)flag, n, partial);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_BLOCK), 0, st, partial, nb, counters);
  // feature rows in the widest vector that the row width and both pointers' alignment allow
  const uintptr_t fa = (uintptr_t)feats_dev | (uintptr_t)feats_out_dev;
  const int v = !feats_dev ? 1 : (c % 4 == 0 && fa % 16 == 0) ? 4 : (c % 2 == 0 && fa % 8 == 0) ? 2 : 1;
  const int cvec = feats_dev ? c / v : 0;
  int shift = -1;
  for (int k = 0; k < 31; ++k)
    if (cvec == (1 << k)) shift = k;
#define EYOC_DROP_CASE(V_)                                                                                                    \
  hipLaunchKernelGGL((k_drop_compact<V_>), dim3(nb), dim3(SCAN_BLOCK), 0, st, (const int*)flag, (const int*)partial, coords_dev, \
                     feats_dev, n, cvec, shift, coords_out_dev, feats_out_dev, row_map_dev)
  if (v == 4) EYOC_DROP_CASE(4);
  else if (v == 2) EYOC_DROP_CASE(2);
  else EYOC_DROP_CASE(1);
#undef EYOC_DROP_CASE
  EYOC_CHECK_HIP(hipGetLastError());
  EYOC_CHECK_HIP(hipMemcpyAsync(host, counters, (1 + MAX_BATCH) * sizeof(int), hipMemcpyDeviceToHost, st));
  EYOC_CHECK_HIP(hipStreamSynchronize(st));
  *n_kept = host[0];
  if (kept_per_batch) memcpy(kept_per_batch, host + 1, MAX_BATCH * sizeof(int32_t));
  return EYOC_OK;
}

int eyoc_remap_rows(eyoc_ctx* ctx, const int64_t* idx_dev, int m, const int32_t* row_map_dev, int n, int64_t* out_dev, void* stream) {
  EYOC_REQUIRE(ctx, EYOC_ERR_INVALID, "eyoc_remap_rows: NULL argument");
  EYOC_REQUIRE(m >= 0 && n >= 0, EYOC_ERR_INVALID, "eyoc_remap_rows: m %d n %d", m, n);
  if (m == 0) return EYOC_OK;
  EYOC_REQUIRE(idx_dev && out_dev && (row_map_dev || n == 0), EYOC_ERR_INVALID, "eyoc_remap_rows: NULL argument");
  hipLaunchKernelGGL(k_remap_rows, dim3(cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)idx_dev, m, row_map_dev, n,
                     (long long*)out_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"
