// Hardest-contrastive loss of the reference's trainer (lib/trainer.py:935-991) and its gradient with respect to both feature matrices,
// on positives that never leave the device (include/eyoc_hip.h has the contract).
//
// Forward, 5 launches: one fill (control block + key table + search minima), hc_prep_kernel (every index checked, the positive keys
// into an open-addressing table by 64-bit compare-and-swap: membership does not depend on the order of the pairs), hc_search_kernel
// (both directions: lane = positive with its row in VGPRs, the candidates of the direction staged through LDS in tiles of HC_T rows and
// read as LDS broadcasts, the four waves of a workgroup take a quarter of every tile and merge by (dist, t); the tiles are split over
// grid.z and merged by a 64-bit integer atomicMax), hc_terms_kernel (mask, the values rounded once, terms, a workgroup's fp64 sums),
// hc_final_kernel (the workgroups' sums in order, the record).
// Backward, 4 launches: two fills (dF0, dF1), hc_weights_kernel (the three scalar factors of every positive and the destination row
// of each of its four contributions), hc_rows_kernel (one workgroup per contribution entry; the FIRST entry of a destination row
// gathers the row's whole list in entry order, sums it in fp64 in slots fixed by the position in that list and writes the row once).
// No floating-point atomics anywhere.  The SEARCH compares in knn1_kernel's arithmetic (knn.hip): d = a - b; s = d * d; acc = acc + s
// in fp32, channels in order, no contraction, sqrtf(acc + 1e-7f) - so t* is eyoc_knn1's.  The two values of a positive that enter the
// loss (pos_d2, and dist of the chosen candidate) are then evaluated once more with an fp64 accumulator and rounded to fp32 once:
// an fp32 chain over 64 channels is up to 8 ulp from the exact value, and the stage tests hold these values to one ulp of fp64.
// The triplet losses of the reference's other two trainers follow below the hardest-contrastive entry points, on the same table and search;
// the random-negative contrastive loss of the base trainer comes last, on the same table.  Those two share one backward (a sorted
// contribution list and rows_kernel, between the hardest-contrastive and the triplet part); the hardest-contrastive backward stays apart: it
// finds a row's entries without a sort and forms its products in fp32 before widening, so moving it onto the list would change its bytes.
#include <type_traits>

#include "pose_math.h"

using namespace eyoc;

namespace {

constexpr int HC_A = EYOC_HCLOSS_ANCHORS;   // positives per workgroup = lanes of a wave
constexpr int HC_T = EYOC_HCLOSS_TILE;      // candidate rows per LDS tile (C = 64: 32 KiB)
constexpr int HC_THREADS = 256;
constexpr int HC_WAVES = HC_THREADS / 64;
constexpr int HC_LIST = 2048;               // entries of a row's list gathered per pass of hc_rows_kernel
constexpr int NO_T = 0x7FFFFFFF;
static_assert(HC_A == 64 && HC_T % (4 * HC_WAVES) == 0, "a wave takes HC_T / HC_WAVES candidates of a tile in groups of four");
static_assert(sizeof(eyoc_hcloss_record) == 48, "eyoc_hcloss_record is 48 bytes");

struct HcCtl {   // the first 256 bytes of the workspace; zeroed together with the table by the forward's fill
  eyoc_hcloss_record rec;
  unsigned int status;   // what the kernels found, by atomicOr
};

struct HcWs {
  HcCtl* ctl;
  unsigned long long* table;   // key + 1, 0 = empty
  unsigned int mask;           // slots - 1
  unsigned long long* best;    // [2][n_used]: ~(distance bits << 32 | t) of the search, 0 = nothing compared
  size_t fill_bytes;           // control block, table and best: zeroed by the forward's one fill
  int nwg;                     // workgroups of the search per direction (>= 1)
  int* tstar;                  // [2][n_used]
  float* dist;                 // [2][n_used]
  float* pos_d2;               // [n_used]
  unsigned int* flags;         // [2][n_used]
  double* part_sum;            // [3][nwg]: positive terms, kept terms 01, kept terms 10
  int* part_cnt;               // [2][nwg]
  float* wts;                  // [3][n_used]: backward factors (positive, 01, 10)
  int* dest;                   // [2][2 n_used]: destination rows in dF0 / dF1 (anchor entries, then candidate entries), -1 = none
  size_t total;
};

size_t table_slots(int n_pairs) {
  size_t s = 2;
  while (s < 2 * (size_t)n_pairs) s <<= 1;
  return s;
}

HcWs carve(void* base, size_t bytes, int n_pairs, int n_used) {
  Carver cv(base, bytes);
  HcWs w;
  const size_t n = (size_t)n_used, slots = table_slots(n_pairs);
  w.ctl = (HcCtl*)cv.take<char>(256);
  w.table = cv.take<unsigned long long>(slots);   // (256 bytes taken above: the table follows the control block directly)
  w.mask = (unsigned int)(slots - 1);
  w.best = cv.take<unsigned long long>(2 * n);
  w.fill_bytes = cv.off;
  w.nwg = n_used > 0 ? cdiv(n_used, HC_A) : 1;
  w.tstar = cv.take<int>(2 * n);
  w.dist = cv.take<float>(2 * n);
  w.pos_d2 = cv.take<float>(n);
  w.flags = cv.take<unsigned int>(2 * n);
  w.part_sum = cv.take<double>(3 * (size_t)w.nwg);
  w.part_cnt = cv.take<int>(2 * (size_t)w.nwg);
  w.wts = cv.take<float>(3 * n);
  w.dest = cv.take<int>(4 * n);
  w.total = align_up(cv.off);
  return w;
}

__device__ inline int wave_sum_i(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // valid in lane 0
}

// f(std::integral_constant<int, C>) for the feature width C = c of a call (16, 32 or 64, checked by every entry point)
template <typename F>
void for_width(int c, F&& f) {
  if (c == 16) f(std::integral_constant<int, 16>());
  else if (c == 32) f(std::integral_constant<int, 32>());
  else f(std::integral_constant<int, 64>());
}

// The ordered sum of a final kernel (one workgroup of HC_THREADS): thread t adds the partials of the workgroups t, t + 256, ... by
// add(b, v, c), wave_sum, lane 0 of every wave to LDS, thread 0 adds the waves in order.  True in thread 0 alone, which holds the totals.
template <int ND, int NI, typename Add>
__device__ inline bool block_sum_ordered(int nblk, Add add, double (&v)[ND], int (&c)[NI]) {
  __shared__ double red_d[HC_WAVES][ND];
  __shared__ int red_i[HC_WAVES][NI];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < ND; ++k) v[k] = 0.0;
#pragma unroll
  for (int k = 0; k < NI; ++k) c[k] = 0;
  for (int b = threadIdx.x; b < nblk; b += HC_THREADS) add(b, v, c);
#pragma unroll
  for (int k = 0; k < ND; ++k) v[k] = wave_sum(v[k]);
#pragma unroll
  for (int k = 0; k < NI; ++k) c[k] = wave_sum_i(c[k]);
  if (lane == 0) {
    for (int k = 0; k < ND; ++k) red_d[wave][k] = v[k];
    for (int k = 0; k < NI; ++k) red_i[wave][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int k = 0; k < ND; ++k) v[k] = 0.0;
  for (int k = 0; k < NI; ++k) c[k] = 0;
  for (int x = 0; x < HC_WAVES; ++x) {
    for (int k = 0; k < ND; ++k) v[k] += red_d[x][k];
    for (int k = 0; k < NI; ++k) c[k] += red_i[x][k];
  }
  return true;
}

// the opening of every backward: both gradients zeroed (an empty matrix has no buffer)
int zero_gradients(float* dF0, int n0, float* dF1, int n1, int c, hipStream_t st) {
  if (n0 > 0) EYOC_CHECK_HIP(hipMemsetAsync(dF0, 0, (size_t)n0 * c * sizeof(float), st));
  if (n1 > 0) EYOC_CHECK_HIP(hipMemsetAsync(dF1, 0, (size_t)n1 * c * sizeof(float), st));
  return EYOC_OK;
}

__device__ inline bool key_member(const HcWs& w, unsigned long long key1) {
  unsigned int s = hash_key(key1) & w.mask;
  for (unsigned int probes = 0; probes <= w.mask; ++probes) {   // bounded: load <= 1/2
    const unsigned long long k = w.table[s];
    if (k == key1) return true;
    if (k == 0ull) return false;
    s = (s + 1) & w.mask;
  }
  return false;
}

// |a - b|^2 of a row held in registers and a row in memory with an fp64 accumulator (the differences of fp32 values are exact in fp64)
template <int C>
__device__ inline double row_d2(const float (&a)[C], const float* __restrict__ b) {
#pragma clang fp contract(off)
  const float4* src = reinterpret_cast<const float4*>(b);
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < C / 4; ++q) {
    const float4 v = src[q];
    double d;
    d = (double)a[4 * q] - (double)v.x;     acc += d * d;
    d = (double)a[4 * q + 1] - (double)v.y; acc += d * d;
    d = (double)a[4 * q + 2] - (double)v.z; acc += d * d;
    d = (double)a[4 * q + 3] - (double)v.w; acc += d * d;
  }
  return acc;
}

// every index of the call checked once; the key of every in-range positive into the table
__global__ __launch_bounds__(HC_THREADS) void hc_prep_kernel(const long long* __restrict__ pairs, int n_pairs,
                                                             const long long* __restrict__ used, int n_used,
                                                             const long long* __restrict__ sel0, int s0,
                                                             const long long* __restrict__ sel1, int s1, int n0, int n1, int n_max, HcWs w) {
  const unsigned long long scale = (unsigned long long)(n0 > n1 ? n0 : n1);
  int bad = 0;
  for (int idx = blockIdx.x * HC_THREADS + threadIdx.x; idx < n_max; idx += gridDim.x * HC_THREADS) {
    if (idx < n_pairs) {
      const long long i = pairs[2 * (size_t)idx], j = pairs[2 * (size_t)idx + 1];
      if (i < 0 || i >= n0 || j < 0 || j >= n1) {
        bad = 1;
      } else {
        const unsigned long long key1 = (unsigned long long)i + (unsigned long long)j * scale + 1ull;
        unsigned int s = hash_key(key1) & w.mask;
        for (unsigned int probes = 0; probes <= w.mask; ++probes) {
          const unsigned long long old = atomicCAS(&w.table[s], 0ull, key1);
          if (old == 0ull || old == key1) break;
          s = (s + 1) & w.mask;
        }
      }
    }
    if (used && idx < n_used) {
      const long long u = used[idx];
      bad |= (u < 0 || u >= n_pairs);
    }
    if (idx < s0) {
      const long long r = sel0[idx];
      bad |= (r < 0 || r >= n0);
    }
    if (idx < s1) {
      const long long r = sel1[idx];
      bad |= (r < 0 || r >= n1);
    }
  }
  if (bad) atomicOr(&w.ctl->status, EYOC_HCLOSS_BAD_INDEX);
}

// the positive of a lane: its indices checked, then its own row of the direction's anchor matrix into registers
template <int C>
__device__ inline bool load_anchor(int p, int dir, const float* __restrict__ F0, int n0, const float* __restrict__ F1, int n1,
                                   const long long* __restrict__ pairs, int n_pairs, const long long* __restrict__ used, int n_used,
                                   float (&a)[C], long long& i, long long& j, int& bad) {
  bool ok = p < n_used;
  i = 0;
  j = 0;
  if (ok) {
    const long long u = used ? used[p] : (long long)p;
    if (u < 0 || u >= n_pairs) {
      ok = false;
      bad = 1;
    } else {
      i = pairs[2 * (size_t)u];
      j = pairs[2 * (size_t)u + 1];
      if (i < 0 || i >= n0 || j < 0 || j >= n1) {
        ok = false;
        bad = 1;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = 0.0f;
  if (ok) {
    const float4* src = reinterpret_cast<const float4*>((dir ? F1 : F0) + (size_t)(dir ? j : i) * C);
#pragma unroll
    for (int q = 0; q < C / 4; ++q) {
      const float4 v = src[q];
      a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
  }
  return ok;
}

// grid (workgroups of 64 positives, direction, candidate split): block z takes the tiles z, z + gridDim.z, ... of the direction's
// candidates.  The minimum over all blocks is merged by a 64-bit integer atomicMax on ~(distance bits << 32 | t): the smallest distance
// and, among equal ones, the lowest t, however the candidates were split (distances are positive, their bits order like the values).
template <int C>
__global__ __launch_bounds__(HC_THREADS) void hc_search_kernel(const float* __restrict__ F0, int n0, const float* __restrict__ F1, int n1,
                                                               const long long* __restrict__ pairs, int n_pairs,
                                                               const long long* __restrict__ used, int n_used,
                                                               const long long* __restrict__ sel0, int s0,
                                                               const long long* __restrict__ sel1, int s1, HcWs w) {
#pragma clang fp contract(off)
  constexpr int C4 = C / 4;
  __shared__ float4 tile[HC_T * C4];
  __shared__ int tile_ok[HC_T];
  __shared__ float sd[HC_WAVES][64];
  __shared__ int sj[HC_WAVES][64];
  const int dir = blockIdx.y;   // 0: anchors F0[i] against F1[sel1], 1: anchors F1[j] against F0[sel0]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const float* __restrict__ FB = dir ? F0 : F1;
  const long long* __restrict__ sel = dir ? sel0 : sel1;
  const int s = dir ? s0 : s1, nb = dir ? n0 : n1;
  if ((int)blockIdx.z * HC_T >= s) return;   // (the other direction has more tiles)
  const int p = blockIdx.x * HC_A + lane;
  int bad = 0;
  long long i, j;
  float a[C];
  const bool ok = load_anchor<C>(p, dir, F0, n0, F1, n1, pairs, n_pairs, used, n_used, a, i, j, bad);
  float best_d = __builtin_inff();
  int best_t = NO_T;
  for (int t0 = blockIdx.z * HC_T; t0 < s; t0 += gridDim.z * HC_T) {
    __syncthreads();   // the previous tile has been consumed
    const int nt = s - t0 < HC_T ? s - t0 : HC_T;
    for (int e = threadIdx.x; e < nt * C4; e += HC_THREADS) {
      const int t = e / C4, q = e % C4;
      const long long r = sel[t0 + t];
      const bool rok = r >= 0 && r < nb;   // checked before it becomes an address
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rok) v = *reinterpret_cast<const float4*>(FB + (size_t)r * C + 4 * q);
      else bad = 1;
      tile[e] = v;
      if (q == 0) tile_ok[t] = rok ? 1 : 0;
    }
    __syncthreads();
    // this wave's quarter of the tile, four candidates side by side (independent chains); every lane reads the same LDS address
    const int lo = wave * (HC_T / HC_WAVES);
    const int hi = nt < lo + HC_T / HC_WAVES ? nt : lo + HC_T / HC_WAVES;
    for (int t = lo; t < hi; t += 4) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int q = 0; q < C4; ++q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // (rows past `hi` hold stale data: computed, never compared)
          const float4 b = tile[(t + k) * C4 + q];
          float d;
          d = a[4 * q] - b.x;     d = d * d; acc[k] = acc[k] + d;
          d = a[4 * q + 1] - b.y; d = d * d; acc[k] = acc[k] + d;
          d = a[4 * q + 2] - b.z; d = d * d; acc[k] = acc[k] + d;
          d = a[4 * q + 3] - b.w; d = d * d; acc[k] = acc[k] + d;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float v = sqrtf(acc[k] + 1e-7f);
        const bool valid = (t + k < hi) && tile_ok[t + k] != 0;
        const bool better = valid & (v < best_d);   // ascending t and a strict compare: ties stay with the lowest t
        best_d = better ? v : best_d;
        best_t = better ? t0 + t + k : best_t;
      }
    }
  }
  sd[wave][lane] = best_d;
  sj[wave][lane] = best_t;
  const int any_bad = __syncthreads_or(bad);   // (also the barrier between the writes above and wave 0's reads)
  if (any_bad && threadIdx.x == 0) atomicOr(&w.ctl->status, EYOC_HCLOSS_BAD_INDEX);
  if (wave != 0) return;
#pragma unroll
  for (int v = 1; v < HC_WAVES; ++v) {
    const float e1 = sd[v][lane];
    const int k1 = sj[v][lane];
    const bool take = (e1 < best_d) | ((e1 == best_d) & (k1 < best_t));
    best_d = take ? e1 : best_d;
    best_t = take ? k1 : best_t;
  }
  if (ok && best_t != NO_T)
    atomicMax(&w.best[(size_t)dir * n_used + p], ~(((unsigned long long)__float_as_uint(best_d) << 32) | (unsigned int)best_t));
}

// one wave per 64 positives and direction (lane = positive): the merged minimum, the two values of the positive rounded once, the key
// lookup, the fp32 terms and the workgroup's fp64 sums
template <int C>
__global__ __launch_bounds__(64) void hc_terms_kernel(const float* __restrict__ F0, int n0, const float* __restrict__ F1, int n1,
                                                      const long long* __restrict__ pairs, int n_pairs,
                                                      const long long* __restrict__ used, int n_used,
                                                      const long long* __restrict__ sel0, int s0, const long long* __restrict__ sel1,
                                                      int s1, float pos_thresh, float neg_thresh, HcWs w) {
#pragma clang fp contract(off)
  const int dir = blockIdx.y;
  const int lane = threadIdx.x;
  const float* __restrict__ FB = dir ? F0 : F1;
  const long long* __restrict__ sel = dir ? sel0 : sel1;
  const int s = dir ? s0 : s1;
  const int p = blockIdx.x * HC_A + lane;
  int bad = 0;
  long long i, j;
  float a[C];
  const bool ok = load_anchor<C>(p, dir, F0, n0, F1, n1, pairs, n_pairs, used, n_used, a, i, j, bad);
  if (bad) atomicOr(&w.ctl->status, EYOC_HCLOSS_BAD_INDEX);
  double pos_term = 0.0, neg_term = 0.0;
  int kept = 0;
  if (ok) {
    unsigned int flags = EYOC_HCLOSS_VALID;
    float dist = 0.0f;
    int tstar = -1;
    const unsigned long long raw = w.best[(size_t)dir * n_used + p];   // 0: no candidate was compared
    const int best_t = (int)(unsigned int)(~raw & 0xFFFFFFFFull);
    if (raw != 0ull && best_t >= 0 && best_t < s) {
      tstar = best_t;
      const unsigned long long scale = (unsigned long long)(n0 > n1 ? n0 : n1);
      const unsigned long long r = (unsigned long long)sel[best_t];   // in range: only checked candidates are compared
      dist = (float)sqrt(row_d2(a, FB + (size_t)r * C) + (double)1e-7f);   // the value of the chosen pair, rounded once
      const unsigned long long key = dir ? r + (unsigned long long)j * scale : (unsigned long long)i + r * scale;
      kept = key_member(w, key + 1ull) ? 0 : 1;
    }
    if (kept) {
      float h = neg_thresh - dist;
      h = h > 0.0f ? h : 0.0f;
      neg_term = (double)(h * h);
    } else {
      flags |= EYOC_HCLOSS_MASKED;
    }
    w.tstar[(size_t)dir * n_used + p] = tstar;
    w.dist[(size_t)dir * n_used + p] = dist;
    w.flags[(size_t)dir * n_used + p] = flags;
    if (dir == 0) {
      const float acc = (float)row_d2(a, F1 + (size_t)j * C);
      w.pos_d2[p] = acc;
      float h = acc - pos_thresh;
      h = h > 0.0f ? h : 0.0f;
      pos_term = (double)h;
    }
  } else if (p < n_used) {   // a positive with a bad index: nothing read, nothing counted
    w.tstar[(size_t)dir * n_used + p] = -1;
    w.dist[(size_t)dir * n_used + p] = 0.0f;
    w.flags[(size_t)dir * n_used + p] = EYOC_HCLOSS_MASKED;
    if (dir == 0) w.pos_d2[p] = 0.0f;
  }
  neg_term = wave_sum(neg_term);
  kept = wave_sum_i(kept);
  if (dir == 0) pos_term = wave_sum(pos_term);
  if (lane == 0) {
    w.part_sum[(size_t)(1 + dir) * w.nwg + blockIdx.x] = neg_term;
    w.part_cnt[(size_t)dir * w.nwg + blockIdx.x] = kept;
    if (dir == 0) w.part_sum[blockIdx.x] = pos_term;
  }
}

__global__ __launch_bounds__(HC_THREADS) void hc_final_kernel(int n_used, HcWs w, eyoc_hcloss_record* __restrict__ out) {
#pragma clang fp contract(off)
  double sum[3];
  int cnt[2];
  const auto add = [&](int b, double (&v)[3], int (&c)[2]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += w.part_sum[(size_t)k * w.nwg + b];
#pragma unroll
    for (int k = 0; k < 2; ++k) c[k] += w.part_cnt[(size_t)k * w.nwg + b];
  };
  if (!block_sum_ordered(w.nwg, add, sum, cnt)) return;
  eyoc_hcloss_record r;
  r.sum_pos = sum[0]; r.sum01 = sum[1]; r.sum10 = sum[2];
  r.n_used = n_used; r.k01 = cnt[0]; r.k10 = cnt[1];
  r.status = w.ctl->status;
  const float nan = __builtin_nanf("");
  // a mean over nothing is 0 / 0 = NaN, the reference's value
  r.pos_loss = r.status ? nan : (float)(sum[0] / (double)n_used);
  r.neg_loss = r.status ? nan : (float)((sum[1] / (double)cnt[0] + sum[2] / (double)cnt[1]) / 2.0);
  w.ctl->rec = r;
  *out = r;
}

// the scalar factor of each of a positive's three terms and the destination rows of its contributions
__global__ __launch_bounds__(HC_THREADS) void hc_weights_kernel(const long long* __restrict__ pairs, int n_pairs,
                                                                const long long* __restrict__ used, int n_used,
                                                                const long long* __restrict__ sel0, int s0,
                                                                const long long* __restrict__ sel1, int s1, int n0, int n1,
                                                                float pos_thresh, float neg_thresh, const float* __restrict__ g_pos,
                                                                const float* __restrict__ g_neg, HcWs w) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * HC_THREADS + threadIdx.x;
  if (p >= n_used) return;
  const size_t n = (size_t)n_used;
  const eyoc_hcloss_record rec = w.ctl->rec;
  const double gp = (double)*g_pos, gn = (double)*g_neg;
  const unsigned int f01 = w.flags[p], f10 = w.flags[n + p];
  const long long u = used ? used[p] : (long long)p;
  long long i = -1, j = -1;
  if (u >= 0 && u < n_pairs) {
    i = pairs[2 * (size_t)u];
    j = pairs[2 * (size_t)u + 1];
  }
  const bool valid = (f01 & f10 & EYOC_HCLOSS_VALID) && i >= 0 && i < n0 && j >= 0 && j < n1;
  float wp = 0.0f, w01 = 0.0f, w10 = 0.0f;
  long long r01 = -1, r10 = -1;   // rows of the hardest negatives in F1 / F0
  if (valid) {
    if (w.pos_d2[p] - pos_thresh > 0.0f) wp = (float)(gp * 2.0 / (double)rec.n_used);
    const int t01 = w.tstar[p], t10 = w.tstar[n + p];
    if (!(f01 & EYOC_HCLOSS_MASKED) && t01 >= 0 && t01 < s1 && rec.k01 > 0) {
      const float d = w.dist[p];
      const float h = neg_thresh - d;
      r01 = sel1[t01];
      if (h > 0.0f && r01 >= 0 && r01 < n1) w01 = (float)(-gn * (double)h / ((double)rec.k01 * (double)d));
    }
    if (!(f10 & EYOC_HCLOSS_MASKED) && t10 >= 0 && t10 < s0 && rec.k10 > 0) {
      const float d = w.dist[n + p];
      const float h = neg_thresh - d;
      r10 = sel0[t10];
      if (h > 0.0f && r10 >= 0 && r10 < n0) w10 = (float)(-gn * (double)h / ((double)rec.k10 * (double)d));
    }
  }
  w.wts[p] = wp;
  w.wts[n + p] = w01;
  w.wts[2 * n + p] = w10;
  int* dest0 = w.dest;            // rows of dF0: anchor entries (positive term + 01), candidate entries (10)
  int* dest1 = w.dest + 2 * n;    // rows of dF1: anchor entries (positive term + 10), candidate entries (01)
  dest0[p] = valid ? (int)i : -1;
  dest0[n + p] = w10 != 0.0f ? (int)r10 : -1;
  dest1[p] = valid ? (int)j : -1;
  dest1[n + p] = w01 != 0.0f ? (int)r01 : -1;
}

// One workgroup per entry of a matrix's destination list; the first entry of a row does the row: it gathers the row's later entries in
// order (256 at a time, compacted through ballots).  C lanes take one entry (lane = channel), 256 / C entries side by side: entry k of
// the ROW'S list goes to slot k mod (256 / C), the slots are added in order.  (Tried: one barrier-synchronised scan from the start of
// the list in rounds of 1024 entries instead of the barrier-free first-entry loop - 107 against 65 us at n_used = 4096, dropped.)
template <int C>
__global__ __launch_bounds__(HC_THREADS) void hc_rows_kernel(const float* __restrict__ F0, const float* __restrict__ F1,
                                                             const long long* __restrict__ pairs, const long long* __restrict__ used,
                                                             const long long* __restrict__ sel0, const long long* __restrict__ sel1,
                                                             int n_used, HcWs w, float* __restrict__ dF0, float* __restrict__ dF1) {
#pragma clang fp contract(off)
  constexpr int G = HC_THREADS / C;
  __shared__ int list[HC_LIST];
  __shared__ int wcnt[HC_WAVES];
  __shared__ double slot_acc[HC_THREADS];
  const int m = blockIdx.y;   // 0: dF0, 1: dF1
  const int E = 2 * n_used, e = blockIdx.x;
  const size_t n = (size_t)n_used;
  const int* __restrict__ dest = w.dest + (size_t)m * 2 * n;
  const int row = dest[e];
  if (row < 0) return;
  // the first entry of the row?  (a loop without barriers: most workgroups are first, or leave here)
  int found = 0;
  for (int k = threadIdx.x; k < e; k += HC_THREADS) found |= dest[k] == row ? 1 : 0;
  if (__syncthreads_or(found)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = threadIdx.x / C, ch = threadIdx.x % C;
  const float* __restrict__ wp = w.wts;
  const float* __restrict__ w01 = w.wts + n;
  const float* __restrict__ w10 = w.wts + 2 * n;
  const int* __restrict__ t01 = w.tstar;
  const int* __restrict__ t10 = w.tstar + n;
  double acc = 0.0;
  int rank0 = 0;   // position in the row's list of list[0]
  int pos = e;
  while (pos < E) {
    int cnt = 0;
    while (pos < E && cnt + HC_THREADS <= HC_LIST) {
      const int k = pos + threadIdx.x;
      const bool hit = k < E && dest[k] == row;
      const unsigned long long bal = __ballot(hit);
      if (lane == 0) wcnt[wave] = __popcll(bal);
      __syncthreads();
      int off = cnt, tot = 0;
#pragma unroll
      for (int x = 0; x < HC_WAVES; ++x) {
        const int c = wcnt[x];
        off += x < wave ? c : 0;
        tot += c;
      }
      if (hit) list[off + __popcll(bal & ((1ull << lane) - 1ull))] = k;
      __syncthreads();
      cnt += tot;
      pos += HC_THREADS;
    }
    for (int q = (slot - rank0 % G + G) % G; q < cnt; q += G) {
      const int k = list[q];
      const int p = k < n_used ? k : k - n_used;
      const long long u = used ? used[p] : (long long)p;
      const long long i = pairs[2 * (size_t)u], j = pairs[2 * (size_t)u + 1];   // (checked by hc_weights_kernel: dest >= 0)
      if (k < n_used) {
        const float a0 = F0[(size_t)i * C + ch], a1 = F1[(size_t)j * C + ch];
        const float own = m ? a1 : a0, other = m ? a0 : a1;
        acc += (double)(wp[p] * (own - other));
        const float wn = m ? w10[p] : w01[p];
        if (wn != 0.0f) {
          const float b = m ? F0[(size_t)sel0[t10[p]] * C + ch] : F1[(size_t)sel1[t01[p]] * C + ch];
          acc += (double)(wn * (own - b));
        }
      } else {
        // a candidate entry: this row is the hardest negative b of positive p in the other matrix's direction
        const float an = m ? F0[(size_t)i * C + ch] : F1[(size_t)j * C + ch];
        const float b = m ? F1[(size_t)row * C + ch] : F0[(size_t)row * C + ch];
        const float wn = m ? w01[p] : w10[p];
        acc += (double)(-(wn * (an - b)));
      }
    }
    rank0 += cnt;
    __syncthreads();   // the list is rewritten by the next pass
  }
  slot_acc[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x >= C) return;
  double total = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) total += slot_acc[g * C + threadIdx.x];
  float* __restrict__ dF = m ? dF1 : dF0;
  dF[(size_t)row * C + threadIdx.x] = w.ctl->rec.status ? __builtin_nanf("") : (float)total;
}

// the first three launches of a forward, shared by the hardest-contrastive and the triplet losses: the fill (control block, key table,
// search minima), the key table with the index check, the search of both directions
int launch_prep_search(const float* F0, int n0, const float* F1, int n1, int c, const long long* P, int n_pairs, const long long* U, int n_used,
                       const long long* S0, int s0, const long long* S1, int s1, const HcWs& w, hipStream_t st) {
  EYOC_CHECK_HIP(hipMemsetAsync(w.ctl, 0, w.fill_bytes, st));
  int n_max = n_pairs;
  n_max = n_used > n_max ? n_used : n_max;
  n_max = s0 > n_max ? s0 : n_max;
  n_max = s1 > n_max ? s1 : n_max;
  int pg = cdiv(n_max, HC_THREADS);
  pg = pg < 1 ? 1 : (pg > 4096 ? 4096 : pg);
  hipLaunchKernelGGL(hc_prep_kernel, dim3(pg), dim3(HC_THREADS), 0, st, P, n_pairs, U, n_used, S0, s0, S1, s1, n0, n1, n_max, w);
  // the candidate tiles split over grid.z until ~512 workgroups are in flight (the answer does not depend on the split)
  const int s_max = s0 > s1 ? s0 : s1;
  int tiles = cdiv(s_max, HC_T), zs = cdiv(512, 2 * w.nwg);
  tiles = tiles < 1 ? 1 : tiles;
  zs = zs > tiles ? tiles : zs;
  const dim3 grid(w.nwg, 2, zs);
  for_width(c, [&](auto cc) {
    hipLaunchKernelGGL((hc_search_kernel<decltype(cc)::value>), grid, dim3(HC_THREADS), 0, st, F0, n0, F1, n1, P, n_pairs, U, n_used, S0, s0,
                       S1, s1, w);
  });
  return EYOC_OK;
}

int check_args(const char* what, const eyoc_ctx* ctx, const void* F0, int n0, const void* F1, int n1, int c, const void* pairs, int n_pairs,
               const void* used, int n_used, const void* sel0, int s0, const void* sel1, int s1, const void* ws, size_t ws_bytes) {
  EYOC_REQUIRE(ctx, EYOC_ERR_INVALID, "%s: NULL ctx", what);
  EYOC_REQUIRE(c == 16 || c == 32 || c == 64, EYOC_ERR_INVALID, "%s: feature dimension %d not supported (16/32/64)", what, c);
  EYOC_REQUIRE(n0 >= 0 && n1 >= 0 && n_pairs >= 0 && n_used >= 0 && s0 >= 0 && s1 >= 0, EYOC_ERR_INVALID, "%s: negative count", what);
  EYOC_REQUIRE(n_pairs <= (1 << 28) && n_used <= (1 << 28), EYOC_ERR_INVALID, "%s: more than 2^28 positives", what);
  EYOC_REQUIRE(used || n_used == n_pairs || n_used == 0, EYOC_ERR_INVALID, "%s: used = NULL means all positives, n_used %d != n_pairs %d", what, n_used,
               n_pairs);
  EYOC_REQUIRE((F0 || n0 == 0) && (F1 || n1 == 0) && (pairs || n_pairs == 0) && (sel0 || s0 == 0) && (sel1 || s1 == 0), EYOC_ERR_INVALID,
               "%s: NULL argument", what);
  EYOC_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "%s: the workspace must be 256-byte aligned", what);
  EYOC_REQUIRE(ws_bytes >= eyoc_hcloss_workspace_bytes(n_pairs, n_used, s0, s1, c), EYOC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed",
               what, ws_bytes, eyoc_hcloss_workspace_bytes(n_pairs, n_used, s0, s1, c));
  return EYOC_OK;
}

}  // namespace

extern "C" {

size_t eyoc_hcloss_workspace_bytes(int n_pairs, int n_used, int s0, int s1, int c) {
  (void)s0; (void)s1; (void)c;
  if (n_pairs < 0 || n_used < 0) return 0;
  return carve(nullptr, 0, n_pairs, n_used).total;
}

int eyoc_hcloss_workspace_layout(int n_pairs, int n_used, int s0, int s1, int c, eyoc_hcloss_layout* out) {
  EYOC_REQUIRE(out && n_pairs >= 0 && n_used >= 0 && s0 >= 0 && s1 >= 0, EYOC_ERR_INVALID, "eyoc_hcloss_workspace_layout: invalid argument");
  EYOC_REQUIRE(c == 16 || c == 32 || c == 64, EYOC_ERR_INVALID, "eyoc_hcloss_workspace_layout: feature dimension %d not supported", c);
  char* const base = (char*)(uintptr_t)4096;   // (a Carver without a base hands out no pointers: carve from a stand-in, never dereferenced)
  const HcWs w = carve(base, 0, n_pairs, n_used);
  out->anchors = HC_A;
  out->tile = HC_T;
  out->n_used = n_used;
  out->table_slots = (int32_t)(w.mask + 1);
  out->total = w.total;
  out->off_record = (uint64_t)((char*)w.ctl - base);
  out->off_tstar = (uint64_t)((char*)w.tstar - base);
  out->off_dist = (uint64_t)((char*)w.dist - base);
  out->off_pos_d2 = (uint64_t)((char*)w.pos_d2 - base);
  out->off_flags = (uint64_t)((char*)w.flags - base);
  return EYOC_OK;
}

int eyoc_hcloss_forward(eyoc_ctx* ctx, const float* F0, int n0, const float* F1, int n1, int c, const int64_t* pairs, int n_pairs,
                        const int64_t* used, int n_used, const int64_t* sel0, int s0, const int64_t* sel1, int s1, float pos_thresh,
                        float neg_thresh, eyoc_hcloss_record* record_out, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_args("eyoc_hcloss_forward", ctx, F0, n0, F1, n1, c, pairs, n_pairs, used, n_used, sel0, s0, sel1, s1, ws, ws_bytes))
    return rc;
  EYOC_REQUIRE(record_out, EYOC_ERR_INVALID, "eyoc_hcloss_forward: NULL record");
  hipStream_t st = (hipStream_t)stream;
  const HcWs w = carve(ws, ws_bytes, n_pairs, n_used);
  const long long* P = (const long long*)pairs;
  const long long* U = (const long long*)used;
  const long long* S0 = (const long long*)sel0;
  const long long* S1 = (const long long*)sel1;
  if (int rc = launch_prep_search(F0, n0, F1, n1, c, P, n_pairs, U, n_used, S0, s0, S1, s1, w, st)) return rc;
  const dim3 grid_terms(w.nwg, 2);
  for_width(c, [&](auto cc) {
    hipLaunchKernelGGL((hc_terms_kernel<decltype(cc)::value>), grid_terms, dim3(64), 0, st, F0, n0, F1, n1, P, n_pairs, U, n_used, S0, s0, S1,
                       s1, pos_thresh, neg_thresh, w);
  });
  hipLaunchKernelGGL(hc_final_kernel, dim3(1), dim3(HC_THREADS), 0, st, n_used, w, record_out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_hcloss_backward(eyoc_ctx* ctx, const float* F0, int n0, const float* F1, int n1, int c, const int64_t* pairs, int n_pairs,
                         const int64_t* used, int n_used, const int64_t* sel0, int s0, const int64_t* sel1, int s1, float pos_thresh,
                         float neg_thresh, const float* g_pos, const float* g_neg, float* dF0, float* dF1, void* ws, size_t ws_bytes,
                         void* stream) {
  if (int rc = check_args("eyoc_hcloss_backward", ctx, F0, n0, F1, n1, c, pairs, n_pairs, used, n_used, sel0, s0, sel1, s1, ws, ws_bytes))
    return rc;
  EYOC_REQUIRE(g_pos && g_neg && (dF0 || n0 == 0) && (dF1 || n1 == 0), EYOC_ERR_INVALID, "eyoc_hcloss_backward: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const HcWs w = carve(ws, ws_bytes, n_pairs, n_used);
  const long long* P = (const long long*)pairs;
  const long long* U = (const long long*)used;
  const long long* S0 = (const long long*)sel0;
  const long long* S1 = (const long long*)sel1;
  if (int rc = zero_gradients(dF0, n0, dF1, n1, c, st)) return rc;
  if (n_used == 0) return EYOC_OK;   // no positive, no contribution
  hipLaunchKernelGGL(hc_weights_kernel, dim3(cdiv(n_used, HC_THREADS)), dim3(HC_THREADS), 0, st, P, n_pairs, U, n_used, S0, s0, S1, s1, n0,
                     n1, pos_thresh, neg_thresh, g_pos, g_neg, w);
  const dim3 grid(2 * n_used, 2);
  for_width(c, [&](auto cc) {
    hipLaunchKernelGGL((hc_rows_kernel<decltype(cc)::value>), grid, dim3(HC_THREADS), 0, st, F0, F1, P, U, S0, S1, n_used, w, dF0, dF1);
  });
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// The backward the triplet and the contrastive losses share: a weights kernel of the loss writes one contribution entry per (term,
// destination row), sort_and_sum_rows sorts (destination, entry number) stably and rows_kernel sums every run of equal destinations.
namespace {

// the destination of an entry as a sort key: 0 is the empty entry and sorts ahead of every row
__host__ __device__ inline unsigned int contrib_key(unsigned int row, int matrix) { return 2u * row + (unsigned int)matrix + 1u; }
__host__ __device__ inline int key_matrix(unsigned int key) { return (int)((key - 1u) & 1u); }
__host__ __device__ inline size_t key_row(unsigned int key) { return (size_t)((key - 1u) >> 1); }

struct Contrib {
  int ncon;                    // entries
  unsigned int *key, *key_s;   // contrib_key of the destination; sorted
  int *idx, *idx_s;            // entry numbers; sorted along
  float *w, *w2;               // the factor of an entry; its second factor (0: none), NULL in a list of one factor
  int *r, *r2;                 // the rows of the OTHER matrix they scale the difference to
  void* sort_tmp;
  size_t sort_bytes;
  const unsigned int* status;  // the status word of the loss's record (set by the loss's carve)
};

Contrib carve_contrib(Carver& cv, int ncon, bool two_factors) {
  Contrib l;
  const size_t nc = (size_t)ncon;
  l.ncon = ncon;
  l.key = cv.take<unsigned int>(nc);
  l.key_s = cv.take<unsigned int>(nc);
  l.idx = cv.take<int>(nc);
  l.idx_s = cv.take<int>(nc);
  l.w = cv.take<float>(nc);
  l.w2 = two_factors ? cv.take<float>(nc) : nullptr;
  l.r = cv.take<int>(nc);
  l.r2 = two_factors ? cv.take<int>(nc) : nullptr;
  l.sort_bytes = align_up(sort_rows_tmp_bytes(ncon, 32));
  l.sort_tmp = cv.take<char>(l.sort_bytes);
  l.status = nullptr;
  return l;
}

// what follows the HcWs a loss's workspace starts with
Carver carver_behind(const HcWs& hc, void* base, size_t bytes) {
  return Carver(base ? (char*)base + hc.total : nullptr, bytes > hc.total ? bytes - hc.total : 0);
}

// One workgroup per position of the sorted list.  The first position of a run of equal destinations does the row: C lanes take one entry
// (lane = channel), 256 / C entries side by side, entry k of the run goes to slot k mod (256 / C), fp64 accumulators, the slots are added
// in order and rounded once.  Every other position leaves after two loads, so the list is read a bounded number of times however long a
// run is.  TWO: the entries carry a second factor and row.  (The loop bound is q < ncon - k, not k + q < ncon: with the latter the compiler
// indexes key_s from k + q in every step instead of stepping a pointer, +1.2 % on the kernel at 3.2 M entries.)
template <int C, bool TWO>
__global__ __launch_bounds__(HC_THREADS) void rows_kernel(const float* __restrict__ F0, const float* __restrict__ F1, Contrib l,
                                                          float* __restrict__ dF0, float* __restrict__ dF1) {
#pragma clang fp contract(off)
  constexpr int G = HC_THREADS / C;
  __shared__ double slot_acc[HC_THREADS];
  const int k = blockIdx.x;
  const unsigned int key = l.key_s[k];
  if (key == 0u) return;
  if (k > 0 && l.key_s[k - 1] == key) return;
  const int m = key_matrix(key);
  const size_t row = key_row(key);
  const int slot = threadIdx.x / C, ch = threadIdx.x % C;
  const float* __restrict__ FO = m ? F0 : F1;   // the other matrix
  const double own = (double)(m ? F1 : F0)[row * C + ch];
  double acc = 0.0;
  for (int q = slot; q < l.ncon - k && l.key_s[k + q] == key; q += G) {
    const int e = l.idx_s[k + q];
    acc += (double)l.w[e] * (own - (double)FO[(size_t)l.r[e] * C + ch]);
    if constexpr (TWO) {
      const float wn = l.w2[e];
      if (wn != 0.0f) acc += (double)wn * (own - (double)FO[(size_t)l.r2[e] * C + ch]);
    }
  }
  slot_acc[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x >= C) return;
  double total = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) total += slot_acc[g * C + threadIdx.x];
  float* __restrict__ dF = m ? dF1 : dF0;
  dF[row * C + threadIdx.x] = *l.status ? __builtin_nanf("") : (float)total;
}

// the end of a backward, after the loss's weights kernel: the sort and the row sums
template <bool TWO>
int sort_and_sum_rows(const Contrib& l, const float* F0, int n0, const float* F1, int n1, int c, float* dF0, float* dF1, hipStream_t st) {
  // as many bits as the greatest key has; equal keys keep their entry order (a radix sort is stable)
  const unsigned long long top = contrib_key((unsigned int)(n0 > n1 ? n0 : n1) - 1u, 1);
  int bits = 1;
  while ((1ull << bits) <= top) ++bits;
  if (int rc = sort_rows_by_key(l.sort_tmp, l.sort_bytes, l.key, l.key_s, l.idx, l.idx_s, l.ncon, bits, st)) return rc;
  for_width(c, [&](auto cc) {
    hipLaunchKernelGGL((rows_kernel<decltype(cc)::value, TWO>), dim3(l.ncon), dim3(HC_THREADS), 0, st, F0, F1, l, dF0, dF1);
  });
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// Triplet and hardest-triplet loss (lib/trainer.py:567-621, :701-782; include/eyoc_hip.h has the contract).  The workspace starts with
// an HcWs of the same (n_pairs, n_used): hc_prep_kernel and hc_search_kernel run on it unchanged (key table, index check, t*).
// Forward, 5 launches: the fill, hc_prep_kernel, hc_search_kernel, tr_terms_kernel (grid.y = direction 01, direction 10, random triplets;
// lane = term), tr_final_kernel.  Backward: two fills, tr_weights_kernel (three contribution entries per term, entry number = sequence
// number), one stable sort of (destination, entry number) by rocPRIM's radix_sort_pairs, rows_kernel with two factors per entry (linear
// in the list).
namespace {

static_assert(sizeof(eyoc_triplet_record) == 96, "eyoc_triplet_record is 96 bytes");
static_assert(EYOC_TRIPLET_BAD_INDEX == EYOC_HCLOSS_BAD_INDEX, "hc_prep_kernel and hc_search_kernel set the shared status word");

struct TrWs {
  HcWs hc;                     // ctl (status), table, best; tstar, dist and flags [2][n_used] are used as the hcloss forward uses them
  eyoc_triplet_record* rec;
  float* pos_dist;             // [n_used]
  float* term;                 // [2][n_used]
  float *rpos, *rneg, *rterm;  // [n_rand]
  unsigned int* rflags;        // [n_rand]
  int nblk;                    // workgroups of the terms kernel per part (>= 1)
  double* part_sum;            // [3][nblk][3]
  int* part_cnt;               // [3][nblk]
  Contrib list;                // 3 (n_rand + 2 n_used) entries of two factors
  size_t total;
};

TrWs tr_carve(void* base, size_t bytes, int n_pairs, int n_used, int n_rand) {
  TrWs w;
  w.hc = carve(base, bytes, n_pairs, n_used);
  Carver cv = carver_behind(w.hc, base, bytes);
  const size_t n = (size_t)n_used, nr = (size_t)n_rand;
  w.rec = (eyoc_triplet_record*)cv.take<char>(256);
  w.pos_dist = cv.take<float>(n);
  w.term = cv.take<float>(2 * n);
  w.rpos = cv.take<float>(nr);
  w.rneg = cv.take<float>(nr);
  w.rterm = cv.take<float>(nr);
  w.rflags = cv.take<unsigned int>(nr);
  const int most = n_used > n_rand ? n_used : n_rand;
  w.nblk = most > 0 ? cdiv(most, HC_A) : 1;
  w.part_sum = cv.take<double>(9 * (size_t)w.nblk);
  w.part_cnt = cv.take<int>(3 * (size_t)w.nblk);
  w.list = carve_contrib(cv, 3 * (n_rand + 2 * n_used), true);
  w.list.status = w.rec ? &w.rec->status : nullptr;
  w.total = w.hc.total + align_up(cv.off);
  return w;
}

// grid (workgroups of 64 terms, part): part 0 / 1 = hardest direction 01 / 10 (lane = used positive), part 2 = random triplets
template <int C>
__global__ __launch_bounds__(64) void tr_terms_kernel(const float* __restrict__ F0, int n0, const float* __restrict__ F1, int n1,
                                                      const long long* __restrict__ pairs, int n_pairs,
                                                      const long long* __restrict__ used, int n_used,
                                                      const long long* __restrict__ sel0, int s0, const long long* __restrict__ sel1,
                                                      int s1, const long long* __restrict__ rand_idx,
                                                      const long long* __restrict__ negatives, int n_rand, float margin, TrWs w) {
#pragma clang fp contract(off)
  const int part = blockIdx.y;
  const int lane = threadIdx.x;
  const int e = blockIdx.x * HC_A + lane;
  const unsigned long long scale = (unsigned long long)(n0 > n1 ? n0 : n1);
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;   // the kept term; the positive distance (part 0) or the kept negative distance (part 2); d01 / d10
  int kept = 0, bad = 0;
  float a[C];
  if (part < 2) {
    const int dir = part, p = e;
    const long long* __restrict__ sel = dir ? sel0 : sel1;
    const float* __restrict__ FB = dir ? F0 : F1;
    const int s = dir ? s0 : s1;
    long long i, j;
    const bool ok = load_anchor<C>(p, dir, F0, n0, F1, n1, pairs, n_pairs, used, n_used, a, i, j, bad);
    if (ok) {
      const float pos = (float)sqrt(row_d2(a, dir ? F0 + (size_t)i * C : F1 + (size_t)j * C) + (double)1e-7f);
      unsigned int flags = EYOC_TRIPLET_VALID;
      float dist = 0.0f, term = 0.0f;
      int tstar = -1;
      const unsigned long long raw = s > 0 ? w.hc.best[(size_t)dir * n_used + p] : 0ull;   // 0: no candidate was compared
      const int best_t = (int)(unsigned int)(~raw & 0xFFFFFFFFull);
      if (raw != 0ull && best_t >= 0 && best_t < s) {
        tstar = best_t;
        const unsigned long long r = (unsigned long long)sel[best_t];   // in range: only checked candidates are compared
        dist = (float)sqrt(row_d2(a, FB + (size_t)r * C) + (double)1e-7f);
        v2 = (double)dist;
        const unsigned long long key = dir ? r + (unsigned long long)j * scale : (unsigned long long)i + r * scale;
        kept = key_member(w.hc, key + 1ull) ? 0 : 1;
      }
      if (kept) {
        const float t = (pos + margin) - dist;
        if (t > 0.0f) {
          term = t;
          flags |= EYOC_TRIPLET_ACTIVE;
        }
        v0 = (double)term;
      } else {
        flags |= EYOC_TRIPLET_MASKED;
      }
      w.hc.tstar[(size_t)dir * n_used + p] = tstar;
      w.hc.dist[(size_t)dir * n_used + p] = dist;
      w.hc.flags[(size_t)dir * n_used + p] = flags;
      w.term[(size_t)dir * n_used + p] = term;
      if (dir == 0) {
        w.pos_dist[p] = pos;
        v1 = (double)pos;
      }
    } else if (p < n_used) {   // a positive with a bad index: nothing read, nothing counted
      w.hc.tstar[(size_t)dir * n_used + p] = -1;
      w.hc.dist[(size_t)dir * n_used + p] = 0.0f;
      w.hc.flags[(size_t)dir * n_used + p] = EYOC_TRIPLET_MASKED;
      w.term[(size_t)dir * n_used + p] = 0.0f;
      if (dir == 0) w.pos_dist[p] = 0.0f;
    }
  } else if (e < n_rand) {
    const int r = e;
    const long long u = rand_idx[r], n = negatives[r];
    long long ia = -1, iq = -1;
    bool ok = u >= 0 && u < n_pairs && n >= 0 && n < n1;
    if (u >= 0 && u < n_pairs) {
      ia = pairs[2 * (size_t)u];
      iq = pairs[2 * (size_t)u + 1];
      ok = ok && ia >= 0 && ia < n0 && iq >= 0 && iq < n1;
    }
    float pos = 0.0f, neg = 0.0f, term = 0.0f;
    unsigned int flags = EYOC_TRIPLET_MASKED;
    if (!ok) {
      bad = 1;
    } else {
      flags = EYOC_TRIPLET_VALID;
      const unsigned long long key = (unsigned long long)ia + (unsigned long long)n * scale;
      if (key_member(w.hc, key + 1ull)) {
        flags |= EYOC_TRIPLET_MASKED;
      } else {
        const float4* src = reinterpret_cast<const float4*>(F0 + (size_t)ia * C);
#pragma unroll
        for (int q = 0; q < C / 4; ++q) {
          const float4 v = src[q];
          a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
        }
        pos = (float)sqrt(row_d2(a, F1 + (size_t)iq * C) + (double)1e-7f);
        neg = (float)sqrt(row_d2(a, F1 + (size_t)n * C) + (double)1e-7f);
        const float t = (pos + margin) - neg;
        if (t > 0.0f) {
          term = t;
          flags |= EYOC_TRIPLET_ACTIVE;
        }
        kept = 1;
        v0 = (double)term;
        v1 = (double)neg;
      }
    }
    w.rpos[r] = pos;
    w.rneg[r] = neg;
    w.rterm[r] = term;
    w.rflags[r] = flags;
  }
  if (bad) atomicOr(&w.hc.ctl->status, EYOC_TRIPLET_BAD_INDEX);
  v0 = wave_sum(v0);
  v1 = wave_sum(v1);
  v2 = wave_sum(v2);
  kept = wave_sum_i(kept);
  if (lane == 0) {
    double* ps = w.part_sum + ((size_t)part * w.nblk + blockIdx.x) * 3;
    ps[0] = v0; ps[1] = v1; ps[2] = v2;
    w.part_cnt[(size_t)part * w.nblk + blockIdx.x] = kept;
  }
}

__global__ __launch_bounds__(HC_THREADS) void tr_final_kernel(int n_pairs, int n_used, int n_rand, int hardest, TrWs w,
                                                              eyoc_triplet_record* __restrict__ out) {
#pragma clang fp contract(off)
  double sum[9];
  int cnt[3];
  const auto add = [&](int b, double (&v)[9], int (&c)[3]) {
#pragma unroll
    for (int part = 0; part < 3; ++part) {
#pragma unroll
      for (int k = 0; k < 3; ++k) v[3 * part + k] += w.part_sum[((size_t)part * w.nblk + b) * 3 + k];
      c[part] += w.part_cnt[(size_t)part * w.nblk + b];
    }
  };
  if (!block_sum_ordered(w.nblk, add, sum, cnt)) return;
  eyoc_triplet_record r;
  r.sum01 = sum[0]; r.sum_pos_dist = sum[1]; r.sum_d01 = sum[2];
  r.sum10 = sum[3]; r.sum_d10 = sum[5];
  r.sum_rand = sum[6]; r.sum_rand_neg = sum[7];
  r.n_used = n_used; r.n_rand = n_rand; r.k_rand = cnt[2]; r.k01 = cnt[0]; r.k10 = cnt[1];
  r.status = w.hc.ctl->status;
  r.reserved = 0;
  const float nan = __builtin_nanf("");
  const bool none = r.status != 0u || n_used == 0 || n_pairs == 0;
  const double K = (double)(cnt[0] + cnt[1] + cnt[2]);
  // a mean over nothing is 0 / 0 = NaN, the reference's value
  r.loss = none ? nan : (float)(((r.sum_rand + r.sum01) + r.sum10) / K);
  r.pos_dist_mean = none ? nan : (float)(r.sum_pos_dist / (double)n_used);
  r.neg_dist_mean = none ? nan
                         : (hardest ? (float)((r.sum_d01 / (double)n_used + r.sum_d10 / (double)n_used) / 2.0)
                                    : (float)(r.sum_rand_neg / (double)cnt[2]));
  *w.rec = r;
  *out = r;
}

// one thread per term: its three contribution entries (anchor, positive, negative), or three empty ones
__global__ __launch_bounds__(HC_THREADS) void tr_weights_kernel(const long long* __restrict__ pairs, int n_pairs,
                                                                const long long* __restrict__ used, int n_used,
                                                                const long long* __restrict__ sel0, int s0,
                                                                const long long* __restrict__ sel1, int s1,
                                                                const long long* __restrict__ rand_idx,
                                                                const long long* __restrict__ negatives, int n_rand, int n0, int n1,
                                                                const float* __restrict__ g, TrWs w) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * HC_THREADS + threadIdx.x;
  if (t >= n_rand + 2 * n_used) return;
  const eyoc_triplet_record rec = *w.rec;
  const long long K = (long long)rec.k_rand + rec.k01 + rec.k10;
  long long ra = -1, rq = -1, rn = -1;   // rows of the anchor, the positive and the negative
  int mA = 0;                            // the anchor's matrix
  float pos = 0.0f, neg = 0.0f;
  bool emit = false;
  if (t < n_rand) {
    if (w.rflags[t] & EYOC_TRIPLET_ACTIVE) {
      const long long u = rand_idx[t];
      rn = negatives[t];
      if (u >= 0 && u < n_pairs) {
        ra = pairs[2 * (size_t)u];
        rq = pairs[2 * (size_t)u + 1];
      }
      pos = w.rpos[t];
      neg = w.rneg[t];
      emit = ra >= 0 && ra < n0 && rq >= 0 && rq < n1 && rn >= 0 && rn < n1;
    }
  } else {
    const int dir = t - n_rand >= n_used ? 1 : 0;
    const int p = t - n_rand - dir * n_used;
    if (w.hc.flags[(size_t)dir * n_used + p] & EYOC_TRIPLET_ACTIVE) {
      const long long u = used ? used[p] : (long long)p;
      long long i = -1, j = -1;
      if (u >= 0 && u < n_pairs) {
        i = pairs[2 * (size_t)u];
        j = pairs[2 * (size_t)u + 1];
      }
      const int tt = w.hc.tstar[(size_t)dir * n_used + p];
      const int s = dir ? s0 : s1;
      if (tt >= 0 && tt < s) rn = dir ? sel0[tt] : sel1[tt];
      mA = dir;
      ra = dir ? j : i;
      rq = dir ? i : j;
      pos = w.pos_dist[p];
      neg = w.hc.dist[(size_t)dir * n_used + p];
      const int nA = dir ? n1 : n0, nO = dir ? n0 : n1;
      emit = ra >= 0 && ra < nA && rq >= 0 && rq < nO && rn >= 0 && rn < nO;
    }
  }
  emit = emit && K > 0 && n_used > 0 && n_pairs > 0;
  unsigned int key[3] = {0u, 0u, 0u};
  float wq = 0.0f, wn = 0.0f;
  if (emit) {
    const double gk = (double)*g / (double)K;
    wq = (float)(gk / (double)pos);
    wn = (float)(-gk / (double)neg);
    key[0] = contrib_key((unsigned int)ra, mA);
    key[1] = contrib_key((unsigned int)rq, 1 - mA);
    key[2] = contrib_key((unsigned int)rn, 1 - mA);
  }
  const Contrib& l = w.list;
  const size_t e = 3 * (size_t)t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    l.key[e + k] = key[k];
    l.idx[e + k] = (int)(e + k);
  }
  l.w[e] = wq;     l.w2[e] = wn;       l.r[e] = (int)rq;     l.r2[e] = (int)rn;
  l.w[e + 1] = wq; l.w2[e + 1] = 0.0f; l.r[e + 1] = (int)ra; l.r2[e + 1] = 0;
  l.w[e + 2] = wn; l.w2[e + 2] = 0.0f; l.r[e + 2] = (int)ra; l.r2[e + 2] = 0;
}

int tr_check_args(const char* what, const eyoc_ctx* ctx, const void* F0, int n0, const void* F1, int n1, int c, const void* pairs,
                  int n_pairs, const void* used, int n_used, const void* sel0, int s0, const void* sel1, int s1, const void* rand_idx,
                  const void* negatives, int n_rand, const void* ws, size_t ws_bytes) {
  EYOC_REQUIRE(ctx, EYOC_ERR_INVALID, "%s: NULL ctx", what);
  EYOC_REQUIRE(c == 16 || c == 32 || c == 64, EYOC_ERR_INVALID, "%s: feature dimension %d not supported (16/32/64)", what, c);
  EYOC_REQUIRE(n0 >= 0 && n1 >= 0 && n_pairs >= 0 && n_used >= 0 && s0 >= 0 && s1 >= 0 && n_rand >= 0, EYOC_ERR_INVALID,
               "%s: negative count", what);
  EYOC_REQUIRE(n0 <= (1 << 30) && n1 <= (1 << 30), EYOC_ERR_INVALID, "%s: more than 2^30 rows", what);
  EYOC_REQUIRE(n_pairs <= (1 << 28) && n_used <= (1 << 26) && n_rand <= (1 << 26), EYOC_ERR_INVALID,
               "%s: more than 2^28 positives, 2^26 used positives or 2^26 random triplets", what);
  EYOC_REQUIRE((s0 == 0) == (s1 == 0), EYOC_ERR_INVALID, "%s: s0 %d and s1 %d: both zero (no hardest parts) or both positive", what, s0, s1);
  EYOC_REQUIRE(used || n_used == n_pairs || n_used == 0, EYOC_ERR_INVALID, "%s: used = NULL means all positives, n_used %d != n_pairs %d", what, n_used,
               n_pairs);
  EYOC_REQUIRE((F0 || n0 == 0) && (F1 || n1 == 0) && (pairs || n_pairs == 0) && (sel0 || s0 == 0) && (sel1 || s1 == 0) &&
                   ((rand_idx && negatives) || n_rand == 0),
               EYOC_ERR_INVALID, "%s: NULL argument", what);
  EYOC_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "%s: the workspace must be 256-byte aligned", what);
  const size_t need = eyoc_triplet_workspace_bytes(n_pairs, n_used, s0, s1, n_rand, c);
  EYOC_REQUIRE(ws_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
  return EYOC_OK;
}

}  // namespace

extern "C" {

size_t eyoc_triplet_workspace_bytes(int n_pairs, int n_used, int s0, int s1, int n_rand, int c) {
  (void)s0; (void)s1; (void)c;
  if (n_pairs < 0 || n_used < 0 || n_rand < 0 || n_used > (1 << 26) || n_rand > (1 << 26)) return 0;
  return tr_carve(nullptr, 0, n_pairs, n_used, n_rand).total;
}

int eyoc_triplet_workspace_layout(int n_pairs, int n_used, int s0, int s1, int n_rand, int c, eyoc_triplet_layout* out) {
  EYOC_REQUIRE(out && n_pairs >= 0 && n_used >= 0 && s0 >= 0 && s1 >= 0 && n_rand >= 0 && n_used <= (1 << 26) && n_rand <= (1 << 26),
               EYOC_ERR_INVALID, "eyoc_triplet_workspace_layout: invalid argument");
  EYOC_REQUIRE(c == 16 || c == 32 || c == 64, EYOC_ERR_INVALID, "eyoc_triplet_workspace_layout: feature dimension %d not supported", c);
  char* const base = (char*)(uintptr_t)4096;   // (a stand-in base, never dereferenced)
  const TrWs w = tr_carve(base, 0, n_pairs, n_used, n_rand);
  out->anchors = HC_A;
  out->tile = HC_T;
  out->n_used = n_used;
  out->n_rand = n_rand;
  out->table_slots = (int32_t)(w.hc.mask + 1);
  out->n_contrib = w.list.ncon;
  out->total = w.total;
  out->off_record = (uint64_t)((char*)w.rec - base);
  out->off_tstar = (uint64_t)((char*)w.hc.tstar - base);
  out->off_dist = (uint64_t)((char*)w.hc.dist - base);
  out->off_pos_dist = (uint64_t)((char*)w.pos_dist - base);
  out->off_term = (uint64_t)((char*)w.term - base);
  out->off_flags = (uint64_t)((char*)w.hc.flags - base);
  out->off_rand_pos = (uint64_t)((char*)w.rpos - base);
  out->off_rand_neg = (uint64_t)((char*)w.rneg - base);
  out->off_rand_term = (uint64_t)((char*)w.rterm - base);
  out->off_rand_flags = (uint64_t)((char*)w.rflags - base);
  out->off_contrib_key = (uint64_t)((char*)w.list.key - base);
  return EYOC_OK;
}

int eyoc_triplet_forward(eyoc_ctx* ctx, const float* F0, int n0, const float* F1, int n1, int c, const int64_t* pairs, int n_pairs,
                         const int64_t* used, int n_used, const int64_t* sel0, int s0, const int64_t* sel1, int s1,
                         const int64_t* rand_idx, const int64_t* negatives, int n_rand, float margin, eyoc_triplet_record* record_out,
                         void* ws, size_t ws_bytes, void* stream) {
  if (int rc = tr_check_args("eyoc_triplet_forward", ctx, F0, n0, F1, n1, c, pairs, n_pairs, used, n_used, sel0, s0, sel1, s1, rand_idx,
                             negatives, n_rand, ws, ws_bytes))
    return rc;
  EYOC_REQUIRE(record_out, EYOC_ERR_INVALID, "eyoc_triplet_forward: NULL record");
  hipStream_t st = (hipStream_t)stream;
  const TrWs w = tr_carve(ws, ws_bytes, n_pairs, n_used, n_rand);
  const long long* P = (const long long*)pairs;
  const long long* U = (const long long*)used;
  const long long* S0 = (const long long*)sel0;
  const long long* S1 = (const long long*)sel1;
  const long long* RI = (const long long*)rand_idx;
  const long long* NG = (const long long*)negatives;
  // (rand_idx and negatives are checked by the terms kernel, the only reader of both)
  if (int rc = launch_prep_search(F0, n0, F1, n1, c, P, n_pairs, U, n_used, S0, s0, S1, s1, w.hc, st)) return rc;
  const dim3 grid_terms(w.nblk, 3);
  for_width(c, [&](auto cc) {
    hipLaunchKernelGGL((tr_terms_kernel<decltype(cc)::value>), grid_terms, dim3(64), 0, st, F0, n0, F1, n1, P, n_pairs, U, n_used, S0, s0, S1,
                       s1, RI, NG, n_rand, margin, w);
  });
  hipLaunchKernelGGL(tr_final_kernel, dim3(1), dim3(HC_THREADS), 0, st, n_pairs, n_used, n_rand, s1 > 0 ? 1 : 0, w, record_out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_triplet_backward(eyoc_ctx* ctx, const float* F0, int n0, const float* F1, int n1, int c, const int64_t* pairs, int n_pairs,
                          const int64_t* used, int n_used, const int64_t* sel0, int s0, const int64_t* sel1, int s1,
                          const int64_t* rand_idx, const int64_t* negatives, int n_rand, float margin, const float* g, float* dF0,
                          float* dF1, void* ws, size_t ws_bytes, void* stream) {
  (void)margin;
  if (int rc = tr_check_args("eyoc_triplet_backward", ctx, F0, n0, F1, n1, c, pairs, n_pairs, used, n_used, sel0, s0, sel1, s1, rand_idx,
                             negatives, n_rand, ws, ws_bytes))
    return rc;
  EYOC_REQUIRE(g && (dF0 || n0 == 0) && (dF1 || n1 == 0), EYOC_ERR_INVALID, "eyoc_triplet_backward: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const TrWs w = tr_carve(ws, ws_bytes, n_pairs, n_used, n_rand);
  if (int rc = zero_gradients(dF0, n0, dF1, n1, c, st)) return rc;
  if (n_used == 0 || n_pairs == 0) return EYOC_OK;   // no term, no contribution
  hipLaunchKernelGGL(tr_weights_kernel, dim3(cdiv(n_rand + 2 * n_used, HC_THREADS)), dim3(HC_THREADS), 0, st, (const long long*)pairs,
                     n_pairs, (const long long*)used, n_used, (const long long*)sel0, s0, (const long long*)sel1, s1,
                     (const long long*)rand_idx, (const long long*)negatives, n_rand, n0, n1, g, w);
  return sort_and_sum_rows<true>(w.list, F0, n0, F1, n1, c, dF0, dF1, st);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// Random-negative contrastive loss of the reference's base trainer (lib/trainer.py:201-221 and :262-286; include/eyoc_hip.h has the
// contract).  The workspace starts with an HcWs of (n_pairs, 0 used positives): hc_prep_kernel runs on it unchanged (key table, index check
// of the positives).  Forward, 4 launches: the fill (control block + key table), hc_prep_kernel, cl_terms_kernel (grid.y = positives,
// candidate negatives; lane = term), cl_final_kernel.  Backward: two fills, cl_weights_kernel (two contribution entries per term, entry
// number = sequence number), one stable sort of (destination, entry number) by rocPRIM's radix_sort_pairs, rows_kernel with one factor
// per entry.
namespace {

static_assert(sizeof(eyoc_closs_record) == 48, "eyoc_closs_record is 48 bytes");
static_assert(EYOC_CLOSS_BAD_INDEX == EYOC_HCLOSS_BAD_INDEX, "hc_prep_kernel sets the shared status word");

struct ClWs {
  HcWs hc;                     // ctl (status) and the key table; nothing else of it is used
  eyoc_closs_record* rec;
  float* pos_d2;               // [n_pairs]
  float *dist, *term;          // [n_neg]
  unsigned int* flags;         // [n_neg]
  int nblk;                    // workgroups of the terms kernel per part (>= 1)
  double* part_sum;            // [2][nblk]: positives, kept candidates
  int* part_cnt;               // [2][nblk]: kept, active
  Contrib list;                // 2 (n_pairs + n_neg) entries of one factor
  size_t total;
};

ClWs cl_carve(void* base, size_t bytes, int n_pairs, int n_neg) {
  ClWs w;
  w.hc = carve(base, bytes, n_pairs, 0);
  Carver cv = carver_behind(w.hc, base, bytes);
  const size_t np = (size_t)n_pairs, nn = (size_t)n_neg;
  w.rec = (eyoc_closs_record*)cv.take<char>(256);
  w.pos_d2 = cv.take<float>(np);
  w.dist = cv.take<float>(nn);
  w.term = cv.take<float>(nn);
  w.flags = cv.take<unsigned int>(nn);
  const int most = n_pairs > n_neg ? n_pairs : n_neg;
  w.nblk = most > 0 ? cdiv(most, HC_A) : 1;
  w.part_sum = cv.take<double>(2 * (size_t)w.nblk);
  w.part_cnt = cv.take<int>(2 * (size_t)w.nblk);
  w.list = carve_contrib(cv, 2 * (n_pairs + n_neg), false);
  w.list.status = w.rec ? &w.rec->status : nullptr;
  w.total = w.hc.total + align_up(cv.off);
  return w;
}

bool cl_counts_ok(int n_pairs, int n_neg) {
  return n_pairs >= 0 && n_neg >= 0 && (long long)n_pairs + (long long)n_neg < (1ll << 30);
}

// grid (workgroups of 64 terms, part): part 0 = positives (lane = p), part 1 = candidate negatives (lane = q)
template <int C>
__global__ __launch_bounds__(64) void cl_terms_kernel(const float* __restrict__ F0, int n0, const float* __restrict__ F1, int n1,
                                                      const long long* __restrict__ pairs, int n_pairs,
                                                      const long long* __restrict__ neg, int n_neg, float neg_thresh, ClWs w) {
#pragma clang fp contract(off)
  const int part = blockIdx.y;
  const int lane = threadIdx.x;
  const int e = blockIdx.x * HC_A + lane;
  const int count = part ? n_neg : n_pairs;
  double v = 0.0;
  int kept = 0, active = 0, bad = 0;
  if (e < count) {
    const long long* __restrict__ src = part ? neg : pairs;
    const long long i = src[2 * (size_t)e], j = src[2 * (size_t)e + 1];
    const bool ok = i >= 0 && i < n0 && j >= 0 && j < n1;   // checked before either becomes an address
    bool member = false;
    if (ok && part) {
      const unsigned long long scale = (unsigned long long)(n0 > n1 ? n0 : n1);
      member = key_member(w.hc, (unsigned long long)i + (unsigned long long)j * scale + 1ull);
    }
    double d2 = 0.0;
    if (ok && !member) {
      float a[C];
      const float4* row = reinterpret_cast<const float4*>(F0 + (size_t)i * C);
#pragma unroll
      for (int q = 0; q < C / 4; ++q) {
        const float4 x = row[q];
        a[4 * q] = x.x; a[4 * q + 1] = x.y; a[4 * q + 2] = x.z; a[4 * q + 3] = x.w;
      }
      d2 = row_d2(a, F1 + (size_t)j * C);
    }
    bad = ok ? 0 : 1;
    if (part == 0) {
      const float acc = ok ? (float)d2 : 0.0f;   // a positive with a bad index: nothing read, nothing added
      w.pos_d2[e] = acc;
      v = (double)acc;
    } else {
      unsigned int flags = ok ? EYOC_CLOSS_VALID : EYOC_CLOSS_MASKED;
      float dist = 0.0f, term = 0.0f;
      if (ok && member) flags |= EYOC_CLOSS_MASKED;
      if (ok && !member) {
        kept = 1;
        dist = (float)sqrt(d2 + (double)1e-4f);
        const float h = neg_thresh - dist;
        if (h > 0.0f) {
          term = h * h;
          flags |= EYOC_CLOSS_ACTIVE;
          active = 1;
        }
        v = (double)term;
      }
      w.dist[e] = dist;
      w.term[e] = term;
      w.flags[e] = flags;
    }
  }
  if (bad) atomicOr(&w.hc.ctl->status, EYOC_CLOSS_BAD_INDEX);
  v = wave_sum(v);
  kept = wave_sum_i(kept);
  active = wave_sum_i(active);
  if (lane == 0) {
    w.part_sum[(size_t)part * w.nblk + blockIdx.x] = v;
    if (part) {
      w.part_cnt[blockIdx.x] = kept;
      w.part_cnt[(size_t)w.nblk + blockIdx.x] = active;
    }
  }
}

__global__ __launch_bounds__(HC_THREADS) void cl_final_kernel(int n_pairs, int n_neg, ClWs w, eyoc_closs_record* __restrict__ out) {
#pragma clang fp contract(off)
  double sum[2];
  int cnt[2];
  const auto add = [&](int b, double (&v)[2], int (&c)[2]) {   // (a workgroup past the end of its part wrote zeros)
    v[0] += w.part_sum[b];
    v[1] += w.part_sum[(size_t)w.nblk + b];
    c[0] += w.part_cnt[b];
    c[1] += w.part_cnt[(size_t)w.nblk + b];
  };
  if (!block_sum_ordered(w.nblk, add, sum, cnt)) return;
  eyoc_closs_record r;
  r.sum_pos = sum[0]; r.sum_neg = sum[1];
  r.n_pairs = n_pairs; r.n_neg = n_neg; r.k_neg = cnt[0]; r.n_active = cnt[1];
  r.status = w.hc.ctl->status;
  r.reserved = 0;
  const float nan = __builtin_nanf("");
  const bool none = r.status != 0u || n_pairs == 0;
  // a mean over nothing is 0 / 0 = NaN, the reference's value
  r.pos_loss = none ? nan : (float)(sum[0] / (double)n_pairs);
  r.neg_loss = none ? nan : (float)(sum[1] / (double)cnt[0]);
  *w.rec = r;
  *out = r;
}

// one thread per term (positives by p, then candidates by q): its two contribution entries (dF0 row, dF1 row), or two empty ones
__global__ __launch_bounds__(HC_THREADS) void cl_weights_kernel(const long long* __restrict__ pairs, int n_pairs,
                                                                const long long* __restrict__ neg, int n_neg, int n0, int n1,
                                                                float neg_thresh, const float* __restrict__ g_pos,
                                                                const float* __restrict__ g_neg, ClWs w) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * HC_THREADS + threadIdx.x;
  if (t >= n_pairs + n_neg) return;
  const eyoc_closs_record rec = *w.rec;
  long long i = -1, j = -1;
  float f = 0.0f;
  bool emit = false;
  if (t < n_pairs) {
    i = pairs[2 * (size_t)t];
    j = pairs[2 * (size_t)t + 1];
    emit = true;
    f = (float)(2.0 * (double)*g_pos / (double)n_pairs);
  } else {
    const int q = t - n_pairs;
    if ((w.flags[q] & EYOC_CLOSS_ACTIVE) && rec.k_neg > 0) {
      i = neg[2 * (size_t)q];
      j = neg[2 * (size_t)q + 1];
      emit = true;
      const float d = w.dist[q];
      const float h = neg_thresh - d;
      f = (float)(-2.0 * ((double)*g_neg / (double)rec.k_neg) * (double)h / (double)d);
    }
  }
  emit = emit && i >= 0 && i < n0 && j >= 0 && j < n1;
  const Contrib& l = w.list;
  const size_t e = 2 * (size_t)t;
  l.key[e] = emit ? contrib_key((unsigned int)i, 0) : 0u;
  l.key[e + 1] = emit ? contrib_key((unsigned int)j, 1) : 0u;
  l.idx[e] = (int)e;
  l.idx[e + 1] = (int)(e + 1);
  l.w[e] = emit ? f : 0.0f;
  l.w[e + 1] = emit ? f : 0.0f;
  l.r[e] = emit ? (int)j : 0;
  l.r[e + 1] = emit ? (int)i : 0;
}

int cl_check_args(const char* what, const eyoc_ctx* ctx, const void* F0, int n0, const void* F1, int n1, int c, const void* pairs,
                  int n_pairs, const void* neg, int n_neg, const void* ws, size_t ws_bytes) {
  EYOC_REQUIRE(ctx, EYOC_ERR_INVALID, "%s: NULL ctx", what);
  EYOC_REQUIRE(c == 16 || c == 32 || c == 64, EYOC_ERR_INVALID, "%s: feature dimension %d not supported (16/32/64)", what, c);
  EYOC_REQUIRE(n0 >= 0 && n1 >= 0 && n_pairs >= 0 && n_neg >= 0, EYOC_ERR_INVALID, "%s: negative count", what);
  EYOC_REQUIRE(n0 <= (1 << 30) && n1 <= (1 << 30), EYOC_ERR_INVALID, "%s: more than 2^30 rows", what);
  EYOC_REQUIRE(cl_counts_ok(n_pairs, n_neg), EYOC_ERR_INVALID, "%s: n_pairs %d + n_neg %d must stay below 2^30", what, n_pairs, n_neg);
  EYOC_REQUIRE((F0 || n0 == 0) && (F1 || n1 == 0) && (pairs || n_pairs == 0) && (neg || n_neg == 0), EYOC_ERR_INVALID, "%s: NULL argument", what);
  EYOC_REQUIRE(ws && ((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "%s: the workspace must be 256-byte aligned", what);
  const size_t need = eyoc_closs_workspace_bytes(n_pairs, n_neg, c);
  EYOC_REQUIRE(ws_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
  return EYOC_OK;
}

}  // namespace

extern "C" {

size_t eyoc_closs_workspace_bytes(int n_pairs, int n_neg, int c) {
  (void)c;
  if (!cl_counts_ok(n_pairs, n_neg)) return 0;
  return cl_carve(nullptr, 0, n_pairs, n_neg).total;
}

int eyoc_closs_workspace_layout(int n_pairs, int n_neg, int c, eyoc_closs_layout* out) {
  EYOC_REQUIRE(out && cl_counts_ok(n_pairs, n_neg), EYOC_ERR_INVALID, "eyoc_closs_workspace_layout: invalid argument");
  EYOC_REQUIRE(c == 16 || c == 32 || c == 64, EYOC_ERR_INVALID, "eyoc_closs_workspace_layout: feature dimension %d not supported", c);
  char* const base = (char*)(uintptr_t)4096;   // (a stand-in base, never dereferenced)
  const ClWs w = cl_carve(base, 0, n_pairs, n_neg);
  out->anchors = HC_A;
  out->n_pairs = n_pairs;
  out->n_neg = n_neg;
  out->table_slots = (int32_t)(w.hc.mask + 1);
  out->n_contrib = w.list.ncon;
  out->reserved = 0;
  out->total = w.total;
  out->off_record = (uint64_t)((char*)w.rec - base);
  out->off_pos_d2 = (uint64_t)((char*)w.pos_d2 - base);
  out->off_dist = (uint64_t)((char*)w.dist - base);
  out->off_term = (uint64_t)((char*)w.term - base);
  out->off_flags = (uint64_t)((char*)w.flags - base);
  out->off_contrib_key = (uint64_t)((char*)w.list.key - base);
  return EYOC_OK;
}

int eyoc_closs_forward(eyoc_ctx* ctx, const float* F0, int n0, const float* F1, int n1, int c, const int64_t* pairs, int n_pairs,
                       const int64_t* neg, int n_neg, float neg_thresh, eyoc_closs_record* record_out, void* ws, size_t ws_bytes,
                       void* stream) {
  if (int rc = cl_check_args("eyoc_closs_forward", ctx, F0, n0, F1, n1, c, pairs, n_pairs, neg, n_neg, ws, ws_bytes)) return rc;
  EYOC_REQUIRE(record_out, EYOC_ERR_INVALID, "eyoc_closs_forward: NULL record");
  hipStream_t st = (hipStream_t)stream;
  const ClWs w = cl_carve(ws, ws_bytes, n_pairs, n_neg);
  const long long* P = (const long long*)pairs;
  const long long* N = (const long long*)neg;
  EYOC_CHECK_HIP(hipMemsetAsync(w.hc.ctl, 0, w.hc.fill_bytes, st));
  int pg = cdiv(n_pairs, HC_THREADS);
  pg = pg < 1 ? 1 : (pg > 4096 ? 4096 : pg);
  hipLaunchKernelGGL(hc_prep_kernel, dim3(pg), dim3(HC_THREADS), 0, st, P, n_pairs, (const long long*)nullptr, 0, (const long long*)nullptr, 0,
                     (const long long*)nullptr, 0, n0, n1, n_pairs, w.hc);
  const dim3 grid_terms(w.nblk, 2);
  for_width(c, [&](auto cc) {
    hipLaunchKernelGGL((cl_terms_kernel<decltype(cc)::value>), grid_terms, dim3(64), 0, st, F0, n0, F1, n1, P, n_pairs, N, n_neg, neg_thresh, w);
  });
  hipLaunchKernelGGL(cl_final_kernel, dim3(1), dim3(HC_THREADS), 0, st, n_pairs, n_neg, w, record_out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_closs_backward(eyoc_ctx* ctx, const float* F0, int n0, const float* F1, int n1, int c, const int64_t* pairs, int n_pairs,
                        const int64_t* neg, int n_neg, float neg_thresh, const float* g_pos, const float* g_neg, float* dF0, float* dF1,
                        void* ws, size_t ws_bytes, void* stream) {
  if (int rc = cl_check_args("eyoc_closs_backward", ctx, F0, n0, F1, n1, c, pairs, n_pairs, neg, n_neg, ws, ws_bytes)) return rc;
  EYOC_REQUIRE(g_pos && g_neg && (dF0 || n0 == 0) && (dF1 || n1 == 0), EYOC_ERR_INVALID, "eyoc_closs_backward: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const ClWs w = cl_carve(ws, ws_bytes, n_pairs, n_neg);
  if (int rc = zero_gradients(dF0, n0, dF1, n1, c, st)) return rc;
  if (n_pairs == 0) return EYOC_OK;   // both values are NaN by definition: no contribution
  hipLaunchKernelGGL(cl_weights_kernel, dim3(cdiv(n_pairs + n_neg, HC_THREADS)), dim3(HC_THREADS), 0, st, (const long long*)pairs, n_pairs,
                     (const long long*)neg, n_neg, n0, n1, neg_thresh, g_pos, g_neg, w);
  return sort_and_sum_rows<false>(w.list, F0, n0, F1, n1, c, dF0, dF1, st);
}

}  // extern "C"
