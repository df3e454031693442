// Brute-force 1-nearest-neighbour in feature space (lib/eval.py:18-48, lib/metrics.py:22-29 of the
// reference).  One lane owns one query row (its C features live in VGPRs); the targets are transposed once
// (channel-major) and read through the scalar cache as SGPR operands of packed-fp32 ops, so the kernel is pure
// VALU work: 3 packed ops per (query, 2 targets, channel).  The four waves of a block walk interleaved
// groups of targets and grid.y splits the target range; partial minima are merged with one
// 64-bit atomicMin on (distance bits << 32 | index), which also implements "ties go to the lowest
// index" independently of how the work was split.
//
// Arithmetic contract (bit-exact with oracle/matching.py): d = a - b; s = d * d; acc = acc + s in
// fp32, channels in order, no FMA contraction.  It is written down ONCE - knn_load_query, knn_group_distances, knn_candidate, knn_key -
// and both lane-per-query kernels (knn1_kernel, knn1_mutual_kernel) call that text.
//
// Host side: every entry point reads its segment lists through seg_plan, the ctx's scratch is laid out by knn_layout (one function for
// the byte count and for the pointers), and only the public entry points ever grow the scratch - see knn_run.
#include <type_traits>

#include "scan.h"

namespace {

constexpr int MAX_SEG = 128;
struct SegArgs {
  int a[MAX_SEG + 1];
  int b[MAX_SEG + 1];
  int ld[MAX_SEG];              // targets of the segment rounded up to a whole group (row length of its transposed block)
  long long bt_off[MAX_SEG];    // float offset of the segment's transposed block
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int TGROUP = 8;      // targets per inner iteration (four packed pairs)
constexpr int SPLIT_ALIGN = 32;  // split boundaries: every wave of a block starts on a whole group

// targets of segment s, channel-major and padded to a multiple of TGROUP: Bt[bt_off[s] + c * ld[s] + j].
// Padding columns are zero and never compared.
__global__ void knn_transpose_targets(const float* __restrict__ B, SegArgs seg, int C, float* __restrict__ Bt) {
  const int s = blockIdx.z;
  const int b0 = seg.b[s], nb = seg.b[s + 1] - b0, ld = seg.ld[s];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (c4, j): consecutive threads = consecutive targets
  const int c4n = C / 4;
  if (i >= ld * c4n) return;
  const int j = i % ld, c4 = i / ld;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (j < nb) v = *reinterpret_cast<const float4*>(B + (size_t)(b0 + j) * C + 4 * c4);
  float* dst = Bt + seg.bt_off[s] + (size_t)(4 * c4) * ld + j;
  dst[0] = v.x; dst[ld] = v.y; dst[2 * (size_t)ld] = v.z; dst[3 * (size_t)ld] = v.w;
}

// the lane's query `row` (C floats) as packed operands: a[c] = {row[c], row[c]}, the feature in both halves
template <int C>
__device__ __forceinline__ void knn_load_query(const float* row, f32x2 (&a)[C]) {
  const float4* src = reinterpret_cast<const float4*>(row);
#pragma unroll
  for (int i = 0; i < C / 4; ++i) {
    const float4 v = src[i];
    a[4 * i] = f32x2{v.x, v.x}; a[4 * i + 1] = f32x2{v.y, v.y}; a[4 * i + 2] = f32x2{v.z, v.z}; a[4 * i + 3] = f32x2{v.w, v.w};
  }
}

// acc[k] = the contract's value for targets 2 k, 2 k + 1 of the group of TGROUP whose channel-major rows start at `col` (wave-uniform,
// row length ld) against the lane's query `a`: the squared distance, or with DOT -<a, b>.  The one group body of this file: knn1_kernel
// and knn1_mutual_kernel both call it, so the order of operations, the batching of the scalar loads and the sched_barrier placement are
// the same in both (EXPERIMENTS.md "kNN: one group body" has knn1_kernel's registers and times before and after it shared this text).
template <int C, bool DOT>
__device__ __forceinline__ void knn_group_distances(const f32x2 (&a)[C], const float* col, int ld, f32x2 (&acc)[TGROUP / 2]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < TGROUP / 2; ++k) acc[k] = f32x2{0.0f, 0.0f};
  // Channels in batches of CB (eight SGPRs per channel).  Scalar loads return out of order, so a wait is always
  // "all of them": the next batch is therefore issued right AFTER the wait for the current one (behind the first
  // packed op that needs it) and its latency hides behind the rest of the current batch.
  constexpr int CB = C >= 8 ? 4 : C / 2;
  auto load_batch = [&](int cb, f32x2 (&b)[CB][TGROUP / 2]) {
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const float4 lo = *reinterpret_cast<const float4*>(col + (size_t)(cb + c) * ld);
      const float4 hi = *reinterpret_cast<const float4*>(col + (size_t)(cb + c) * ld + 4);
      b[c][0] = f32x2{lo.x, lo.y}; b[c][1] = f32x2{lo.z, lo.w}; b[c][2] = f32x2{hi.x, hi.y}; b[c][3] = f32x2{hi.z, hi.w};
    }
  };
  // the four target pairs side by side, so that dependent packed ops are never back to back (a wait state each)
  auto channel = [&](int c, const f32x2 (&b)[TGROUP / 2]) {
    if (DOT) {
#pragma unroll
      for (int k = 0; k < TGROUP / 2; ++k) acc[k] = __builtin_elementwise_fma(a[c], -b[k], acc[k]);
      return;
    }
    f32x2 d[TGROUP / 2];
#pragma unroll
    for (int k = 0; k < TGROUP / 2; ++k) d[k] = a[c] - b[k];
#pragma unroll
    for (int k = 0; k < TGROUP / 2; ++k) d[k] = d[k] * d[k];
#pragma unroll
    for (int k = 0; k < TGROUP / 2; ++k) acc[k] = acc[k] + d[k];
  };
  f32x2 b0[CB][TGROUP / 2], b1[CB][TGROUP / 2];
  load_batch(0, b0);
#pragma unroll
  for (int cb = 0; cb < C; cb += 2 * CB) {
    __builtin_amdgcn_sched_barrier(0);
    channel(cb, b0[0]);                               // forces the wait for batch b0
    __builtin_amdgcn_sched_barrier(0);
    load_batch(cb + CB, b1);                          // C is a multiple of 2 CB
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 1; c < CB; ++c) channel(cb + c, b0[c]);
    __builtin_amdgcn_sched_barrier(0);
    channel(cb + CB, b1[0]);
    __builtin_amdgcn_sched_barrier(0);
    if (cb + 2 * CB < C) load_batch(cb + 2 * CB, b0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 1; c < CB; ++c) channel(cb + CB + c, b1[c]);
  }
}

// what a (query, target) pair competes with: the contract's value of `knn_group_distances` after the mode's own steps
template <int MODE>
__device__ __forceinline__ float knn_candidate(float v, int dist_type) {
#pragma clang fp contract(off)
  v = dist_type == 1 ? sqrtf(v + 1e-7f) : v;
  if (MODE == 2) {          // acc = -S exactly (the negated chain rounds symmetrically)
    const float w = (2.0f - 2.0f * (-v)) + 1e-6f;
    const float d = sqrtf(w);
    v = d != d ? -1.0f : d;                                        // NaN first: below every distance
  }
  return v;
}

// the 32 bits above the index in a packed minimum: the value's bits, order-preserving for negative values too where there can be any
template <bool DOT>
__device__ __forceinline__ unsigned int knn_key(float v) {
  unsigned int bits = __float_as_uint(v);
  if (DOT) bits = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return bits;
}

// Lane = query (C features in VGPRs); the targets are wave-uniform, so they come through the SCALAR cache
// (s_load of eight consecutive targets of one channel) and feed the packed-fp32 ops as SGPR pairs: no LDS
// traffic at all (the LDS-broadcast version of this kernel was bound by ds_read bandwidth, not by the VALU).
// Two targets share one v_pk_* instruction; each (query, target) still sees the scalar contract.
// DOT: the value minimised is -<a, b> (one packed FMA per channel and target pair) instead of the squared distance:
// the arg-max of the inner product of util/transform_estimation.py:131-133 without its [N0, N1] matrix.
// MODE 2 (dist_type 2, "GemmL2"): the quantity minimised is the reference's sqrt(2 - 2 S + 1e-6) of
// scripts/SC2_PCR/SC2_PCR.py:296-298 with S the same FMA chain as DOT, every later step rounded separately in fp32; a NaN
// (S > 1 + 5e-7: un-normalised descriptors) is smaller than every number and the first one wins, like torch.argmin.
// TOP2: also track the second smallest distance (Lowe's ratio test of the label generator,
// lib/trainer.py:1060-1072); the target range is then NOT split over blocks (a 64-bit atomicMin cannot merge a
// runner-up) and the four waves of the block merge their partial results through LDS.
template <int C, bool TOP2, int MODE>
__global__ __launch_bounds__(256) void knn1_kernel(const float* __restrict__ A, const float* __restrict__ Bt,
                                                   SegArgs seg, int split_len, int dist_type,
                                                   unsigned long long* __restrict__ best, float* __restrict__ second,
                                                   const int* __restrict__ only = nullptr, const int* __restrict__ only_cnt = nullptr) {
#pragma clang fp contract(off)
  constexpr bool DOT = MODE != 0;
  const int s = blockIdx.z;
  const int a0 = seg.a[s], na = seg.a[s + 1] - a0;
  const int nb = seg.b[s + 1] - seg.b[s], ld = seg.ld[s];
  const int t_begin = blockIdx.y * split_len;
  const int t_end = min(nb, t_begin + split_len);
  if (t_begin >= t_end) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // query tiles: one per block - or, in the second pass of the MFMA pre-filter, a few blocks per segment that walk the
  // dense list of the rows it could not decide (any number of them, usually a handful)
  for (int q0 = blockIdx.x * 64;; q0 += gridDim.x * 64) {
  int q = q0 + lane;
  bool q_ok = q < na;
  if (only) {
    const int cnt = only_cnt[s];
    if (q0 >= cnt) return;                                           // the whole block: its four waves share the queries
    q_ok = q0 + lane < cnt;
    q = q_ok ? only[a0 + q0 + lane] : 0;
  } else if (q0 >= na) {
    return;
  }
  f32x2 a[C];
  knn_load_query<C>(A + (size_t)(a0 + (q_ok ? q : 0)) * C, a);
  float best_d = __builtin_inff(), second_d = __builtin_inff();
  int best_j = 0x7FFFFFFF;
  bool any = false;
  // the four waves of the block take interleaved groups of TGROUP targets
  const float* bt = Bt + seg.bt_off[s];
  for (int t = t_begin + wave * TGROUP; t < t_end; t += 4 * TGROUP) {
    f32x2 acc[TGROUP / 2];
    knn_group_distances<C, DOT>(a, bt + t, ld, acc);   // (bt + t: a wave-uniform address)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < TGROUP; ++e) {
      // branch-free on purpose: with branches here LLVM sinks the arithmetic of targets 2..7 below the first
      // compare and keeps every scalar-loaded operand alive until then (SGPR spills)
      const float v = knn_candidate<MODE>((e & 1) ? acc[e / 2].y : acc[e / 2].x, dist_type);
      const bool valid = t + e < t_end;
      const bool better = valid & (v < best_d);
      if (TOP2) {   // the displaced best, or a value between the two, becomes the runner-up (NaNs never enter)
        const float cand = better ? best_d : v;
        second_d = (valid & (cand < second_d)) ? cand : second_d;
      }
      best_d = better ? v : best_d;
      best_j = better ? t + e : best_j;
      any = any | better;
    }
  }
  if (TOP2) {
    __shared__ float sd1[4][64], sd2[4][64];
    __shared__ int sj[4][64];
    sd1[wave][lane] = best_d; sd2[wave][lane] = second_d; sj[wave][lane] = any ? best_j : 0x7FFFFFFF;
    __syncthreads();
    if (wave == 0 && q_ok) {
      float d1 = sd1[0][lane], d2 = sd2[0][lane];
      int j1 = sj[0][lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float e1 = sd1[w][lane], e2 = sd2[w][lane];
        const int k1 = sj[w][lane];
        const bool take = (e1 < d1) | ((e1 == d1) & (k1 < j1));   // smaller distance, ties to the lower index
        const float lose = take ? d1 : e1;                          // the loser of the two bests is a runner-up candidate
        d1 = take ? e1 : d1;
        j1 = take ? k1 : j1;
        float r = d2 < e2 ? d2 : e2;
        d2 = lose < r ? lose : r;
      }
      if (j1 != 0x7FFFFFFF) best[a0 + q] = ((unsigned long long)__float_as_uint(d1) << 32) | (unsigned)j1;
      second[a0 + q] = d2;
    }
    return;
  }
  if (q_ok && any) atomicMin(&best[a0 + q], ((unsigned long long)knn_key<DOT>(best_d) << 32) | (unsigned)best_j);
  if (!only) return;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Mutual nearest neighbours in one sweep (eyoc_knn1_mutual, route 1).  All three distance forms are symmetric bit for bit -
// (a - b)^2 = (b - a)^2, and every term of the FMA chain of <a, b> commutes - so d(i, t), computed once as in knn1_kernel, serves
// the row minimum of query i AND the column minimum of target t: what eyoc_knn1(B, A) would find for row t.  A wave owns 64
// consecutive targets at a time (the four waves of a block interleave such chunks) and walks them in groups of TGROUP; per group
// the 64 lanes' candidates (key << 32 | query row) of the eight targets are reduced by a butterfly that halves the targets a lane
// holds while it doubles the lanes merged (4 + 2 + 1 exchanges, then three more over the upper lane bits: 10 instead of 48), lane
// l ends with the wave's minimum for target l & 7 and the lanes of group g park theirs.  After eight groups lane l holds target
// t0 + l, and ONE wave-wide atomicMin goes to 64 consecutive words of colbest (512 contiguous bytes).  Integer minima: the result
// does not depend on how the grid splits the work, ties go to the lowest row.  A candidate enters the column minimum exactly where
// the reverse query would have taken it: valid lane, valid target, value < +inf (a NaN compares false in modes 0 and 1; in mode 2
// it is the -1 of knn_candidate, below every number, and the lowest row wins).
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long p, int d) {
  const unsigned int lo = __shfl_xor((unsigned int)p, d, 64), hi = __shfl_xor((unsigned int)(p >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long min_u64(unsigned long long x, unsigned long long y) { return y < x ? y : x; }

constexpr int MUT_CHUNK = 64;                    // targets a wave parks before its atomic
constexpr int MUT_SPLIT_ALIGN = 4 * MUT_CHUNK;   // split boundaries: a whole chunk for each of the block's four waves

template <int C, int MODE>
__global__ __launch_bounds__(256) void knn1_mutual_kernel(const float* __restrict__ A, const float* __restrict__ Bt, SegArgs seg,
                                                          int split_len, int dist_type, unsigned long long* __restrict__ best,
                                                          unsigned long long* __restrict__ colbest) {
#pragma clang fp contract(off)
  constexpr bool DOT = MODE != 0;
  const int s = blockIdx.z;
  const int a0 = seg.a[s], na = seg.a[s + 1] - a0;
  const int b0 = seg.b[s], nb = seg.b[s + 1] - b0, ld = seg.ld[s];
  const int t_begin = blockIdx.y * split_len;
  const int t_end = min(nb, t_begin + split_len);
  const int q0 = blockIdx.x * 64;
  if (t_begin >= t_end || q0 >= na) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int q = q0 + lane;
  const bool q_ok = q < na;
  f32x2 a[C];
  knn_load_query<C>(A + (size_t)(a0 + (q_ok ? q : 0)) * C, a);
  float best_d = __builtin_inff();
  int best_j = 0x7FFFFFFF;
  bool any = false;
  const float* bt = Bt + seg.bt_off[s];
  for (int t0 = t_begin + wave * MUT_CHUNK; t0 < t_end; t0 += 4 * MUT_CHUNK) {
    unsigned long long parked = ~0ull;
#pragma unroll 1
    for (int g = 0; g < MUT_CHUNK / TGROUP; ++g) {
      const int t = t0 + g * TGROUP;
      if (t >= t_end) break;                                           // wave-uniform (ld covers the whole group)
      f32x2 acc[TGROUP / 2];
      knn_group_distances<C, DOT>(a, bt + t, ld, acc);
      __builtin_amdgcn_sched_barrier(0);
      unsigned long long p[TGROUP];
#pragma unroll
      for (int e = 0; e < TGROUP; ++e) {
        const float v = knn_candidate<MODE>((e & 1) ? acc[e / 2].y : acc[e / 2].x, dist_type);
        const bool valid = t + e < t_end;
        const bool better = valid & (v < best_d);
        best_d = better ? v : best_d;
        best_j = better ? t + e : best_j;
        any = any | better;
        p[e] = (q_ok & valid & (v < __builtin_inff())) ? (((unsigned long long)knn_key<DOT>(v) << 32) | (unsigned)q) : ~0ull;
      }
      // w[k]: target 2 k + (lane & 1) over lane pairs; x[k]: target 4 k + (lane & 3) over lane quads; y: target lane & 7 over eight lanes
      const bool l1 = lane & 1, l2 = lane & 2, l4 = lane & 4;
      unsigned long long w[TGROUP / 2], x[TGROUP / 4];
#pragma unroll
      for (int k = 0; k < TGROUP / 2; ++k) w[k] = min_u64(l1 ? p[2 * k + 1] : p[2 * k], shfl_xor_u64(l1 ? p[2 * k] : p[2 * k + 1], 1));
#pragma unroll
      for (int k = 0; k < TGROUP / 4; ++k) x[k] = min_u64(l2 ? w[2 * k + 1] : w[2 * k], shfl_xor_u64(l2 ? w[2 * k] : w[2 * k + 1], 2));
      unsigned long long y = min_u64(l4 ? x[1] : x[0], shfl_xor_u64(l4 ? x[0] : x[1], 4));
      y = min_u64(y, shfl_xor_u64(y, 8));
      y = min_u64(y, shfl_xor_u64(y, 16));
      y = min_u64(y, shfl_xor_u64(y, 32));
      parked = (lane >> 3) == g ? y : parked;                          // lane 8 g + e keeps target t0 + 8 g + e
    }
    const int tt = t0 + lane;
    if (tt < t_end && parked != ~0ull) atomicMin(&colbest[b0 + tt], parked);
  }
  if (q_ok && any) atomicMin(&best[a0 + q], ((unsigned long long)knn_key<DOT>(best_d) << 32) | (unsigned)best_j);
}

// flags[i] of row i of segment s: bit 1 = the row has a neighbour j = idx_ab[i], bit 0 = mutual: j has a neighbour too and it is i
__global__ void knn_mutual_flags(SegArgs seg, const long long* __restrict__ idx_ab, const long long* __restrict__ idx_ba,
                                 const unsigned char* __restrict__ has_a, const unsigned char* __restrict__ has_b,
                                 unsigned char* __restrict__ flags) {
  const int s = blockIdx.z;
  const int a0 = seg.a[s], na = seg.a[s + 1] - a0, b0 = seg.b[s];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= na) return;
  unsigned char f = 0;
  if (has_a[a0 + i]) {                                                 // (then the B segment is not empty and j is one of its rows)
    const long long j = idx_ab[a0 + i];
    f = 2 | (has_b[b0 + j] && idx_ba[b0 + j] == i ? 1 : 0);
  }
  flags[a0 + i] = f;
}

// ------------------------------------------------------------------------------------------------------------------
// Stable per-segment compaction of the mutual rows (eyoc_mutual_compact): counts per segment, the flag scan of scan.h, a fill
// pass.  No atomics: the output is the same bytes on every run.
// cnt[s] = rows of segment s the compaction keeps - its mutual rows, or (fewer than min_keep of them) its rows with a neighbour;
// fallback[s] says which.  One workgroup per segment.
__global__ __launch_bounds__(SCAN_BLOCK) void k_mutual_count(SegArgs seg, const unsigned char* __restrict__ flags, int min_keep,
                                                             int* __restrict__ cnt, int* __restrict__ fallback) {
  const int s = blockIdx.x;
  const int a0 = seg.a[s], na = seg.a[s + 1] - a0;
  int m = 0, h = 0;
  for (int i = threadIdx.x; i < na; i += SCAN_BLOCK) {
    const unsigned char f = flags[a0 + i];
    m += f & 1;
    h += (f >> 1) & 1;
  }
  int mt, ht;
  block_exclusive_scan(m, &mt);
  block_exclusive_scan(h, &ht);
  if (threadIdx.x == 0) {
    const bool fb = mt < min_keep;
    cnt[s] = fb ? ht : mt;
    fallback[s] = fb;
  }
}

// keep[i] = 1 iff row i stays, loc[i] = its row inside its segment; block (0, 0, 0) also writes seg_out = the running sum of cnt
__global__ void k_mutual_keep(SegArgs seg, int nseg, const unsigned char* __restrict__ flags, const int* __restrict__ cnt,
                              const int* __restrict__ fallback, int* __restrict__ keep, int* __restrict__ loc,
                              int32_t* __restrict__ seg_out) {
  const int s = blockIdx.z;
  const int a0 = seg.a[s], na = seg.a[s + 1] - a0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) {
    const unsigned char f = flags[a0 + i];
    keep[a0 + i] = fallback[s] ? (f >> 1) & 1 : f & 1;
    loc[a0 + i] = i;
  }
  if (blockIdx.x == 0 && s == 0 && threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < nseg; ++k) { seg_out[k] = run; run += cnt[k]; }
    seg_out[nseg] = run;
  }
}

// partial: the exclusive scan of the tiles' kept rows (k_scan_partials + k_scan_top, SCAN_ITEMS consecutive rows per thread)
__global__ __launch_bounds__(SCAN_BLOCK) void k_mutual_fill(const int* __restrict__ keep, const int* __restrict__ loc,
                                                            const int* __restrict__ partial, const long long* __restrict__ idx_ab,
                                                            int n, long long* __restrict__ rows, long long* __restrict__ corr) {
  const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  int k[SCAN_ITEMS], sum = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) { k[j] = base + j < n ? keep[base + j] : 0; sum += k[j]; }
  int tot;
  int pos = partial[blockIdx.x] + block_exclusive_scan(sum, &tot);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j)
    if (k[j]) {
      rows[pos] = loc[base + j];
      corr[pos] = idx_ab[base + j];
      ++pos;
    }
}

__global__ void knn1_unpack(const unsigned long long* __restrict__ best, int n, long long* __restrict__ idx,
                            float* __restrict__ dist, int dot, unsigned char* __restrict__ has = nullptr) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long p = best[i];
  if (has) has[i] = p != ~0ull;   // (the mutual check: a row without a neighbour reads index 0 like a row whose neighbour is row 0)
  if (p == ~0ull) {  // every candidate compared false (NaN features) or the target set was empty
    if (idx) idx[i] = 0;
    if (dist) dist[i] = __builtin_nanf("");
    return;
  }
  if (idx) idx[i] = (long long)(unsigned)(p & 0xFFFFFFFFull);
  unsigned int bits = (unsigned)(p >> 32);
  if (dot) bits = (bits & 0x80000000u) ? (bits & 0x7FFFFFFFu) : ~bits;   // undo the key, then negate: the inner product
  if (dist) {
    const float v = __uint_as_float(bits);
    dist[i] = dot == 1 ? -v : dot == 2 ? (v < 0.0f ? __builtin_nanf("") : v) : v;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// MFMA pre-filter for the plain index query (SquareL2, no distances asked for, enough rows to fill the chip).
//
// The contract above costs 3 VALU ops per (query, target, channel) - 3.3 ms for the bench's 64 x 5000 x 5000 x 32.  The
// arg-min, however, is almost always decided by a far cheaper score: s(i, j) = |b_j|^2 - 2 <a_i, b_j> with the inner
// product on the fp16 matrix pipe at fp32 accuracy - three v_mfma_f32_16x16x32_f16 on hi / lo-split operands, ONE
// instruction spanning all 32 channels (rows are scaled by a power of two first so that both halves of the split are
// accurate whatever the magnitude of the features; the first version used nine v_mfma_f32_16x16x4_f32: 288 instead
// of 48 matrix cycles per 16 x 16 tile, 1.25 ms instead of 0.45 for the bench's query).  With
// |s(i, j) - (d(i, j) - |a_i|^2)| <= e for every j - d the contract's fp32 value - the contract's arg-min j* satisfies
// s(j*) <= min_j s + 2 e.  So every wave tracks, per query, the smallest score with its index AND the second smallest
// score: if the runner-up is farther than 2 e, the index is final (exact ties included: they would both be within
// 2 e); otherwise the row is flagged and the exact kernel above recomputes it (waves without a flagged row exit at
// once).  e = 128 u (|a_i| + max_j |b_j|)^2, u = 2^-24, covers the rounding of both evaluations with a wide margin
// (the split products err by <= 2^-20 |a||b|, the norm and the contract's own 96 roundings by <= 64 u (|a| + |b|)^2).  Rows with non-finite scores are flagged too.
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
struct SegMfma { long long bm_off[MAX_SEG]; };
constexpr int MF_ROWS = 64;                    // query rows per wave (4 MFMA row tiles)

// power of two that lifts a row's largest |element| into [128, 256): both halves of the fp16 split of the scaled row are
// then as accurate as they can be (a row of all zeros, or with a non-finite element, keeps scale 1)
__device__ inline float split_scale(float maxabs) {
  if (!(maxabs > 0.0f) || !(maxabs < __builtin_inff())) return 1.0f;
  int e;
  (void)frexpf(maxabs, &e);                                          // maxabs = m 2^e, m in [0.5, 1)
  return ldexpf(1.0f, 8 - e);
}

// B operand of v_mfma_f32_16x16x32_f16 per tile of 16 targets, 3 x 64 float4: [0] lane (g, j): the fp16 hi halves of
// channels 8 g .. 8 g + 7 of target 16 t + j, scaled by the target's split_scale; [1] the lo halves; [2] (|b_j|^2,
// 1 / scale_j, 0, 0) (padding targets: norm +inf, everything else 0)
// A wave packs PK_TILES tiles, lane (g, j) of a tile loading only its own eight channels of target j.  The squared norm is the sum the
// first version of this kernel took over the whole row in every lane, spelled out so that it stays that sum bit for bit: per four
// channels (x, y, z, w) the term w^2 + (z^2 + (x^2 + fl(y^2))) with one rounding per fused step, and the eight terms of a row added
// from channel 0 upwards - each lane group computes its two terms, the groups exchange them, every lane adds all eight in that order.
constexpr int PK_TILES = 4;
__device__ inline float pack_term(const float4 v) { return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.x, v.x, v.y * v.y))); }

template <int C>
__global__ __launch_bounds__(256) void knn_pack_targets_mfma(const float* __restrict__ B, SegArgs seg, SegMfma sm, float* __restrict__ Bm,
                                                             int* __restrict__ bmax_bits, int zero_norm) {
  static_assert(C == 32, "one 16x16x32 MFMA spans the 32 channels");
  __shared__ int wmax[4];
  const int s = blockIdx.z;
  const int b0 = seg.b[s], nb = seg.b[s + 1] - b0;
  const int n16 = (nb + 15) / 16;
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4;
  const int t0 = (blockIdx.x * 4 + wave) * PK_TILES;
  int nb2 = 0;                                                         // bits of the largest |b|^2 this lane has seen
#pragma unroll
  for (int u = 0; u < PK_TILES; ++u) {
    const int t = t0 + u, j = 16 * t + (l & 15);
    if (t >= n16) break;                                               // wave-uniform
    float4* dst = reinterpret_cast<float4*>(Bm + sm.bm_off[s]) + (size_t)t * 3 * 64 + l;
    const bool ok = j < nb;
    const float4* row = reinterpret_cast<const float4*>(B + (size_t)(b0 + (ok ? j : 0)) * C) + 2 * g;
    const float4 v0 = row[0], v1 = row[1];
    const float mine[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const float term0 = pack_term(v0), term1 = pack_term(v1);
    float mx = fmaxf(fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w))),
                     fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w))));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float n2 = __shfl(term0, l & 15, 64) + __shfl(term1, l & 15, 64);
#pragma unroll
    for (int h = 1; h < 4; ++h) {
      n2 = n2 + __shfl(term0, (l & 15) + 16 * h, 64);
      n2 = n2 + __shfl(term1, (l & 15) + 16 * h, 64);
    }
    if (!(n2 == n2)) mx = __builtin_nanf("");                          // a NaN element: fmaxf would have dropped it
    const float sc = split_scale(mx);
    half8_t hi, lo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x = ok ? mine[i] * sc : 0.0f;
      const _Float16 h = (_Float16)x;
      hi[i] = h;
      lo[i] = (_Float16)(x - (float)h);
    }
    dst[0] = __builtin_bit_cast(float4, hi);
    dst[64] = __builtin_bit_cast(float4, lo);
    dst[128] = make_float4(ok ? (zero_norm ? 0.0f : n2) : __builtin_inff(), ok ? 1.0f / sc : 0.0f, 0.f, 0.f);   // zero_norm: score -2 <a, b>
    nb2 = max(nb2, (ok && n2 == n2) ? __float_as_int(n2) : 0);        // non-negative floats order like ints
  }
  // the segment's largest |b|^2: one atomic per workgroup (= per 16 tiles of 16 targets).  One per target - 5000 on one word per
  // segment - was most of this kernel's time at first, and one per tile still put ~310 in a row on every segment's word
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) nb2 = max(nb2, __shfl_xor(nb2, d, 64));
  if (l == 0) wmax[wave] = nb2;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m > 0) atomicMax(bmax_bits + s, m);
  }
}

__global__ void knn_row_norms(const float* __restrict__ A, int n, int C, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float n2 = 0.f;
  if ((C & 3) == 0) {                                                  // 16-byte loads, the same sum in the same order
    const float4* row = reinterpret_cast<const float4*>(A + (size_t)i * C);
    for (int q = 0; q < C / 4; ++q) {
      const float4 v = row[q];
      n2 += v.x * v.x; n2 += v.y * v.y; n2 += v.z * v.z; n2 += v.w * v.w;
    }
  } else {
    for (int c = 0; c < C; ++c) n2 += A[(size_t)i * C + c] * A[(size_t)i * C + c];
  }
  out[i] = n2;
}

// Second pass of the pre-filter for the plain SquareL2 query, lane = TARGET: the handful of rows the MFMA scores could not
// decide are few (0.35 % on the bench) but every one needs all targets of its segment.  With lane = query (knn1_kernel) a wave
// has 17 of its 64 lanes busy and walks its targets through dependent scalar loads (152 us, plus the 50 us transposition of
// the targets that only this pass needed).  Here a workgroup keeps 256 targets in registers (one row per lane), stages the
// listed queries in LDS (256 at a time) and evaluates the contract - d = a - b; acc = acc + d * d over the channels in order, no
// contraction - for every (listed query, its target); the wave's smallest (distance bits, index) goes to the same 64-bit
// atomicMin.  Same values, same tie rule (lowest index), NaN / inf candidates never enter.
template <int C>
__global__ __launch_bounds__(256) void knn1_list_kernel(const float* __restrict__ A, const float* __restrict__ B, SegArgs seg,
                                                        unsigned long long* __restrict__ best, const int* __restrict__ only,
                                                        const int* __restrict__ only_cnt) {
#pragma clang fp contract(off)
  constexpr int QB = 256;
  __shared__ __attribute__((aligned(16))) float qs[QB][C];
  __shared__ int qrow[QB];
  const int s = blockIdx.z;
  const int cnt = only_cnt[s];
  const int a0 = seg.a[s], b0 = seg.b[s], nb = seg.b[s + 1] - b0;
  if (cnt <= 0 || (int)blockIdx.x * 256 >= nb) return;                 // workgroup-uniform
  const int lane = threadIdx.x & 63;
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;              // this lane's target
  float b[C];
  {
    const float4* src = reinterpret_cast<const float4*>(B + (size_t)(b0 + (j < nb ? j : nb - 1)) * C);
#pragma unroll
    for (int i = 0; i < C / 4; ++i) { const float4 v = src[i]; b[4 * i] = v.x; b[4 * i + 1] = v.y; b[4 * i + 2] = v.z; b[4 * i + 3] = v.w; }
  }
  for (int q0 = 0; q0 < cnt; q0 += QB) {
    const int nq = min(QB, cnt - q0);
    __syncthreads();
    for (int e = threadIdx.x; e < nq * (C / 4); e += 256) {
      const int qi = e / (C / 4), part = e % (C / 4);
      const int row = only[a0 + q0 + qi];
      if (part == 0) qrow[qi] = row;
      reinterpret_cast<float4*>(qs[qi])[part] = reinterpret_cast<const float4*>(A + (size_t)(a0 + row) * C)[part];
    }
    __syncthreads();
    for (int i = 0; i < nq; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float d = qs[i][c] - b[c];
        d = d * d;
        acc = acc + d;
      }
      unsigned long long p = (j < nb && acc < __builtin_inff()) ? (((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)j) : ~0ull;
#pragma unroll
      for (int dlt = 32; dlt >= 1; dlt >>= 1) {
        const unsigned int lo = __shfl_xor((unsigned int)p, dlt, 64), hi = __shfl_xor((unsigned int)(p >> 32), dlt, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        p = o < p ? o : p;
      }
      if (lane == 0 && p != ~0ull) atomicMin(&best[a0 + qrow[i]], p);
    }
  }
}

template <int C, int MODE>
__global__ __launch_bounds__(256) void knn_mfma_kernel(const float* __restrict__ A, const float* __restrict__ Bm, SegArgs seg,
                                                       SegMfma sm, const float* __restrict__ anorm,
                                                       const int* __restrict__ bmax_bits,
                                                       unsigned long long* __restrict__ best, int* __restrict__ flist,
                                                       int* __restrict__ fcnt) {
  static_assert(C == 32, "one 16x16x32 MFMA spans the 32 channels");
  constexpr int RT = MF_ROWS / 16;
  const int s = blockIdx.z;
  const int a0 = seg.a[s], na = seg.a[s + 1] - a0;
  const int nb = seg.b[s + 1] - seg.b[s];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int q0 = (blockIdx.x * 4 + wave) * MF_ROWS;
  if (q0 >= na || nb <= 0) return;                                  // wave-uniform; no barrier in this kernel
  const int jl = lane & 15, g = lane >> 4;
  // A fragments: row tile r: channels 8 g .. 8 g + 7 of query q0 + 16 r + jl, scaled per row, split into fp16 hi / lo;
  // mrow[r][e] = -2 / scale of query 16 r + 4 g + e (the rows this lane holds in the MFMA result)
  half8_t ah[RT], al[RT];
  float mrow[RT][4];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int i = q0 + 16 * r + jl;
    const float* row = A + (size_t)(a0 + (i < na ? i : na - 1)) * C + 8 * g;
    const float4 v0 = *reinterpret_cast<const float4*>(row), v1 = *reinterpret_cast<const float4*>(row + 4);
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    float mx = 0.f, sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { mx = fmaxf(mx, fabsf(x[k])); sum += x[k]; }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (!(sum == sum)) mx = __builtin_nanf("");                        // a NaN anywhere in the row
    const float sc = split_scale(mx);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float y = x[k] * sc;
      const _Float16 h = (_Float16)y;
      ah[r][k] = h;
      al[r][k] = (_Float16)(y - (float)h);
    }
    const float inv = -2.0f / sc;                                      // of row jl of the tile
#pragma unroll
    for (int e = 0; e < 4; ++e) mrow[r][e] = __shfl(inv, 4 * g + e, 64);
  }
  // per lane: queries 16 r + 4 g + e (e = 0..3) against the targets j = jl (mod 16)
  float m1[RT][4], m2[RT][4];
  int j1[RT][4];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) { m1[r][e] = __builtin_inff(); m2[r][e] = __builtin_inff(); j1[r][e] = 0x7FFFFFFF; }
  const float4* bm = reinterpret_cast<const float4*>(Bm + sm.bm_off[s]) + lane;
  const int n16 = (nb + 15) / 16;
  float4 bf[2][3];
#pragma unroll
  for (int q = 0; q < 3; ++q) bf[0][q] = bm[q * 64];
  for (int t = 0; t < n16; t += 2) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int tt = t + half;
      if (tt >= n16) break;                                          // wave-uniform
      {   // unconditional (the last tile re-loads itself): a load inside a branch is waited for on the spot
        const int tn = tt + 1 < n16 ? tt + 1 : tt;
#pragma unroll
        for (int q = 0; q < 3; ++q) bf[half ^ 1][q] = bm[((size_t)tn * 3 + q) * 64];
      }
      const int jt = 16 * tt + jl;
      const half8_t bh = __builtin_bit_cast(half8_t, bf[half][0]), bl = __builtin_bit_cast(half8_t, bf[half][1]);
      const float bn = bf[half][2].x, binv = bf[half][2].y;          // of target jt
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[r], bh, acc, 0, 0, 0);   // D[query 4 g + e][target jl]
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[r], bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[r], bh, acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = fmaf(acc[e] * binv, mrow[r][e], bn);         // |b|^2 - 2 <a, b>
          const bool better = v < m1[r][e];
          const float lose = better ? m1[r][e] : v;                  // NaN scores never enter
          m2[r][e] = lose < m2[r][e] ? lose : m2[r][e];
          m1[r][e] = better ? v : m1[r][e];
          j1[r][e] = better ? jt : j1[r][e];
        }
      }
    }
  }
  // merge the 16 lanes of a group (same queries, interleaved targets): smaller score, ties to the lower index; the
  // loser's best and both runner-ups compete for the runner-up
  const float bmax = sqrtf(__int_as_float(bmax_bits[s]));
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a1 = m1[r][e], a2 = m2[r][e];
      int k1 = j1[r][e];
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const float o1 = __shfl_xor(a1, d, 64), o2 = __shfl_xor(a2, d, 64);
        const int ok1 = __shfl_xor(k1, d, 64);
        const bool take = (o1 < a1) | ((o1 == a1) & (ok1 < k1));
        const float lose = take ? a1 : o1;
        a1 = take ? o1 : a1;
        k1 = take ? ok1 : k1;
        const float rr = a2 < o2 ? a2 : o2;
        a2 = lose < rr ? lose : rr;
      }
      const int i = q0 + 16 * r + 4 * g + e;
      if (jl == 0 && i < na) {
        const float an = sqrtf(anorm[a0 + i]);
        const float err = 128.0f * 5.9604645e-8f * (an + bmax) * (an + bmax);
        // decided: a finite best whose runner-up is out of reach.  (a2 - a1 <= 2 err, NaN / inf anywhere: not decided)
        bool decided = (a1 < __builtin_inff()) & (a1 > -__builtin_inff()) & (a2 - a1 > 2.0f * err) & (k1 != 0x7FFFFFFF);
        if (MODE == 2) {
          // score = -2 S.  sqrt(2 - 2 S + 1e-6) in fp32 can round two different S to one distance (then the LOWER
          // index wins, not the larger S): S1 > S2 + 3 * 2^-22 (1 + |S|) guarantees d1 < d2 strictly, so the runner-up
          // must also be farther than cm = 2^-19 (1 + |a| |b|max) in score units; and no S may exceed 1 (a NaN
          // distance beats everything): every S_j < 1 is implied by a1 > -2 + err
          const float cm = 1.9073486e-6f * (1.0f + an * bmax);
          decided = decided & (a2 - a1 > 2.0f * err + cm) & (a1 > -2.0f + err);
        }
        best[a0 + i] = decided ? (unsigned long long)(unsigned)k1 : ~0ull;
        if (!decided) flist[a0 + atomicAdd(fcnt + s, 1)] = i;            // the segment's undecided rows, densely (any order)
      }
    }
}

// dense distance matrix (lib/metrics.py:22-29) with the same arithmetic contract as knn1_kernel
__global__ void pdist_kernel(const float* __restrict__ A, int n, const float* __restrict__ B, int m, int c,
                             int dist_type, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)n * m) return;
  const int i = (int)(idx / m), j = (int)(idx % m);
  const float* a = A + (size_t)i * c;
  const float* b = B + (size_t)j * c;
  float acc = 0.0f;
  for (int k = 0; k < c; ++k) {
    const float d = a[k] - b[k];
    acc = acc + d * d;
  }
  if (dist_type == 1) acc = sqrtf(acc + 1e-7f);
  out[idx] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// Host side.

// floats of the packed targets of a segment of `nb` rows: 3 x 64 float4 per tile of 16 targets
long long packed_target_floats(int nb) { return (long long)eyoc::cdiv(nb, 16) * 3 * 64 * 4; }

// What the segment lists of a call come to.  seg_plan is the one pass every entry point makes over its lists, and the only place that
// fills a SegArgs; everything about the targets (ld, bt_off, bm_off, bt_floats, bm_floats) describes the b side.
struct SegPlan {
  SegArgs seg;
  SegMfma sm;
  int n_a, n_b;                      // rows in all
  int max_na, max_nb, max_ld;
  long long bt_floats, bm_floats;    // the transposed / the packed targets of all segments
  long long waves_a, waves_b;        // waves of MF_ROWS rows
};

// seg_a / seg_b: nseg + 1 offsets each; a caller with one list passes NULL for the other side, whose segments are then empty.  c: the
// width of the rows (it only sizes the transposed targets).  Refuses nseg outside [1, MAX_SEG] and a decreasing list; whether a list
// must start at 0 is the entry point's own rule.
int seg_plan(const char* who, const int32_t* seg_a, const int32_t* seg_b, int nseg, int c, SegPlan* p) {
  EYOC_REQUIRE(nseg >= 1 && nseg <= MAX_SEG, EYOC_ERR_INVALID, "%s: nseg %d not in [1,%d]", who, nseg, MAX_SEG);
  *p = SegPlan{};
  for (int s = 0; s <= nseg; ++s) {
    p->seg.a[s] = seg_a ? seg_a[s] : 0;
    p->seg.b[s] = seg_b ? seg_b[s] : 0;
  }
  for (int s = 0; s < nseg; ++s) {
    const int na = p->seg.a[s + 1] - p->seg.a[s], nb = p->seg.b[s + 1] - p->seg.b[s];
    EYOC_REQUIRE(na >= 0 && nb >= 0, EYOC_ERR_INVALID, "%s: negative segment length", who);
    p->max_na = na > p->max_na ? na : p->max_na;
    p->max_nb = nb > p->max_nb ? nb : p->max_nb;
    p->seg.ld[s] = eyoc::cdiv(nb, TGROUP) * TGROUP;
    p->max_ld = p->seg.ld[s] > p->max_ld ? p->seg.ld[s] : p->max_ld;
    p->seg.bt_off[s] = p->bt_floats;
    p->bt_floats += (long long)p->seg.ld[s] * c;
    p->sm.bm_off[s] = p->bm_floats;
    p->bm_floats += packed_target_floats(nb);
    p->waves_a += eyoc::cdiv(na, MF_ROWS);
    p->waves_b += eyoc::cdiv(nb, MF_ROWS);
  }
  p->n_a = p->seg.a[nseg] - p->seg.a[0];
  p->n_b = p->seg.b[nseg] - p->seg.b[0];
  return EYOC_OK;
}

bool knn_width_ok(int c) { return c == 4 || c == 16 || c == 32 || c == 64 || c == 128; }

// f(std::integral_constant<int, C>) for the width c (one that knn_width_ok accepts)
template <typename F>
void dispatch_width(int c, F&& f) {
  switch (c) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: f(std::integral_constant<int, 128>{}); break;
  }
}

// grid.y: the targets of the longest segment in nsplit pieces of split_len, a multiple of `align`, so that about 4096 blocks fly
// (`blocks` of them before splitting); !may_split: one piece
struct SplitPlan { int nsplit, split_len; };
SplitPlan split_plan(int blocks, int max_nb, int align, bool may_split) {
  const int max_splits = eyoc::cdiv(max_nb, align);
  int nsplit = may_split ? 4096 / (blocks > 0 ? blocks : 1) : 1;
  nsplit = nsplit < 1 ? 1 : nsplit > max_splits ? max_splits : nsplit;
  const int split_len = eyoc::cdiv(eyoc::cdiv(max_nb, nsplit), align) * align;
  return {eyoc::cdiv(max_nb, split_len), split_len};
}

template <int C>
void launch_knn(const float* A, const float* Bt, const SegPlan& p, int nseg, int dist_type, unsigned long long* best, float* second,
                bool dot, hipStream_t st, const int* only, const int* only_cnt) {
  const int qtiles = only ? 2 : eyoc::cdiv(p.max_na, 64);   // second pass of the pre-filter: two blocks per (segment, split) walk the list
  const SplitPlan sp = split_plan(qtiles * nseg, p.max_nb, SPLIT_ALIGN, !second);   // (a runner-up cannot be merged over blocks)
  const dim3 grid(qtiles, sp.nsplit, nseg);
  if (second) hipLaunchKernelGGL((knn1_kernel<C, true, 0>), grid, dim3(256), 0, st, A, Bt, p.seg, sp.split_len, dist_type, best, second, (const int*)nullptr, (const int*)nullptr);
  else if (dot) hipLaunchKernelGGL((knn1_kernel<C, false, 1>), grid, dim3(256), 0, st, A, Bt, p.seg, sp.split_len, 0, best, second, (const int*)nullptr, (const int*)nullptr);
  else if (dist_type == 2) hipLaunchKernelGGL((knn1_kernel<C, false, 2>), grid, dim3(256), 0, st, A, Bt, p.seg, sp.split_len, 0, best, second, only, only_cnt);
  else hipLaunchKernelGGL((knn1_kernel<C, false, 0>), grid, dim3(256), 0, st, A, Bt, p.seg, sp.split_len, dist_type, best, second, only, only_cnt);
}

template <int C>
void launch_knn_mutual(const float* A, const float* Bt, const SegPlan& p, int nseg, int dist_type, unsigned long long* best,
                       unsigned long long* colbest, hipStream_t st) {
  const int qtiles = eyoc::cdiv(p.max_na, 64);
  const SplitPlan sp = split_plan(qtiles * nseg, p.max_nb, MUT_SPLIT_ALIGN, true);
  const dim3 grid(qtiles, sp.nsplit, nseg);
  if (dist_type == 2) hipLaunchKernelGGL((knn1_mutual_kernel<C, 2>), grid, dim3(256), 0, st, A, Bt, p.seg, sp.split_len, 0, best, colbest);
  else hipLaunchKernelGGL((knn1_mutual_kernel<C, 0>), grid, dim3(256), 0, st, A, Bt, p.seg, sp.split_len, dist_type, best, colbest);
}

void launch_transpose(const float* B_dev, const SegPlan& p, int nseg, int c, float* Bt, hipStream_t st) {
  hipLaunchKernelGGL(knn_transpose_targets, dim3(eyoc::cdiv((long long)p.max_ld * (c / 4), 256), 1, nseg), dim3(256), 0, st, B_dev, p.seg, c, Bt);
}

// bmax (one word per segment) must be zero when this runs
void launch_pack_targets(const float* B_dev, const SegPlan& p, int nseg, float* Bm, int* bmax, int zero_norm, hipStream_t st) {
  hipLaunchKernelGGL(knn_pack_targets_mfma<32>, dim3(eyoc::cdiv(eyoc::cdiv(p.max_nb, 16), 4 * PK_TILES), 1, nseg), dim3(256), 0, st, B_dev, p.seg,
                     p.sm, Bm, bmax, zero_norm);
}

// MFMA pre-filter (see knn_mfma_kernel): `plain` index queries - no distances, no runner-up, no inner product - that fill the chip
// (a single pair - 79 waves, each walking all 5000 targets - takes 0.15 ms there against 0.10 in the exact kernel)
bool knn_prefilter_on(const eyoc_ctx* ctx, const SegPlan& p, int c, int dist_type, bool plain) {
  const int knob = ctx->knobs.knn_prefilter;
  return knob != 0 && plain && dist_type != 1 && c == 32 && p.max_nb > 0 && (p.waves_a >= 512 || knob == 2);
}

// The arrays of one one-way query, carved in ONE place: on a null base every pointer is null and `bytes` is what the query needs, on a
// workspace they are the arrays.  The byte count and the carving are the same code, so they cannot drift apart.
struct KnnWs {
  unsigned long long* best;   // [n_a] packed minima
  float* Bt;                  // the transposed targets, 64 bytes of slack behind them
  float *Bm, *anorm;          // pre-filter: the packed targets, |a|^2 per row
  int *flags, *bmax, *fcnt;   // pre-filter: the undecided rows per segment; bmax[MAX_SEG] and fcnt[MAX_SEG] are one array (one memset), 64 bytes of slack behind it
  size_t bytes;
};
KnnWs knn_layout(void* base, const SegPlan& p, bool prefilter) {
  eyoc::Carver cv(base, 0);
  KnnWs w = {};
  w.best = cv.take<unsigned long long>(p.n_a);
  w.Bt = cv.take<float>(p.bt_floats + 16);
  if (prefilter) {
    w.Bm = cv.take<float>(p.bm_floats);
    w.anorm = cv.take<float>(p.n_a);
    w.flags = cv.take<int>(p.n_a);
    w.bmax = cv.take<int>(2 * MAX_SEG + 16);
    w.fcnt = base ? w.bmax + MAX_SEG : nullptr;
  }
  w.bytes = eyoc::align_up(cv.off);
  return w;
}

// One one-way query of p.n_a > 0 rows on a workspace of the caller's (256-byte aligned).  It carves, it never allocates: no path from
// here reaches eyoc_ctx::ensure_scratch, whose growth frees the old buffer.  That is what lets eyoc_knn1_mutual keep arrays of its own in
// the same scratch across two of these runs - a workspace too small for the layout is EYOC_ERR_WORKSPACE here, not a buffer freed under
// queued kernels.  The guarantee is this structure; no test can see it (the scratch only grows, in a test process it has grown before).
// has_dev: see knn1_unpack.
int knn_run(const eyoc_ctx* ctx, void* ws, size_t ws_bytes, const SegPlan& p, int nseg, const float* A_dev, const float* B_dev, int c,
            int dist_type, bool dot, int64_t* idx_dev, float* dist_dev, float* second_dev, unsigned char* has_dev, hipStream_t st) {
  const bool prefilter = knn_prefilter_on(ctx, p, c, dist_type, !dot && !second_dev && !dist_dev);
  const KnnWs w = knn_layout(ws, p, prefilter);
  EYOC_REQUIRE(w.bytes <= ws_bytes, EYOC_ERR_WORKSPACE, "kNN query: workspace %zu < %zu bytes", ws_bytes, w.bytes);
  EYOC_CHECK_HIP(hipMemsetAsync(w.best, 0xFF, (size_t)p.n_a * sizeof(unsigned long long), st));
  if (prefilter) {
    EYOC_CHECK_HIP(hipMemsetAsync(w.bmax, 0, 2 * MAX_SEG * sizeof(int), st));
    launch_pack_targets(B_dev, p, nseg, w.Bm, w.bmax, dist_type == 2 ? 1 : 0, st);
    hipLaunchKernelGGL(knn_row_norms, dim3(eyoc::cdiv(p.n_a, 256)), dim3(256), 0, st, A_dev, p.n_a, c, w.anorm);
    const dim3 grid(eyoc::cdiv(p.max_na, 4 * MF_ROWS), 1, nseg);
    if (dist_type == 2)
      hipLaunchKernelGGL((knn_mfma_kernel<32, 2>), grid, dim3(256), 0, st, A_dev, w.Bm, p.seg, p.sm, w.anorm, w.bmax, w.best, w.flags, w.fcnt);
    else
      hipLaunchKernelGGL((knn_mfma_kernel<32, 0>), grid, dim3(256), 0, st, A_dev, w.Bm, p.seg, p.sm, w.anorm, w.bmax, w.best, w.flags, w.fcnt);
  }
  if (prefilter && dist_type == 0) {
    // the undecided rows, lane = target (no transposed copy of the targets needed)
    hipLaunchKernelGGL(knn1_list_kernel<32>, dim3(eyoc::cdiv(p.max_nb, 256), 1, nseg), dim3(256), 0, st, A_dev, B_dev, p.seg, w.best,
                       (const int*)w.flags, (const int*)w.fcnt);
  } else if (p.max_nb > 0) {
    launch_transpose(B_dev, p, nseg, c, w.Bt, st);
    dispatch_width(c, [&](auto width) {
      launch_knn<decltype(width)::value>(A_dev, w.Bt, p, nseg, dist_type, w.best, second_dev, dot, st, w.flags, w.fcnt);   // (null without the pre-filter)
    });
  }
  hipLaunchKernelGGL(knn1_unpack, dim3(eyoc::cdiv(p.n_a, 256)), dim3(256), 0, st, w.best, p.n_a, (long long*)idx_dev, dist_dev,
                     dot ? 1 : dist_type == 2 ? 2 : 0, has_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// eyoc_knn1 / eyoc_knn2 / eyoc_dotmax: the checks, ONE growth of the scratch to the layout's size, the run
int knn_query(const char* who, eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a, const int32_t* seg_b,
              int nseg, int dist_type, bool dot, int64_t* idx_dev, float* dist_dev, float* second_dev, void* stream) {
  EYOC_REQUIRE(ctx && A_dev && B_dev && seg_a && seg_b, EYOC_ERR_INVALID, "%s: NULL argument", who);
  EYOC_REQUIRE(dist_type >= 0 && dist_type <= 2, EYOC_ERR_INVALID, "%s: dist_type %d", who, dist_type);
  EYOC_REQUIRE(!(dist_type == 2 && (dot || second_dev)), EYOC_ERR_INVALID, "%s: dist_type 2 is a 1-NN mode", who);
  EYOC_REQUIRE(knn_width_ok(c), EYOC_ERR_INVALID, "%s: feature dimension %d not supported (4/16/32/64/128)", who, c);
  SegPlan p;
  if (int rc = seg_plan(who, seg_a, seg_b, nseg, c, &p)) return rc;
  if (p.n_a == 0) return EYOC_OK;
  EYOC_REQUIRE(seg_a[0] == 0, EYOC_ERR_INVALID, "%s: seg_a[0] must be 0", who);
  hipStream_t st = (hipStream_t)stream;
  const size_t need = knn_layout(nullptr, p, knn_prefilter_on(ctx, p, c, dist_type, !dot && !second_dev && !dist_dev)).bytes;
  if (int rc = ctx->ensure_scratch(need, st)) return rc;
  return knn_run(ctx, ctx->scratch, need, p, nseg, A_dev, B_dev, c, dist_type, dot, idx_dev, dist_dev, second_dev, nullptr, st);
}

// eyoc_knn1_mutual's share of the scratch: [has_a | has_b | idx_ba when the caller wants none] in front, then the fused route's three
// arrays or `dir`, dir_bytes for the two one-way runs (one after the other in the same bytes).  Null base: the byte count, like knn_layout.
struct MutualWs {
  unsigned char *has_a, *has_b;
  long long* idx_ba;
  unsigned long long *best, *colbest;
  float* Bt;
  char* dir;
  size_t bytes;
};
MutualWs mutual_layout(void* base, const SegPlan& p, bool own_idx_ba, bool fused, size_t dir_bytes) {
  eyoc::Carver cv(base, 0);
  MutualWs w = {};
  w.has_a = cv.take<unsigned char>(p.n_a);
  w.has_b = cv.take<unsigned char>(p.n_b);
  if (own_idx_ba) w.idx_ba = cv.take<long long>(p.n_b);
  if (fused) {
    w.best = cv.take<unsigned long long>(p.n_a);
    w.colbest = cv.take<unsigned long long>(p.n_b);
    w.Bt = cv.take<float>(p.bt_floats + 16);
  } else {
    w.dir = cv.take<char>(dir_bytes);
  }
  w.bytes = eyoc::align_up(cv.off);
  return w;
}

}  // namespace

extern "C" int eyoc_knn_prefilter(eyoc_ctx* ctx, int mode) {
  if (!ctx) return -1;
  const int prev = ctx->knobs.knn_prefilter;
  if (mode >= 0 && mode <= 2) ctx->knobs.knn_prefilter = mode;
  return prev;
}

extern "C" int eyoc_knn_pack_targets(eyoc_ctx* ctx, const float* B_dev, const int32_t* seg_b, int nseg, int zero_norm, float* packed_dev,
                                     size_t packed_floats, int32_t* bmax_dev, void* stream) {
  EYOC_REQUIRE(ctx && B_dev && seg_b && packed_dev && bmax_dev, EYOC_ERR_INVALID, "eyoc_knn_pack_targets: NULL argument");
  SegPlan p;
  if (int rc = seg_plan("eyoc_knn_pack_targets", nullptr, seg_b, nseg, 32, &p)) return rc;
  EYOC_REQUIRE((size_t)p.bm_floats <= packed_floats, EYOC_ERR_INVALID, "eyoc_knn_pack_targets: %lld floats needed, %zu given", p.bm_floats, packed_floats);
  hipStream_t st = (hipStream_t)stream;
  EYOC_CHECK_HIP(hipMemsetAsync(bmax_dev, 0, (size_t)nseg * sizeof(int32_t), st));
  if (p.max_nb > 0) launch_pack_targets(B_dev, p, nseg, packed_dev, bmax_dev, zero_norm ? 1 : 0, st);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

extern "C" int eyoc_knn1(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a,
                         const int32_t* seg_b, int nseg, int dist_type, int64_t* idx_dev, float* dist_dev,
                         void* stream) {
  return knn_query("eyoc_knn1", ctx, A_dev, B_dev, c, seg_a, seg_b, nseg, dist_type, false, idx_dev, dist_dev, nullptr, stream);
}

extern "C" int eyoc_dotmax(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a,
                           const int32_t* seg_b, int nseg, int64_t* idx_dev, float* weight_dev, void* stream) {
  return knn_query("eyoc_dotmax", ctx, A_dev, B_dev, c, seg_a, seg_b, nseg, 0, true, idx_dev, weight_dev, nullptr, stream);
}

extern "C" int eyoc_knn2(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a,
                         const int32_t* seg_b, int nseg, int64_t* idx_dev, float* d1_dev, float* d2_dev, void* stream) {
  EYOC_REQUIRE(d2_dev != nullptr, EYOC_ERR_INVALID, "eyoc_knn2: d2_dev is NULL");
  return knn_query("eyoc_knn2", ctx, A_dev, B_dev, c, seg_a, seg_b, nseg, 0, false, idx_dev, d1_dev, d2_dev, stream);
}

// ------------------------------------------------------------------------------------------------------------------
// mutual nearest neighbours
extern "C" int eyoc_knn_mutual_select(eyoc_ctx* ctx, int mode) {
  if (!ctx) return -1;
  const int prev = ctx->knobs.knn_mutual;
  if (mode >= -1 && mode <= 1) ctx->knobs.knn_mutual = mode;
  return prev + 2;
}

extern "C" int eyoc_knn1_mutual(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a, const int32_t* seg_b,
                                int nseg, int dist_type, int64_t* idx_ab_dev, int64_t* idx_ba_dev, uint8_t* mutual_dev, void* stream) {
  const char* who = "eyoc_knn1_mutual";
  EYOC_REQUIRE(ctx && A_dev && B_dev && seg_a && seg_b, EYOC_ERR_INVALID, "%s: NULL argument", who);
  EYOC_REQUIRE(dist_type >= 0 && dist_type <= 2, EYOC_ERR_INVALID, "%s: dist_type %d", who, dist_type);
  EYOC_REQUIRE(knn_width_ok(c), EYOC_ERR_INVALID, "%s: feature dimension %d not supported (4/16/32/64/128)", who, c);
  SegPlan ab, ba;   // A's rows against the targets B, and the reverse query
  if (int rc = seg_plan(who, seg_a, seg_b, nseg, c, &ab)) return rc;
  if (int rc = seg_plan(who, seg_b, seg_a, nseg, c, &ba)) return rc;
  EYOC_REQUIRE(seg_a[0] == 0 && seg_b[0] == 0, EYOC_ERR_INVALID, "%s: seg_a[0] and seg_b[0] must be 0", who);
  hipStream_t st = (hipStream_t)stream;
  const int n_a = ab.n_a, n_b = ab.n_b;
  if (n_a == 0 && (n_b == 0 || !idx_ba_dev)) return EYOC_OK;
  EYOC_REQUIRE((n_a == 0 || (idx_ab_dev && mutual_dev)), EYOC_ERR_INVALID, "%s: NULL output", who);
  // auto, as measured (EXPERIMENTS.md "Mutual nearest-neighbour filter"): the fused sweep for c = 32 queries that do not fill the chip in
  // either direction (< 512 waves of MF_ROWS rows: eyoc_knn1 runs its exact kernel there, twice; a single 5000 x 5000 pair: 0.19 against
  // 0.30 ms), two one-way queries where the MFMA pre-filter carries them (64 pairs: 1.4 against 4.6 ms) and for every shape class that
  // was not measured (other widths, whose fused kernel spills)
  const int route = ctx->knobs.knn_mutual >= 0 ? ctx->knobs.knn_mutual : (c == 32 && ab.waves_a < 512 && ab.waves_b < 512) ? 1 : 0;
  const bool fused = route != 0 && ab.max_na > 0 && ab.max_nb > 0;
  // the scratch grows HERE, once, to the front plus the larger of the two directions' layouts; knn_run below gets its slice and cannot grow it
  const size_t need_ab = knn_layout(nullptr, ab, knn_prefilter_on(ctx, ab, c, dist_type, true)).bytes;
  const size_t need_ba = knn_layout(nullptr, ba, knn_prefilter_on(ctx, ba, c, dist_type, true)).bytes;
  const size_t dir_bytes = need_ab > need_ba ? need_ab : need_ba;
  if (int rc = ctx->ensure_scratch(mutual_layout(nullptr, ab, !idx_ba_dev, fused, dir_bytes).bytes, st)) return rc;
  const MutualWs w = mutual_layout(ctx->scratch, ab, !idx_ba_dev, fused, dir_bytes);
  long long* idx_ba = idx_ba_dev ? (long long*)idx_ba_dev : w.idx_ba;
  if (!fused) {
    // both one-way queries as eyoc_knn1 runs them (a side without rows has nothing to write)
    int rc = EYOC_OK;
    if (n_a) rc = knn_run(ctx, w.dir, dir_bytes, ab, nseg, A_dev, B_dev, c, dist_type, false, idx_ab_dev, nullptr, nullptr, w.has_a, st);
    if (rc) return rc;
    if (n_b) rc = knn_run(ctx, w.dir, dir_bytes, ba, nseg, B_dev, A_dev, c, dist_type, false, (int64_t*)idx_ba, nullptr, nullptr, w.has_b, st);
    if (rc) return rc;
  } else {
    EYOC_CHECK_HIP(hipMemsetAsync(w.best, 0xFF, (size_t)n_a * 8, st));
    EYOC_CHECK_HIP(hipMemsetAsync(w.colbest, 0xFF, (size_t)n_b * 8, st));
    launch_transpose(B_dev, ab, nseg, c, w.Bt, st);
    dispatch_width(c, [&](auto width) { launch_knn_mutual<decltype(width)::value>(A_dev, w.Bt, ab, nseg, dist_type, w.best, w.colbest, st); });
    hipLaunchKernelGGL(knn1_unpack, dim3(eyoc::cdiv(n_a, 256)), dim3(256), 0, st, w.best, n_a, (long long*)idx_ab_dev, (float*)nullptr, 0, w.has_a);
    hipLaunchKernelGGL(knn1_unpack, dim3(eyoc::cdiv(n_b, 256)), dim3(256), 0, st, w.colbest, n_b, idx_ba, (float*)nullptr, 0, w.has_b);
  }
  if (n_a)
    hipLaunchKernelGGL(knn_mutual_flags, dim3(eyoc::cdiv(ab.max_na, 256), 1, nseg), dim3(256), 0, st, ab.seg, (const long long*)idx_ab_dev,
                       (const long long*)idx_ba, (const unsigned char*)w.has_a, (const unsigned char*)w.has_b, (unsigned char*)mutual_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

extern "C" int eyoc_mutual_compact(eyoc_ctx* ctx, const int64_t* idx_ab_dev, const uint8_t* mutual_dev, const int32_t* seg_a, int nseg,
                                   int min_keep, int64_t* rows_dev, int64_t* corr_dev, int32_t* seg_out_dev, void* stream) {
  EYOC_REQUIRE(ctx && seg_a && seg_out_dev, EYOC_ERR_INVALID, "eyoc_mutual_compact: NULL argument");
  SegPlan p;
  if (int rc = seg_plan("eyoc_mutual_compact", seg_a, nullptr, nseg, 0, &p)) return rc;
  EYOC_REQUIRE(min_keep >= 0 && seg_a[0] == 0, EYOC_ERR_INVALID, "eyoc_mutual_compact: min_keep %d, seg_a[0] %d", min_keep, seg_a[0]);
  hipStream_t st = (hipStream_t)stream;
  const int n = p.n_a;
  if (n == 0) {
    EYOC_CHECK_HIP(hipMemsetAsync(seg_out_dev, 0, (size_t)(nseg + 1) * sizeof(int32_t), st));
    return EYOC_OK;
  }
  EYOC_REQUIRE(idx_ab_dev && mutual_dev && rows_dev && corr_dev, EYOC_ERR_INVALID, "eyoc_mutual_compact: NULL argument");
  const int tiles = eyoc::cdiv(n, SCAN_TILE);
  int *cnt = nullptr, *keep = nullptr, *loc = nullptr, *partial = nullptr;
  auto carve = [&](void* base) {
    eyoc::Carver cv(base, 0);
    cnt = cv.take<int>(2 * MAX_SEG);      // + fallback[MAX_SEG]
    keep = cv.take<int>(n);
    loc = cv.take<int>(n);
    partial = cv.take<int>(tiles + 2);    // [tiles] + the total behind them
    return eyoc::align_up(cv.off);
  };
  if (int rc = ctx->ensure_scratch(carve(nullptr), st)) return rc;
  carve(ctx->scratch);
  int* fallback = cnt + MAX_SEG;
  hipLaunchKernelGGL(k_mutual_count, dim3(nseg), dim3(SCAN_BLOCK), 0, st, p.seg, (const unsigned char*)mutual_dev, min_keep, cnt, fallback);
  hipLaunchKernelGGL(k_mutual_keep, dim3(eyoc::cdiv(p.max_na, 256), 1, nseg), dim3(256), 0, st, p.seg, nseg, (const unsigned char*)mutual_dev,
                     (const int*)cnt, (const int*)fallback, keep, loc, seg_out_dev);
  hipLaunchKernelGGL(k_scan_partials, dim3(tiles), dim3(SCAN_BLOCK), 0, st, (const int*)keep, n, partial);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(SCAN_BLOCK), 0, st, partial, tiles, partial + tiles);
  hipLaunchKernelGGL(k_mutual_fill, dim3(tiles), dim3(SCAN_BLOCK), 0, st, (const int*)keep, (const int*)loc, (const int*)partial,
                     (const long long*)idx_ab_dev, n, (long long*)rows_dev, (long long*)corr_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

extern "C" int eyoc_pdist(eyoc_ctx* ctx, const float* A_dev, int n, const float* B_dev, int m, int c, int dist_type,
                          float* out_dev, void* stream) {
  EYOC_REQUIRE(ctx && A_dev && B_dev && out_dev, EYOC_ERR_INVALID, "eyoc_pdist: NULL argument");
  EYOC_REQUIRE(n >= 0 && m >= 0 && c >= 1, EYOC_ERR_INVALID, "eyoc_pdist: bad shape %d x %d x %d", n, m, c);
  EYOC_REQUIRE(dist_type == 0 || dist_type == 1, EYOC_ERR_INVALID, "eyoc_pdist: dist_type %d", dist_type);
  const long long total = (long long)n * m;
  if (total == 0) return EYOC_OK;
  hipLaunchKernelGGL(pdist_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A_dev, n,
                     B_dev, m, c, dist_type, out_dev);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}
