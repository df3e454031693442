// Instance normalisation over the rows of a sparse tensor (MinkowskiInstanceNorm, model/common.py:7-8; the norm inside every residual
// block of the ResUNetIN2 family, model/residual_block.py:60-61): per INSTANCE b (column 0 of the level's coordinates) and channel
//   mean = sum_{r in b} x / n_b,  var = sum_{r in b} (x - mean)^2 / n_b  (biased),  y = (x - mean) / sqrt(var + eps) * weight + bias
// [+ residual] [ReLU], and its backward dx = weight invstd (g - mean_b(g) - xhat mean_b(g xhat)), dweight = sum g xhat, dbias = sum g
// over ALL rows.  No running statistics: eval mode is training mode.  Unlike batch norm (bn.hip) the statistics belong to the input, so
// nothing folds into weights, and the reduction is SEGMENTED: the rows of one instance need not be contiguous (Z-ordered maps).
//
// Streaming passes like bn.hip: lanes along channels (coalesced), float4 element-wise passes, fp64 partial sums about a shift (the
// instance's first row in plan order; see k_bn_partial MODE 0 for why) written to the workspace and added in a FIXED order.  No
// floating-point atomics anywhere.
//
// Batch invariance.  An instance's rows, in plan order, are cut into chunks of IN_CHUNK rows; one workgroup sums one chunk (thread
// (sub, ch) takes the chunk's rows sub, sub + 256 / c, ...; the subs meet in ascending order), and the chunks of an instance meet in
// the order k_in_final walks them, which depends on their number alone.  So the bytes of an instance's statistics, y and dx rows are a
// function of that instance's rows and of nothing else: not of the other instances, of how the rows interleave, of the grid or of timing.
#include "spconv.h"

using namespace eyoc;

namespace {

constexpr int IN_CHUNK = 64;          // rows per partial sum (bn.hip sums 64 rows per workgroup below 65536 rows)
constexpr int IN_PLAN_ROWS = 1024;    // rows per workgroup of the plan's counting sort
constexpr int IN_MAX_INST = 1024;     // the library's batch limit (pack_key keeps 10 bits of batch index)

// The plan, int32 words: header {identity, n, n_inst, bad ids}, seg [n_inst + 1], cseg [n_inst + 1] (first chunk of every instance),
// perm [n], inst [n] (instance of every row), then the sort's scratch: counts [row blocks][n_inst] and two flag words.
struct PlanLayout {
  size_t seg, cseg, perm, inst, counts, flags, words;
};
inline size_t up4(size_t v) { return (v + 3) / 4 * 4; }
PlanLayout plan_layout(int n, int n_inst) {
  PlanLayout L;
  L.seg = 4;
  L.cseg = L.seg + up4((size_t)n_inst + 1);
  L.perm = L.cseg + up4((size_t)n_inst + 1);
  L.inst = L.perm + up4((size_t)n);
  L.counts = L.inst + up4((size_t)n);
  L.flags = L.counts + up4((size_t)cdiv(n, IN_PLAN_ROWS) * n_inst);
  L.words = L.flags + 4;
  return L;
}
struct PlanView {               // what the kernels read
  const int32_t *hdr, *seg, *cseg, *perm, *inst;
};
PlanView plan_view(const void* plan, int n, int n_inst) {
  const PlanLayout L = plan_layout(n, n_inst);
  const int32_t* p = (const int32_t*)plan;
  return {p, p + L.seg, p + L.cseg, p + L.perm, p + L.inst};
}

bool in_shape_ok(int n, int c) { return n >= 1 && c >= 4 && c <= 256 && 256 % c == 0; }
bool in_inst_ok(int n_inst) { return n_inst >= 1 && n_inst <= IN_MAX_INST; }
int in_max_chunks(int n, int n_inst) { return cdiv(n, IN_CHUNK) + n_inst; }      // sum_b ceil(n_b / R) <= n / R + n_inst

// ---------------------------------------------------------------------------------------------- plan: a stable counting sort
// Pass 1: counts[block][id] over the block's rows (integer LDS atomics COUNT; nothing is handed out by them), the row's instance, and
// two flags: an id outside [0, n_inst), an id below its predecessor's.
__global__ __launch_bounds__(256) void k_in_plan_count(const int32_t* __restrict__ coords, int n, int n_inst, int32_t* __restrict__ inst,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ flags) {
  __shared__ int hist[IN_MAX_INST];
  for (int i = threadIdx.x; i < n_inst; i += 256) hist[i] = 0;
  __syncthreads();
  const int r0 = blockIdx.x * IN_PLAN_ROWS, r1 = min(n, r0 + IN_PLAN_ROWS);
  int bad = 0, down = 0;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const int id = coords[(size_t)r * 4];
    inst[r] = id;
    if (id < 0 || id >= n_inst) { bad = 1; continue; }
    atomicAdd(&hist[id], 1);
    if (r > 0 && coords[(size_t)(r - 1) * 4] > id) down = 1;
  }
  if (bad) atomicOr(&flags[0], 1);
  if (down) atomicOr(&flags[1], 1);
  __syncthreads();
  for (int i = threadIdx.x; i < n_inst; i += 256) counts[(size_t)blockIdx.x * n_inst + i] = hist[i];
}

// Pass 2 (one workgroup): counts[block][id] -> rows of the id in earlier blocks; seg, cseg by a serial walk of <= 1024 totals; header.
__global__ __launch_bounds__(1024) void k_in_plan_scan(int32_t* __restrict__ counts, int blocks, int n, int n_inst, const int32_t* __restrict__ flags,
                                                       int32_t* __restrict__ hdr, int32_t* __restrict__ seg, int32_t* __restrict__ cseg) {
  __shared__ int total[IN_MAX_INST];
  const int i = threadIdx.x;
  if (i < n_inst) {
    // eight loads in flight per step: one load, one store at a time is a memory latency per row block, 2 ms for the 3737 + ... row
    // blocks of a 64-pair batch's four levels (a thread owns its column, so the order of its loads and stores is free)
    int run = 0, b = 0;
    for (; b + 8 <= blocks; b += 8) {
      int v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = counts[(size_t)(b + j) * n_inst + i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        counts[(size_t)(b + j) * n_inst + i] = run;
        run += v[j];
      }
    }
    for (; b < blocks; ++b) {
      const int v = counts[(size_t)b * n_inst + i];
      counts[(size_t)b * n_inst + i] = run;
      run += v;
    }
    total[i] = run;
  }
  __syncthreads();
  if (i == 0) {
    int rows = 0, chunks = 0;
    for (int b = 0; b < n_inst; ++b) {
      seg[b] = rows;
      cseg[b] = chunks;
      rows += total[b];
      chunks += (total[b] + IN_CHUNK - 1) / IN_CHUNK;
    }
    seg[n_inst] = rows;
    cseg[n_inst] = chunks;
    hdr[0] = flags[1] ? 0 : 1;      // identity: the ids never step down, perm is 0, 1, 2 ... and is not read
    hdr[1] = n;
    hdr[2] = n_inst;
    hdr[3] = flags[0];
  }
}

// Pass 3: perm[seg[id] + rows of id in earlier blocks + rows of id EARLIER IN THIS BLOCK] = row - the slot is computed, not claimed.
// `hdr` (optional): the build that never reads the header back (in_plan_build_nosync) launches this pass always and leaves the identity
// decision to it - an identity plan's perm is not read, so it stays unwritten.
__global__ __launch_bounds__(256) void k_in_plan_place(const int32_t* __restrict__ inst, int n, int n_inst, const int32_t* __restrict__ counts,
                                                       const int32_t* __restrict__ seg, int32_t* __restrict__ perm, const int32_t* __restrict__ hdr) {
  __shared__ int ids[IN_PLAN_ROWS];
  if (hdr && hdr[0]) return;
  const int r0 = blockIdx.x * IN_PLAN_ROWS, m = min(n - r0, IN_PLAN_ROWS);
  for (int i = threadIdx.x; i < m; i += 256) ids[i] = inst[r0 + i];
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += 256) {
    const int id = ids[i];
    if (id < 0 || id >= n_inst) continue;
    int rank = 0;
    for (int k = 0; k < i; ++k) rank += ids[k] == id;
    const int slot = seg[id] + counts[(size_t)blockIdx.x * n_inst + id] + rank;
    if (slot >= 0 && slot < n) perm[slot] = r0 + i;
  }
}

// the perm of an identity plan (never read by the kernels; written so that the plan's words are defined)
__global__ __launch_bounds__(256) void k_in_plan_iota(int32_t* __restrict__ perm, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) perm[i] = i;
}

// ---------------------------------------------------------------------------------------------- the sums
// the chunk a workgroup owns: instance b with cseg[b] <= blockIdx.x < cseg[b + 1], rows [p0, p1) in plan order
__device__ inline bool chunk_of(const PlanView& P, int n, int n_inst, int& b, int& p0, int& p1) {
  if (P.hdr[1] != n || P.hdr[2] != n_inst || P.hdr[3]) return false;          // not the plan of this tensor
  const int k = blockIdx.x;
  if (k >= P.cseg[n_inst]) return false;
  int lo = 0, hi = n_inst;                       // the last b with cseg[b] <= k (empty instances share their successor's value)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (P.cseg[mid] <= k) lo = mid; else hi = mid;
  }
  b = lo;
  p0 = P.seg[b] + (k - P.cseg[b]) * IN_CHUNK;
  p1 = min(P.seg[b + 1], p0 + IN_CHUNK);
  return p0 >= 0 && p1 <= n;
}

// one channel of a row: fp32 rows, or SPLIT16 rows (spconv.h: hi + lo, the value split16_decode4 gives - so the sums below are, bit
// for bit, those of the fp32 kernel on the decoded rows).  One channel per lane keeps the summation order of the fp32 pass; a wave's 32
// lanes of a channel block read the block's 64 contiguous hi bytes, then its 64 lo bytes: whole 128-byte lines either way.
template <bool SPLIT>
__device__ inline float ld1(const float* row, int ch) {
  if (!SPLIT) return row[ch];
  const char* p = reinterpret_cast<const char*>(row) + (ch >> 5) * 128 + (ch & 31) * 2;
  return (float)*reinterpret_cast<const _Float16*>(p) + (float)*reinterpret_cast<const _Float16*>(p + SPLIT16_LO);
}

// partial[chunk][0..c) = sum of a, [c..2c) = sum of b over the chunk's rows.  MODE 0: a = x - s, b = (x - s)^2, s = the instance's
// first row in plan order.  MODE 1: a = g, b = g * xhat (g = dy where y > 0 when `y` is given).
template <int MODE, bool SPLIT = false>
__global__ __launch_bounds__(256) void k_in_partial(const float* __restrict__ x, int ld_x, const float* __restrict__ y, int ld_y,
                                                    const float* __restrict__ dy, int ld_dy, int n, int c, PlanView P, int n_inst,
                                                    const float* __restrict__ stats, float eps, double* __restrict__ partial) {
  __shared__ double sa[256], sb[256];
  int b, p0, p1;
  if (!chunk_of(P, n, n_inst, b, p0, p1)) return;
  const bool ident = P.hdr[0] != 0;
  const int ch = threadIdx.x % c, sub = threadIdx.x / c, nsub = 256 / c;
  double a = 0.0, bb = 0.0, shift = 0.0;
  float mean = 0.f, invstd = 0.f;
  if (MODE == 0) {
    const int first = ident ? P.seg[b] : P.perm[P.seg[b]];
    shift = (unsigned)first < (unsigned)n ? (double)ld1<SPLIT>(x + (size_t)first * ld_x, ch) : 0.0;
  } else {
    mean = stats[(size_t)b * 2 * c + ch];
    invstd = 1.0f / sqrtf(stats[(size_t)b * 2 * c + c + ch] + eps);
  }
  for (int p = p0 + sub; p < p1; p += nsub) {
    const int r = ident ? p : P.perm[p];
    if ((unsigned)r >= (unsigned)n) continue;
    const float xv = ld1<SPLIT>(x + (size_t)r * ld_x, ch);
    if (MODE == 0) {
      const double d = (double)xv - shift;
      a += d;
      bb += d * d;
    } else {
      float g = dy[(size_t)r * ld_dy + ch];
      if (y && !(y[(size_t)r * ld_y + ch] > 0.0f)) g = 0.0f;
      a += (double)g;
      bb += (double)g * (double)((xv - mean) * invstd);
    }
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = bb;
  __syncthreads();
  if (sub == 0) {
    for (int s = 1; s < nsub; ++s) { a += sa[s * c + ch]; bb += sb[s * c + ch]; }    // fixed order
    partial[(size_t)blockIdx.x * 2 * c + ch] = a;
    partial[(size_t)blockIdx.x * 2 * c + c + ch] = bb;
  }
}

// One workgroup per (two channels, instance), like k_bn_final: thread t adds column (t & 3) = (channel, a / b) of the instance's chunks
// t >> 2, t >> 2 + 64, ... in ascending order, the 64 sums meet in a fixed tree.  MODE 0: stats[b] = {mean, biased variance}.
// MODE 1: isum[b] = {sum g, sum g xhat} (fp64: k_in_param_grads adds them over the instances; the apply pass rounds them to fp32).
// An instance without rows writes nothing.
template <int MODE, bool SPLIT = false>
__global__ __launch_bounds__(256) void k_in_final(const double* __restrict__ partial, const float* __restrict__ x, int ld_x, int n, int c, PlanView P,
                                                  int n_inst, float* __restrict__ stats, double* __restrict__ isum) {
  __shared__ double red[256];
  if (P.hdr[1] != n || P.hdr[2] != n_inst || P.hdr[3]) return;
  const int col = threadIdx.x & 3, sub = threadIdx.x >> 2;
  const int ch = blockIdx.x * 2 + (col >> 1), ab = col & 1;
  // gridDim.y == n_inst: one instance per workgroup.  The packed plan (launch_in_layer) does not know how many of its IN_MAX_INST ids
  // have rows and walks them with a small grid; an instance's arithmetic does not depend on which workgroup does it.
  for (int b = blockIdx.y; b < n_inst; b += gridDim.y) {
    const int nb = P.seg[b + 1] - P.seg[b];
    if (nb <= 0) continue;
    const int k0 = P.cseg[b], k1 = P.cseg[b + 1];
    double s = 0.0;
    if (ch < c)
      for (int k = k0 + sub; k < k1; k += 64) s += partial[(size_t)k * 2 * c + ab * c + ch];
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
      if (sub < w) red[threadIdx.x] += red[threadIdx.x + 4 * w];
      __syncthreads();
    }
    if (threadIdx.x < 4 && ab == 0 && ch < c) {
      const double a = red[threadIdx.x], bb = red[threadIdx.x + 1];
      if (MODE == 0) {
        const int first = P.hdr[0] ? P.seg[b] : P.perm[P.seg[b]];
        const double x0 = (unsigned)first < (unsigned)n ? (double)ld1<SPLIT>(x + (size_t)first * ld_x, ch) : 0.0;
        const double ms = a / nb;
        double v = bb / nb - ms * ms;
        if (v < 0.0) v = 0.0;
        stats[(size_t)b * 2 * c + ch] = (float)(x0 + ms);
        stats[(size_t)b * 2 * c + c + ch] = (float)v;
      } else {
        isum[(size_t)b * 2 * c + ch] = a;
        isum[(size_t)b * 2 * c + c + ch] = bb;
      }
    }
    __syncthreads();                                                      // red is free for the next instance
  }
}

// dbias[ch] = sum_b isum[b][ch], dweight[ch] = sum_b isum[b][c + ch], instances in ascending id (those without rows skipped)
__global__ __launch_bounds__(256) void k_in_param_grads(const double* __restrict__ isum, int n, int c, PlanView P, int n_inst,
                                                        float* __restrict__ dweight, float* __restrict__ dbias) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * c || P.hdr[1] != n || P.hdr[2] != n_inst || P.hdr[3]) return;
  double s = 0.0;
  for (int b = 0; b < n_inst; ++b)
    if (P.seg[b + 1] > P.seg[b]) s += isum[(size_t)b * 2 * c + t];
  if (t < c) dbias[t] = (float)s; else dweight[t - c] = (float)s;
}

// ---------------------------------------------------------------------------------------------- the element-wise passes
__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// y = (x - mean_b) * invstd_b * weight + bias [+ residual] [ReLU]; the arithmetic of k_bn_apply per element.  SPLIT: x, residual and y
// are SPLIT16 rows (8 bytes of hi halves + 8 bytes of lo halves per lane, the lanes of a channel block side by side) - decode, the same
// arithmetic, encode; like every writer of SPLIT16 rows it feeds the range guard (spconv.h split16_guard).  In place (y == x) is fine:
// a thread reads its four channels before it writes them.
template <bool SPLIT>
__global__ __launch_bounds__(256) void k_in_apply(const float* x, int ld_x, int n, int c, PlanView P, int n_inst,
                                                  const float* __restrict__ stats, const float* __restrict__ weight, const float* __restrict__ bias,
                                                  float eps, int relu, const float* res, int ld_res, float* y, int ld_y, unsigned int* range) {
  const int c4 = c / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool live = i < (long long)n * c4 && P.hdr[1] == n && P.hdr[2] == n_inst && !P.hdr[3];
  const int r = live ? (int)(i / c4) : 0, q = live ? (int)(i % c4) * 4 : 0;
  const int b = live ? P.inst[r] : 0;
  live = live && (unsigned)b < (unsigned)n_inst;
  float mx = 0.0f;
  if (live) {
    const float4 v = SPLIT ? split16_load4(x + (size_t)r * ld_x, q) : ld4(x + (size_t)r * ld_x + q);
    const float4 m = ld4(stats + (size_t)b * 2 * c + q), va = ld4(stats + (size_t)b * 2 * c + c + q);
    const float4 g = ld4(weight + q), be = ld4(bias + q);
    float4 o;
    o.x = (v.x - m.x) * (1.0f / sqrtf(va.x + eps)) * g.x + be.x;
    o.y = (v.y - m.y) * (1.0f / sqrtf(va.y + eps)) * g.y + be.y;
    o.z = (v.z - m.z) * (1.0f / sqrtf(va.z + eps)) * g.z + be.z;
    o.w = (v.w - m.w) * (1.0f / sqrtf(va.w + eps)) * g.w + be.w;
    if (res) {
      const float4 t = SPLIT ? split16_load4(res + (size_t)r * ld_res, q) : ld4(res + (size_t)r * ld_res + q);
      o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
    }
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    if (SPLIT) { split16_track(mx, o); split16_store4(y + (size_t)r * ld_y, q, o); }
    else *reinterpret_cast<float4*>(y + (size_t)r * ld_y + q) = o;
  }
  if (SPLIT) {
    for (int o = 32; o; o >>= 1) mx = split16_merge(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) split16_report(range, mx);
  }
}

__device__ inline float in_dx(float x, float g, float mean, float var, float eps, float w, float sa, float sb, float inv_n) {
  const float invstd = 1.0f / sqrtf(var + eps);
  const float xhat = (x - mean) * invstd;
  return w * invstd * (g - sa * inv_n - xhat * sb * inv_n);
}

// dx = weight * invstd_b * (g - sum_b(g) / n_b - xhat * sum_b(g xhat) / n_b); dres = g (the residual's gradient) when asked for
__global__ __launch_bounds__(256) void k_in_backward_apply(const float* __restrict__ x, int ld_x, const float* __restrict__ y, int ld_y,
                                                           const float* __restrict__ dy, int ld_dy, int n, int c, PlanView P, int n_inst,
                                                           const float* __restrict__ stats, const float* __restrict__ weight, float eps,
                                                           const double* __restrict__ isum, float* __restrict__ dx, int ld_dx,
                                                           float* __restrict__ dres, int ld_dres) {
  const int c4 = c / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * c4 || P.hdr[1] != n || P.hdr[2] != n_inst || P.hdr[3]) return;
  const int r = (int)(i / c4), q = (int)(i % c4) * 4;
  const int b = P.inst[r];
  if ((unsigned)b >= (unsigned)n_inst) return;
  const float4 v = ld4(x + (size_t)r * ld_x + q);
  float4 g = ld4(dy + (size_t)r * ld_dy + q);
  if (y) {
    const float4 yo = ld4(y + (size_t)r * ld_y + q);
    if (!(yo.x > 0.0f)) g.x = 0.0f;
    if (!(yo.y > 0.0f)) g.y = 0.0f;
    if (!(yo.z > 0.0f)) g.z = 0.0f;
    if (!(yo.w > 0.0f)) g.w = 0.0f;
  }
  const float* st = stats + (size_t)b * 2 * c;
  const double* su = isum + (size_t)b * 2 * c;
  const float4 m = ld4(st + q), va = ld4(st + c + q), w = ld4(weight + q);
  const float inv_n = 1.0f / (float)(P.seg[b + 1] - P.seg[b]);
  float4 o;
  o.x = in_dx(v.x, g.x, m.x, va.x, eps, w.x, (float)su[q + 0], (float)su[c + q + 0], inv_n);
  o.y = in_dx(v.y, g.y, m.y, va.y, eps, w.y, (float)su[q + 1], (float)su[c + q + 1], inv_n);
  o.z = in_dx(v.z, g.z, m.z, va.z, eps, w.z, (float)su[q + 2], (float)su[c + q + 2], inv_n);
  o.w = in_dx(v.w, g.w, m.w, va.w, eps, w.w, (float)su[q + 3], (float)su[c + q + 3], inv_n);
  *reinterpret_cast<float4*>(dx + (size_t)r * ld_dx + q) = o;
  if (dres) *reinterpret_cast<float4*>(dres + (size_t)r * ld_dres + q) = g;
}

struct InWorkspace {
  double *partial, *isum;
  size_t bytes;
};
InWorkspace in_workspace(void* ws, int n, int c, int n_inst) {
  Carver cv(ws, ~(size_t)0);
  InWorkspace W;
  W.partial = cv.take<double>((size_t)in_max_chunks(n, n_inst) * 2 * c);
  W.isum = cv.take<double>((size_t)n_inst * 2 * c);
  W.bytes = align_up(cv.off);
  return W;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// eyoc_in_forward on fp32 rows (SPLIT = false) or SPLIT16 rows: the three launches
template <bool SPLIT>
int in_forward_launch(const float* x_dev, int n, int c, int ld_x, const PlanView& P, int n_inst, int final_rows, const float* weight_dev,
                             const float* bias_dev, float eps, int relu, const float* residual_dev, int ld_res, float* y_dev, int ld_y,
                             float* stats_dev, double* partial, unsigned int* range, hipStream_t st) {
  hipLaunchKernelGGL((k_in_partial<0, SPLIT>), dim3(in_max_chunks(n, n_inst)), dim3(256), 0, st, x_dev, ld_x, (const float*)nullptr, 0,
                     (const float*)nullptr, 0, n, c, P, n_inst, (const float*)nullptr, eps, partial);
  hipLaunchKernelGGL((k_in_final<0, SPLIT>), dim3(cdiv(c, 2), final_rows), dim3(256), 0, st, (const double*)partial, x_dev, ld_x, n, c, P, n_inst,
                     stats_dev, (double*)nullptr);
  hipLaunchKernelGGL(k_in_apply<SPLIT>, dim3(cdiv((long long)n * (c / 4), 256)), dim3(256), 0, st, x_dev, ld_x, n, c, P, n_inst,
                     (const float*)stats_dev, weight_dev, bias_dev, eps, relu, residual_dev, ld_res, y_dev, ld_y, range);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // namespace

extern "C" {

int eyoc_in_chunk_rows(void) { return IN_CHUNK; }

size_t eyoc_in_plan_bytes(int n, int n_inst) {
  if (n < 1 || !in_inst_ok(n_inst)) return 0;
  return align_up(plan_layout(n, n_inst).words * sizeof(int32_t));
}

int eyoc_in_plan_layout(int n, int n_inst, int64_t* offsets_out) {
  EYOC_REQUIRE(offsets_out && n >= 1 && in_inst_ok(n_inst), EYOC_ERR_INVALID, "eyoc_in_plan_layout: n %d, n_inst %d (1 .. %d)", n, n_inst, IN_MAX_INST);
  const PlanLayout L = plan_layout(n, n_inst);
  offsets_out[0] = 0;
  offsets_out[1] = (int64_t)L.seg * 4;
  offsets_out[2] = (int64_t)L.perm * 4;
  offsets_out[3] = (int64_t)L.inst * 4;
  return EYOC_OK;
}

int eyoc_in_plan_build(eyoc_ctx* ctx, const int32_t* coords_dev, int n, int n_inst, void* plan_dev, size_t plan_bytes, void* stream) {
  EYOC_REQUIRE(ctx && coords_dev && plan_dev, EYOC_ERR_INVALID, "eyoc_in_plan_build: NULL argument");
  EYOC_REQUIRE(n >= 1 && in_inst_ok(n_inst), EYOC_ERR_INVALID, "eyoc_in_plan_build: n %d, n_inst %d (1 .. %d)", n, n_inst, IN_MAX_INST);
  EYOC_REQUIRE(plan_bytes >= eyoc_in_plan_bytes(n, n_inst), EYOC_ERR_WORKSPACE, "eyoc_in_plan_build: plan %zu < %zu bytes", plan_bytes,
               eyoc_in_plan_bytes(n, n_inst));
  hipStream_t st = (hipStream_t)stream;
  const PlanLayout L = plan_layout(n, n_inst);
  int32_t* p = (int32_t*)plan_dev;
  const int blocks = cdiv(n, IN_PLAN_ROWS);
  EYOC_CHECK_HIP(hipMemsetAsync(p + L.flags, 0, 4 * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_in_plan_count, dim3(blocks), dim3(256), 0, st, coords_dev, n, n_inst, p + L.inst, p + L.counts, p + L.flags);
  hipLaunchKernelGGL(k_in_plan_scan, dim3(1), dim3(1024), 0, st, p + L.counts, blocks, n, n_inst, p + L.flags, p, p + L.seg, p + L.cseg);
  EYOC_CHECK_HIP(hipGetLastError());
  // the one read-back of a plan's life: ids outside [0, n_inst) are refused (the kernels of such a plan do nothing), and an identity
  // plan skips the placement (k_in_plan_place ranks a row among its workgroup's 1024 by a serial walk: 80 us per level measured, which
  // a collated batch in the caller's order - or in Z-order, whose key leads with the batch index - never needs)
  int32_t hdr[4] = {0, 0, 0, 0};
  EYOC_CHECK_HIP(hipMemcpyAsync(hdr, p, sizeof(hdr), hipMemcpyDeviceToHost, st));
  EYOC_CHECK_HIP(hipStreamSynchronize(st));
  EYOC_REQUIRE(hdr[3] == 0, EYOC_ERR_INVALID, "eyoc_in_plan_build: an instance id outside [0, %d)", n_inst);
  if (hdr[0])
    hipLaunchKernelGGL(k_in_plan_iota, dim3(cdiv(n, 256)), dim3(256), 0, st, p + L.perm, n);
  else
    hipLaunchKernelGGL(k_in_plan_place, dim3(blocks), dim3(256), 0, st, p + L.inst, n, n_inst, p + L.counts, p + L.seg, p + L.perm,
                       (const int32_t*)nullptr);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

size_t eyoc_in_workspace_bytes(int n, int c, int n_inst) {
  return in_shape_ok(n, c) && in_inst_ok(n_inst) ? in_workspace(nullptr, n, c, n_inst).bytes : 0;
}

static int in_forward_checked(const char* who, bool split, eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const void* plan_dev, int n_inst,
                              const float* weight_dev, const float* bias_dev, float eps, int relu, const float* residual_dev, int ld_res, float* y_dev,
                              int ld_y, float* stats_dev, unsigned int* range_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx && x_dev && plan_dev && weight_dev && bias_dev && y_dev && stats_dev && ws_dev, EYOC_ERR_INVALID, "%s: NULL argument", who);
  EYOC_REQUIRE(in_shape_ok(n, c) && in_inst_ok(n_inst), EYOC_ERR_INVALID, "%s: n %d, c %d (a divisor of 256, >= 4), n_inst %d (1 .. %d)", who, n,
               c, n_inst, IN_MAX_INST);
  const int q = split ? 32 : 4;                 // SPLIT16 rows: whole 32-channel blocks
  EYOC_REQUIRE(c % q == 0 && ld_x >= c && ld_y >= c && ld_x % q == 0 && ld_y % q == 0 && (!residual_dev || (ld_res >= c && ld_res % q == 0)),
               EYOC_ERR_INVALID, "%s: leading dimensions %d / %d / %d (multiples of %d, >= c = %d)", who, ld_x, ld_y, ld_res, q, c);
  EYOC_REQUIRE(aligned16(x_dev) && aligned16(y_dev) && aligned16(residual_dev) && aligned16(stats_dev) && aligned16(weight_dev) && aligned16(bias_dev),
               EYOC_ERR_INVALID, "%s: tensors must be 16-byte aligned", who);
  EYOC_REQUIRE(((uintptr_t)ws_dev & 255) == 0, EYOC_ERR_INVALID, "%s: workspace must be 256-byte aligned", who);
  EYOC_REQUIRE(ws_bytes >= eyoc_in_workspace_bytes(n, c, n_inst), EYOC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes,
               eyoc_in_workspace_bytes(n, c, n_inst));
  hipStream_t st = (hipStream_t)stream;
  const PlanView P = plan_view(plan_dev, n, n_inst);
  const InWorkspace W = in_workspace(ws_dev, n, c, n_inst);
  if (split)
    return in_forward_launch<true>(x_dev, n, c, ld_x, P, n_inst, n_inst, weight_dev, bias_dev, eps, relu, residual_dev, ld_res, y_dev, ld_y, stats_dev,
                                   W.partial, range_dev, st);
  return in_forward_launch<false>(x_dev, n, c, ld_x, P, n_inst, n_inst, weight_dev, bias_dev, eps, relu, residual_dev, ld_res, y_dev, ld_y, stats_dev,
                                  W.partial, nullptr, st);
}

int eyoc_in_forward(eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const void* plan_dev, int n_inst, const float* weight_dev,
                    const float* bias_dev, float eps, int relu, const float* residual_dev, int ld_res, float* y_dev, int ld_y,
                    float* stats_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  return in_forward_checked("eyoc_in_forward", false, ctx, x_dev, n, c, ld_x, plan_dev, n_inst, weight_dev, bias_dev, eps, relu, residual_dev, ld_res,
                            y_dev, ld_y, stats_dev, nullptr, ws_dev, ws_bytes, stream);
}

int eyoc_in_forward_split16(eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const void* plan_dev, int n_inst, const float* weight_dev,
                            const float* bias_dev, float eps, int relu, const float* residual_dev, int ld_res, float* y_dev, int ld_y,
                            float* stats_dev, unsigned int* range_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  return in_forward_checked("eyoc_in_forward_split16", true, ctx, x_dev, n, c, ld_x, plan_dev, n_inst, weight_dev, bias_dev, eps, relu, residual_dev,
                            ld_res, y_dev, ld_y, stats_dev, range_dev, ws_dev, ws_bytes, stream);
}

int eyoc_in_backward(eyoc_ctx* ctx, const float* x_dev, int ld_x, const float* y_dev, int ld_y, const float* dy_dev, int ld_dy, int n, int c,
                     const void* plan_dev, int n_inst, const float* weight_dev, const float* stats_dev, float eps, float* dx_dev, int ld_dx,
                     float* dres_dev, int ld_dres, float* dweight_dev, float* dbias_dev, void* ws_dev, size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx && x_dev && dy_dev && plan_dev && weight_dev && stats_dev && dx_dev && dweight_dev && dbias_dev && ws_dev, EYOC_ERR_INVALID,
               "eyoc_in_backward: NULL argument");
  EYOC_REQUIRE(in_shape_ok(n, c) && in_inst_ok(n_inst), EYOC_ERR_INVALID, "eyoc_in_backward: n %d, c %d (a divisor of 256, >= 4), n_inst %d (1 .. %d)", n,
               c, n_inst, IN_MAX_INST);
  EYOC_REQUIRE(ld_x >= c && ld_dy >= c && ld_dx >= c && ld_x % 4 == 0 && ld_dy % 4 == 0 && ld_dx % 4 == 0 && (!y_dev || (ld_y >= c && ld_y % 4 == 0)) &&
                   (!dres_dev || (ld_dres >= c && ld_dres % 4 == 0)),
               EYOC_ERR_INVALID, "eyoc_in_backward: leading dimensions %d / %d / %d / %d / %d (multiples of 4, >= c = %d)", ld_x, ld_y, ld_dy, ld_dx,
               ld_dres, c);
  EYOC_REQUIRE(aligned16(x_dev) && aligned16(y_dev) && aligned16(dy_dev) && aligned16(dx_dev) && aligned16(dres_dev) && aligned16(stats_dev) &&
                   aligned16(weight_dev),
               EYOC_ERR_INVALID, "eyoc_in_backward: tensors must be 16-byte aligned");
  EYOC_REQUIRE(((uintptr_t)ws_dev & 255) == 0, EYOC_ERR_INVALID, "eyoc_in_backward: workspace must be 256-byte aligned");
  EYOC_REQUIRE(ws_bytes >= eyoc_in_workspace_bytes(n, c, n_inst), EYOC_ERR_WORKSPACE, "eyoc_in_backward: workspace %zu < %zu bytes", ws_bytes,
               eyoc_in_workspace_bytes(n, c, n_inst));
  hipStream_t st = (hipStream_t)stream;
  const PlanView P = plan_view(plan_dev, n, n_inst);
  const InWorkspace W = in_workspace(ws_dev, n, c, n_inst);
  hipLaunchKernelGGL(k_in_partial<1>, dim3(in_max_chunks(n, n_inst)), dim3(256), 0, st, x_dev, ld_x, y_dev, ld_y, dy_dev, ld_dy, n, c, P, n_inst, stats_dev,
                     eps, W.partial);
  hipLaunchKernelGGL(k_in_final<1>, dim3(cdiv(c, 2), n_inst), dim3(256), 0, st, (const double*)W.partial, x_dev, ld_x, n, c, P, n_inst, (float*)nullptr,
                     W.isum);
  hipLaunchKernelGGL(k_in_param_grads, dim3(cdiv(2 * c, 256)), dim3(256), 0, st, (const double*)W.isum, n, c, P, n_inst, dweight_dev, dbias_dev);
  hipLaunchKernelGGL(k_in_backward_apply, dim3(cdiv((long long)n * (c / 4), 256)), dim3(256), 0, st, x_dev, ld_x, y_dev, ld_y, dy_dev, ld_dy, n, c, P,
                     n_inst, stats_dev, weight_dev, eps, (const double*)W.isum, dx_dev, ld_dx, dres_dev, ld_dres);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- the packed plan's side (model.hip)
// The forward knows neither how many instances a batch holds nor may it read anything back, so its plans are built for IN_MAX_INST ids
// (the maps' own batch limit: eyoc_maps_build refuses larger indices, an id outside the plan cannot occur): ids without rows cost a
// seg entry each, k_in_final walks them with IN_FINAL_ROWS workgroups per channel pair.
namespace eyoc {

constexpr int IN_FINAL_ROWS = 32;

size_t in_plan_bytes_nosync(int n) { return eyoc_in_plan_bytes(n, IN_MAX_INST); }

// eyoc_in_plan_build without its read-back: count, scan, place - the placement decides on the device whether it has anything to do
int in_plan_build_nosync(const int32_t* coords_dev, int n, void* plan_dev, hipStream_t st) {
  const PlanLayout L = plan_layout(n, IN_MAX_INST);
  int32_t* p = (int32_t*)plan_dev;
  const int blocks = cdiv(n, IN_PLAN_ROWS);
  EYOC_CHECK_HIP(hipMemsetAsync(p + L.flags, 0, 4 * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_in_plan_count, dim3(blocks), dim3(256), 0, st, coords_dev, n, IN_MAX_INST, p + L.inst, p + L.counts, p + L.flags);
  hipLaunchKernelGGL(k_in_plan_scan, dim3(1), dim3(1024), 0, st, p + L.counts, blocks, n, IN_MAX_INST, p + L.flags, p, p + L.seg, p + L.cseg);
  hipLaunchKernelGGL(k_in_plan_place, dim3(blocks), dim3(256), 0, st, p + L.inst, n, IN_MAX_INST, p + L.counts, p + L.seg, p + L.perm,
                     (const int32_t*)p);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// workspace of one instance-norm layer of the plan: the partial sums and the statistics [IN_MAX_INST][2 c]
size_t in_layer_workspace_bytes(int n, int c) {
  if (!in_shape_ok(n, c)) return 0;
  return in_workspace(nullptr, n, c, IN_MAX_INST).bytes + align_up((size_t)IN_MAX_INST * 2 * c * sizeof(float));
}

int launch_in_layer(const float* x, int ld_x, int n, int c, const void* plan, const float* weight, const float* bias, float eps, int relu,
                    const float* res, int ld_res, float* y, int ld_y, bool split, unsigned int* range, void* ws, hipStream_t st) {
  const int q = split ? 32 : 4;
  EYOC_REQUIRE(in_shape_ok(n, c) && c % q == 0 && ld_x % q == 0 && ld_y % q == 0 && (!res || ld_res % q == 0) && aligned16(x) && aligned16(y) &&
                   aligned16(res), EYOC_ERR_INVALID, "model: instance norm over %d rows of %d channels (rows of %d -> %d floats)", n, c, ld_x, ld_y);
  const PlanView P = plan_view(plan, n, IN_MAX_INST);
  const InWorkspace W = in_workspace(ws, n, c, IN_MAX_INST);
  float* stats = (float*)((char*)ws + W.bytes);
  if (split)
    return in_forward_launch<true>(x, n, c, ld_x, P, IN_MAX_INST, IN_FINAL_ROWS, weight, bias, eps, relu, res, ld_res, y, ld_y, stats, W.partial, range, st);
  return in_forward_launch<false>(x, n, c, ld_x, P, IN_MAX_INST, IN_FINAL_ROWS, weight, bias, eps, relu, res, ld_res, y, ld_y, stats, W.partial, nullptr, st);
}

}  // namespace eyoc
