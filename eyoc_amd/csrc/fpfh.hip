// FPFH descriptors for a batch of clouds (include/eyoc_hip.h, "FPFH descriptors"): Open3D's compute_fpfh_feature with a hybrid
// (radius + max_nn) search restated.  The fifth user of the cell grid of grid.h: like the normals of icp.hip section 5 a cloud is the
// target AND the query side of its own grid, d2 = (dx dx + dy dy) + dz dz in fp64 on the fp32 points, cell edge radius (1 + 2^-20).
// Per chunk of <= 64 clouds:
//   fills         status, the chunk's output rows, counts and histograms = 0 (a RANGE cloud keeps them)
//   k_fp_keys     one thread per row: target_key (RANGE for a non-finite point or a cell outside the key range), RANGE for a non-finite
//                 normal, the same key on the query side
//   build_grid
//   k_fp_search   a. 32 cell-sorted rows of one cloud per workgroup of 128 threads, FOUR lanes per row.  The row's list - the first
//                 max_nn - 1 OTHER rows inside the radius by (d2, j), which is k_nrm_search's list without the row itself (except where max_nn
//                 or more duplicates sort ahead of the row and push it out of that list: eyoc_hip.h) - sits in LDS
//                 row by row; the four lanes see every candidate together, count the entries below it (each a quarter of the list, two
//                 quad shuffles) and move the entries above it up one place from the top (each every fourth entry: all loads of a step
//                 come before its stores, and a step reads nothing a step before it wrote).  Then the workgroup copies its lists to
//                 the workspace in blocks of 64 rows, entry m of row slot l at [block][m][l]: j (int) and d2 (double), k per slot.
//   k_fp_spfh     b. one wave per block of 64 rows, lane = row: the stored list once, the pair feature of Open3D in fp64, three
//                 integer counters per neighbour in LDS (counter c of lane l at word [c * 64 + l]); one 48-byte record per row, at the
//                 row's own index: bytes 0..32 the counts, bytes 36..39 k, the rest 0 - three 16-byte loads for whoever gathers it
//   k_fp_fpfh     c. the same blocks, lane = row: the list again, the neighbour's record, W and G as 33 + 3 fp64 registers summed in
//                 list order, the row finished and rounded once; the wave's rows leave through an LDS tile as one contiguous store
//                 per row (33 or 64 floats)
// Nothing is searched twice, nothing is read back, no floating-point atomics: a row's bytes depend on its own cloud only.
// EXPERIMENTS.md "FPFH descriptors" has the reasons for the launch shape of stage a and the stage times.
#include "common.h"
#include "grid.h"

namespace eyoc {
namespace {

constexpr int FP_BLOCK = 64;        // rows per block of the stored lists = lanes of stages b and c
constexpr int FP_ROWS = 32;         // rows per workgroup of stage a
constexpr int FP_QUAD = 4;          // lanes per row of stage a
constexpr int FP_MAX_NN = 128;
constexpr int FP_BINS = 33;
constexpr int FP_REC_WORDS = 12;    // the 48-byte record

// row stride of the LDS lists in entries: the smallest value >= cap that is 4 mod 32, so that the eight rows of a 32-lane group start
// 8 dwords (doubles) / 4 dwords (ints) apart modulo the banks and the four entries a quad touches lie side by side
inline int list_stride(int cap) { return (cap + 27) / 32 * 32 + 4; }

__global__ __launch_bounds__(ICP_BLOCK) void k_fp_keys(IcpSegs s, const float* __restrict__ pts, const float* __restrict__ normals, double edge,
                                                       int* __restrict__ status, unsigned long long* __restrict__ tkey, int* __restrict__ trow,
                                                       unsigned long long* __restrict__ qkey, int* __restrict__ qrow) {
  const int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i >= s.tgt[s.n_pairs]) return;
  const int b = pair_of(s.tgt, s.n_pairs, i);
  bool ok;
  const unsigned long long key = target_key(pts, i, b, edge, false, &ok);
  trow[i] = i; qrow[i] = i;
  tkey[i] = key; qkey[i] = key;
  for (int a = 0; a < 3; ++a) ok = ok && isfinite(normals[(size_t)i * 3 + a]);
  if (!ok) atomicOr(&status[b], EYOC_ICP_RANGE);
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(FP_ROWS * FP_QUAD) void k_fp_search(IcpSegs s, const float* __restrict__ pts, const int* __restrict__ qrow_sorted,
                                                                 IcpGrid g, double edge, double r2, int cap, int stride,
                                                                 const int* __restrict__ status, int* __restrict__ lj, double* __restrict__ ld,
                                                                 int* __restrict__ kk) {
  extern __shared__ double fp_list[];     // 32 x stride doubles (d2), 32 x stride ints (j), 32 ints (entries per row)
  const int blk = blockIdx.x >> 1, half = blockIdx.x & 1;     // two workgroups per block of 64 rows
  const int b = pair_of(s.wg, s.n_pairs, blk);                // uniform: kernel arguments and the workgroup index
  if (status[b]) return;                                      // the cloud keeps its zeros
  double* const dd_all = fp_list;
  int* const jj_all = reinterpret_cast<int*>(fp_list + (size_t)FP_ROWS * stride);
  int* const nn = jj_all + (size_t)FP_ROWS * stride;
  const int r = threadIdx.x / FP_QUAD, sub = threadIdx.x % FP_QUAD;
  const int local = (blk - s.wg[b]) * FP_BLOCK + half * FP_ROWS + r;
  double* const dd = dd_all + (size_t)r * stride;
  int* const jj = jj_all + (size_t)r * stride;
  int n = 0;
  if (local < s.src[b + 1] - s.src[b]) {     // the four lanes of a row decide everything below alike: they hold the same values
    const int qi = qrow_sorted[s.src[b] + local];
    const int self = qi - s.tgt[b];
    const double x[3] = {(double)pts[(size_t)qi * 3], (double)pts[(size_t)qi * 3 + 1], (double)pts[(size_t)qi * 3 + 2]};
    int c[3];
    if (cell_of(x[0], edge, &c[0]) && cell_of(x[1], edge, &c[1]) && cell_of(x[2], edge, &c[2])) {     // (status 0: always)
      probe_cells(g, b, c, [&](const float4 q) {
        const double dx = (double)q.x - x[0], dy = (double)q.y - x[1], dz = (double)q.z - x[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (!(d < r2)) return;
        const int j = __float_as_int(q.w);
        if (j == self) return;
        if (n == cap) {                      // full: the largest leaves if the new entry is smaller
          const double dl = dd[cap - 1];
          if (!(d < dl || (d == dl && j < jj[cap - 1]))) return;
          n = cap - 1;
        }
        int pos = 0;                         // entries below (d2, j): a quarter of the list per lane; the loads of four steps together
#pragma unroll 4
        for (int m = sub; m < n; m += FP_QUAD) {
          const double dp = dd[m];
          pos += (dp < d || (dp == d && jj[m] < j)) ? 1 : 0;
        }
        pos += __shfl_xor(pos, 1);
        pos += __shfl_xor(pos, 2);
        __builtin_amdgcn_wave_barrier();
        // entries above move up one place, from the top.  The four lanes must take every step TOGETHER - a step's loads before its
        // stores, in all four - so the trip count is the quad's (top and pos are the same in its four lanes), a lane without an entry
        // in a step is predicated off inside it, and a wave barrier stands between the loads and the stores.  (With a trip count per
        // lane, an unrolled body and its remainder loop are different paths: the lanes on one stored over entries the others had not
        // loaded yet - wrong lists.)
        for (int top = n - 1; top >= pos; top -= FP_QUAD) {
          const int m = top - sub;
          const bool mine = m >= pos;
          double dp = 0.0;
          int jp = 0;
          if (mine) {
            dp = dd[m];
            jp = jj[m];
          }
          __builtin_amdgcn_wave_barrier();
          if (mine) {
            dd[m + 1] = dp;
            jj[m + 1] = jp;
          }
        }     // (the next step loads entries below everything this one stored: nothing to order between them)
        __builtin_amdgcn_wave_barrier();
        if (sub == 0) {
          dd[pos] = d;
          jj[pos] = j;
        }
        ++n;
      });
    }
  }
  if (sub == 0) nn[r] = n;
  __syncthreads();
  const size_t base = (size_t)blk * FP_BLOCK * cap + (size_t)half * FP_ROWS;
  for (int e = threadIdx.x; e < cap * FP_ROWS; e += FP_ROWS * FP_QUAD) {
    const int m = e / FP_ROWS, rr = e % FP_ROWS;
    if (m < nn[rr]) {
      lj[base + (size_t)m * FP_BLOCK + rr] = jj_all[(size_t)rr * stride + m];
      ld[base + (size_t)m * FP_BLOCK + rr] = dd_all[(size_t)rr * stride + m];
    }
  }
  if (threadIdx.x < FP_ROWS) kk[(size_t)blk * FP_BLOCK + half * FP_ROWS + threadIdx.x] = nn[threadIdx.x];
}

// bin of coordinate t (already scaled to [0, 11]): floor, clamped to 0..10; a NaN goes to 0
__device__ inline int fp_bin(double t) {
  const double f = floor(t);
  return !(f >= 0.0) ? 0 : (f >= 10.0 ? 10 : (int)f);
}

#pragma clang fp contract(off)
__device__ inline double fp_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Open3D's ComputePairFeatures, operation by operation; f = (f0, f1, f2)
#pragma clang fp contract(off)
__device__ inline void fp_pair(const double* p1, const double* n1_in, const double* p2, const double* n2_in, double* f) {
  f[0] = 0.0; f[1] = 0.0; f[2] = 0.0;
  double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double len = sqrt(fp_dot(d, d));
  if (len == 0.0) return;
  double n1[3] = {n1_in[0], n1_in[1], n1_in[2]}, n2[3] = {n2_in[0], n2_in[1], n2_in[2]};
  const double a1 = fp_dot(n1, d) / len, a2 = fp_dot(n2, d) / len;
  double f2;
  if (acos(fabs(a1)) > acos(fabs(a2))) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double t = n1[a];
      n1[a] = n2[a]; n2[a] = t;
      d[a] = -d[a];
    }
    f2 = -a2;
  } else {
    f2 = a1;
  }
  double v[3] = {d[1] * n1[2] - d[2] * n1[1], d[2] * n1[0] - d[0] * n1[2], d[0] * n1[1] - d[1] * n1[0]};
  const double vn = sqrt(fp_dot(v, v));
  if (vn == 0.0) return;
  v[0] /= vn; v[1] /= vn; v[2] /= vn;
  const double w[3] = {n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]};
  f[1] = fp_dot(v, n2);
  f[0] = atan2(fp_dot(w, n2), fp_dot(n1, n2));
  f[2] = f2;
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(FP_BLOCK) void k_fp_spfh(IcpSegs s, const float* __restrict__ pts, const float* __restrict__ normals,
                                                      const int* __restrict__ qrow_sorted, int cap, const int* __restrict__ status,
                                                      const int* __restrict__ lj, const int* __restrict__ kk, uint4* __restrict__ rec,
                                                      uint8_t* __restrict__ hist, int* __restrict__ count) {
  __shared__ unsigned int h[FP_BINS * FP_BLOCK];     // counter c of lane l at [c * 64 + l]: a lane's column is its own (one wave, no barrier)
  const int blk = blockIdx.x, lane = threadIdx.x;
  const int b = pair_of(s.wg, s.n_pairs, blk);
  if (status[b]) return;
  const int local = (blk - s.wg[b]) * FP_BLOCK + lane;
  if (local >= s.src[b + 1] - s.src[b]) return;
  const int qi = qrow_sorted[s.src[b] + local];
  const int k = kk[(size_t)blk * FP_BLOCK + lane];
  const double p1[3] = {(double)pts[(size_t)qi * 3], (double)pts[(size_t)qi * 3 + 1], (double)pts[(size_t)qi * 3 + 2]};
  const double n1[3] = {(double)normals[(size_t)qi * 3], (double)normals[(size_t)qi * 3 + 1], (double)normals[(size_t)qi * 3 + 2]};
#pragma unroll
  for (int c = 0; c < FP_BINS; ++c) h[c * FP_BLOCK + lane] = 0u;
  const int* const list = lj + (size_t)blk * FP_BLOCK * cap + lane;
  const double pi = 3.14159265358979323846;
  for (int m = 0; m < k; ++m) {
    const size_t jr = (size_t)s.tgt[b] + (size_t)list[(size_t)m * FP_BLOCK];
    const double p2[3] = {(double)pts[jr * 3], (double)pts[jr * 3 + 1], (double)pts[jr * 3 + 2]};
    const double n2[3] = {(double)normals[jr * 3], (double)normals[jr * 3 + 1], (double)normals[jr * 3 + 2]};
    double f[3];
    fp_pair(p1, n1, p2, n2, f);
    const int b0 = fp_bin(11.0 * (f[0] + pi) / (2.0 * pi));
    const int b1 = 11 + fp_bin(11.0 * (f[1] + 1.0) * 0.5);
    const int b2 = 22 + fp_bin(11.0 * (f[2] + 1.0) * 0.5);
    h[b0 * FP_BLOCK + lane] += 1u;
    h[b1 * FP_BLOCK + lane] += 1u;
    h[b2 * FP_BLOCK + lane] += 1u;
  }
  unsigned int w[FP_REC_WORDS];
#pragma unroll
  for (int i = 0; i < FP_REC_WORDS; ++i) w[i] = 0u;
#pragma unroll
  for (int c = 0; c < FP_BINS; ++c) w[c / 4] |= h[c * FP_BLOCK + lane] << (8 * (c % 4));     // a count is at most k <= 127
  w[9] = (unsigned int)k;
  uint4* const out = rec + (size_t)qi * 3;
  out[0] = make_uint4(w[0], w[1], w[2], w[3]);
  out[1] = make_uint4(w[4], w[5], w[6], w[7]);
  out[2] = make_uint4(w[8], w[9], w[10], w[11]);
  if (count) count[qi] = k;
  if (hist) {
#pragma unroll
    for (int c = 0; c < FP_BINS; ++c) hist[(size_t)qi * FP_BINS + c] = (uint8_t)((w[c / 4] >> (8 * (c % 4))) & 0xFFu);
  }
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(FP_BLOCK) void k_fp_fpfh(IcpSegs s, const int* __restrict__ qrow_sorted, int cap, const int* __restrict__ status,
                                                      const int* __restrict__ lj, const double* __restrict__ ld, const int* __restrict__ kk,
                                                      const uint4* __restrict__ rec, int normalize, int out_stride, float* __restrict__ out) {
  __shared__ float tile[FP_BLOCK * FP_BINS];     // row l at [l * 33 ...]: 33 is odd, a column is conflict-free
  __shared__ int ids[FP_BLOCK];
  const int blk = blockIdx.x, lane = threadIdx.x;
  const int b = pair_of(s.wg, s.n_pairs, blk);
  if (status[b]) return;                         // uniform
  const int local = (blk - s.wg[b]) * FP_BLOCK + lane;
  const bool live = local < s.src[b + 1] - s.src[b];
  int qi = -1;
  if (live) {
    qi = qrow_sorted[s.src[b] + local];
    const int k = kk[(size_t)blk * FP_BLOCK + lane];
    const int* const list = lj + (size_t)blk * FP_BLOCK * cap + lane;
    const double* const dist = ld + (size_t)blk * FP_BLOCK * cap + lane;
    double W[FP_BINS], G[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < FP_BINS; ++c) W[c] = 0.0;
    for (int m = 0; m < k; ++m) {
      const double d2 = dist[(size_t)m * FP_BLOCK];
      const uint4* const rj = rec + ((size_t)s.tgt[b] + (size_t)list[(size_t)m * FP_BLOCK]) * 3;
      const uint4 u0 = rj[0], u1 = rj[1], u2 = rj[2];
      if (!(d2 > 0.0)) continue;                 // a coincident point adds nothing
      const unsigned int w[9] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w, u2.x};
      const int kj = (int)u2.y;
      if (kj == 0) continue;                     // S_j = 0
      const double scale = 100.0 / (double)kj;
#pragma unroll
      for (int c = 0; c < FP_BINS; ++c) {        // neighbour by neighbour, bins ascending: the order of W and of G
        const double cnt = (double)((w[c / 4] >> (8 * (c % 4))) & 0xFFu);
        const double term = (cnt * scale) / d2;
        W[c] += term;
        G[c / 11] += term;
      }
    }
    double F[FP_BINS];
    if (k == 0) {
#pragma unroll
      for (int c = 0; c < FP_BINS; ++c) F[c] = 0.0;
    } else {
      const uint4* const ri = rec + (size_t)qi * 3;
      const uint4 u0 = ri[0], u1 = ri[1], u2 = ri[2];
      const unsigned int w[9] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w, u2.x};
      const double scale = 100.0 / (double)k;
      double inv[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) inv[a] = G[a] != 0.0 ? 100.0 / G[a] : 0.0;
#pragma unroll
      for (int c = 0; c < FP_BINS; ++c) {
        const double cnt = (double)((w[c / 4] >> (8 * (c % 4))) & 0xFFu);
        F[c] = W[c] * inv[c / 11] + cnt * scale;
      }
    }
    if (normalize) {
      double sq = 0.0;
#pragma unroll
      for (int c = 0; c < FP_BINS; ++c) sq += F[c] * F[c];
      const double den = sqrt(sq) + 1e-6;
#pragma unroll
      for (int c = 0; c < FP_BINS; ++c) F[c] = F[c] / den;
    }
#pragma unroll
    for (int c = 0; c < FP_BINS; ++c) tile[lane * FP_BINS + c] = (float)F[c];
  }
  ids[lane] = qi;
  __syncthreads();
  if (lane >= out_stride) return;
  for (int r = 0; r < FP_BLOCK; ++r) {
    const int row = ids[r];
    if (row < 0) continue;                       // uniform
    out[(size_t)row * out_stride + lane] = lane < FP_BINS ? tile[r * FP_BINS + lane] : 0.f;
  }
}

struct FpfhWorkspace {
  GridWorkspace grid;
  int *lj, *kk;
  double* ld;
  uint4* rec;
};

// row slots of the largest chunk a call with these totals can hold: every cloud's rows padded to blocks of 64
size_t fp_slots(int n_clouds, int total) { return (size_t)total + (size_t)FP_BLOCK * (n_clouds < ICP_CHUNK ? n_clouds : ICP_CHUNK); }

size_t fp_carve(void* base, size_t bytes, int n_clouds, int total, int max_nn, FpfhWorkspace* w) {
  Carver c(base, bytes);
  carve_grid(c, total, total, 1, &w->grid);
  const size_t slots = fp_slots(n_clouds, total), cap = (size_t)(max_nn - 1);
  w->lj = c.take<int>(slots * cap);
  w->ld = c.take<double>(slots * cap);
  w->kk = c.take<int>(slots);
  w->rec = c.take<uint4>((size_t)total * 3);
  return align_up(c.off);
}

// one chunk of <= ICP_CHUNK clouds; every pointer is already that of the chunk's first row / cloud
int fp_chunk(const float* pts, const float* normals, const int32_t* seg, int n_clouds, double radius, int max_nn, int normalize, int out_stride,
             float* out, uint8_t* hist, int32_t* count, int32_t* status, const FpfhWorkspace& w, hipStream_t st) {
  IcpSegs s = make_segs(seg, seg, n_clouds);
  for (int b = 0; b < n_clouds; ++b) s.wg[b + 1] = s.wg[b] + cdiv(s.src[b + 1] - s.src[b], FP_BLOCK);     // blocks of 64 rows here
  const int n = s.tgt[n_clouds], blocks = s.wg[n_clouds];
  const double edge = radius * RM_EDGE_MARGIN, r2 = radius * radius;
  const int cap = max_nn - 1, stride = list_stride(cap);
  EYOC_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)n_clouds * sizeof(int32_t), st));
  if (n == 0) return EYOC_OK;
  EYOC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)n * out_stride * sizeof(float), st));
  if (count) EYOC_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), st));
  if (hist) EYOC_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)n * FP_BINS, st));
  const GridWorkspace& gw = w.grid;
  hipLaunchKernelGGL(k_fp_keys, dim3(cdiv(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, s, pts, normals, edge, status, gw.tkey, gw.trow, gw.qkey, gw.qrow);
  IcpGrid g;
  const int rc = build_grid(s, pts, status, gw, st, &g);
  if (rc != EYOC_OK) return rc;
  const size_t lds = (size_t)FP_ROWS * stride * (sizeof(double) + sizeof(int)) + FP_ROWS * sizeof(int);     // max_nn = 128: 50 816 bytes
  hipLaunchKernelGGL(k_fp_search, dim3(2 * blocks), dim3(FP_ROWS * FP_QUAD), lds, st, s, pts, gw.qrow_sorted, g, edge, r2, cap, stride, status, w.lj,
                     w.ld, w.kk);
  hipLaunchKernelGGL(k_fp_spfh, dim3(blocks), dim3(FP_BLOCK), 0, st, s, pts, normals, gw.qrow_sorted, cap, status, w.lj, w.kk, w.rec, hist, count);
  hipLaunchKernelGGL(k_fp_fpfh, dim3(blocks), dim3(FP_BLOCK), 0, st, s, gw.qrow_sorted, cap, status, w.lj, w.ld, w.kk, w.rec, normalize, out_stride,
                     out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // namespace
}  // namespace eyoc

extern "C" size_t eyoc_fpfh_workspace_bytes(int n_clouds, int total, int max_nn) {
  if (n_clouds < 1 || total < 0 || max_nn < 2 || max_nn > eyoc::FP_MAX_NN) return 0;
  eyoc::FpfhWorkspace w;
  return eyoc::fp_carve(nullptr, 0, n_clouds, total, max_nn, &w);
}

extern "C" int eyoc_fpfh_batched(eyoc_ctx* ctx, const float* pts_dev, const float* normals_dev, const int32_t* seg_host, int n_clouds,
                                 double radius, int max_nn, int normalize, int out_stride, float* out_dev, uint8_t* hist_dev,
                                 int32_t* count_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  using namespace eyoc;
  const char* what = "eyoc_fpfh_batched";
  int bad = check_grid_head(what, ctx && seg_host && status_dev && workspace_dev, n_clouds, workspace_dev);
  if (bad != EYOC_OK) return bad;
  EYOC_REQUIRE(std::isfinite(radius) && radius > 0.0, EYOC_ERR_INVALID, "%s: radius must be positive and finite", what);
  EYOC_REQUIRE(max_nn >= 2 && max_nn <= FP_MAX_NN, EYOC_ERR_INVALID, "%s: max_nn = %d is outside [2, %d]", what, max_nn, FP_MAX_NN);
  EYOC_REQUIRE(out_stride == 33 || out_stride == 64, EYOC_ERR_INVALID, "%s: out_stride = %d is neither 33 nor 64", what, out_stride);
  bad = check_segments(what, n_clouds, {seg_host});
  if (bad != EYOC_OK) return bad;
  const int total = seg_host[n_clouds];
  EYOC_REQUIRE(total == 0 || (pts_dev && normals_dev && out_dev), EYOC_ERR_INVALID, "%s: NULL cloud, normals or output", what);
  FpfhWorkspace w;
  const size_t need = fp_carve(workspace_dev, workspace_bytes, n_clouds, total, max_nn, &w);
  EYOC_REQUIRE(workspace_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (eyoc_fpfh_workspace_bytes)", what, workspace_bytes,
               need);
  EYOC_CHECK_HIP(hipSetDevice(ctx->device));
  return for_each_chunk(n_clouds, [&](int b0, int nc) {
    const size_t o = (size_t)seg_host[b0];
    return fp_chunk(pts_dev + 3 * o, normals_dev + 3 * o, seg_host + b0, nc, radius, max_nn, normalize, out_stride,
                    out_dev + (size_t)out_stride * o, hist_dev ? hist_dev + (size_t)eyoc::FP_BINS * o : nullptr,
                    count_dev ? count_dev + o : nullptr, status_dev + b0, w, (hipStream_t)stream);
  });
}
