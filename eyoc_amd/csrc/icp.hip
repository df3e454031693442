// The cell grid over 3-D points, and its three users (include/eyoc_hip.h, "ICP refinement", eyoc_posed_nn_grid and eyoc_radius_matches_*).
//
// 1. THE GRID (grid.h, which fpfh.hip includes as well): a batch of target clouds as cells of one edge, searched by queries that look at
//   the 27 cells around their own.
//   target_key   cell key of one target row (pair << 54 | biased cell); tells the caller when the row is non-finite or outside the key range
//   2 x rocPRIM radix sort (stable, pair index in the top key bits: a pair's order never depends on its neighbours): targets and queries
//   k_icp_build  target points into sorted order (x, y, z, row local to the pair) + open-addressing table key -> (first row, count), 16 bytes per slot;
//                integer atomics only - which slot a key lands in may differ from run to run, what a lookup returns does not
//   probe_cells  the search itself: plane by plane, the 9 first probes of a plane issued together, a bounded linear probe, a run's points
//                four at a time; the caller's functor sees every candidate once, in an order that only depends on the grid
//   GridWorkspace / carve_grid / make_segs / build_grid: the arrays, the chunk's segments and the launches between a user's key kernel and its search
//                (carve_grid's `tables` > 1 + chunk_grid: one table per chunk, for the user whose grids outlive their chunk)
// 2. ICP (eyoc_icp_batched, eyoc_icp_correspondences).  One call = one grid build + (max_iteration + 1) evaluations, nothing read back in between:
//   k_icp_init   one thread per pair: T = init, BAD_INIT / empty-segment (FEW) pairs are finished here
//   k_icp_keys   one thread per target / source row: target_key, RANGE for non-finite points and target cells outside the key range; the
//                source key is the cell of the point under the initial pose
//   build_grid
//   k_icp_eval   256 sorted source rows of one pair per workgroup, lane = row: pose in fp64, probe_cells, reduce the 17 sums
//                lane -> wave -> workgroup in a fixed order, ONE partial record per workgroup (no floating-point atomics)
//   k_icp_solve  one wave per pair: partials in a fixed order (lane l takes workgroups l, l + 64, ..., then the shuffle tree), fitness / rmse, convergence, Kabsch, T = U T, done flag
// The evaluation's arithmetic is the contract's expression evaluated in fp64 without contraction (no FMA), so d2 does not depend on
// how the compiler schedules it.
// 3. POSED NEAREST NEIGHBOUR (eyoc_posed_nn_grid): k_pnn_init, k_pnn_keys, build_grid, k_pnn_search - fp32 arithmetic, see its section.
// 4. RADIUS MATCHES (eyoc_radius_matches_count / _fill): EVERY target inside the gate, fp64; a count pass, a scan and a fill pass over grids
//    that stay in the workspace between the two calls, see its section.
// 5. NORMALS (eyoc_normals_batched): the clouds are targets and queries of their own grid; every neighbour inside the radius, the first
//    max_nn by (d2, row) kept in a lane-strided list in LDS, covariance in list order, smallest eigenvector - fp64, see its section.
// 6. POINT-TO-PLANE ICP (eyoc_icp_plane_batched): section 2's kernels with PLANE = true - the same evaluation, 29 sums instead of 17,
//    a 6 x 6 LDL^T solve instead of Kabsch, see its section.
// The users differ in what they do with a candidate (the functor handed to probe_cells), in the query half of their key kernel and in
// their own arrays; everything else about the grid exists once, in grid.h.
#include <cmath>
#include <initializer_list>

#include "common.h"
#include "grid.h"
#include "pose_math.h"

namespace eyoc {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// 2. ICP: the queries are the source rows under the pair's current pose, fp64
// ---------------------------------------------------------------------------------------------------------------------
constexpr int ICP_SUMS = 17;       // count, sum d2, sum p (3), sum q (3), sum p q^T (9)
constexpr int PLANE_SUMS = 29;     // point-to-plane (section 6): count, sum d2, sum J J^T (upper triangle, 21), sum J r (6)

__global__ void k_icp_init(IcpSegs s, const double* __restrict__ init, eyoc_icp_result* __restrict__ res, int* __restrict__ done) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= s.n_pairs) return;
  eyoc_icp_result r;
  bool finite = true;
  for (int k = 0; k < 16; ++k) {
    r.T[k] = init ? init[(size_t)b * 16 + k] : (k % 5 == 0 ? 1.0 : 0.0);
    finite = finite && isfinite(r.T[k]);
  }
  r.fitness = 0.0; r.inlier_rmse = 0.0;
  r.correspondences = 0; r.iterations = 0; r.reserved = 0;
  r.status = 0;
  if (!finite) r.status = EYOC_ICP_BAD_INIT;
  else if (s.src[b + 1] == s.src[b] || s.tgt[b + 1] == s.tgt[b]) r.status = EYOC_ICP_FEW;
  res[b] = r;
  done[b] = r.status != 0;
}

// PLANE (section 6): the target rows also carry a normal - checked here (a non-finite one is RANGE), stored once as 16 bytes in the
// target's own row order so that the evaluation reads the winner's normal with one load
template <bool PLANE>
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_keys(IcpSegs s, const float* __restrict__ src, const float* __restrict__ tgt, double edge,
                                                        eyoc_icp_result* __restrict__ res, int* __restrict__ done,
                                                        unsigned long long* __restrict__ tkey, int* __restrict__ trow,
                                                        unsigned long long* __restrict__ skey, int* __restrict__ srow,
                                                        int32_t* __restrict__ corr, double* __restrict__ d2,
                                                        const float* __restrict__ nrm, float4* __restrict__ nrm4) {
  const int n_tgt = s.tgt[s.n_pairs], n_src = s.src[s.n_pairs];
  int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i < n_tgt) {
    const int b = pair_of(s.tgt, s.n_pairs, i);
    bool ok;
    trow[i] = i;
    const bool bad_init = res[b].status & EYOC_ICP_BAD_INIT;
    tkey[i] = target_key(tgt, i, b, edge, bad_init, &ok);
    if constexpr (PLANE) {
      float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!bad_init) {
        n4 = make_float4(nrm[(size_t)i * 3], nrm[(size_t)i * 3 + 1], nrm[(size_t)i * 3 + 2], 0.f);
        ok = ok && isfinite(n4.x) && isfinite(n4.y) && isfinite(n4.z);
      }
      nrm4[i] = n4;
    }
    if (!ok) { atomicOr(&res[b].status, EYOC_ICP_RANGE); done[b] = 1; }
    return;
  }
  i -= n_tgt;
  if (i >= n_src) return;
  const int b = pair_of(s.src, s.n_pairs, i);
  srow[i] = i;
  if (corr) corr[i] = -1;
  if (d2) d2[i] = INFINITY;
  unsigned long long key = pack_key(b, -COORD_BIAS, -COORD_BIAS, -COORD_BIAS);
  if (!(res[b].status & EYOC_ICP_BAD_INIT)) {       // a pair with a bad init has nothing else read
    const double x = src[(size_t)i * 3], y = src[(size_t)i * 3 + 1], z = src[(size_t)i * 3 + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
      atomicOr(&res[b].status, EYOC_ICP_RANGE);
      done[b] = 1;
    } else {
      // the order of the source rows only decides which lanes share a wave: a posed point outside the key range keeps the lowest key
      const double* T = res[b].T;
      int c[3];
      bool ok = true;
      for (int k = 0; k < 3; ++k) ok = ok && cell_of(T[4 * k] * x + T[4 * k + 1] * y + T[4 * k + 2] * z + T[4 * k + 3], edge, &c[k]);
      if (ok) key = pack_key(b, c[0], c[1], c[2]);
    }
  }
  skey[i] = key;
}

#pragma clang fp contract(off)
// PLANE (section 6): the search and the outputs are the same; what a correspondence adds to the sums differs
template <bool PLANE>
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_eval(IcpSegs s, const float* __restrict__ src, const int* __restrict__ srow_sorted, IcpGrid g,
                                                        double edge, double r2, const eyoc_icp_result* __restrict__ res,
                                                        const int* __restrict__ done, double* __restrict__ partial,
                                                        int32_t* __restrict__ corr, double* __restrict__ d2_out,
                                                        const float4* __restrict__ nrm4) {
  constexpr int ICP_SUMS = PLANE ? PLANE_SUMS : eyoc::ICP_SUMS;     // (shadows the file's constant: the lines below are the point-to-point kernel's own)
  __shared__ int sb;
  __shared__ double red[ICP_BLOCK / 64][ICP_SUMS];
  if (threadIdx.x == 0) sb = pair_of(s.wg, s.n_pairs, blockIdx.x);
  __syncthreads();
  const int b = sb;
  if (done[b]) return;                                   // uniform per workgroup
  const int local = (blockIdx.x - s.wg[b]) * ICP_BLOCK + threadIdx.x;   // counted from the pair's own first row
  const bool live = local < s.src[b + 1] - s.src[b];
  double v[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) v[k] = 0.0;
  if (live) {
    const int row = srow_sorted[s.src[b] + local];
    const double* T = res[b].T;
    const double x = src[(size_t)row * 3], y = src[(size_t)row * 3 + 1], z = src[(size_t)row * 3 + 2];
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = T[4 * k] * x + T[4 * k + 1] * y + T[4 * k + 2] * z + T[4 * k + 3];
    int c[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && cell_of(p[k], edge, &c[k]);
    double best = INFINITY;
    int best_row = -1;
    float4 best_q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok)
      probe_cells(g, b, c, [&](const float4 q) {
        const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
        const double d = dx * dx + dy * dy + dz * dz;
        const int qrow = __float_as_int(q.w);
        if (d < best || (d == best && qrow < best_row)) { best = d; best_row = qrow; best_q = q; }
      });
    const bool hit = best_row >= 0 && best < r2;
    if (corr) corr[row] = hit ? best_row : -1;
    if (d2_out) d2_out[row] = hit ? best : INFINITY;
    if (hit) {
      const double q[3] = {(double)best_q.x, (double)best_q.y, (double)best_q.z};
      v[0] = 1.0; v[1] = best;
      if constexpr (PLANE) {
        // r = (p - q) . n, J = (p x n, n): A = J J^T (upper triangle, row by row), g = J r
        const float4 nf = nrm4[s.tgt[b] + best_row];
        const double n[3] = {(double)nf.x, (double)nf.y, (double)nf.z};
        const double r = ((p[0] - q[0]) * n[0] + (p[1] - q[1]) * n[1]) + (p[2] - q[2]) * n[2];
        const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
        int at = 2;
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
          for (int l = k; l < 6; ++l) v[at++] = J[k] * J[l];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[23 + k] = J[k] * r;
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          v[2 + k] = p[k]; v[5 + k] = q[k];
#pragma unroll
          for (int l = 0; l < 3; ++l) v[8 + 3 * k + l] = p[k] * q[l];
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) {
    const double w = wave_sum(v[k]);
    if (lane == 0) red[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < ICP_SUMS) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < ICP_BLOCK / 64; ++w) t += red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * ICP_SUMS + threadIdx.x] = t;
  }
}

// The point-to-plane step (section 6): A xi = -g from the sums S[2 .. 22] (upper triangle of A, row by row) and S[23 .. 28] (g), by
// LDL^T without pivoting.  false: a pivot d_k is not above 2^-30 A_kk (A_kk before elimination - a scale-free test per variable; a NaN
// pivot fails it too), xi is then meaningless.  Every loop has constant bounds: the 6 x 6 arrays stay in registers.
__device__ inline bool plane_step(const double* S, double* xi) {
  double A[6][6], L[6][6], d[6], y[6];
  int at = 2;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int l = k; l < 6; ++l) A[k][l] = S[at++];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double dk = A[k][k];
#pragma unroll
    for (int m = 0; m < k; ++m) dk -= L[k][m] * L[k][m] * d[m];
    ok = ok && dk > 0x1p-30 * A[k][k];
    d[k] = dk;
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      double v = A[k][i];
#pragma unroll
      for (int m = 0; m < k; ++m) v -= L[i][m] * L[k][m] * d[m];
      L[i][k] = v / dk;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {           // L y = -g
    y[k] = -S[23 + k];
#pragma unroll
    for (int m = 0; m < k; ++m) y[k] -= L[k][m] * y[m];
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {          // L^T xi = D^-1 y
    xi[k] = y[k] / d[k];
#pragma unroll
    for (int m = k + 1; m < 6; ++m) xi[k] -= L[m][k] * xi[m];
  }
  return ok;
}

// evaluation `e` (0 = the one under the initial pose) of every pair that is still running
template <bool PLANE>
__global__ __launch_bounds__(64) void k_icp_solve(IcpSegs s, const double* __restrict__ partial, eyoc_icp_result* __restrict__ res,
                                                  int* __restrict__ done, int e, int max_iteration, double rel_fitness, double rel_rmse) {
  constexpr int ICP_SUMS = PLANE ? PLANE_SUMS : eyoc::ICP_SUMS;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (done[b]) return;
  // a fixed order that only depends on the pair's own workgroup count: lane l adds workgroups l, l + 64, ... in that order, then the
  // wave's shuffle tree adds the lanes
  double S[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) S[k] = 0.0;
  for (int w = s.wg[b] + lane; w < s.wg[b + 1]; w += 64)
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k) S[k] += partial[(size_t)w * ICP_SUMS + k];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; ++k) S[k] = wave_sum(S[k]);
  if (lane != 0) return;
  eyoc_icp_result& r = res[b];
  const double n = S[0];
  const double fitness = n / (double)(s.src[b + 1] - s.src[b]);
  const double rmse = n > 0.0 ? sqrt(S[1] / n) : 0.0;
  const bool converged = e > 0 && fabs(r.fitness - fitness) < rel_fitness && fabs(r.inlier_rmse - rmse) < rel_rmse;
  r.fitness = fitness; r.inlier_rmse = rmse;
  r.correspondences = (int)n; r.iterations = e;
  int status = r.status;
  if (converged) status |= EYOC_ICP_CONVERGED;
  if (n < 3.0) status |= EYOC_ICP_FEW;
  r.status = status;
  if (converged || n < 3.0 || e >= max_iteration) { done[b] = 1; return; }
  double R[3][3], t[3], Tn[12];
  if constexpr (PLANE) {
    double xi[6];
    if (!plane_step(S, xi)) {       // a direction the correspondences do not constrain: the pair stops with its current T
      r.status = status | EYOC_ICP_SINGULAR;
      done[b] = 1;
      return;
    }
    const double sa = sin(xi[0]), ca = cos(xi[0]), sb = sin(xi[1]), cb = cos(xi[1]), sg = sin(xi[2]), cg = cos(xi[2]);
    R[0][0] = cb * cg; R[0][1] = sa * sb * cg - ca * sg; R[0][2] = ca * sb * cg + sa * sg;       // Rz(gamma) Ry(beta) Rx(alpha)
    R[1][0] = cb * sg; R[1][1] = sa * sb * sg + ca * cg; R[1][2] = ca * sb * sg - sa * cg;
    R[2][0] = -sb;     R[2][1] = sa * cb;                R[2][2] = ca * cb;
    for (int k = 0; k < 3; ++k) t[k] = xi[3 + k];
  } else {
    double cp[3], cq[3], H[3][3];
    for (int k = 0; k < 3; ++k) { cp[k] = S[2 + k] / n; cq[k] = S[5 + k] / n; }
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) H[k][l] = S[8 + 3 * k + l] - n * cp[k] * cq[l];
    kabsch_rotation(H, R);
    for (int k = 0; k < 3; ++k) t[k] = cq[k] - (R[k][0] * cp[0] + R[k][1] * cp[1] + R[k][2] * cp[2]);
  }
  for (int k = 0; k < 3; ++k) {
    for (int l = 0; l < 4; ++l) Tn[4 * k + l] = R[k][0] * r.T[l] + R[k][1] * r.T[4 + l] + R[k][2] * r.T[8 + l];
    Tn[4 * k + 3] += t[k];
  }
  for (int k = 0; k < 12; ++k) r.T[k] = Tn[k];
}

struct IcpWorkspace {
  GridWorkspace grid;
  int* done;
  double* partial;
  float4* nrm4;      // point-to-plane only: the target normals, 16 bytes per row
};

size_t carve(void* base, size_t bytes, int n_pairs, int total_src, int total_tgt, IcpWorkspace* w, bool plane = false) {
  Carver c(base, bytes);
  const int chunk = n_pairs < ICP_CHUNK ? n_pairs : ICP_CHUNK;
  carve_grid(c, total_src, total_tgt, 1, &w->grid);
  w->done = c.take<int>(chunk > 0 ? chunk : 1);
  w->partial = c.take<double>(((size_t)cdiv(total_src, ICP_BLOCK) + chunk + 1) * (plane ? PLANE_SUMS : ICP_SUMS));
  w->nrm4 = plane ? c.take<float4>(total_tgt) : nullptr;
  return align_up(c.off);
}

// one chunk of <= ICP_CHUNK pairs; every pointer is already that of the chunk's first row
template <bool PLANE>
int run_chunk(const float* src, const float* tgt, const float* nrm, const int32_t* seg_src, const int32_t* seg_tgt, int n_pairs, const double* init,
              const eyoc_icp_params& p, eyoc_icp_result* res, int32_t* corr, double* d2, const IcpWorkspace& w, hipStream_t st) {
  const IcpSegs s = make_segs(seg_src, seg_tgt, n_pairs);
  const int n_src = s.src[n_pairs], n_tgt = s.tgt[n_pairs], n_wg = s.wg[n_pairs];
  const double edge = p.max_distance, r2 = p.max_distance * p.max_distance;
  hipLaunchKernelGGL(k_icp_init, dim3(cdiv(n_pairs, 64)), dim3(64), 0, st, s, init, res, w.done);
  if (n_src + n_tgt > 0)
    hipLaunchKernelGGL(k_icp_keys<PLANE>, dim3(cdiv((long long)n_src + n_tgt, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, s, src, tgt, edge, res, w.done,
                       w.grid.tkey, w.grid.trow, w.grid.qkey, w.grid.qrow, corr, d2, nrm, w.nrm4);
  if (n_src == 0 || n_tgt == 0) {       // every pair has an empty segment: k_icp_init finished them all
    EYOC_CHECK_HIP(hipGetLastError());
    return EYOC_OK;
  }
  IcpGrid g;
  const int rc = build_grid(s, tgt, w.done, w.grid, st, &g);
  if (rc != EYOC_OK) return rc;
  for (int e = 0; e <= p.max_iteration; ++e) {
    hipLaunchKernelGGL(k_icp_eval<PLANE>, dim3(n_wg), dim3(ICP_BLOCK), 0, st, s, src, w.grid.qrow_sorted, g, edge, r2, res, w.done, w.partial, corr,
                       d2, w.nrm4);
    hipLaunchKernelGGL(k_icp_solve<PLANE>, dim3(n_pairs), dim3(64), 0, st, s, w.partial, res, w.done, e, p.max_iteration, p.relative_fitness,
                       p.relative_rmse);
  }
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// `plane`: eyoc_icp_plane_batched (section 6), `nrm` its target normals; the point-to-point entry points pass false / nullptr
int run(const char* what, eyoc_ctx* ctx, const float* src, const float* tgt, const int32_t* seg_src, const int32_t* seg_tgt, int n_pairs,
        const double* init, const eyoc_icp_params& p, eyoc_icp_result* res, int32_t* corr, double* d2, void* ws, size_t ws_bytes, void* stream,
        bool plane = false, const float* nrm = nullptr) {
  int bad = check_grid_head(what, ctx && seg_src && seg_tgt && res && ws, n_pairs, ws);
  if (bad != EYOC_OK) return bad;
  EYOC_REQUIRE(std::isfinite(p.max_distance) && p.max_distance > 0.0, EYOC_ERR_INVALID, "%s: max_distance must be positive and finite", what);
  EYOC_REQUIRE(p.max_iteration >= 0 && p.max_iteration <= 100000, EYOC_ERR_INVALID, "%s: max_iteration = %d is outside [0, 100000]", what,
               p.max_iteration);
  bad = check_segments(what, n_pairs, {seg_src, seg_tgt});
  if (bad != EYOC_OK) return bad;
  EYOC_REQUIRE((seg_src[n_pairs] == 0 || src) && (seg_tgt[n_pairs] == 0 || tgt), EYOC_ERR_INVALID, "%s: NULL cloud", what);
  EYOC_REQUIRE(!plane || seg_tgt[n_pairs] == 0 || nrm, EYOC_ERR_INVALID, "%s: NULL target normals", what);
  IcpWorkspace w;
  const size_t need = carve(ws, ws_bytes, n_pairs, seg_src[n_pairs], seg_tgt[n_pairs], &w, plane);
  EYOC_REQUIRE(ws_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (%s)", what, ws_bytes, need,
               plane ? "eyoc_icp_plane_workspace_bytes" : "eyoc_icp_workspace_bytes");
  EYOC_CHECK_HIP(hipSetDevice(ctx->device));
  return for_each_chunk(n_pairs, [&](int b0, int np) {
    const size_t so = (size_t)seg_src[b0], to = (size_t)seg_tgt[b0];
    const float* s0 = src ? src + 3 * so : nullptr;
    const float* t0 = tgt ? tgt + 3 * to : nullptr;
    const double* i0 = init ? init + 16 * (size_t)b0 : nullptr;
    IcpWorkspace wc = w;
    if (plane) {
      wc.nrm4 += to;
      return run_chunk<true>(s0, t0, nrm ? nrm + 3 * to : nullptr, seg_src + b0, seg_tgt + b0, np, i0, p, res + b0, corr ? corr + so : nullptr,
                             d2 ? d2 + so : nullptr, wc, (hipStream_t)stream);
    }
    return run_chunk<false>(s0, t0, nullptr, seg_src + b0, seg_tgt + b0, np, i0, p, res + b0, corr ? corr + so : nullptr,
                            d2 ? d2 + so : nullptr, wc, (hipStream_t)stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. Posed nearest neighbour with a gate (eyoc_posed_nn_grid): what eyoc_knn2(c = 4) + the 2 m gate of lib/trainer.py:1198-1211 return,
// without the [n0, n1] sweep.  The second user of the grid of section 1: the queries are selected source rows under the pair's pose, and
// the arithmetic is fp32, the brute-force kernel's:  p_r = ((T0 x + T1 y) + T2 z) + T3,  d2 = (dx dx + dy dy) + dz dz,  no contraction.
//   k_pnn_init    one thread per pair: BAD_INIT for a non-finite pose
//   k_pnn_keys    targets: target_key; queries: bounds of the selected row, the posed point (stored once, 16 bytes, so the search and the
//                 key see the same point), its cell key, outputs preset to -1 / +inf
//   build_grid
//   k_pnn_search  256 cell-sorted queries of one pair per workgroup, lane = query: probe_cells, minimum over (d2, row), gate
//
// Cell edge.  The gate is sqrtf(d2) < r in fp32 (u = 2^-24, sqrtf correctly rounded).  A target that passes it has, per axis, with
// dxf = fl(p - q) = (p - q)(1 + e), |e| <= u:  fl(dxf dxf) >= dxf^2 (1 - u) and the two additions of non-negative terms lose at most a
// factor (1 - u) each, so d2 >= dxf^2 (1 - u)^3 (a square that underflows belongs to a |p - q| < 2^-63: inside any cell edge); the gate
// gives sqrt(d2) < r / (1 - u), hence |p - q| <= |dxf| / (1 - u) < r (1 - u)^-3.5 < r (1 + 4 u).  The cells are floor(v / edge) of the
// exact fp32 values in fp64: the two rounded quotients are each within 2^-53 * 2^17 = 2^-36 of the true ones (|cell| < 2^17), so they
// differ by at most |p - q| / edge + 2^-35, and two floors differ by at most 1 when that is <= 1.  edge = r (1 + 2^-20) = r (1 + 16 u)
// leaves |p - q| / edge < (1 + 4 u) / (1 + 16 u) < 1 - 11 u, and 11 u > 2^-35 (+ one rounding of edge itself, 2^-53): every target that
// passes the fp32 gate lies in the 27 cells around the query's.  The global minimum over (d2, row), when it passes the gate, is therefore
// among the candidates, together with every row that ties with it; when it does not pass, nothing does.
constexpr double PNN_EDGE_MARGIN = 1.0 + 1.0 / 1048576.0;

struct PnnSrc { int base[ICP_CHUNK + 1]; };   // first source row of every pair of the chunk (IcpSegs::src holds the QUERY segments)

__global__ void k_pnn_init(int n_pairs, const float* __restrict__ T, int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_pairs) return;
  bool finite = true;
  for (int k = 0; k < 16; ++k) finite = finite && isfinite(T[(size_t)b * 16 + k]);
  status[b] = finite ? 0 : EYOC_ICP_BAD_INIT;
}

__global__ __launch_bounds__(ICP_BLOCK) void k_pnn_keys(IcpSegs s, PnnSrc sb, const float* __restrict__ src, const float* __restrict__ tgt,
                                                        const float* __restrict__ Ts, const long long* __restrict__ sel, double edge,
                                                        int* __restrict__ status, unsigned long long* __restrict__ tkey, int* __restrict__ trow,
                                                        unsigned long long* __restrict__ qkey, int* __restrict__ qrow, float4* __restrict__ qpts,
                                                        long long* __restrict__ idx_out, float* __restrict__ d2_out) {
#pragma clang fp contract(off)
  const int n_tgt = s.tgt[s.n_pairs], n_q = s.src[s.n_pairs];
  int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i < n_tgt) {
    const int b = pair_of(s.tgt, s.n_pairs, i);
    bool ok;
    trow[i] = i;
    tkey[i] = target_key(tgt, i, b, edge, status[b] & EYOC_ICP_BAD_INIT, &ok);
    if (!ok) atomicOr(&status[b], EYOC_ICP_RANGE);
    return;
  }
  i -= n_tgt;
  if (i >= n_q) return;
  const int b = pair_of(s.src, s.n_pairs, i);
  qrow[i] = i;
  idx_out[i] = -1;
  if (d2_out) d2_out[i] = INFINITY;
  unsigned long long key = pack_key(b, -COORD_BIAS, -COORD_BIAS, -COORD_BIAS);
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!(status[b] & EYOC_ICP_BAD_INIT)) {
    const long long local = sel ? sel[i] : (long long)(i - s.src[b]);
    bool ok = local >= 0 && local < (long long)(sb.base[b + 1] - sb.base[b]);      // a selection outside the segment is never read
    if (ok) {
      const float* a = src + 3 * ((size_t)sb.base[b] + (size_t)local);
      const float x = a[0], y = a[1], z = a[2];
      const float* T = Ts + 16 * (size_t)b;
      p.x = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
      p.y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
      p.z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
      int c[3];
      ok = isfinite(x) && isfinite(y) && isfinite(z);
      ok = ok && cell_of((double)p.x, edge, &c[0]) && cell_of((double)p.y, edge, &c[1]) && cell_of((double)p.z, edge, &c[2]);
      if (ok) key = pack_key(b, c[0], c[1], c[2]);
    }
    if (!ok) atomicOr(&status[b], EYOC_ICP_RANGE);
  }
  qpts[i] = p;
  qkey[i] = key;
}

__global__ __launch_bounds__(ICP_BLOCK) void k_pnn_search(IcpSegs s, const int* __restrict__ qrow_sorted, const float4* __restrict__ qpts, IcpGrid g,
                                                          double edge, float max_dist, const int* __restrict__ status,
                                                          long long* __restrict__ idx_out, float* __restrict__ d2_out) {
#pragma clang fp contract(off)
  const int b = pair_of(s.wg, s.n_pairs, blockIdx.x);     // uniform: kernel arguments and the workgroup index
  if (status[b]) return;                                  // every output of the pair stays -1
  const int local = (blockIdx.x - s.wg[b]) * ICP_BLOCK + threadIdx.x;
  if (local >= s.src[b + 1] - s.src[b]) return;           // no barrier below
  const int qi = qrow_sorted[s.src[b] + local];
  const float4 p = qpts[qi];
  int c[3];
  if (!(cell_of((double)p.x, edge, &c[0]) && cell_of((double)p.y, edge, &c[1]) && cell_of((double)p.z, edge, &c[2]))) return;   // (status 0: never)
  float best = INFINITY;
  int best_row = -1;
  // d2 = (dx dx + dy dy) + dz dz with x and y as an explicit pair: they are the low half of a 16-byte load, an aligned register pair
  // for the packed subtract and multiply.  Left to itself the compiler pairs y with z, which costs a move per run of points wherever
  // the register allocator does not happen to place the load on an odd register (EXPERIMENTS.md "One cell grid in icp.hip").
  typedef float pair_t __attribute__((ext_vector_type(2)));
  const pair_t pxy = {p.x, p.y};
  probe_cells(g, b, c, [&](const float4 q) {
    const pair_t qxy = {q.x, q.y};
    pair_t dxy = pxy - qxy;
    dxy *= dxy;
    const float dz = p.z - q.z;
    const float d = (dxy.x + dxy.y) + dz * dz;
    const int qrow = __float_as_int(q.w);
    if (d < best || (d == best && qrow < best_row)) { best = d; best_row = qrow; }
  });
  const bool hit = best_row >= 0 && sqrtf(best) < max_dist;
  idx_out[qi] = hit ? best_row : -1;
  if (d2_out) d2_out[qi] = hit ? best : INFINITY;
}

struct PnnWorkspace {
  GridWorkspace grid;
  float4* qpts;
};

size_t pnn_carve(void* base, size_t bytes, int total_q, int total_tgt, PnnWorkspace* w) {
  Carver c(base, bytes);
  carve_grid(c, total_q, total_tgt, 1, &w->grid);
  w->qpts = c.take<float4>(total_q);
  return align_up(c.off);
}

// one chunk of <= ICP_CHUNK pairs; every pointer is already that of the chunk's first row / query / pair
int pnn_chunk(const float* src, const float* tgt, const int32_t* seg_src, const int32_t* seg_tgt, const int32_t* seg_q, int n_pairs,
              const float* T, float max_dist, const int64_t* sel, int64_t* idx_out, float* d2_out, int32_t* status, const PnnWorkspace& w,
              hipStream_t st) {
  const IcpSegs s = make_segs(seg_q, seg_tgt, n_pairs);
  PnnSrc sb;
  for (int b = 0; b <= n_pairs; ++b) sb.base[b] = seg_src[b] - seg_src[0];
  const int n_q = s.src[n_pairs], n_tgt = s.tgt[n_pairs], n_wg = s.wg[n_pairs];
  const double edge = (double)max_dist * PNN_EDGE_MARGIN;
  hipLaunchKernelGGL(k_pnn_init, dim3(cdiv(n_pairs, 64)), dim3(64), 0, st, n_pairs, T, status);
  if (n_q + n_tgt > 0)
    hipLaunchKernelGGL(k_pnn_keys, dim3(cdiv((long long)n_q + n_tgt, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, s, sb, src, tgt, T, (const long long*)sel,
                       edge, status, w.grid.tkey, w.grid.trow, w.grid.qkey, w.grid.qrow, w.qpts, (long long*)idx_out, d2_out);
  if (n_q == 0 || n_tgt == 0) {        // nothing to search: every output is already -1
    EYOC_CHECK_HIP(hipGetLastError());
    return EYOC_OK;
  }
  IcpGrid g;
  const int rc = build_grid(s, tgt, status, w.grid, st, &g);
  if (rc != EYOC_OK) return rc;
  hipLaunchKernelGGL(k_pnn_search, dim3(n_wg), dim3(ICP_BLOCK), 0, st, s, w.grid.qrow_sorted, w.qpts, g, edge, max_dist, status,
                     (long long*)idx_out, d2_out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// 4. Radius matches (eyoc_radius_matches_count / eyoc_radius_matches_fill): util/pointcloud.py:53-66 for a batch of pairs - for every
// source row under the pair's pose EVERY target row with d2 < radius^2, as (i, j), ascending by (d2, j) inside a source row, cut to the
// first K.  The third user of the grid of section 1; fp64 like ICP, the posed point evaluated as eyoc_posed_nn_grid writes it.
//   k_rm_init    one thread per pair: BAD_INIT for a non-finite pose
//   k_rm_keys    targets: target_key; sources: the posed point in fp64, stored as three doubles (the count, the fill and the key see the
//                same point), its cell key, the row's count preset to 0.  RANGE is set here
//   build_grid
//   k_rm_count   256 cell-sorted source rows of one pair per workgroup, lane = row: probe_cells, count d2 < r2, min(count, K) at the
//                row's ORIGINAL index
//   exclusive 64-bit scan over all source rows of the call (rocPRIM, integers): offsets, offsets[total_src] = total
//   k_rm_fill    the same traversal; the lane owns pairs_out / d2_out [offsets[i], offsets[i + 1]) and inserts every match at its
//                place by (d2, j) - d2_out is the key's storage, nothing of size `total` lives in the workspace
// The output length depends on the data, so the host reads the total between the two calls and every chunk's grid has to survive
// until the fill: the row arrays of the workspace are the call's totals, a chunk uses its own rows, and the tables of the chunks sit
// behind one another (chunk_grid).
//
// Cell edge.  (i, j) is a match iff d2 < r2, r2 = fl(r r) <= r^2 (1 + u), u = 2^-53, everything fp64.  The posed point p is a stored
// fp64 value and q an fp32 one, exact in fp64; per axis dxf = fl(p - q) = (p - q)(1 + e), |e| <= u, fl(dxf dxf) >= dxf^2 (1 - u), and
// the two additions of non-negative terms lose at most a factor (1 - u) each: d2 >= dxf^2 (1 - u)^3 (a square that underflows belongs
// to a |p - q| < 2^-500: inside any cell edge that passes the r2 > 0 a match needs).  A match therefore has |p - q| <= |dxf| / (1 - u)
// < r (1 + u)^0.5 (1 - u)^-2.5 < r (1 + 4 u) on every axis.  The cells are floor(fl(v / edge)): with |cell| < 2^17 each rounded quotient
// is within 2^17 * 2^-53 = 2^-36 of the true one, so the two quotients differ by at most |p - q| / edge + 2^-35, and two floors differ by
// at most 1 when that is <= 1.  edge = fl(r (1 + 2^-20)) >= r (1 + 2^-20)(1 - u) leaves |p - q| / edge < (1 + 4 u) / ((1 + 2^-20)(1 - u))
// < 1 - 2^-21, and 2^-21 > 2^-35: every match lies in the 27 cells around the source's, with no exception at a cell face (the ICP grid,
// edge = r, has one).  So the matches found are exactly those of the n0 x n1 sweep.
// RM_EDGE_MARGIN = 1 + 2^-20 itself stands in grid.h: sections 4 and 5 and fpfh.hip form their cell edge with it.

__global__ void k_rm_init(int n_pairs, const double* __restrict__ T, int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_pairs) return;
  bool finite = true;
  if (T)
    for (int k = 0; k < 16; ++k) finite = finite && isfinite(T[(size_t)b * 16 + k]);
  status[b] = finite ? 0 : EYOC_ICP_BAD_INIT;
}

__global__ __launch_bounds__(ICP_BLOCK) void k_rm_keys(IcpSegs s, const float* __restrict__ src, const float* __restrict__ tgt,
                                                       const double* __restrict__ Ts, double edge, int* __restrict__ status,
                                                       unsigned long long* __restrict__ tkey, int* __restrict__ trow,
                                                       unsigned long long* __restrict__ qkey, int* __restrict__ qrow, double* __restrict__ qpts,
                                                       long long* __restrict__ counts) {
#pragma clang fp contract(off)
  const int n_tgt = s.tgt[s.n_pairs], n_q = s.src[s.n_pairs];
  int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i < n_tgt) {
    const int b = pair_of(s.tgt, s.n_pairs, i);
    bool ok;
    trow[i] = i;
    tkey[i] = target_key(tgt, i, b, edge, status[b] & EYOC_ICP_BAD_INIT, &ok);
    if (!ok) atomicOr(&status[b], EYOC_ICP_RANGE);
    return;
  }
  i -= n_tgt;
  if (i >= n_q) return;
  const int b = pair_of(s.src, s.n_pairs, i);
  qrow[i] = i;
  counts[i] = 0;
  unsigned long long key = pack_key(b, -COORD_BIAS, -COORD_BIAS, -COORD_BIAS);
  double p[3] = {0.0, 0.0, 0.0};
  if (!(status[b] & EYOC_ICP_BAD_INIT)) {
    const float xf = src[(size_t)i * 3], yf = src[(size_t)i * 3 + 1], zf = src[(size_t)i * 3 + 2];
    const double x = xf, y = yf, z = zf;
    bool ok = isfinite(xf) && isfinite(yf) && isfinite(zf);
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double t[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) t[l] = Ts ? Ts[(size_t)b * 16 + 4 * k + l] : (k == l ? 1.0 : 0.0);     // NULL: the identity
      p[k] = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
      ok = ok && cell_of(p[k], edge, &c[k]);
    }
    if (ok) key = pack_key(b, c[0], c[1], c[2]);
    else atomicOr(&status[b], EYOC_ICP_RANGE);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) qpts[(size_t)i * 3 + k] = p[k];
  qkey[i] = key;
}

// what count and fill share: the workgroup's pair and the lane's source row (sorted by cell), its stored posed point and its cell.
// false: nothing to do for this lane (a pair with a status, a lane past the pair's rows).  No barrier anywhere in the two kernels.
__device__ __forceinline__ bool rm_query(const IcpSegs& s, const int* __restrict__ qrow_sorted, const double* __restrict__ qpts, double edge,
                                         const int* __restrict__ status, int* b, int* qi, double* p, int* c) {
  *b = pair_of(s.wg, s.n_pairs, blockIdx.x);     // uniform: kernel arguments and the workgroup index
  if (status[*b]) return false;
  const int local = (blockIdx.x - s.wg[*b]) * ICP_BLOCK + threadIdx.x;
  if (local >= s.src[*b + 1] - s.src[*b]) return false;
  *qi = qrow_sorted[s.src[*b] + local];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = qpts[(size_t)*qi * 3 + k];
    ok = ok && cell_of(p[k], edge, &c[k]);
  }
  return ok;     // (status 0: always)
}

__global__ __launch_bounds__(ICP_BLOCK) void k_rm_count(IcpSegs s, const int* __restrict__ qrow_sorted, const double* __restrict__ qpts, IcpGrid g,
                                                        double edge, double r2, int max_per_source, const int* __restrict__ status,
                                                        long long* __restrict__ counts) {
#pragma clang fp contract(off)
  int b, qi, c[3];
  double p[3];
  if (!rm_query(s, qrow_sorted, qpts, edge, status, &b, &qi, p, c)) return;
  int n = 0;     // at most the pair's target rows
  probe_cells(g, b, c, [&](const float4 q) {
    const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
    const double d = (dx * dx + dy * dy) + dz * dz;
    n += d < r2;
  });
  counts[qi] = max_per_source > 0 && n > max_per_source ? max_per_source : n;
}

// offsets: the scan, counted like `counts` from the chunk's first source row.  The lane's slice is [offsets[qi], offsets[qi + 1]); a
// slice that does not lie inside [0, total) is not written (a `total` that is not the scan's, a workspace touched since the count).
__global__ __launch_bounds__(ICP_BLOCK) void k_rm_fill(IcpSegs s, const int* __restrict__ qrow_sorted, const double* __restrict__ qpts, IcpGrid g,
                                                       double edge, double r2, const int* __restrict__ status,
                                                       const long long* __restrict__ offsets, long long total, long long* pairs_out,
                                                       double* d2_out) {
#pragma clang fp contract(off)
  int b, qi, c[3];
  double p[3];
  if (!rm_query(s, qrow_sorted, qpts, edge, status, &b, &qi, p, c)) return;
  const long long lo = offsets[qi], hi = offsets[qi + 1];
  if (lo < 0 || hi <= lo || hi > total) return;
  const long long len = hi - lo, i_local = qi - s.src[b];
  long long* const jj = pairs_out + 2 * lo + 1;     // the slice's j column (stride 2)
  double* const dd = d2_out + lo;
  for (long long k = 0; k < len; ++k) pairs_out[2 * (lo + k)] = i_local;
  long long n = 0;
  probe_cells(g, b, c, [&](const float4 q) {
    const double dx = p[0] - (double)q.x, dy = p[1] - (double)q.y, dz = p[2] - (double)q.z;
    const double d = (dx * dx + dy * dy) + dz * dz;
    if (!(d < r2)) return;
    const long long j = __float_as_int(q.w);
    long long pos;
    if (n < len) pos = n++;
    else {                              // full (the slice is the first K of the list): the largest leaves if the new match is smaller
      pos = len - 1;
      const double dl = dd[pos];
      if (!(d < dl || (d == dl && j < jj[2 * pos]))) return;
    }
    for (; pos > 0; --pos) {            // entries above (d2, j) move up one place
      const double dp = dd[pos - 1];
      const long long jp = jj[2 * (pos - 1)];
      if (dp < d || (dp == d && jp < j)) break;
      dd[pos] = dp;
      jj[2 * pos] = jp;
    }
    dd[pos] = d;
    jj[2 * pos] = j;
  });
}

struct RmWorkspace {
  GridWorkspace grid;     // row arrays: the call's totals; cells: every chunk's table, behind one another
  double* qpts;           // the posed source points, 3 doubles per row
  void* scan_tmp;
  size_t scan_bytes;
};

size_t rm_carve(void* base, size_t bytes, int n_pairs, int total_src, int total_tgt, RmWorkspace* w) {
  Carver c(base, bytes);
  carve_grid(c, total_src, total_tgt, cdiv(n_pairs, ICP_CHUNK), &w->grid);
  w->qpts = c.take<double>((size_t)total_src * 3);
  w->scan_bytes = scan_offsets64_tmp_bytes(total_src + 1);
  w->scan_tmp = c.take<char>(w->scan_bytes);
  return align_up(c.off);
}

// the grid arrays of one chunk inside a workspace carved for several tables: its own rows of the row arrays (the chunk's first source
// / target row: so / to), its table `cell0` slots into `cells`, sized for its own targets
GridWorkspace chunk_grid(const GridWorkspace& w, size_t so, size_t to, size_t cell0, int n_tgt) {
  GridWorkspace v = w;
  v.tkey += to; v.tkey_sorted += to; v.trow += to; v.trow_sorted += to; v.pts += to;
  v.qkey += so; v.qkey_sorted += so; v.qrow += so; v.qrow_sorted += so;
  v.cells += cell0;
  v.cap = table_capacity(n_tgt);
  return v;
}

// one chunk of <= ICP_CHUNK pairs; every pointer is already that of the chunk's first row / pair, `gw` the chunk's own grid arrays
int rm_count_chunk(const float* src, const float* tgt, const IcpSegs& s, const double* T, double radius, int max_per_source,
                   long long* counts, int32_t* status, const GridWorkspace& gw, double* qpts, hipStream_t st) {
  const int n_src = s.src[s.n_pairs], n_tgt = s.tgt[s.n_pairs], n_wg = s.wg[s.n_pairs];
  const double edge = radius * RM_EDGE_MARGIN, r2 = radius * radius;
  hipLaunchKernelGGL(k_rm_init, dim3(cdiv(s.n_pairs, 64)), dim3(64), 0, st, s.n_pairs, T, status);
  if (n_src + n_tgt > 0)
    hipLaunchKernelGGL(k_rm_keys, dim3(cdiv((long long)n_src + n_tgt, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, s, src, tgt, T, edge, status, gw.tkey,
                       gw.trow, gw.qkey, gw.qrow, qpts, counts);
  if (n_src == 0 || n_tgt == 0) {        // nothing to search: every count is already 0
    EYOC_CHECK_HIP(hipGetLastError());
    return EYOC_OK;
  }
  IcpGrid g;
  const int rc = build_grid(s, tgt, status, gw, st, &g);
  if (rc != EYOC_OK) return rc;
  hipLaunchKernelGGL(k_rm_count, dim3(n_wg), dim3(ICP_BLOCK), 0, st, s, gw.qrow_sorted, qpts, g, edge, r2, max_per_source, status, counts);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int rm_fill_chunk(const IcpSegs& s, double radius, const long long* offsets, long long total, const int32_t* status, long long* pairs_out,
                  double* d2_out, const GridWorkspace& gw, const double* qpts, hipStream_t st) {
  if (s.src[s.n_pairs] == 0 || s.tgt[s.n_pairs] == 0) return EYOC_OK;     // the count built no grid for this chunk
  const IcpGrid g{gw.cells, gw.cap - 1, gw.pts};
  hipLaunchKernelGGL(k_rm_fill, dim3(s.wg[s.n_pairs]), dim3(ICP_BLOCK), 0, st, s, gw.qrow_sorted, qpts, g, radius * RM_EDGE_MARGIN, radius * radius,
                     status, offsets, total, pairs_out, d2_out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// both entry points: fill = false is the count (total, pairs_out and d2_out unused)
int rm_run(const char* what, bool fill, eyoc_ctx* ctx, const float* src, const float* tgt, const int32_t* seg_src, const int32_t* seg_tgt, int n_pairs,
           const double* T, double radius, int max_per_source, int64_t* offsets, int32_t* status, int64_t total, int64_t* pairs_out,
           double* d2_out, void* ws, size_t ws_bytes, void* stream) {
  int bad = check_grid_head(what, ctx && seg_src && seg_tgt && offsets && status && ws, n_pairs, ws);
  if (bad != EYOC_OK) return bad;
  EYOC_REQUIRE(std::isfinite(radius) && radius > 0.0, EYOC_ERR_INVALID, "%s: radius must be positive and finite", what);
  EYOC_REQUIRE(max_per_source >= 0, EYOC_ERR_INVALID, "%s: max_per_source = %d is negative (0 = all)", what, max_per_source);
  bad = check_segments(what, n_pairs, {seg_src, seg_tgt});
  if (bad != EYOC_OK) return bad;
  const int total_src = seg_src[n_pairs], total_tgt = seg_tgt[n_pairs];
  EYOC_REQUIRE((total_src == 0 || src) && (total_tgt == 0 || tgt), EYOC_ERR_INVALID, "%s: NULL cloud", what);
  if (fill) {
    EYOC_REQUIRE(total >= 0, EYOC_ERR_INVALID, "%s: total = %lld is negative", what, (long long)total);
    EYOC_REQUIRE(total == 0 || (pairs_out && d2_out), EYOC_ERR_INVALID, "%s: NULL output for %lld matches", what, (long long)total);
  }
  RmWorkspace w;
  const size_t need = rm_carve(ws, ws_bytes, n_pairs, total_src, total_tgt, &w);
  EYOC_REQUIRE(ws_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (eyoc_radius_matches_workspace_bytes)", what, ws_bytes, need);
  EYOC_CHECK_HIP(hipSetDevice(ctx->device));
  if (fill && total == 0) return EYOC_OK;
  hipStream_t st = (hipStream_t)stream;
  size_t cell0 = 0;
  const int rc = for_each_chunk(n_pairs, [&](int b0, int np) {
    const size_t so = (size_t)seg_src[b0], to = (size_t)seg_tgt[b0];
    const IcpSegs s = make_segs(seg_src + b0, seg_tgt + b0, np);
    const GridWorkspace gw = chunk_grid(w.grid, so, to, cell0, s.tgt[np]);
    cell0 += gw.cap;
    if (fill)
      return rm_fill_chunk(s, radius, (const long long*)offsets + so, total, status + b0, (long long*)pairs_out, d2_out, gw, w.qpts + 3 * so, st);
    return rm_count_chunk(src ? src + 3 * so : nullptr, tgt ? tgt + 3 * to : nullptr, s, T ? T + 16 * (size_t)b0 : nullptr, radius, max_per_source,
                          (long long*)offsets + so, status + b0, gw, w.qpts + 3 * so, st);
  });
  if (rc != EYOC_OK || fill) return rc;
  EYOC_CHECK_HIP(hipMemsetAsync(offsets + total_src, 0, sizeof(int64_t), st));
  return scan_offsets64(w.scan_tmp, w.scan_bytes, (long long*)offsets, total_src + 1, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// 5. Normals (eyoc_normals_batched): Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) restated for a batch of clouds.
// The fourth user of the grid of section 1: a cloud is the target AND the query side of its own grid, the query's point is the row
// itself (fp32, exact in fp64), so d = x_j - x_i is ONE rounding per axis and d2 = (dx dx + dy dy) + dz dz as in section 4.
//   status = 0   one fill per chunk
//   k_nrm_keys   one thread per row: target_key (RANGE for a non-finite point or a cell outside the key range), the same key on the
//                query side, normal and count preset to 0
//   build_grid
//   k_nrm_search 64 cell-sorted rows of one cloud per workgroup (ONE wave: nothing is shared, no barrier), lane = row.  The lane keeps
//                the first `cap` neighbours by (d2, j) in a list in LDS, inserted as in k_rm_fill: entry m of lane l is d2 at double
//                [m * 64 + l] and j at int [m * 64 + l] behind the doubles - consecutive lanes on consecutive banks, 12 bytes per entry,
//                cap * 768 bytes per workgroup, asked for at the launch (max_nn = 30: 22.5 KiB, 64: 48 KiB).  Then the offsets of the
//                list's rows are read again in list order for S1 and S2.  max_nn = 0 (all neighbours): cap = 64 and further passes,
//                each keeping the next 64 entries above the last one of the pass before, until a pass saw no more than 64.
// Cell edge: fl(radius (1 + 2^-20)), section 4's derivation with p = x_i exact - the neighbours found are exactly those of the n x n sweep.
// The sums are added in list order by one lane: a row's normal does not depend on the launch, on the slot placement or on another cloud.
constexpr int NRM_BLOCK = 64;
constexpr int NRM_MAX_NN = 64;

__global__ __launch_bounds__(ICP_BLOCK) void k_nrm_keys(IcpSegs s, const float* __restrict__ pts, double edge, int* __restrict__ status,
                                                        unsigned long long* __restrict__ tkey, int* __restrict__ trow,
                                                        unsigned long long* __restrict__ qkey, int* __restrict__ qrow,
                                                        float* __restrict__ normals, int* __restrict__ count) {
  const int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i >= s.tgt[s.n_pairs]) return;
  const int b = pair_of(s.tgt, s.n_pairs, i);
  bool ok;
  const unsigned long long key = target_key(pts, i, b, edge, false, &ok);
  trow[i] = i; qrow[i] = i;
  tkey[i] = key; qkey[i] = key;
  if (!ok) atomicOr(&status[b], EYOC_ICP_RANGE);
  normals[(size_t)i * 3] = 0.f; normals[(size_t)i * 3 + 1] = 0.f; normals[(size_t)i * 3 + 2] = 0.f;
  if (count) count[i] = 0;
}

__global__ __launch_bounds__(NRM_BLOCK) void k_nrm_search(IcpSegs s, const float* __restrict__ pts, const int* __restrict__ qrow_sorted, IcpGrid g,
                                                          double edge, double r2, int max_nn, int cap, const int* __restrict__ status,
                                                          float* __restrict__ normals, int* __restrict__ count) {
  extern __shared__ double nrm_list[];     // cap x 64 doubles (d2), then cap x 64 ints (j)
  const int b = pair_of(s.wg, s.n_pairs, blockIdx.x);     // uniform: kernel arguments and the workgroup index
  if (status[b]) return;                                  // the cloud keeps its zeros
  const int local = (blockIdx.x - s.wg[b]) * NRM_BLOCK + threadIdx.x;
  if (local >= s.src[b + 1] - s.src[b]) return;           // no barrier below
  double* const dd = nrm_list + threadIdx.x;
  int* const jj = reinterpret_cast<int*>(nrm_list + (size_t)cap * NRM_BLOCK) + threadIdx.x;
  const int qi = qrow_sorted[s.src[b] + local];
  const double x[3] = {(double)pts[(size_t)qi * 3], (double)pts[(size_t)qi * 3 + 1], (double)pts[(size_t)qi * 3 + 2]};
  int c[3];
  if (!(cell_of(x[0], edge, &c[0]) && cell_of(x[1], edge, &c[1]) && cell_of(x[2], edge, &c[2]))) return;   // (status 0: never)
  double S1[3] = {0.0, 0.0, 0.0}, S2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // S2: xx, xy, xz, yy, yz, zz
  double last_d = -1.0;      // a pass takes the entries above (last_d, last_j); every d2 is >= 0
  int last_j = -1, k = 0;
  for (;;) {
    int n = 0, above = 0;
    probe_cells(g, b, c, [&](const float4 q) {
      const double dx = (double)q.x - x[0], dy = (double)q.y - x[1], dz = (double)q.z - x[2];
      const double d = (dx * dx + dy * dy) + dz * dz;
      if (!(d < r2)) return;
      const int j = __float_as_int(q.w);
      if (!(d > last_d || (d == last_d && j > last_j))) return;
      ++above;
      int pos;
      if (n < cap) pos = n++;
      else {                              // full: the largest leaves if the new entry is smaller
        pos = cap - 1;
        const double dl = dd[pos * NRM_BLOCK];
        if (!(d < dl || (d == dl && j < jj[pos * NRM_BLOCK]))) return;
      }
      for (; pos > 0; --pos) {            // entries above (d2, j) move up one place
        const double dp = dd[(pos - 1) * NRM_BLOCK];
        const int jp = jj[(pos - 1) * NRM_BLOCK];
        if (dp < d || (dp == d && jp < j)) break;
        dd[pos * NRM_BLOCK] = dp;
        jj[pos * NRM_BLOCK] = jp;
      }
      dd[pos * NRM_BLOCK] = d;
      jj[pos * NRM_BLOCK] = j;
    });
    for (int m = 0; m < n; ++m) {
      const float* q = pts + 3 * ((size_t)s.tgt[b] + (size_t)jj[m * NRM_BLOCK]);
      const double d[3] = {(double)q[0] - x[0], (double)q[1] - x[1], (double)q[2] - x[2]};
      S1[0] += d[0]; S1[1] += d[1]; S1[2] += d[2];
      S2[0] += d[0] * d[0]; S2[1] += d[0] * d[1]; S2[2] += d[0] * d[2];
      S2[3] += d[1] * d[1]; S2[4] += d[1] * d[2]; S2[5] += d[2] * d[2];
    }
    k += n;
    if (max_nn > 0 || above <= cap) break;
    last_d = dd[(n - 1) * NRM_BLOCK];
    last_j = jj[(n - 1) * NRM_BLOCK];
  }
  if (count) count[qi] = k;
  if (k < 3) return;                       // the zero vector
  const double kk = (double)k, m[3] = {S1[0] / kk, S1[1] / kk, S1[2] / kk};
  double C[3][3], w[3], v[3][3];
  C[0][0] = S2[0] / kk - m[0] * m[0]; C[0][1] = S2[1] / kk - m[0] * m[1]; C[0][2] = S2[2] / kk - m[0] * m[2];
  C[1][1] = S2[3] / kk - m[1] * m[1]; C[1][2] = S2[4] / kk - m[1] * m[2]; C[2][2] = S2[5] / kk - m[2] * m[2];
  C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
  jacobi_eig3(C, w, v);
  double nv[3] = {v[2][0], v[2][1], v[2][2]};     // the smallest eigenvalue's vector
  const double len = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
  const double dot = (nv[0] * x[0] + nv[1] * x[1]) + nv[2] * x[2];
  const double first = nv[0] != 0.0 ? nv[0] : (nv[1] != 0.0 ? nv[1] : nv[2]);
  const double sign = dot > 0.0 || (dot == 0.0 && first < 0.0) ? -1.0 : 1.0;       // towards the origin; undecided: first component positive
#pragma unroll
  for (int a = 0; a < 3; ++a) normals[(size_t)qi * 3 + a] = (float)(sign * (nv[a] / len));
}

size_t nrm_carve(void* base, size_t bytes, int total, GridWorkspace* w) {
  Carver c(base, bytes);
  carve_grid(c, total, total, 1, w);
  return align_up(c.off);
}

// one chunk of <= ICP_CHUNK clouds; every pointer is already that of the chunk's first row / cloud
int nrm_chunk(const float* pts, const int32_t* seg, int n_clouds, double radius, int max_nn, float* normals, int32_t* count, int32_t* status,
              const GridWorkspace& w, hipStream_t st) {
  IcpSegs s = make_segs(seg, seg, n_clouds);
  for (int b = 0; b < n_clouds; ++b) s.wg[b + 1] = s.wg[b] + cdiv(s.src[b + 1] - s.src[b], NRM_BLOCK);     // 64 rows per workgroup here
  const int n = s.tgt[n_clouds];
  const double edge = radius * RM_EDGE_MARGIN, r2 = radius * radius;
  const int cap = max_nn > 0 ? max_nn : NRM_MAX_NN;
  EYOC_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)n_clouds * sizeof(int32_t), st));
  if (n == 0) return EYOC_OK;
  hipLaunchKernelGGL(k_nrm_keys, dim3(cdiv(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, s, pts, edge, status, w.tkey, w.trow, w.qkey, w.qrow, normals,
                     count);
  IcpGrid g;
  const int rc = build_grid(s, pts, status, w, st, &g);
  if (rc != EYOC_OK) return rc;
  hipLaunchKernelGGL(k_nrm_search, dim3(s.wg[n_clouds]), dim3(NRM_BLOCK), (size_t)cap * NRM_BLOCK * (sizeof(double) + sizeof(int)), st, s, pts,
                     w.qrow_sorted, g, edge, r2, max_nn, cap, status, normals, count);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// 6. Point-to-plane ICP (eyoc_icp_plane_batched): section 2 with PLANE = true.  The evaluation - search, gate, fitness, rmse, FEW,
// convergence - is k_icp_eval's own code; a correspondence (p, q, n) adds r = (p - q) . n and J = (p x n, n) to A = sum J J^T and
// g = sum J r instead of the Kabsch moments, reduced in the same fixed order; k_icp_solve solves A xi = -g (plane_step: LDL^T, a small
// pivot is SINGULAR) and applies U = [Rz Ry Rx | t].  A target without a usable normal (the zero vector of section 5) adds zeros.
// ---------------------------------------------------------------------------------------------------------------------

}  // namespace
}  // namespace eyoc

extern "C" size_t eyoc_icp_workspace_bytes(int n_pairs, int total_src, int total_tgt) {
  if (n_pairs < 1 || total_src < 0 || total_tgt < 0) return 0;
  eyoc::IcpWorkspace w;
  return eyoc::carve(nullptr, 0, n_pairs, total_src, total_tgt, &w);
}

extern "C" int eyoc_icp_batched(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                                const int32_t* seg_tgt_host, int n_pairs, const double* init_dev, const eyoc_icp_params* params,
                                eyoc_icp_result* results_dev, int32_t* corr_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  EYOC_REQUIRE(params, EYOC_ERR_INVALID, "eyoc_icp_batched: NULL params");
  EYOC_REQUIRE(std::isfinite(params->relative_fitness) && std::isfinite(params->relative_rmse), EYOC_ERR_INVALID,
               "eyoc_icp_batched: the convergence thresholds must be finite");
  return eyoc::run("eyoc_icp_batched", ctx, src_dev, tgt_dev, seg_src_host, seg_tgt_host, n_pairs, init_dev, *params, results_dev, corr_dev,
                   nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" int eyoc_icp_correspondences(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                                        const int32_t* seg_tgt_host, int n_pairs, const double* T_dev, double max_distance, int32_t* corr_dev,
                                        double* d2_dev, eyoc_icp_result* results_dev, void* workspace_dev, size_t workspace_bytes,
                                        void* stream) {
  eyoc_icp_params p;
  p.max_distance = max_distance;
  p.relative_fitness = p.relative_rmse = 0.0;
  p.max_iteration = 0;
  p.flags = 0;
  return eyoc::run("eyoc_icp_correspondences", ctx, src_dev, tgt_dev, seg_src_host, seg_tgt_host, n_pairs, T_dev, p, results_dev, corr_dev,
                   d2_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" size_t eyoc_posed_nn_grid_workspace_bytes(int n_pairs, int total_queries, int total_tgt) {
  if (n_pairs < 1 || total_queries < 0 || total_tgt < 0) return 0;
  eyoc::PnnWorkspace w;
  return eyoc::pnn_carve(nullptr, 0, total_queries, total_tgt, &w);
}

extern "C" int eyoc_posed_nn_grid(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                                  const int32_t* seg_tgt_host, int n_pairs, const float* T_dev, float max_dist, const int64_t* sel_dev,
                                  const int32_t* seg_sel_host, int64_t* idx_out_dev, float* d2_out_dev, int32_t* status_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream) {
  using namespace eyoc;
  const char* what = "eyoc_posed_nn_grid";
  int bad = check_grid_head(what, ctx && seg_src_host && seg_tgt_host && T_dev && status_dev && workspace_dev, n_pairs, workspace_dev);
  if (bad != EYOC_OK) return bad;
  EYOC_REQUIRE(std::isfinite(max_dist) && max_dist > 0.0f, EYOC_ERR_INVALID, "%s: max_dist must be positive and finite", what);
  EYOC_REQUIRE((sel_dev == nullptr) == (seg_sel_host == nullptr), EYOC_ERR_INVALID, "%s: a selection needs its segments (and the other way round)", what);
  const int32_t* seg_q = seg_sel_host ? seg_sel_host : seg_src_host;
  bad = check_segments(what, n_pairs, {seg_src_host, seg_tgt_host, seg_q});
  if (bad != EYOC_OK) return bad;
  const int total_q = seg_q[n_pairs];
  EYOC_REQUIRE((seg_src_host[n_pairs] == 0 || src_dev) && (seg_tgt_host[n_pairs] == 0 || tgt_dev) && (total_q == 0 || idx_out_dev), EYOC_ERR_INVALID,
               "%s: NULL cloud or output", what);
  EYOC_REQUIRE(total_q == 0 || seg_src_host[n_pairs] > 0, EYOC_ERR_INVALID, "%s: queries without source rows", what);
  PnnWorkspace w;
  const size_t need = pnn_carve(workspace_dev, workspace_bytes, total_q, seg_tgt_host[n_pairs], &w);
  EYOC_REQUIRE(workspace_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (eyoc_posed_nn_grid_workspace_bytes)", what, workspace_bytes,
               need);
  EYOC_CHECK_HIP(hipSetDevice(ctx->device));
  return for_each_chunk(n_pairs, [&](int b0, int np) {
    const size_t so = (size_t)seg_src_host[b0], to = (size_t)seg_tgt_host[b0], qo = (size_t)seg_q[b0];
    return pnn_chunk(src_dev ? src_dev + 3 * so : nullptr, tgt_dev ? tgt_dev + 3 * to : nullptr, seg_src_host + b0, seg_tgt_host + b0, seg_q + b0, np,
                     T_dev + 16 * (size_t)b0, max_dist, sel_dev ? sel_dev + qo : nullptr, idx_out_dev ? idx_out_dev + qo : nullptr,
                     d2_out_dev ? d2_out_dev + qo : nullptr, status_dev + b0, w, (hipStream_t)stream);
  });
}

extern "C" size_t eyoc_radius_matches_workspace_bytes(int n_pairs, int total_src, int total_tgt) {
  if (n_pairs < 1 || total_src < 0 || total_tgt < 0) return 0;
  eyoc::RmWorkspace w;
  return eyoc::rm_carve(nullptr, 0, n_pairs, total_src, total_tgt, &w);
}

extern "C" int eyoc_radius_matches_count(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                                         const int32_t* seg_tgt_host, int n_pairs, const double* T_dev, double radius, int max_per_source,
                                         int64_t* offsets_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return eyoc::rm_run("eyoc_radius_matches_count", false, ctx, src_dev, tgt_dev, seg_src_host, seg_tgt_host, n_pairs, T_dev, radius, max_per_source,
                      offsets_dev, status_dev, 0, nullptr, nullptr, workspace_dev, workspace_bytes, stream);
}

extern "C" int eyoc_radius_matches_fill(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                                        const int32_t* seg_tgt_host, int n_pairs, const double* T_dev, double radius, int max_per_source,
                                        const int64_t* offsets_dev, const int32_t* status_dev, int64_t total, int64_t* pairs_out_dev,
                                        double* d2_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return eyoc::rm_run("eyoc_radius_matches_fill", true, ctx, src_dev, tgt_dev, seg_src_host, seg_tgt_host, n_pairs, T_dev, radius, max_per_source,
                      const_cast<int64_t*>(offsets_dev), const_cast<int32_t*>(status_dev), total, pairs_out_dev, d2_out_dev, workspace_dev,
                      workspace_bytes, stream);
}

extern "C" size_t eyoc_normals_workspace_bytes(int n_clouds, int total) {
  if (n_clouds < 1 || total < 0) return 0;
  eyoc::GridWorkspace w;
  return eyoc::nrm_carve(nullptr, 0, total, &w);
}

extern "C" int eyoc_normals_batched(eyoc_ctx* ctx, const float* pts_dev, const int32_t* seg_host, int n_clouds, double radius, int max_nn,
                                    float* normals_dev, int32_t* count_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                                    void* stream) {
  using namespace eyoc;
  const char* what = "eyoc_normals_batched";
  int bad = check_grid_head(what, ctx && seg_host && status_dev && workspace_dev, n_clouds, workspace_dev);
  if (bad != EYOC_OK) return bad;
  EYOC_REQUIRE(std::isfinite(radius) && radius > 0.0, EYOC_ERR_INVALID, "%s: radius must be positive and finite", what);
  EYOC_REQUIRE(max_nn >= 0 && max_nn <= NRM_MAX_NN, EYOC_ERR_INVALID, "%s: max_nn = %d is outside [0, %d] (0 = all)", what, max_nn, NRM_MAX_NN);
  bad = check_segments(what, n_clouds, {seg_host});
  if (bad != EYOC_OK) return bad;
  const int total = seg_host[n_clouds];
  EYOC_REQUIRE(total == 0 || (pts_dev && normals_dev), EYOC_ERR_INVALID, "%s: NULL cloud or output", what);
  GridWorkspace w;
  const size_t need = nrm_carve(workspace_dev, workspace_bytes, total, &w);
  EYOC_REQUIRE(workspace_bytes >= need, EYOC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (eyoc_normals_workspace_bytes)", what, workspace_bytes,
               need);
  EYOC_CHECK_HIP(hipSetDevice(ctx->device));
  return for_each_chunk(n_clouds, [&](int b0, int nc) {
    const size_t o = (size_t)seg_host[b0];
    return nrm_chunk(pts_dev ? pts_dev + 3 * o : nullptr, seg_host + b0, nc, radius, max_nn, normals_dev ? normals_dev + 3 * o : nullptr,
                     count_dev ? count_dev + o : nullptr, status_dev + b0, w, (hipStream_t)stream);
  });
}

extern "C" size_t eyoc_icp_plane_workspace_bytes(int n_pairs, int total_src, int total_tgt) {
  if (n_pairs < 1 || total_src < 0 || total_tgt < 0) return 0;
  eyoc::IcpWorkspace w;
  return eyoc::carve(nullptr, 0, n_pairs, total_src, total_tgt, &w, true);
}

extern "C" int eyoc_icp_plane_batched(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const float* tgt_normals_dev,
                                      const int32_t* seg_src_host, const int32_t* seg_tgt_host, int n_pairs, const double* init_dev,
                                      const eyoc_icp_params* params, eyoc_icp_result* results_dev, int32_t* corr_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream) {
  EYOC_REQUIRE(params, EYOC_ERR_INVALID, "eyoc_icp_plane_batched: NULL params");
  EYOC_REQUIRE(std::isfinite(params->relative_fitness) && std::isfinite(params->relative_rmse), EYOC_ERR_INVALID,
               "eyoc_icp_plane_batched: the convergence thresholds must be finite");
  return eyoc::run("eyoc_icp_plane_batched", ctx, src_dev, tgt_dev, seg_src_host, seg_tgt_host, n_pairs, init_dev, *params, results_dev, corr_dev,
                   nullptr, workspace_dev, workspace_bytes, stream, true, tgt_normals_dev);
}
