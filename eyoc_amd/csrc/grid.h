// The cell grid over 3-D points that icp.hip (sections 2 to 6) and fpfh.hip search: section 1 of icp.hip's head comment describes the
// pieces.  Everything here has internal linkage (an unnamed namespace per translation unit): a file that includes it gets its own
// k_icp_build and its own host helpers, compiled from this one text.
#pragma once
#include <cmath>
#include <initializer_list>

#include "common.h"

namespace eyoc {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// 1. The grid
// ---------------------------------------------------------------------------------------------------------------------
constexpr int ICP_BLOCK = 256;
constexpr int ICP_CHUNK = 64;      // pairs per set of launches: their segments travel as kernel arguments
constexpr double CELL_LIMIT = 131072.0;   // |cell| < 2^17 (COORD_BIAS)

struct IcpSegs {
  int n_pairs;
  int src[ICP_CHUNK + 1], tgt[ICP_CHUNK + 1];     // query (ICP: source) and target segments, counted from the chunk's first row
  int wg[ICP_CHUNK + 1];     // first search workgroup of every pair (ICP_BLOCK queries each)
};

__device__ inline int pair_of(const int* seg, int n_pairs, int row) {   // seg ascending, row < seg[n_pairs]
  int b = 0;
  while (b + 1 < n_pairs && seg[b + 1] <= row) ++b;
  return b;
}

// cell of one fp64 coordinate: false when it is not finite or outside the key range (nothing is cast then)
__device__ inline bool cell_of(double v, double edge, int* c) {
  const double f = floor(v / edge);
  if (!(f >= -CELL_LIMIT && f < CELL_LIMIT)) return false;   // NaN fails both comparisons
  *c = (int)f;
  return true;
}

// key of target row i of pair b.  *ok = false: the row is not finite or its cell is outside the key range (the caller flags the pair; the
// key is then the pair's lowest, like every row's of a pair whose pose is bad: nothing of such a pair is read)
__device__ inline unsigned long long target_key(const float* __restrict__ tgt, int i, int b, double edge, bool bad_init, bool* ok) {
  *ok = true;
  if (!bad_init) {
    int c[3];
    for (int k = 0; k < 3; ++k) {
      const float v = tgt[(size_t)i * 3 + k];
      *ok = *ok && isfinite(v) && cell_of((double)v, edge, &c[k]);
    }
    if (*ok) return pack_key(b, c[0], c[1], c[2]);
  }
  return pack_key(b, -COORD_BIAS, -COORD_BIAS, -COORD_BIAS);
}

// one slot of the open-addressing table: 16 bytes, so that a probe is ONE load.  The table is filled with 0xFF bytes: key = KEY_EMPTY
// and more = -1, i.e. the slot's run holds more + 1 rows starting at sorted row first.
struct __align__(16) IcpCell {
  unsigned long long key;
  int first, more;
};

struct IcpGrid {
  const IcpCell* cells;
  unsigned int mask;
  const float4* pts;     // sorted target points: x, y, z, row local to the pair (int bits)
};

__device__ inline IcpCell load_cell(const IcpCell* cells, unsigned int slot) {
  const uint4 v = *reinterpret_cast<const uint4*>(cells + slot);
  IcpCell c;
  c.key = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
  c.first = (int)v.z; c.more = (int)v.w;
  return c;
}

// `skip[b]` != 0: pair b is never searched (and a RANGE pair's keys mean nothing)
__global__ __launch_bounds__(ICP_BLOCK) void k_icp_build(IcpSegs s, const float* __restrict__ tgt, const unsigned long long* __restrict__ key_sorted,
                                                         const int* __restrict__ row_sorted, const int* __restrict__ skip, float4* __restrict__ pts,
                                                         IcpCell* __restrict__ cells, unsigned int mask) {
  const int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i >= s.tgt[s.n_pairs]) return;
  const unsigned long long key = key_sorted[i];
  const int b = (int)(key >> 54), row = row_sorted[i];
  pts[i] = make_float4(tgt[(size_t)row * 3], tgt[(size_t)row * 3 + 1], tgt[(size_t)row * 3 + 2], __int_as_float(row - s.tgt[b]));
  if (skip[b]) return;
  unsigned int slot = hash_key(key) & mask;
  for (unsigned int probes = 0; probes <= mask; ++probes) {     // bounded: capacity >= 2 x rows
    const unsigned long long seen = atomicCAS(&cells[slot].key, KEY_EMPTY, key);
    if (seen == KEY_EMPTY || seen == key) {
      atomicAdd(&cells[slot].more, 1);
      if (i == 0 || key_sorted[i - 1] != key) cells[slot].first = i;
      return;
    }
    slot = (slot + 1) & mask;
  }
}

// The search: every target point in the 27 cells around cell c of pair b goes to each(q) once (q = x, y, z, local row bits), plane by
// plane (ox), cell by cell (o), in run order.  What a candidate means - the distance expression, the minimum - is the caller's; so is
// the floating-point mode, which the functor takes from the kernel it is written in.  Grid and functor arrive by value: through a
// reference to the kernel argument the callers compile to longer code (EXPERIMENTS.md "One cell grid in icp.hip").
template <typename Each>
__device__ __forceinline__ void probe_cells(const IcpGrid g, const int b, const int* c, Each each) {
  for (int ox = -1; ox <= 1; ++ox) {
    // the first probes of a plane's 9 cells are independent loads: issued together, then resolved one by one
    unsigned long long key[9];
    unsigned int slot[9];
    IcpCell cell[9];
    const int cx = c[0] + ox;
#pragma unroll
    for (int o = 0; o < 9; ++o) {
      const int cy = c[1] + o / 3 - 1, cz = c[2] + o % 3 - 1;
      const bool inside = cx >= -COORD_BIAS && cx < COORD_BIAS && cy >= -COORD_BIAS && cy < COORD_BIAS && cz >= -COORD_BIAS && cz < COORD_BIAS;
      key[o] = inside ? pack_key(b, cx, cy, cz) : KEY_EMPTY;      // KEY_EMPTY is no cell's key (the pair bits are never all ones)
      slot[o] = hash_key(key[o]) & g.mask;
      cell[o] = load_cell(g.cells, slot[o]);
    }
#pragma unroll
    for (int o = 0; o < 9; ++o) {
      if (key[o] == KEY_EMPTY) continue;
      IcpCell e = cell[o];
      unsigned int sl = slot[o];
      for (unsigned int probes = 0; e.key != key[o] && e.key != KEY_EMPTY && probes < g.mask; ++probes) {   // bounded: never full
        sl = (sl + 1) & g.mask;
        e = load_cell(g.cells, sl);
      }
      if (e.key != key[o]) continue;
      // the run's points four at a time: the loads of a group are issued together (the index is clamped inside the run, a
      // repeated point is not evaluated twice)
      const int n = e.more + 1;
      for (int j = 0; j < n; j += 4) {
        float4 q4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q4[u] = g.pts[e.first + (j + u < n ? j + u : n - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j + u >= n) break;
          each(q4[u]);
        }
      }
    }
  }
}

unsigned int table_capacity(int total_tgt) {
  unsigned int cap = 64;
  while (cap < 2u * (unsigned)total_tgt) cap <<= 1;
  return cap;
}

// slots for `tables` tables that hold total_tgt rows between them.  One table is sized exactly; of several, each has
// table_capacity(its own rows) slots, which is 64 or less than 4 x its rows: 64 per table + 4 per row hold them all
size_t table_slots(int total_tgt, int tables) {
  return tables <= 1 ? (size_t)table_capacity(total_tgt) : (size_t)64 * tables + (size_t)4 * total_tgt;
}

// what the grid and its two sorts need; a user carves its own arrays behind it
struct GridWorkspace {
  unsigned long long *tkey, *tkey_sorted, *qkey, *qkey_sorted;
  IcpCell* cells;
  int *trow, *trow_sorted, *qrow, *qrow_sorted;
  float4* pts;
  void* sort_tmp;
  size_t sort_bytes;
  unsigned int cap;
};

// the layout for the LARGEST chunk a call with these totals can hold.  tables = 1: every chunk reuses it.  tables > 1 (a user whose
// grids outlive their chunk): the row arrays are the call's, a chunk uses its own rows of them, and `cells` has room for one table per
// chunk behind one another (chunk_grid)
void carve_grid(Carver& c, int total_q, int total_tgt, int tables, GridWorkspace* w) {
  w->cap = table_capacity(total_tgt);
  w->tkey = c.take<unsigned long long>(total_tgt);
  w->tkey_sorted = c.take<unsigned long long>(total_tgt);
  w->qkey = c.take<unsigned long long>(total_q);
  w->qkey_sorted = c.take<unsigned long long>(total_q);
  w->cells = c.take<IcpCell>(table_slots(total_tgt, tables));
  w->trow = c.take<int>(total_tgt);
  w->trow_sorted = c.take<int>(total_tgt);
  w->qrow = c.take<int>(total_q);
  w->qrow_sorted = c.take<int>(total_q);
  w->pts = c.take<float4>(total_tgt);
  const size_t a = sort_rows64_tmp_bytes(total_tgt > 0 ? total_tgt : 1), b = sort_rows64_tmp_bytes(total_q > 0 ? total_q : 1);
  w->sort_bytes = a > b ? a : b;
  w->sort_tmp = c.take<char>(w->sort_bytes);
}

// the segments of one chunk of <= ICP_CHUNK pairs, counted from the chunk's first query / target row
IcpSegs make_segs(const int32_t* seg_q, const int32_t* seg_tgt, int n_pairs) {
  IcpSegs s;
  s.n_pairs = n_pairs;
  for (int b = 0; b <= n_pairs; ++b) {
    s.src[b] = seg_q[b] - seg_q[0];
    s.tgt[b] = seg_tgt[b] - seg_tgt[0];
  }
  s.wg[0] = 0;
  for (int b = 0; b < n_pairs; ++b) s.wg[b + 1] = s.wg[b] + cdiv(s.src[b + 1] - s.src[b], ICP_BLOCK);
  return s;
}

// from the keys a user's key kernel wrote (both sides non-empty) to the grid its search reads: sorted queries in w.qrow_sorted
int build_grid(const IcpSegs& s, const float* tgt, const int* skip, const GridWorkspace& w, hipStream_t st, IcpGrid* g) {
  const int n_q = s.src[s.n_pairs], n_tgt = s.tgt[s.n_pairs];
  int rc = sort_rows_by_key64(w.sort_tmp, w.sort_bytes, w.tkey, w.tkey_sorted, w.trow, w.trow_sorted, n_tgt, 60, st);
  if (rc != EYOC_OK) return rc;
  rc = sort_rows_by_key64(w.sort_tmp, w.sort_bytes, w.qkey, w.qkey_sorted, w.qrow, w.qrow_sorted, n_q, 60, st);
  if (rc != EYOC_OK) return rc;
  EYOC_CHECK_HIP(hipMemsetAsync(w.cells, 0xFF, (size_t)w.cap * sizeof(IcpCell), st));
  hipLaunchKernelGGL(k_icp_build, dim3(cdiv(n_tgt, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, s, tgt, w.tkey_sorted, w.trow_sorted, skip, w.pts, w.cells,
                     w.cap - 1);
  *g = IcpGrid{w.cells, w.cap - 1, w.pts};
  return EYOC_OK;
}

// The argument checks every entry point shares, before anything touches the device, in the two parts an entry point puts its own
// checks between.  First what must hold before a segment is read; `pointers`: the caller's mandatory ones, the segments among them.
int check_grid_head(const char* what, bool pointers, int n_pairs, const void* ws) {
  EYOC_REQUIRE(pointers, EYOC_ERR_INVALID, "%s: NULL argument", what);
  EYOC_REQUIRE(n_pairs >= 1 && n_pairs <= 1024, EYOC_ERR_INVALID, "%s: n_pairs = %d is outside [1, 1024]", what, n_pairs);
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "%s: workspace must be 256-byte aligned", what);
  return EYOC_OK;
}

// then every segment list of the call (n_pairs + 1 offsets each)
int check_segments(const char* what, int n_pairs, std::initializer_list<const int32_t*> segs) {
  for (const int32_t* seg : segs) EYOC_REQUIRE(seg[0] == 0, EYOC_ERR_INVALID, "%s: segments must start at 0", what);
  for (int b = 0; b < n_pairs; ++b)
    for (const int32_t* seg : segs)
      EYOC_REQUIRE(seg[b + 1] >= seg[b], EYOC_ERR_INVALID, "%s: segment offsets must not decrease (pair %d)", what, b);
  return EYOC_OK;
}

// every chunk of <= ICP_CHUNK pairs in turn: chunk(first pair, pairs)
template <typename Chunk>
int for_each_chunk(int n_pairs, Chunk&& chunk) {
  for (int b0 = 0; b0 < n_pairs; b0 += ICP_CHUNK) {
    const int rc = chunk(b0, n_pairs - b0 < ICP_CHUNK ? n_pairs - b0 : ICP_CHUNK);
    if (rc != EYOC_OK) return rc;
  }
  return EYOC_OK;
}

// cell edge of the users that must find EXACTLY the rows of the n x n sweep with d2 < r^2: edge = fl(r (1 + 2^-20)); icp.hip section 4
// derives the margin
constexpr double RM_EDGE_MARGIN = 1.0 + 1.0 / 1048576.0;

}  // namespace
}  // namespace eyoc
