// The network's first convolution (C_in = 1 in production, 5^3 or 3^3 window): five kernels and ONE launcher.
//   conv1_kernel        one lane per output row probes the ks^3 offsets in the level-0 hash table            (Conv1Path::Probe)
//   conv1_tree_kernel   the same sums in exact fp32 from the octree links, no hash probes                    (Tree)
//   conv1_mfma_kernel   the window of 16 rows assembled in LDS, one split16 GEMM per tile                     (Mfma)
//   conv1_bf_kernel     level-1 block feature vectors staged per 256-parent tile, rows grouped by class      (Bf)
//   conv1_bfp_kernel    ... from persistent workgroups, class weights loaded once: the production kernel     (Bfp)
// What they share is written once, in the device helpers below; which of them runs is conv1_path() and nothing else.
#include <type_traits>

#include "spconv.h"

using namespace eyoc;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- shared device pieces -----------------------------------------------------------------------------------------------
// Window position of child `cs` of coarse block `kc` (of the 27 around the parent) for a fine row of parity class `cls` (its
// child slot in its parent: x | y << 1 | z << 2), -1: outside the ks^3 window.
__device__ __forceinline__ int conv1_window_pos(int ks, int cls, int kc, int cs) {
  const int r = ks / 2;
  const int dx = 2 * (kc % 3 - 1) + (cs & 1) - (cls & 1), dy = 2 * ((kc / 3) % 3 - 1) + ((cs >> 1) & 1) - ((cls >> 1) & 1),
            dz = 2 * (kc / 9 - 1) + (cs >> 2) - (cls >> 2);
  const bool in = dx >= -r && dx <= r && dy >= -r && dy <= r && dz >= -r && dz <= r;
  return in ? (dx + r) + ks * (dy + r) + ks * ks * (dz + r) : -1;
}
// ... as a table over the 8 x 216 (class, block, child) slots.  miss: what a slot outside the window holds - 127 for the block-vector
// kernels (row 127 of their weight copy is zero), -1 for conv1_mfma_kernel (no write)
__device__ __forceinline__ void conv1_fill_ktab(signed char (*ktab)[216], int ks, int miss, int threads) {
  for (int e = threadIdx.x; e < 8 * 216; e += threads) {
    const int cls = e / 216, sl = e % 216;
    const int k = conv1_window_pos(ks, cls, sl >> 3, sl & 7);
    ktab[cls][sl] = (signed char)(k >= 0 ? k : miss);
  }
}

// W[k][c] * 2^sh split into fp16 halves (2^sh = wsc lifts the layer's largest weight into [256, 512): the lo halves stay normal and
// no hi half leaves the fp16 range; 2^8 without a.wscale); rows k >= K are zero
__device__ __forceinline__ float conv1_wscale(const Conv1Args& a) { return a.wscale ? a.wscale[0] : 256.0f; }
__device__ __forceinline__ float conv1_iwscale(const Conv1Args& a) { return a.wscale ? a.wscale[1] : 1.0f / 256.0f; }
__device__ __forceinline__ void conv1_weight_halves(const Conv1Args& a, int K, int k, int c, float wsc, _Float16& hi, _Float16& lo) {
  const float w = k < K ? a.w[(size_t)k * 32 + c] * wsc : 0.0f;
  hi = (_Float16)w;
  lo = (_Float16)(w - (float)hi);
}
// the whole kernel into LDS as [128][32] hi / lo; row 127 = zeros (K <= 125)
__device__ __forceinline__ void conv1_stage_weights(const Conv1Args& a, _Float16 (*w5h)[32], _Float16 (*w5l)[32], int threads) {
  const int K = a.ks * a.ks * a.ks;
  const float wsc = conv1_wscale(a);
  for (int e = threadIdx.x; e < 128 * 32; e += threads) conv1_weight_halves(a, K, e / 32, e % 32, wsc, (&w5h[0][0])[e], (&w5l[0][0])[e]);
}
// a class's weights: lane (g, j) of k-step t holds W[window position of (block 4 t + g, child i)][channel 16 tt + j], i = 0..7
__device__ __forceinline__ void conv1_class_weights(const signed char* kt, const _Float16 (*w5h)[32], const _Float16 (*w5l)[32], int g, int j,
                                                    half8_t (&wh)[7][2], half8_t (&wl)[7][2]) {
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int kc = 4 * t + g;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int kp = kc < 27 ? (int)kt[kc * 8 + i] : 127;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        wh[t][tt][i] = w5h[kp][16 * tt + j];
        wl[t][tt][i] = w5l[kp][16 * tt + j];
      }
    }
  }
}
// the block vector of a level-1 row: its eight child features as fp16 hi / lo halves, 0 where bit q of `present` is clear
__device__ __forceinline__ void conv1_block_vector(const float (&f)[8], unsigned int present, _Float16* cfh, _Float16* cfl) {
  half8_t h8, l8;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float x = (present >> q) & 1u ? f[q] : 0.f;
    h8[q] = (_Float16)x;
    l8[q] = (_Float16)(x - (float)h8[q]);
  }
  *reinterpret_cast<half8_t*>(cfh) = h8;
  *reinterpret_cast<half8_t*>(cfl) = l8;
}
// class compaction, second half: the rows of ONE class go into the tile's lists.  bm: this wave's ballot of the parents that have the
// child (v >= 0), ccnt_q[0 .. w): what the waves in front of it counted for the class
__device__ __forceinline__ void conv1_place_class(const int* ccnt_q, int w, unsigned long long bm, int v, int f0, int parent,
                                                  unsigned short* lrow_q, unsigned char* lpar_q) {
  int base = 0;
  for (int i = 0; i < w; ++i) base += ccnt_q[i];
  if (v >= 0) {
    const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)bm, 0u));   // set bits below this lane
    lrow_q[pos] = (unsigned short)(v - f0);
    lpar_q[pos] = (unsigned char)parent;
  }
}
// one split16 k-step over NT channel tiles: hi * hi, hi * lo, lo * hi, in that order
template <int NT>
__device__ __forceinline__ void conv1_mfma_step(const half8_t (&wh)[NT], const half8_t (&wl)[NT], const half8_t vh, const half8_t vl, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], vh, acc[t], 0, 0, 0);
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], vl, acc[t], 0, 0, 0);
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], vh, acc[t], 0, 0, 0);
  }
}
// epilogue of the MFMA kernels: lane (g, j) holds channels 16 t + 4 g .. + 3 of row o.  bias: 32 floats, global or LDS
template <int NT>
__device__ __forceinline__ void conv1_mfma_store(const Conv1Args& a, int o, int g, const f32x4 (&acc)[NT], float iwsc, const float* bias, float& mx) {
  float* dst = a.out + (size_t)o * a.ld_out;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ch0 = 16 * t + 4 * g;
    const float4 b = *reinterpret_cast<const float4*>(bias + ch0);
    const float4 v = make_float4(acc[t][0] * iwsc + b.x, acc[t][1] * iwsc + b.y, acc[t][2] * iwsc + b.z, acc[t][3] * iwsc + b.w);
    split16_track(mx, v);
    if (a.out_split) split16_store4(dst, ch0, v);
    else *reinterpret_cast<float4*>(dst + ch0) = v;
  }
}
// epilogue of the scalar kernels: one lane holds all COUT channels of row o
template <int COUT>
__device__ __forceinline__ void conv1_scalar_store(const Conv1Args& a, int o, const float (&acc)[COUT]) {
  float* dst = a.out + (size_t)o * a.ld_out;
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < COUT; i += 4) {
    float4 v;
    v.x = acc[i] + a.bias[i]; v.y = acc[i + 1] + a.bias[i + 1];
    v.z = acc[i + 2] + a.bias[i + 2]; v.w = acc[i + 3] + a.bias[i + 3];
    split16_track(mx, v);
    if (a.out_split) split16_store4(dst, i, v);
    else *reinterpret_cast<float4*>(dst + i) = v;
  }
  if (a.out_split) split16_report(a.range, mx);
}

// ------------------------------------------------------------------------------------------------
// first convolution (C_in = 1 in production): one lane per output row probes the ks^3 offsets in
// the level-0 hash table and accumulates f * W[k] from an LDS copy of the (BN-folded) kernel.
// ------------------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void conv1_kernel(Conv1Args a) {
  constexpr int W_FLOATS = 8192;  // 32 KB of LDS for a slab of offsets
  __shared__ __attribute__((aligned(16))) float ws[W_FLOATS];
  const int o = blockIdx.x * 256 + threadIdx.x;
  const bool ok = o < a.n;
  int4 c = make_int4(0, 0, 0, 0);
  if (ok) c = reinterpret_cast<const int4*>(a.coords)[o];
  float acc[COUT];
#pragma unroll
  for (int i = 0; i < COUT; ++i) acc[i] = 0.0f;
  const int K = a.ks * a.ks * a.ks, r = a.ks / 2;
  const int per_k = a.cin * COUT;
  const int kslab = W_FLOATS / per_k;
  for (int k0 = 0; k0 < K; k0 += kslab) {
    const int kn = min(kslab, K - k0);
    __syncthreads();
    for (int i = threadIdx.x; i < kn * per_k; i += 256) ws[i] = a.w[(size_t)k0 * per_k + i];
    __syncthreads();
    for (int kk = 0; kk < kn; ++kk) {
      const int k = k0 + kk;
      const int dx = k % a.ks - r, dy = (k / a.ks) % a.ks - r, dz = k / (a.ks * a.ks) - r;
      int idx = -1;
      if (ok) idx = hash_lookup(a.table, pack_key(c.x, c.y + dx, c.z + dy, c.w + dz));
      if (__ballot(idx >= 0) == 0ull) continue;
      for (int ci = 0; ci < a.cin; ++ci) {
        const float f = idx >= 0 ? a.in[(size_t)(a.in_perm ? a.in_perm[idx] : idx) * a.cin + ci] : 0.0f;
        const float* wk = ws + (kk * a.cin + ci) * COUT;
#pragma unroll
        for (int i = 0; i < COUT; ++i) acc[i] = fmaf(f, wk[i], acc[i]);
      }
    }
  }
  if (ok) conv1_scalar_store<COUT>(a, o, acc);
}

// Same convolution without hash probes: the ks^3 window (ks = 3 or 5) of a voxel lies inside the 27
// level-1 blocks around its parent, whose rows come from the level-1 stride-1 table and whose
// occupants come from the 8-entry child vectors (one 32-byte read per block).  ~1 KB of table reads
// per output row instead of 125 probes of a 64-bit-key hash table.
template <int COUT>
__global__ __launch_bounds__(256) void conv1_tree_kernel(Conv1Args a) {
  constexpr int LDW = COUT + 4;   // padded weight rows: lanes hold different offsets k, keep them on different banks
  extern __shared__ float wsm[];
  const int K = a.ks * a.ks * a.ks;
  for (int i = threadIdx.x; i < K * a.cin * COUT; i += 256) wsm[(i / COUT) * LDW + i % COUT] = a.w[i];
  __syncthreads();
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.n) return;
  const int4 c = reinterpret_cast<const int4*>(a.coords)[o];
  const int cls = (c.y & 1) | ((c.z & 1) << 1) | ((c.w & 1) << 2);
  const int p = a.parent[o];
  float acc[COUT];
#pragma unroll
  for (int i = 0; i < COUT; ++i) acc[i] = 0.0f;
#pragma unroll 1
  for (int kc = 0; kc < 27; ++kc) {
    const int B = kc == 13 ? p : a.s1c[(size_t)kc * a.nc + p];
    if (B < 0) continue;
    const int4 lo = reinterpret_cast<const int4*>(a.children)[2 * (size_t)B];
    const int4 hi = reinterpret_cast<const int4*>(a.children)[2 * (size_t)B + 1];
    const int ch[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int cs = 0; cs < 8; ++cs) {
      const int idx = ch[cs];
      const int k = conv1_window_pos(a.ks, cls, kc, cs);
      if (idx < 0 || k < 0) continue;
      for (int ci = 0; ci < a.cin; ++ci) {
        const float f = a.in[(size_t)(a.in_perm ? a.in_perm[idx] : idx) * a.cin + ci];
        const float4* wk = reinterpret_cast<const float4*>(wsm + (k * a.cin + ci) * LDW);
#pragma unroll
        for (int i = 0; i < COUT / 4; ++i) {
          const float4 w4 = wk[i];
          acc[4 * i] = fmaf(f, w4.x, acc[4 * i]); acc[4 * i + 1] = fmaf(f, w4.y, acc[4 * i + 1]);
          acc[4 * i + 2] = fmaf(f, w4.z, acc[4 * i + 2]); acc[4 * i + 3] = fmaf(f, w4.w, acc[4 * i + 3]);
        }
      }
    }
  }
  conv1_scalar_store<COUT>(a, o, acc);
}

// The same first convolution (C_in = 1, 5^3 or 3^3 window, 32 output channels) as MFMA work.  conv1_tree_kernel walks the
// 216 (coarse block, child) slots of a row in lock step - a wave executes every slot although ~12 % of its lanes hold a
// neighbour there - and pays 32 FMAs with lane-varying weight rows per slot: 1.65 ms on the 3.8 M-row batch.  Here a wave
// takes 16 output rows, its four 16-lane groups walk a quarter of the coarse blocks each (a neighbour's feature goes to
// column k = its window position of the row's line in an LDS tile, as fp16 hi / lo halves), and the products are ONE
// [16 x 128] x [128 x 32] split16 GEMM per tile: 4 k-steps x 3 terms x 2 channel tiles = 24 MFMAs, weights resident in
// registers (pre-scaled by 2^8 so that their lo halves stay normal).
__global__ __launch_bounds__(256, 4) void conv1_mfma_kernel(Conv1Args a) {
  constexpr int COUT = 32, KP = 128, KPS = KP + 8, NT = COUT / 16, NQ = KP / 32;
  // row stride KP + 8 halves = 272 B = 68 dwords: the 16 rows of a tile that write the SAME window position (one ds_write_b16, lanes of
  // one parity class) land in 16 different banks - at 256 B they all hit one (a 16-way conflict on every write: measured 1.1 -> ? ms)
  __shared__ __attribute__((aligned(16))) _Float16 xt[4][2][16][KPS];   // [wave][hi / lo][row][window position]
  __shared__ __attribute__((aligned(8))) signed char ktab[8][216];                                // window position of slot (block kc, child cs) for a row of parity class cls, -1: outside
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int K = a.ks * a.ks * a.ks;
  conv1_fill_ktab(ktab, a.ks, -1, 256);
  __syncthreads();
  // weight fragments (A operand): lane (g, j): W[k = 32 q + 8 g + i][cout = 16 t + j] * 2^sh, split
  const float wsc = conv1_wscale(a), iwsc = conv1_iwscale(a);
  half8_t wh[NQ][NT], wl[NQ][NT];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        _Float16 h, l;
        conv1_weight_halves(a, K, 32 * q + 8 * g + i, 16 * t + j, wsc, h, l);
        wh[q][t][i] = h;
        wl[q][t][i] = l;
      }
  _Float16 (*xh)[KPS] = xt[wave][0];
  _Float16 (*xl)[KPS] = xt[wave][1];
  const int n_tiles = (a.n + 15) / 16;
  // persistent waves: the weight fragments above are loaded once per wave, not once per 16 rows
  for (int tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += gridDim.x * 4) {
  const int o = tile * 16 + j;                                      // this lane's row (the 4 groups share it)
  // clear the tile: 16 rows x 256 B x 2 = 8 KB per wave
  {
    float4* z = reinterpret_cast<float4*>(&xt[wave][0][0][0]);
#pragma unroll
    for (int i = 0; i < (2 * 16 * KPS * 2 / 16 + 63) / 64; ++i)
      if (i * 64 + lane < 2 * 16 * KPS * 2 / 16) z[i * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (o < a.n) {
    const int4 c = reinterpret_cast<const int4*>(a.coords)[o];
    const signed char* kt = ktab[(c.y & 1) | ((c.z & 1) << 1) | ((c.w & 1) << 2)];
    const int p = a.parent[o];
    // per half of the group's (up to 7) coarse blocks: three rounds of independent loads - the blocks, their child
    // vectors, the features of ALL their children back to back (absent / outside slots read row 0; a load inside a
    // branch would wait for its data before the next slot starts) - then the LDS writes
    const float* __restrict__ fin = a.in;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      constexpr int NB = 4;
      int Bk[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int kc = g + 4 * (half * NB + i);
        Bk[i] = kc >= 27 ? -1 : kc == 13 ? p : a.s1c[(size_t)kc * a.nc + p];
      }
      int ch[NB][8];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        int4 lo = make_int4(-1, -1, -1, -1), hi = make_int4(-1, -1, -1, -1);
        if (Bk[i] >= 0) {
          lo = reinterpret_cast<const int4*>(a.children)[2 * (size_t)Bk[i]];
          hi = reinterpret_cast<const int4*>(a.children)[2 * (size_t)Bk[i] + 1];
        }
        ch[i][0] = lo.x; ch[i][1] = lo.y; ch[i][2] = lo.z; ch[i][3] = lo.w;
        ch[i][4] = hi.x; ch[i][5] = hi.y; ch[i][6] = hi.z; ch[i][7] = hi.w;
      }
      int kk[NB][8];
      float fv[NB][8];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int kc = g + 4 * (half * NB + i);
        const unsigned long long k8 = kc < 27 ? *reinterpret_cast<const unsigned long long*>(kt + kc * 8) : ~0ull;   // 8 positions
#pragma unroll
        for (int cs = 0; cs < 8; ++cs) {
          const int idx = ch[i][cs];
          const int kpos = (int)(signed char)(k8 >> (8 * cs));
          const bool ok = idx >= 0 && kpos >= 0;
          kk[i][cs] = ok ? kpos : -1;
          fv[i][cs] = fin[ok ? idx : 0];
        }
      }
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int cs = 0; cs < 8; ++cs)
          if (kk[i][cs] >= 0) {
            const float f = fv[i][cs];
            const _Float16 h = (_Float16)f;
            xh[j][kk[i][cs]] = h;
            xl[j][kk[i][cs]] = (_Float16)(f - (float)h);
          }
    }
  }
  // the wave's LDS operations execute in order; the wait makes the writes of the other lanes visible to the reads below
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const half8_t vh = *reinterpret_cast<const half8_t*>(&xh[j][32 * q + 8 * g]);   // B operand: X[k = 32 q + 8 g + i][row j]
    const half8_t vl = *reinterpret_cast<const half8_t*>(&xl[j][32 * q + 8 * g]);
    conv1_mfma_step<NT>(wh[q], wl[q], vh, vl, acc);
  }
  if (o < a.n) {
    float mx = 0.f;
    conv1_mfma_store<NT>(a, o, g, acc, iwsc, a.bias, mx);
    if (a.out_split) split16_report(a.range, mx);
  }
  __builtin_amdgcn_wave_barrier();                                   // the next tile's clear stays behind this tile's operand reads
  }
}

// out[i, :] = in[perm[i], :] for narrow rows (the network input, C_in = 1 in production)
__global__ void k_permute_rows(const float* __restrict__ in, const int32_t* __restrict__ perm, int n, int c, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * c) return;
  const int r = (int)(i / c), j = (int)(i - (long long)r * c);
  out[i] = in[(size_t)perm[r] * c + j];
}

}  // namespace

namespace eyoc {

int launch_permute_rows(const float* in, const int32_t* perm, int n, int c, float* out, hipStream_t st) {
  if (n <= 0) return EYOC_OK;
  hipLaunchKernelGGL(k_permute_rows, dim3((unsigned)cdiv((long long)n * c, 256)), dim3(256), 0, st, in, perm, n, c, out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

// ---- first convolution as a K = 27 sparse convolution over level-1 BLOCK FEATURE VECTORS (round 5; Z-ordered maps, C_in = 1,
// 32 output channels, split16 downstream).  conv1_mfma_kernel above probes, for EVERY fine row, the 27 coarse blocks around its
// parent and their 8 children each (~60 dependent loads per lane and 16-row tile) although the ~2.4 children of a parent share
// all of them and neighbouring parents most.  Round 3's conv1_st_kernel staged the child features of a 256-parent level-1 tile's
// neighbourhood in LDS once (the tile record the staged stride-1 kernel of level 1 uses) but still assembled, per fine row, a
// [128]-entry line of window positions in LDS (zero the tile, then one conditional 2-byte write per child in the window) before
// it could multiply: 0.8 ms per 128 clouds for 0.5 GB of compulsory traffic, bound by that assembly and its dependent loads.
// Here nothing is assembled (0.49 ms; the old kernel is gone).  The 8 child features of a level-1 block - one 16-byte
// line of fp16 hi halves, one of lo halves - ARE an MFMA operand piece: for the fine row in column j, k-slot group g of k-step t
// is the block vector of neighbour block 4 t + g of the row's parent, read straight from the staged vectors (the slot comes
// from the level-1 tile record, as in the staged stride-1 kernel).  The weights are what depends on the row: which of the 216
// (block, child) pairs lies where in the row's 5^3 window is a function of the row's PARITY CLASS (its child slot in its
// parent), so the tile's fine rows are grouped by class - the class is the child slot, the rows of class q are `children[p][q]`
// of the tile's 256 parents: eight ballot compactions, no sort - and a wave multiplies all 16-row chunks of one class against
// that class's [216 x 32] weight matrix, gathered once per (tile, class) from an LDS copy of the [125 x 32] kernel into 112
// registers.  42 MFMAs per 16 rows instead of 24 (the matrix pipe idles in this layer either way), no operand tile, no
// per-row dependent global loads: the tile's rulebook entries are staged in LDS with the block vectors.
// Same products as conv1_mfma_kernel, summed in another order (blocks, not window positions): equal to fp32 rounding
// (tests/test_gpu_split16.py).  Timing-only ablations (round 5, EXPERIMENTS.md; their switches are gone): the class-weight gathers
// 0.07 ms, the LDS copy of the kernel 0.04 ms of the 0.49; the rest is the tile's dependent stage rounds and its stores.
__global__ __launch_bounds__(256, 2) void conv1_bf_kernel(Conv1Args a) {
  constexpr int COUT = 32, NT = COUT / 16, NS7 = 7;
  constexpr int NSLOT = ST_NPASS * ST_UMAX + 1, ZSLOT = NSLOT - 1;
  __shared__ __attribute__((aligned(16))) _Float16 cfh[NSLOT][8], cfl[NSLOT][8];     // block vectors of the staged level-1 rows
  __shared__ __attribute__((aligned(16))) _Float16 w5h[128][COUT], w5l[128][COUT];   // the kernel, scaled and split; row 127 = zeros
  __shared__ __attribute__((aligned(16))) unsigned short ent[27 * 64 * 4];           // pass-0 rulebook entries of the tile
  __shared__ unsigned short lrow[8][ST_TILE];                                        // fine rows of class q (minus the tile's first fine row)
  __shared__ unsigned char lpar[8][ST_TILE];                                         // ... and their parents (local index)
  __shared__ signed char ktab[8][216];
  __shared__ unsigned char inv[ST_TILE];
  __shared__ int ccnt[8][4], ctot[8];
  __shared__ int f0s;
  __shared__ __attribute__((aligned(16))) float bias_s[COUT];                        // (as conv1_bfp_kernel keeps it: the shared epilogue reads it per chunk)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const unsigned char* lr = a.local1 + (size_t)tile * ST_LR_BYTES;
  inv[threadIdx.x] = lr[ST_INV_OFF + threadIdx.x];
  if (threadIdx.x < COUT) bias_s[threadIdx.x] = a.bias[threadIdx.x];
  conv1_fill_ktab(ktab, a.ks, 127, 256);
  conv1_stage_weights(a, w5h, w5l, 256);
  {   // the tile's pass-0 entries: 13.5 KB, 16 bytes per load
    const uint4* src = reinterpret_cast<const uint4*>(lr + ST_LOC_OFF);
    uint4* dst = reinterpret_cast<uint4*>(ent);
    for (int e = threadIdx.x; e < 27 * 64 * 4 * 2 / 16; e += 256) dst[e] = src[e];
  }
  // ---- stage: block vectors of the tile's distinct level-1 rows (three rounds of independent loads: row numbers, child links, child features)
  const int n_u = *reinterpret_cast<const int*>(lr);
  const int* __restrict__ U = reinterpret_cast<const int*>(lr + 16);
  const float* __restrict__ fin = a.in;
  {
    constexpr int NS = (NSLOT + 255) / 256;
    int u[NS];
    int4 c0[NS], c1[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = (int)threadIdx.x + 256 * i;
      u[i] = s < n_u ? U[s] : -1;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      c0[i] = c1[i] = make_int4(-1, -1, -1, -1);
      if (u[i] >= 0) {
        c0[i] = reinterpret_cast<const int4*>(a.children)[2 * (size_t)u[i]];
        c1[i] = reinterpret_cast<const int4*>(a.children)[2 * (size_t)u[i] + 1];
      }
    }
    float f[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int v[8] = {c0[i].x, c0[i].y, c0[i].z, c0[i].w, c1[i].x, c1[i].y, c1[i].z, c1[i].w};
#pragma unroll
      for (int q = 0; q < 8; ++q) f[i][q] = (256 * i < n_u && v[q] >= 0) ? fin[v[q]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = (int)threadIdx.x + 256 * i;
      if (s < n_u || s == ZSLOT) conv1_block_vector(f[i], s < n_u ? 0xffu : 0u, cfh[s], cfl[s]);
    }
  }
  // ---- the tile's fine rows by class: thread p holds parent p's child links
  {
    const int prow = tile * ST_TILE + (int)threadIdx.x;
    int v[8];
    if (prow < a.nc) {
      const int4 c0 = reinterpret_cast<const int4*>(a.children)[2 * (size_t)prow], c1 = reinterpret_cast<const int4*>(a.children)[2 * (size_t)prow + 1];
      v[0] = c0.x; v[1] = c0.y; v[2] = c0.z; v[3] = c0.w; v[4] = c1.x; v[5] = c1.y; v[6] = c1.z; v[7] = c1.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = -1;
    }
    if (threadIdx.x == 0) {                              // the tile's first fine row: the first child of its first parent (Z-order)
      int m = a.n;
#pragma unroll
      for (int q = 0; q < 8; ++q) if (v[q] >= 0 && v[q] < m) m = v[q];
      f0s = m;
    }
    unsigned long long bm[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      bm[q] = __ballot(v[q] >= 0);
      if (lane == 0) ccnt[q][wave] = __popcll(bm[q]);
    }
    __syncthreads();
    const int f0 = f0s;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      conv1_place_class(ccnt[q], wave, bm[q], v[q], f0, (int)threadIdx.x, lrow[q], lpar[q]);
      if (threadIdx.x == 0) ctot[q] = ccnt[q][0] + ccnt[q][1] + ccnt[q][2] + ccnt[q][3];
    }
  }
  __syncthreads();
  const int f0 = f0s;
  const int n_pass = n_u > ST_UMAX ? 2 : 1;
  const unsigned short* __restrict__ loc = reinterpret_cast<const unsigned short*>(lr + ST_LOC_OFF);
  const float iwsc = conv1_iwscale(a);
  float mx = 0.f;
  for (int qi = 0; qi < 2; ++qi) {
    const int q = wave + 4 * qi;                         // this wave's class
    const int nq = ctot[q];
    if (nq == 0) continue;                               // wave-uniform
    half8_t wh[NS7][NT], wl[NS7][NT];
    conv1_class_weights(ktab[q], w5h, w5l, g, j, wh, wl);
    for (int c0 = 0; c0 < nq; c0 += 16) {
      const int idx = c0 + j;
      const bool ok = idx < nq;
      const int pl = lpar[q][ok ? idx : 0];
      const int o = f0 + (int)lrow[q][ok ? idx : 0];
      const int sl = inv[pl];
      const int ew = (sl >> 6) * 16 + (sl & 15), ec = (sl >> 4) & 3;
      f32x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NS7; ++t) {
        const int kc = 4 * t + g;
        int slot = ZSLOT;
        if (kc < 27) {
          const int e0 = ent[(kc * 64 + ew) * 4 + ec] >> 6;                            // entry = 64 l + swizzle
          if (e0 != ST_UMAX) slot = e0;
          else if (n_pass > 1) {                                                        // rare: the neighbour sits in the second pass
            const int e1 = loc[((size_t)(27 + kc) * 64 + ew) * 4 + ec] >> 6;
            if (e1 != ST_UMAX) slot = ST_UMAX + e1;
          }
        }
        const half8_t vh = *reinterpret_cast<const half8_t*>(&cfh[slot][0]);
        const half8_t vl = *reinterpret_cast<const half8_t*>(&cfl[slot][0]);
        conv1_mfma_step<NT>(wh[t], wl[t], vh, vl, acc);
      }
      if (ok) conv1_mfma_store<NT>(a, o, g, acc, iwsc, bias_s, mx);
    }
  }
  if (a.out_split) split16_report(a.range, mx);
}

// ---- the same first convolution from PERSISTENT workgroups (eyoc_spconv_select_conv1_kernel(3)).  conv1_bf_kernel's workgroups live for
// one tile (~600 fine rows) and each of them rebuilds ktab, re-reads and re-splits the kernel, gathers two class weight matrices and
// sits through three dependent rounds of global loads before its first MFMA.  None of the weight work depends on the tile.  Here one
// 512-thread workgroup per CU walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... (static order, no atomics; every output row still
// belongs to exactly one wave); wave q IS parity class q and keeps the class's [224 x 32] hi / lo weight fragments in 112 registers
// for its whole life; and the tile record lives in one of TWO LDS buffers: while the waves multiply a tile out of one, the next
// tile's loads are in flight in registers - its row numbers U were asked for a whole tile earlier, its child links go out at the top
// of the tile, its child features between the two halves of the wave's chunks - and at the end of the tile they are converted into
// the other buffer, where the eight ballots of the next tile's class compaction run as well (two barriers per tile).  All loads are
// unconditional on clamped indices (a load inside a branch is waited for on the spot), past the last tile they re-read it.
// Same products in the same order as conv1_bf_kernel (k-steps 0..6, hh / hl / lh), same slot lookup, same epilogue: bit-identical
// output rows and range-guard words (tests/test_gpu_conv1_persistent.py).
struct alignas(16) Conv1Tile {
  static constexpr int NSLOT = ST_NPASS * ST_UMAX + 1;
  _Float16 cfh[NSLOT][8], cfl[NSLOT][8];       // block vectors of the staged level-1 rows; slot NSLOT - 1 = zeros
  unsigned short ent[27 * 64 * 4];             // pass-0 rulebook entries
  unsigned short lrow[8][ST_TILE];             // fine rows of class q (minus f0)
  unsigned char lpar[8][ST_TILE];              // ... and their parents (local index)
  unsigned char inv[ST_TILE];
  int ctot[8];
  int f0, pad[3];
};
struct alignas(16) Conv1Shared {
  Conv1Tile tile[2];
  _Float16 w5h[128][32], w5l[128][32];         // the kernel, scaled and split; row 127 = zeros (read once, at kernel start)
  signed char ktab[8][216];
  float bias[32];
  int ccnt[8][4], f0h[2], pad[2];
};
static_assert(sizeof(Conv1Shared) <= 160 * 1024, "conv1_bfp_kernel: one workgroup per CU, within its LDS");
extern __shared__ __attribute__((aligned(16))) unsigned char conv1p_smem[];

__global__ __launch_bounds__(512, 1) void conv1_bfp_kernel(Conv1Args a, int n_tiles) {
  constexpr int COUT = 32, NT = COUT / 16, NS7 = 7;
  constexpr int NSLOT = Conv1Tile::NSLOT, ZSLOT = NSLOT - 1;
  constexpr int NS = (NSLOT + 511) / 512;                // staged rows per thread
  constexpr int NENT = 27 * 64 * 4 * 2 / 16;             // 16-byte pieces of a tile's pass-0 entries
  Conv1Shared& S = *reinterpret_cast<Conv1Shared*>(conv1p_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int G = gridDim.x;
  const int4* __restrict__ child4 = reinterpret_cast<const int4*>(a.children);
  const float* __restrict__ fin = a.in;
  // row numbers of the first tile's stage: in flight under the weight work
  int tn = blockIdx.x;                                   // the tile being staged (< n_tiles: the grid is at most n_tiles)
  int nu_n, un[NS];
  {
    const unsigned char* lr = a.local1 + (size_t)tn * ST_LR_BYTES;
    nu_n = *reinterpret_cast<const int*>(lr);
#pragma unroll
    for (int i = 0; i < NS; ++i) un[i] = reinterpret_cast<const int*>(lr + 16)[min(tid + 512 * i, ST_UCAP - 1)];
  }
  conv1_fill_ktab(S.ktab, a.ks, 127, 512);
  conv1_stage_weights(a, S.w5h, S.w5l, 512);
  if (tid < 32) {                                        // the zero vector of both buffers: written once, no stage touches it
    const int b = tid >> 4, e = tid & 15;
    (e < 8 ? S.tile[b].cfh[ZSLOT][e] : S.tile[b].cfl[ZSLOT][e - 8]) = (_Float16)0.f;
  }
  if (tid >= 64 && tid < 64 + COUT) S.bias[tid - 64] = a.bias[tid - 64];
  __syncthreads();
  // this wave's class = its index
  half8_t wh[NS7][NT], wl[NS7][NT];
  conv1_class_weights(S.ktab[wave], S.w5h, S.w5l, g, j, wh, wl);
  const float iwsc = conv1_iwscale(a);
  float mx = 0.f;
  int tc = -1, nu_c = 0;                                 // the tile being multiplied (none yet) and its distinct rows
  for (int it = 0;; ++it) {
    const Conv1Tile& B = S.tile[it & 1];                 // multiplied now (filled during the previous tile)
    Conv1Tile& N = S.tile[(it & 1) ^ 1];                 // filled now (last read during the previous tile)
    // ---- loads for tile tn.  Round 2: the child links of its staged rows (their numbers arrived during the previous tile)
    const unsigned char* lrn = a.local1 + (size_t)min(tn, n_tiles - 1) * ST_LR_BYTES;
    int4 c0[NS], c1[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int u = tid + 512 * i < nu_n ? min(max(un[i], 0), a.nc - 1) : 0;
      c0[i] = child4[2 * (size_t)u];
      c1[i] = child4[2 * (size_t)u + 1];
    }
    // ... its pass-0 entries and its inverse map
    const uint4* esrc = reinterpret_cast<const uint4*>(lrn + ST_LOC_OFF);
    const uint4 en0 = esrc[tid], en1 = esrc[min(tid + 512, NENT - 1)];
    const unsigned int invw = reinterpret_cast<const unsigned int*>(lrn + ST_INV_OFF)[lane];
    // ---- tile tc: this wave's class, 16 rows at a time
    const int nq = tc >= 0 ? B.ctot[wave] : 0;
    const int f0 = B.f0;
    const int n_pass = nu_c > ST_UMAX ? 2 : 1;
    const unsigned short* __restrict__ loc = reinterpret_cast<const unsigned short*>(a.local1 + (size_t)max(tc, 0) * ST_LR_BYTES + ST_LOC_OFF);
    auto chunk = [&](const int c0r) __attribute__((always_inline)) {
      const int idx = c0r + j;
      const bool ok = idx < nq;
      const int pl = B.lpar[wave][ok ? idx : 0];
      const int o = f0 + (int)B.lrow[wave][ok ? idx : 0];
      const int sl = B.inv[pl];
      const int ew = (sl >> 6) * 16 + (sl & 15), ec = (sl >> 4) & 3;
      f32x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      // the seven slots first (independent LDS reads; conv1_bf_kernel's lookup, with the rare second-pass branch made wave-uniform
      // and taken once per chunk instead of splitting every k-step off behind its own dependent read)
      int slot[NS7];
#pragma unroll
      for (int t = 0; t < NS7; ++t) {
        const int kc = min(4 * t + g, 26);
        const int e0 = B.ent[(kc * 64 + ew) * 4 + ec] >> 6;                             // entry = 64 l + swizzle
        slot[t] = 4 * t + g < 27 ? e0 : -1;                                             // -1: no such block; ST_UMAX: not in pass 0
      }
      if (n_pass > 1) {                                                                 // rare: neighbours may sit in the second pass
#pragma unroll
        for (int t = 0; t < NS7; ++t) {
          const int e1 = loc[((27 + min(4 * t + g, 26)) * 64 + ew) * 4 + ec] >> 6;
          slot[t] = slot[t] != ST_UMAX ? slot[t] : e1 != ST_UMAX ? ST_UMAX + e1 : -1;
        }
      } else {
#pragma unroll
        for (int t = 0; t < NS7; ++t) slot[t] = slot[t] == ST_UMAX ? -1 : slot[t];
      }
#pragma unroll
      for (int t = 0; t < NS7; ++t) {
        const int sl_t = slot[t] < 0 ? ZSLOT : slot[t];
        const half8_t vh = *reinterpret_cast<const half8_t*>(&B.cfh[sl_t][0]);
        const half8_t vl = *reinterpret_cast<const half8_t*>(&B.cfl[sl_t][0]);
        conv1_mfma_step<NT>(wh[t], wl[t], vh, vl, acc);
      }
      if (ok) conv1_mfma_store<NT>(a, o, g, acc, iwsc, S.bias, mx);
    };
    const int nch = (nq + 15) >> 4, nch0 = (nch + 1) >> 1;
    for (int c = 0; c < nch0; ++c) chunk(16 * c);
    // ---- the entries and the inverse map go to the other buffer (nothing reads it during this tile), then round 3 for tile tn: the
    // child features (the links arrived under the first half), half of one of its own parents' child links per thread, and round 1 of
    // the tile after it
    reinterpret_cast<uint4*>(N.ent)[tid] = en0;
    if (tid + 512 < NENT) reinterpret_cast<uint4*>(N.ent)[tid + 512] = en1;
    if (tid < 64) reinterpret_cast<unsigned int*>(N.inv)[tid] = invw;
    float f[NS][8];
    unsigned int vmask = 0;                              // bit 8 i + q: child q of staged row i exists
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int v[8] = {c0[i].x, c0[i].y, c0[i].z, c0[i].w, c1[i].x, c1[i].y, c1[i].z, c1[i].w};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        f[i][q] = fin[max(v[q], 0)];
        vmask |= v[q] >= 0 ? 1u << (8 * i + q) : 0u;                // (the links die here: 24 registers less under the second half)
      }
    }
    const int pl_own = tid & 255, hf = tid >> 8;
    const int prow = min(tn, n_tiles - 1) * ST_TILE + pl_own;
    const int4 own = child4[2 * (size_t)min(prow, a.nc - 1) + hf];
    int nu_2, un2[NS];
    {
      const unsigned char* lr2 = a.local1 + (size_t)min(tn + G, n_tiles - 1) * ST_LR_BYTES;
      nu_2 = *reinterpret_cast<const int*>(lr2);
#pragma unroll
      for (int i = 0; i < NS; ++i) un2[i] = reinterpret_cast<const int*>(lr2 + 16)[min(tid + 512 * i, ST_UCAP - 1)];
    }
    for (int c = nch0; c < nch; ++c) chunk(16 * c);
    // ---- tile tn into the other buffer
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int s = tid + 512 * i;
      if (s < nu_n) conv1_block_vector(f[i], vmask >> (8 * i), N.cfh[s], N.cfl[s]);
    }
    // its fine rows by class: thread (hf, p) holds children 4 hf .. 4 hf + 3 of parent p; wave w counts parents 64 (w & 3) ...
    int v[4] = {own.x, own.y, own.z, own.w};
    if (prow >= a.nc) v[0] = v[1] = v[2] = v[3] = -1;
    if (pl_own == 0) {                                   // the tile's first fine row: the first child of its first parent (Z-order)
      int m = a.n;
#pragma unroll
      for (int q = 0; q < 4; ++q) if (v[q] >= 0 && v[q] < m) m = v[q];
      S.f0h[hf] = m;
    }
    unsigned long long bm[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bm[q] = __ballot(v[q] >= 0);
      if (lane == 0) S.ccnt[4 * hf + q][wave & 3] = __popcll(bm[q]);
    }
    lds_barrier();
    const int f0n = min(S.f0h[0], S.f0h[1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) conv1_place_class(S.ccnt[4 * hf + q], wave & 3, bm[q], v[q], f0n, pl_own, N.lrow[4 * hf + q], N.lpar[4 * hf + q]);
    if (tid < 8) N.ctot[tid] = S.ccnt[tid][0] + S.ccnt[tid][1] + S.ccnt[tid][2] + S.ccnt[tid][3];
    if (tid == 0) N.f0 = f0n;
    lds_barrier();
    tc = tn;
    nu_c = nu_n;
    if (tc >= n_tiles) break;
    tn += G;
    nu_n = nu_2;
#pragma unroll
    for (int i = 0; i < NS; ++i) un[i] = un2[i];
  }
  if (a.out_split) split16_report(a.range, mx);
}

// Of the class compaction of a tile's parents only the placement (conv1_place_class) is shared: the ballots and counts around it run
// over one workgroup of eight classes behind __syncthreads in conv1_bf_kernel, over two half-workgroups of four classes each between
// the two lds_barriers in conv1_bfp_kernel, with the first fine row reduced over both halves - a common form would shorten neither.

namespace {

size_t conv1_tree_lds(const Conv1Args& a) { return (size_t)a.ks * a.ks * a.ks * a.cin * (a.cout + 4) * sizeof(float); }

// the two templated kernels' instances: f(std::integral_constant<int, C_out>)
template <class F>
int conv1_for_cout(int cout, F&& f) {
  switch (cout) {
    case 32: f(std::integral_constant<int, 32>{}); return EYOC_OK;
    case 64: f(std::integral_constant<int, 64>{}); return EYOC_OK;
    case 128: f(std::integral_constant<int, 128>{}); return EYOC_OK;
    default: set_error("conv1: C_out %d not in {32,64,128}", cout); return EYOC_ERR_INVALID;
  }
}

// conv1_bfp_kernel's grid limit - one workgroup per compute unit - and its dynamic-LDS attribute: asked for once per ctx (every
// time without one)
int conv1_bfp_setup(const eyoc_ctx* cctx, int* cus) {
  eyoc_ctx* ctx = const_cast<eyoc_ctx*>(cctx);
  *cus = ctx ? ctx->n_cus : 0;
  if (*cus <= 0) {
    int dev = 0;
    EYOC_CHECK_HIP(hipGetDevice(&dev));
    EYOC_CHECK_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    EYOC_REQUIRE(*cus > 0, EYOC_ERR_INVALID, "conv1: device reports %d compute units", *cus);
    if (ctx) ctx->n_cus = *cus;
  }
  if (!ctx || !ctx->conv1p_attr_set) {
    EYOC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv1_bfp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Conv1Shared)));
    if (ctx) ctx->conv1p_attr_set = true;
  }
  return EYOC_OK;
}

}  // namespace

// Which kernel takes the layer: a pure function of the arguments and the ctx's switches, for the launcher below and for
// eyoc_model_forward, which builds the level-0 hash table only for Probe.
Conv1Path conv1_path(const Conv1Args& a) {
  // the octree walk in any form: links present, a window inside the 27 coarse blocks, the walker's padded weights within 64 KB of LDS
  if (!(a.parent && a.children && a.s1c && (a.ks == 3 || a.ks == 5) && conv1_tree_lds(a) <= 64 * 1024)) return Conv1Path::Probe;
  // C_in = 1, 32 output channels, split16 activations downstream (the large-batch path): the MFMA formulation.  Its
  // products carry 22-bit significands like every split16 layer; fp32 consumers keep the exact-fp32 walker
  const int knob = knobs_of(a.ctx).conv1_kernel;
  if (!(knob != 2 && a.cin == 1 && a.cout == 32 && a.out_split && a.ks * a.ks * a.ks < 128 && !a.in_perm)) return Conv1Path::Tree;
  if (a.local1 && knob == 3) return Conv1Path::Bfp;      // Z-ordered maps: block vectors from persistent workgroups, one per CU
  if (a.local1 && knob == 1) return Conv1Path::Bf;       // ... staged per 256-parent tile
  return Conv1Path::Mfma;
}

int launch_conv1(const Conv1Args& a, hipStream_t st) {
  EYOC_REQUIRE(a.ks == 1 || a.ks == 3 || a.ks == 5 || a.ks == 7, EYOC_ERR_INVALID, "conv1: kernel size %d", a.ks);
  EYOC_REQUIRE(a.cin >= 1 && a.cin * a.cout <= 8192, EYOC_ERR_INVALID, "conv1: C_in %d x C_out %d too large", a.cin, a.cout);
  EYOC_REQUIRE(a.ld_out % 4 == 0, EYOC_ERR_INVALID, "conv1: ld_out must be a multiple of 4");
  if (a.n == 0) return EYOC_OK;
  const dim3 grid(cdiv(a.n, 256));
  int rc = EYOC_OK;
  switch (conv1_path(a)) {
    case Conv1Path::Probe:
      rc = conv1_for_cout(a.cout, [&](auto c) { hipLaunchKernelGGL((conv1_kernel<decltype(c)::value>), grid, dim3(256), 0, st, a); });
      break;
    case Conv1Path::Tree:
      rc = conv1_for_cout(a.cout, [&](auto c) { hipLaunchKernelGGL((conv1_tree_kernel<decltype(c)::value>), grid, dim3(256), conv1_tree_lds(a), st, a); });
      break;
    case Conv1Path::Mfma: {
      const int wgs = cdiv(a.n, 64);
      hipLaunchKernelGGL(conv1_mfma_kernel, dim3(wgs < 2560 ? wgs : 2560), dim3(256), 0, st, a);   // 10 workgroups per CU, persistent
      break;
    }
    case Conv1Path::Bf:
      hipLaunchKernelGGL(conv1_bf_kernel, dim3(cdiv(a.nc, ST_TILE)), dim3(256), 0, st, a);
      break;
    case Conv1Path::Bfp: {
      int cus = 0;
      if ((rc = conv1_bfp_setup(a.ctx, &cus))) break;
      const int n_tiles = cdiv(a.nc, ST_TILE), want = knobs_of(a.ctx).conv1_workgroups > 0 ? knobs_of(a.ctx).conv1_workgroups : cus;
      hipLaunchKernelGGL(conv1_bfp_kernel, dim3(n_tiles < want ? n_tiles : want), dim3(512), sizeof(Conv1Shared), st, a, n_tiles);
      break;
    }
  }
  if (rc) return rc;
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // namespace eyoc
