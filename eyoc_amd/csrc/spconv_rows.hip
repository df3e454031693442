// A stride-1 3x3x3 SPLIT16 layer for a LIST of output rows (gfx950): the last decoder layer of a forward whose caller reads only a
// sample of the rows (eyoc_model_forward_rows: registration matches 5000 rows per cloud, a sixth of the batch).
//
// The staged kernel (spconv_st.hip) earns its stage because the 256 rows of a tile share their neighbours; sampled rows share
// almost none, so here every input row goes straight from memory into the MFMA operand registers.  What is kept is the ORDER in
// which the staged kernel sums a row's products - the result is the full layer's, bit for bit:
//
//   for pass in 0 .. n_pass-1:            (a neighbour belongs to the pass the row's TILE RECORD stages it in)
//     for qb in 0 .. cin/32-1:
//       for k in 0 .. 26:
//         acc = mfma(W_hi, X_hi, acc); acc = mfma(W_hi, X_lo, acc); acc = mfma(W_lo, X_hi, acc)
//
// with a zero operand wherever a row has no neighbour at (pass, k): an accumulator that starts at +0 never becomes -0, so zero
// products - and skipped blocks of them - leave it as it is.  That is also why a 16-row chunk may mix rows of one-pass and of
// two-pass tiles: the wave runs the second pass when any of its rows has a neighbour there.
//
// A wave takes 64 rows x 64 output channels (4 chunks x 4 channel tiles: every weight fragment, 442 KB per layer from L2, serves
// four chunks).  Lane l first looks up the 27 neighbours of row l in its tile record (inv -> slot -> entry -> U, as
// conv1_bf_kernel does) and leaves them in LDS; then lane (g, j) gathers, per offset, pieces g of the hi and of the lo halves of
// the four rows 16 c + j.  Missing neighbours read a row of zeros, so the loads are unconditional and one offset ahead.
#include "spconv.h"

using namespace eyoc;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RW = 4;                  // waves per workgroup, 64 rows each (independent: no barrier)
constexpr int PASS_BIT = 28;           // neighbour word: input row (< 2^24) | pass << 28; -1 = none

struct RowsArgs {
  SpconvArgs a;
  const unsigned char* local;          // the level's 256-row tile records
  const int32_t* rows;                 // [n_rows] internal output rows
  int n_rows;
  const float* skip;                   // SPLIT16 rows whose first block is copied behind the layer's channels
  int ld_skip;
  float* out;                          // [n_rows, cout + 32] SPLIT16 rows
  const float* zero;                   // 256 bytes of zeros
  unsigned int* pairs;                 // += (row, offset) pairs multiplied
};

__global__ __launch_bounds__(RW * 64, 2) void spconv_rows_kernel(RowsArgs ra) {
  const SpconvArgs& a = ra.a;
  __shared__ __attribute__((aligned(16))) int nb[RW][27][64];            // [k][4 j + c]: neighbour word of row 16 c + j
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int base = ((int)blockIdx.x * RW + wave) * 64;
  if (base >= ra.n_rows) return;

  // ---- neighbours of row `lane` from its tile record
  const int mine = base + lane;
  const int r = mine < ra.n_rows ? ra.rows[mine] : -1;
  int cnt = 0;
  bool second = false;
  {
    const unsigned char* lr = ra.local + (size_t)(r >= 0 ? r >> 8 : 0) * ST_LR_BYTES;
    const int n_u = reinterpret_cast<const int*>(lr)[0];
    const int* U = reinterpret_cast<const int*>(lr + 16);
    const unsigned short* loc = reinterpret_cast<const unsigned short*>(lr + ST_LOC_OFF);
    const int sl = lr[ST_INV_OFF + (r >= 0 ? r & 255 : 0)];
    const int ew = (sl >> 6) * 16 + (sl & 15), ec = (sl >> 4) & 3;
    const bool two = n_u > ST_UMAX;
    int e0[27], e1[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      e0[k] = loc[(k * 64 + ew) * 4 + ec] >> 6;                          // entry = 64 l + swizzle
      e1[k] = two ? loc[((27 + k) * 64 + ew) * 4 + ec] >> 6 : ST_UMAX;    // (a one-pass tile's second block is not written)
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      int v = -1;
      if (r >= 0 && n_u >= 0) {
        if (e0[k] < ST_UMAX) v = U[e0[k]];
        else if (e1[k] < ST_UMAX) v = U[ST_UMAX + e1[k]] | (1 << PASS_BIT);
      }
      nb[wave][k][4 * j + g] = v;                                        // this lane's row is row j of chunk g
      cnt += v >= 0;
      second |= v >= (1 << PASS_BIT);
    }
  }
  const int n_pass = __ballot(second) != 0ull ? 2 : 1;                   // wave-uniform
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane == 0 && ra.pairs) atomicAdd(ra.pairs, (unsigned)cnt);
  __builtin_amdgcn_s_waitcnt(0xc07f);                                    // lgkmcnt(0): the wave's own LDS writes (no other wave reads them)
  __builtin_amdgcn_wave_barrier();

  // ---- weights: the packing launch_spconv_st reads (CT = 64 = one slice; CC input channels per item)
  const int CC = a.cin % 64 == 0 ? 64 : 32 /* spconv_cc */, JQ = CC / 16, ncc = a.cin / CC, tile4 = CC * 64 / 4;
  const int nqb = a.cin / 32, n_steps = nqb * 27;
  const char* wb = reinterpret_cast<const char*>(a.w) + lane * 16;
  const char* inb = reinterpret_cast<const char*>(a.in) + g * 16;
  const char* zb = reinterpret_cast<const char*>(ra.zero) + g * 16;
  const size_t row_bytes = (size_t)a.ld_in * 4;

  f32x4 acc[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // operands and weight fragments of step s = 27 qb + k of `pass`; -> whether any row of the wave has a neighbour there
  auto load = [&](int pass, int s, half8_t (&X)[4][2], half8_t (&W)[4][2]) -> bool {
    const int qb = s / 27, k = s - qb * 27;
    const int4 nv = *reinterpret_cast<const int4*>(&nb[wave][k][4 * j]);
    const int v[4] = {nv.x, nv.y, nv.z, nv.w};
    bool any = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool has = v[c] >= 0 && (v[c] >> PASS_BIT) == pass;
      any |= has;
      const char* p = has ? inb + (size_t)(v[c] & ((1 << PASS_BIT) - 1)) * row_bytes + qb * 128 : zb;
      X[c][0] = *reinterpret_cast<const half8_t*>(p);
      X[c][1] = *reinterpret_cast<const half8_t*>(p + SPLIT16_LO);
    }
    const int cc = (qb * 32) / CC, qp = ((qb * 32) % CC) / 32;
    const char* wp = wb + ((size_t)((k * ncc + cc) * tile4) + 2 * qp * 64) * 16;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int p = 0; p < 2; ++p) W[t][p] = *reinterpret_cast<const half8_t*>(wp + (t * JQ + p) * 1024);
    return __ballot(any) != 0ull;
  };
  auto multiply = [&](const half8_t (&X)[4][2], const half8_t (&W)[4][2]) {
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W[t][term == 2 ? 1 : 0], X[c][term == 1 ? 1 : 0], acc[c][t], 0, 0, 0);
  };

  half8_t XA[4][2], XB[4][2], WA[4][2], WB[4][2];
  for (int pass = 0; pass < n_pass; ++pass) {
    bool anyA = load(pass, 0, XA, WA), anyB = false;
    for (int s = 0; s < n_steps; s += 2) {                               // n_steps = 27 * cin / 32; an odd count ends on set A
      if (s + 1 < n_steps) anyB = load(pass, s + 1, XB, WB);
      if (anyA) multiply(XA, WA);
      if (s + 1 >= n_steps) break;
      if (s + 2 < n_steps) anyA = load(pass, s + 2, XA, WA);
      if (anyB) multiply(XB, WB);
    }
  }

  // ---- epilogue (spconv_st_kernel's): lane (g, j) holds channels 16 t + 4 g .. + 3 of row 16 c + j
  const float os = a.out_scale ? *a.out_scale : 1.0f;
  float4 b4[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) b4[t] = a.bias ? *reinterpret_cast<const float4*>(a.bias + 16 * t + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
  float mx = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int i = base + 16 * c + j;
    if (i >= ra.n_rows) continue;
    const int o = ra.rows[i];
    float* dst = ra.out + (size_t)i * (a.cout + 32);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ch = 16 * t + 4 * g;
      float4 v = make_float4(acc[c][t][0] * os + b4[t].x, acc[c][t][1] * os + b4[t].y, acc[c][t][2] * os + b4[t].z,
                             acc[c][t][3] * os + b4[t].w);
      if (a.res) {
        const float4 q = split16_load4(a.res + (size_t)o * a.ld_res, ch);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
      }
      if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      split16_track(mx, v);
      split16_store4(dst, ch, v);
    }
    // the row's 32 skip channels, byte for byte: pieces g and 4 + g of their 128-byte block
    const uint4* sp = reinterpret_cast<const uint4*>(ra.skip + (size_t)o * ra.ld_skip);
    uint4* dp = reinterpret_cast<uint4*>(dst + a.cout);
    dp[g] = sp[g];
    dp[4 + g] = sp[4 + g];
  }
  split16_report(a.range, mx);
}

// inv[row_perm[i]] = i
__global__ __launch_bounds__(256) void k_invert_perm(const int32_t* __restrict__ perm, int n, int32_t* __restrict__ inv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) inv[perm[i]] = i;
}

// the caller's row numbers -> internal rows (a number outside [0, n) is clamped into it: the gathers stay inside the tensors);
// block 0 also clears the row of zeros
__global__ __launch_bounds__(256) void k_rows_internal(const long long* __restrict__ rows, int n_rows, const int32_t* __restrict__ inv, int n,
                                                       int32_t* __restrict__ out, float* __restrict__ zero) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 64) zero[threadIdx.x] = 0.f;
  if (i >= n_rows) return;
  long long r = rows[i];
  r = r < 0 ? 0 : r >= n ? n - 1 : r;
  out[i] = inv ? inv[r] : (int32_t)r;
}

// out[i, :] = in[rows[i], :] (the fallback of eyoc_model_forward_rows: the full forward's rows); c % 4 == 0
__global__ __launch_bounds__(256) void k_take_rows(const float* __restrict__ in, int n, int c4, const long long* __restrict__ rows, int n_rows,
                                                   float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = t / c4;
  const int q = (int)(t % c4);
  if (i >= n_rows) return;
  long long r = rows[i];
  r = r < 0 ? 0 : r >= n ? n - 1 : r;
  reinterpret_cast<float4*>(out)[i * c4 + q] = reinterpret_cast<const float4*>(in)[r * c4 + q];
}

}  // namespace

namespace eyoc {

bool spconv_rows_supported(const SpconvArgs& a) {
  return a.math == 1 && a.K == 27 && a.cout == 64 && a.cin % 32 == 0 && a.ld_in % 32 == 0 && a.out_split && !a.l2norm && !a.out_perm &&
         a.n_in < (1 << 24) && (!a.res || a.ld_res % 32 == 0);
}

size_t spconv_rows_scratch_bytes(int n_level_rows, int n_rows) {
  return align_up((size_t)n_level_rows * 4) + align_up((size_t)n_rows * 4) + 256;
}

int launch_spconv_rows(const SpconvArgs& a, const unsigned char* local_dev, const int32_t* row_perm, const int64_t* rows_dev, int n_rows,
                       const float* skip, int ld_skip, float* out, void* scratch, unsigned int* pairs, hipStream_t st) {
  EYOC_REQUIRE(spconv_rows_supported(a) && local_dev && rows_dev && skip && out && scratch && ld_skip % 32 == 0, EYOC_ERR_INVALID,
               "spconv_rows: unsupported layer");
  if (n_rows <= 0) return EYOC_OK;
  Carver cv(scratch, spconv_rows_scratch_bytes(a.n_out, n_rows));
  int32_t* inv = cv.take<int32_t>((size_t)a.n_out);
  int32_t* internal = cv.take<int32_t>((size_t)n_rows);
  float* zero = cv.take<float>(64);
  if (row_perm) hipLaunchKernelGGL(k_invert_perm, dim3(cdiv(a.n_out, 256)), dim3(256), 0, st, row_perm, a.n_out, inv);
  hipLaunchKernelGGL(k_rows_internal, dim3(cdiv(n_rows, 256)), dim3(256), 0, st, (const long long*)rows_dev, n_rows,
                     row_perm ? inv : (const int32_t*)nullptr, a.n_out, internal, zero);
  RowsArgs ra{a, local_dev, internal, n_rows, skip, ld_skip, out, zero, pairs};
  hipLaunchKernelGGL(spconv_rows_kernel, dim3(cdiv(n_rows, RW * 64)), dim3(RW * 64), 0, st, ra);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int launch_take_rows(const float* in, int n, int c, const int64_t* rows_dev, int n_rows, float* out, hipStream_t st) {
  EYOC_REQUIRE(in && rows_dev && out && c % 4 == 0 && n > 0, EYOC_ERR_INVALID, "take_rows: bad argument");
  if (n_rows <= 0) return EYOC_OK;
  hipLaunchKernelGGL(k_take_rows, dim3(cdiv((long long)n_rows * (c / 4), 256)), dim3(256), 0, st, in, n, c / 4, (const long long*)rows_dev,
                     n_rows, out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // namespace eyoc
