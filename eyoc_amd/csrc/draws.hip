// Device-side draws of the training losses: a counter-based generator (Philox4x32-10) and the two draw primitives the reference's
// trainers use - np.random.choice(n, k, replace=False) (lib/trainer.py:445-449, :715-719, :754-760, :946-955) and
// floor(rand(N, 2) * [n0, n1]) (lib/trainer.py:212-218).  include/eyoc_hip.h has the layout of counter and key and the contract.
//
// Every number is a pure function of (seed, call, slot, index): no device state, no atomics, no dependence on the launch geometry.
// Plain streaming kernels: one element per lane, 64-bit results written with ordinary (vector) stores.  The 20 32 x 32 -> 64
// multiplies per element are nothing at a few hundred thousand elements; the radix sort of the subset draw is the cost.
#include "common.h"

namespace eyoc {

constexpr int DRAW_THREADS = 256;
constexpr int DRAW_SLOTS = EYOC_DRAW_MAX_SLOTS;
constexpr unsigned long long DRAW_CALL_LIMIT = 1ull << 60;

struct Philox4 {
  unsigned int x[4];
};

// Philox4x32-10 (Salmon et al., SC'11) from its definition; host and device run the same integer arithmetic
__host__ __device__ inline Philox4 philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0,
                                                 unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned int)p1;
    c3 = (unsigned int)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the counter / key layout of include/eyoc_hip.h
__host__ __device__ inline Philox4 draw_words(unsigned long long seed, unsigned long long call, int slot, unsigned long long index) {
  return philox4x32_10((unsigned int)index, (unsigned int)(index >> 32), (unsigned int)call,
                       (unsigned int)(call >> 32) | ((unsigned int)slot << 28), (unsigned int)seed, (unsigned int)(seed >> 32));
}

struct DrawSlots {
  int n_off[DRAW_SLOTS + 1];   // slot s owns elements [n_off[s], n_off[s + 1]) of the key list (empty for a slot that draws nothing)
  int k_off[DRAW_SLOTS + 1];   // ... and [k_off[s], k_off[s + 1]) of the output
};

struct DrawWs {
  unsigned long long *key, *key_s;
  int *val, *val_s;
  void* sort_tmp;
  size_t sort_bytes, total;
};

static DrawWs draw_carve(void* base, size_t bytes, int total_n) {
  DrawWs w;
  Carver cv(base, bytes);
  const size_t n = (size_t)total_n;
  w.key = cv.take<unsigned long long>(n);
  w.key_s = cv.take<unsigned long long>(n);
  w.val = cv.take<int>(n);
  w.val_s = cv.take<int>(n);
  w.sort_bytes = align_up(sort_rows64_tmp_bytes(total_n));
  w.sort_tmp = cv.take<char>(w.sort_bytes);
  w.total = align_up(cv.off);
  return w;
}

// element e of the key list: (slot << 61) | 61 generator bits, value = the element's index inside its slot
__global__ __launch_bounds__(DRAW_THREADS) void draw_keys_kernel(unsigned long long seed, unsigned long long call, DrawSlots s, int total,
                                                                 unsigned long long* __restrict__ key, int* __restrict__ val) {
  const long long e = (long long)blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (e >= total) return;
  int slot = 0;
#pragma unroll
  for (int t = 1; t < DRAW_SLOTS; ++t) slot += (e >= s.n_off[t]) ? 1 : 0;
  const int i = (int)e - s.n_off[slot];
  const Philox4 r = draw_words(seed, call, slot, (unsigned long long)i);
  const unsigned long long x = ((unsigned long long)r.x[1] << 32) | r.x[0];
  key[e] = ((unsigned long long)slot << 61) | (x >> 3);
  val[e] = i;
}

// output j: the first k values of every slot's sorted run, back to back
__global__ __launch_bounds__(DRAW_THREADS) void draw_take_kernel(DrawSlots s, int total_k, const int* __restrict__ val_s,
                                                                 long long* __restrict__ out) {
  const long long j = (long long)blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (j >= total_k) return;
  int slot = 0;
#pragma unroll
  for (int t = 1; t < DRAW_SLOTS; ++t) slot += (j >= s.k_off[t]) ? 1 : 0;
  out[j] = (long long)val_s[s.n_off[slot] + ((int)j - s.k_off[slot])];
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_pairs_kernel(unsigned long long seed, unsigned long long call, int slot, int n_rows,
                                                                  unsigned long long n0, unsigned long long n1,
                                                                  long long* __restrict__ out) {
  const long long r = (long long)blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (r >= n_rows) return;
  const Philox4 w = draw_words(seed, call, slot, (unsigned long long)r);
  const unsigned long long x0 = ((unsigned long long)w.x[1] << 32) | w.x[0], x1 = ((unsigned long long)w.x[3] << 32) | w.x[2];
  out[2 * r] = (long long)__umul64hi(x0, n0);
  out[2 * r + 1] = (long long)__umul64hi(x1, n1);
}

}  // namespace eyoc

using namespace eyoc;

extern "C" {

size_t eyoc_draw_workspace_bytes(int total_n) {
  if (total_n <= 0) return 0;
  return draw_carve(nullptr, 0, total_n).total;
}

int eyoc_draw_subsets(eyoc_ctx* ctx, uint64_t seed, uint64_t call, int n_slots, const int* n, const int* k, int64_t* out_idx, void* ws,
                      size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx, EYOC_ERR_INVALID, "eyoc_draw_subsets: NULL ctx");
  EYOC_REQUIRE(n_slots >= 0 && n_slots <= DRAW_SLOTS, EYOC_ERR_INVALID, "eyoc_draw_subsets: %d slots (0 .. %d)", n_slots, DRAW_SLOTS);
  EYOC_REQUIRE(n_slots == 0 || (n && k), EYOC_ERR_INVALID, "eyoc_draw_subsets: NULL size array");
  EYOC_REQUIRE(call < DRAW_CALL_LIMIT, EYOC_ERR_INVALID, "eyoc_draw_subsets: call number %llu is not below 2^60", (unsigned long long)call);
  DrawSlots s;
  long long total_n = 0, total_k = 0;
  for (int t = 0; t < DRAW_SLOTS; ++t) {
    s.n_off[t] = (int)total_n;
    s.k_off[t] = (int)total_k;
    if (t >= n_slots) continue;
    EYOC_REQUIRE(n[t] >= 0 && k[t] >= 0 && k[t] <= n[t], EYOC_ERR_INVALID, "eyoc_draw_subsets: slot %d draws %d of %d", t, k[t], n[t]);
    if (k[t] == 0) continue;                      // a slot that draws nothing puts no keys into the sort
    total_n += n[t];
    total_k += k[t];
    EYOC_REQUIRE(total_n <= 0x7FFFFFFFll, EYOC_ERR_INVALID, "eyoc_draw_subsets: more than 2^31 - 1 elements in one call");
  }
  s.n_off[DRAW_SLOTS] = (int)total_n;
  s.k_off[DRAW_SLOTS] = (int)total_k;
  if (total_k == 0) return EYOC_OK;
  EYOC_REQUIRE(out_idx && ws, EYOC_ERR_INVALID, "eyoc_draw_subsets: NULL output or workspace");
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "eyoc_draw_subsets: workspace must be 256-byte aligned");
  const DrawWs w = draw_carve(ws, ws_bytes, (int)total_n);
  EYOC_REQUIRE(w.total <= ws_bytes, EYOC_ERR_WORKSPACE, "eyoc_draw_subsets: workspace %zu < %zu bytes", ws_bytes, w.total);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(draw_keys_kernel, dim3(cdiv(total_n, DRAW_THREADS)), dim3(DRAW_THREADS), 0, st, (unsigned long long)seed,
                     (unsigned long long)call, s, (int)total_n, w.key, w.val);
  // all 64 bits: the slot number on top keeps every slot's run together and in slot order; equal keys keep their index order
  if (int rc = sort_rows_by_key64(w.sort_tmp, w.sort_bytes, w.key, w.key_s, w.val, w.val_s, (int)total_n, 64, st)) return rc;
  hipLaunchKernelGGL(draw_take_kernel, dim3(cdiv(total_k, DRAW_THREADS)), dim3(DRAW_THREADS), 0, st, s, (int)total_k, (const int*)w.val_s,
                     (long long*)out_idx);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

int eyoc_draw_pairs(eyoc_ctx* ctx, uint64_t seed, uint64_t call, int slot, int n_rows, int n0, int n1, int64_t* out, void* stream) {
  EYOC_REQUIRE(ctx, EYOC_ERR_INVALID, "eyoc_draw_pairs: NULL ctx");
  EYOC_REQUIRE(slot >= 0 && slot < DRAW_SLOTS, EYOC_ERR_INVALID, "eyoc_draw_pairs: slot %d (0 .. %d)", slot, DRAW_SLOTS - 1);
  EYOC_REQUIRE(call < DRAW_CALL_LIMIT, EYOC_ERR_INVALID, "eyoc_draw_pairs: call number %llu is not below 2^60", (unsigned long long)call);
  EYOC_REQUIRE(n_rows >= 0 && n0 >= 0 && n1 >= 0, EYOC_ERR_INVALID, "eyoc_draw_pairs: negative size");
  if (n_rows == 0) return EYOC_OK;
  EYOC_REQUIRE(n0 > 0 && n1 > 0, EYOC_ERR_INVALID, "eyoc_draw_pairs: %d pairs from %d x %d rows", n_rows, n0, n1);
  EYOC_REQUIRE(out, EYOC_ERR_INVALID, "eyoc_draw_pairs: NULL output");
  hipLaunchKernelGGL(draw_pairs_kernel, dim3(cdiv(n_rows, DRAW_THREADS)), dim3(DRAW_THREADS), 0, (hipStream_t)stream,
                     (unsigned long long)seed, (unsigned long long)call, slot, n_rows, (unsigned long long)n0, (unsigned long long)n1,
                     (long long*)out);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

}  // extern "C"
