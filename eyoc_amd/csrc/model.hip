// ResUNet2 family (ResUNetBN2C in production): weight packing and the forward schedule.
// Mirrors ResUNet2.__init__/forward (model/resunet.py:18-193) and BasicBlockBase.forward
// (model/residual_block.py:37-53) with every batch norm folded into the convolution before it
// (eval mode, model/common.py:4-6) and every ReLU / residual add / concat fused into a conv epilogue.
// The ResUNetIN2 family (model/resunet.py:229-251; eyoc_model_create_in, block_norm 1) keeps the stage norms folded; inside the residual
// blocks (model/residual_block.py:60-61) every convolution writes its raw sums and the instance norm behind it is a layer of its own
// (M_INORM: statistics per instance and channel, then normalise + weight / bias [+ residual] + ReLU in place - inorm.hip), on the plan's
// own row formats (fp32 / SPLIT16): 37 layers instead of 23, no new activation buffer.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "spconv.h"

using namespace eyoc;

namespace {

enum MapSel { M_CONV1, M_S1, M_DOWN, M_UP, M_IDENT, M_AFFINE, M_INORM };   // M_AFFINE: a batch norm that stands alone (ResUNetExpanded's norm<i>_2): y = x * scale + shift per channel
// M_INORM: an instance norm (the blocks of the ResUNetIN2 family, model/residual_block.py:60-61): its statistics belong to the input, so it
// folds into nothing - one layer behind the raw convolution, in place, with the block's ReLU / residual (inorm.hip launch_in_layer)
constexpr float IN_EPS = 1e-8f;      // MinkowskiInstanceNorm's (model/common.py:7-8)

struct LayerPlan {
  std::string name;      // conv name in the state_dict ("block2.conv1")
  std::string norm;      // norm folded into it ("" = none)
  int K, cin, cout;
  MapSel map;
  int level;             // table level (fine level for DOWN/UP); rows of the OUTPUT for S1
  int out_level;         // level whose row count is n_out
  int in_buf, in_col, out_buf, out_col, res_buf;  // buffer ids (-1 none)
  int relu, l2norm, has_bias;
  size_t w_off = 0, b_off = 0;  // float offsets into the blob
  size_t w16_off = 0, s_off = 0;  // SPLIT16 copy of the weights (same size) and the layer's out_scale scalar (spconv layers only)
};

// activation buffers
enum Buf { B_IN = 0, B_X1, B_T1, B_CAT1, B_X2, B_T2, B_CAT2, B_X4, B_T4, B_CAT4, B_X8, B_T8, B_Y8, B_D4, B_DT4, B_D2,
           B_DT2, B_D1, B_DT1, B_H,
           B_U1, B_U2, B_U4, B_U8, B_UD4, B_UD2, B_UD1,    // ResUNetExpanded only (width 0 otherwise): the first block's output of a stage
           B_OUT, B_COUNT };

struct BufPlan { int level, width; };

size_t pad64(size_t v) { return (v + 63) / 64 * 64; }
bool is_norm_layer(MapSel m) { return m == M_AFFINE || m == M_INORM; }   // no products: per-channel parameters at w_off / b_off only

}  // namespace

struct eyoc_model {
  eyoc_model_desc desc;
  int block_norm = 0;      // 0: batch norm inside the residual blocks (folded), 1: instance norm (M_INORM layers); eyoc_model_create_in
  std::vector<LayerPlan> layers;
  BufPlan bufs[B_COUNT];
  float* blob = nullptr;
  size_t blob_floats = 0;
  int math = -1;           // -1 automatic, 0 fp32 MFMA, 1 SPLIT16 (eyoc_model_set_math)
  int timing = 0;
  std::vector<hipEvent_t> events;     // two sets of layers + 1 events (eyoc_model_timing_slot)
  int slot = 0;
  hipEvent_t progress_event = nullptr;   // eyoc_model_set_progress_event: recorded in front of layer `progress_layer` of every forward
  int progress_layer = -1;
  unsigned int* range = nullptr;      // device: {overflow flag of the forward in flight, max |activation| bits (probe), probe switch, sticky overflow flag} - split16_guard in spconv.h
  int probe = 0;
  // What a forward leaves behind in its (const) model - forward_impl is the one writer.  math: what the last forward used;
  // eyoc_model_forward_rows: it computed its last 3^3 layer (index sampled_layer) and the 1x1 tail for sampled_rows listed rows only
  // (-1: it was a full forward), range word 6 holds the (row, offset) pairs that layer multiplied; events_valid: a timed forward
  // has recorded into that event set
  struct Last { int math = 0, sampled_layer = -1, sampled_rows = 0, events_valid[2] = {0, 0}; } last;
};

namespace {

void build_plan(const eyoc_model_desc& d, int block_norm, std::vector<LayerPlan>& L, BufPlan* bufs) {
  const int* C = d.channels;
  const int* T = d.tr_channels;
  const int K1 = d.conv1_kernel_size * d.conv1_kernel_size * d.conv1_kernel_size;
  bufs[B_IN] = {0, d.in_channels};
  bufs[B_X1] = {0, C[1]}; bufs[B_T1] = {0, C[1]}; bufs[B_CAT1] = {0, T[2] + C[1]};
  bufs[B_X2] = {1, C[2]}; bufs[B_T2] = {1, C[2]}; bufs[B_CAT2] = {1, T[3] + C[2]};
  bufs[B_X4] = {2, C[3]}; bufs[B_T4] = {2, C[3]}; bufs[B_CAT4] = {2, T[4] + C[3]};
  bufs[B_X8] = {3, C[4]}; bufs[B_T8] = {3, C[4]}; bufs[B_Y8] = {3, C[4]};
  bufs[B_D4] = {2, T[4]}; bufs[B_DT4] = {2, T[4]};
  bufs[B_D2] = {1, T[3]}; bufs[B_DT2] = {1, T[3]};
  bufs[B_D1] = {0, T[2]}; bufs[B_DT1] = {0, T[2]};
  bufs[B_H] = {0, T[1]};
  bufs[B_OUT] = {0, d.out_channels};
  const int ex = d.expanded ? 1 : 0;
  bufs[B_U1] = {0, ex * C[1]}; bufs[B_U2] = {1, ex * C[2]}; bufs[B_U4] = {2, ex * C[3]}; bufs[B_U8] = {3, ex * C[4]};
  bufs[B_UD4] = {2, ex * T[4]}; bufs[B_UD2] = {1, ex * T[3]}; bufs[B_UD1] = {0, ex * T[2]};

  auto conv = [&](const char* name, const char* norm, int K, int cin, int cout, MapSel map, int level, int out_level,
                  int in_buf, int in_col, int out_buf, int out_col, int res_buf, int relu) {
    LayerPlan p;
    p.name = name; p.norm = norm; p.K = K; p.cin = cin; p.cout = cout; p.map = map; p.level = level;
    p.out_level = out_level; p.in_buf = in_buf; p.in_col = in_col; p.out_buf = out_buf; p.out_col = out_col;
    p.res_buf = res_buf; p.relu = relu; p.l2norm = 0; p.has_bias = 0;
    L.push_back(p);
  };
  auto block1 = [&](const std::string& name, int c, int level, int x_buf, int t_buf, int out_buf, int out_col) {
    if (block_norm == 1) {
      // BasicBlockIN: the convolution writes its raw sums (scale 1, shift 0), the norm runs in place behind it - conv1 -> t, norm1 + ReLU
      // on t; conv2 -> the block's destination (a column range of a concat buffer), norm2 + residual x + ReLU there.  No new buffer.
      conv((name + ".conv1").c_str(), "", 27, c, c, M_S1, level, level, x_buf, 0, t_buf, 0, -1, 0);
      conv((name + ".norm1").c_str(), (name + ".norm1").c_str(), 0, c, c, M_INORM, level, level, t_buf, 0, t_buf, 0, -1, 1);
      conv((name + ".conv2").c_str(), "", 27, c, c, M_S1, level, level, t_buf, 0, out_buf, out_col, -1, 0);
      conv((name + ".norm2").c_str(), (name + ".norm2").c_str(), 0, c, c, M_INORM, level, level, out_buf, out_col, out_buf, out_col, x_buf, 1);
      return;
    }
    conv((name + ".conv1").c_str(), (name + ".norm1").c_str(), 27, c, c, M_S1, level, level, x_buf, 0, t_buf, 0, -1, 1);
    conv((name + ".conv2").c_str(), (name + ".norm2").c_str(), 27, c, c, M_S1, level, level, t_buf, 0, out_buf, out_col,
         x_buf, 1);
  };
  // a stage's block(s): ResUNet2 runs block<i>; ResUNetExpanded (model/resunet.py:409-473) runs block<i> -> relu (the block's own
  // last ReLU already) -> norm<i>_2 -> block<i>_2.  The stand-alone norm cannot be folded into a neighbour: its shift reaches
  // block<i>_2.conv1 only through the neighbours a row HAS, and it is the residual of block<i>_2.conv2 - so it is one layer of its own
  // (x -> u by block<i>, u -> x by the norm: x is free once block<i>.conv2 has read it as its residual)
  auto block = [&](const std::string& stage, int c, int level, int x_buf, int t_buf, int u_buf, int out_buf, int out_col) {
    if (!d.expanded) { block1("block" + stage, c, level, x_buf, t_buf, out_buf, out_col); return; }
    block1("block" + stage, c, level, x_buf, t_buf, u_buf, 0);
    conv(("norm" + stage + "_2").c_str(), ("norm" + stage + "_2").c_str(), 0, c, c, M_AFFINE, level, level, u_buf, 0, x_buf, 0, -1, 0);
    block1("block" + stage + "_2", c, level, x_buf, t_buf, out_buf, out_col);
  };
  // encoder (model/resunet.py:143-161)
  conv("conv1", "norm1", K1, d.in_channels, C[1], M_CONV1, 0, 0, B_IN, 0, B_X1, 0, -1, 0);
  block("1", C[1], 0, B_X1, B_T1, B_U1, B_CAT1, T[2]);
  conv("conv2", "norm2", 27, C[1], C[2], M_DOWN, 0, 1, B_CAT1, T[2], B_X2, 0, -1, 0);
  block("2", C[2], 1, B_X2, B_T2, B_U2, B_CAT2, T[3]);
  conv("conv3", "norm3", 27, C[2], C[3], M_DOWN, 1, 2, B_CAT2, T[3], B_X4, 0, -1, 0);
  block("3", C[3], 2, B_X4, B_T4, B_U4, B_CAT4, T[4]);
  conv("conv4", "norm4", 27, C[3], C[4], M_DOWN, 2, 3, B_CAT4, T[4], B_X8, 0, -1, 0);
  block("4", C[4], 3, B_X8, B_T8, B_U8, B_Y8, 0);
  // decoder (model/resunet.py:163-186); ME.cat order is [decoder | skip]
  conv("conv4_tr", "norm4_tr", 27, C[4], T[4], M_UP, 2, 2, B_Y8, 0, B_D4, 0, -1, 0);
  block("4_tr", T[4], 2, B_D4, B_DT4, B_UD4, B_CAT4, 0);
  conv("conv3_tr", "norm3_tr", 27, C[3] + T[4], T[3], M_UP, 1, 1, B_CAT4, 0, B_D2, 0, -1, 0);
  block("3_tr", T[3], 1, B_D2, B_DT2, B_UD2, B_CAT2, 0);
  conv("conv2_tr", "norm2_tr", 27, C[2] + T[3], T[2], M_UP, 0, 0, B_CAT2, 0, B_D1, 0, -1, 0);
  block("2_tr", T[2], 0, B_D1, B_DT1, B_UD1, B_CAT1, 0);
  conv("conv1_tr", "", 1, C[1] + T[2], T[1], M_IDENT, 0, 0, B_CAT1, 0, B_H, 0, -1, 1);
  conv("final", "", 1, T[1], d.out_channels, M_IDENT, 0, 0, B_H, 0, B_OUT, 0, -1, 0);
  L.back().has_bias = 1;
  L.back().l2norm = d.normalize_feature ? 1 : 0;
  size_t off = 0;
  for (auto& p : L) {
    p.w_off = off;
    off += is_norm_layer(p.map) ? pad64((size_t)p.cout) : pad64((size_t)p.K * p.cin * p.cout);    // a stand-alone norm: its scale (an instance norm: its weight) per channel
    p.b_off = off;
    off += pad64((size_t)p.cout);
  }
  // second half of the blob: the SPLIT16 packing of every sparse-conv layer (spconv_wave.hip, MATH = 1)
  for (auto& p : L) {
    if (is_norm_layer(p.map)) continue;
    if (p.map != M_CONV1) {
      p.w16_off = off;
      off += pad64((size_t)p.K * p.cin * p.cout);
    }
    p.s_off = off;      // sparse-conv layers: out_scale; the first convolution: {2^sh, 2^-sh} of its MFMA kernels' weight halves
    off += 64;
  }
}

// y = x * scale[c] + shift[c] on fp32 or SPLIT16 rows (the format of its neighbours in the plan); one thread per 4 channels.  SPLIT16
// rows carry the range guard like every other kernel that writes them (spconv.h split16_guard)
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_affine(const float* __restrict__ in, int ld_in, int n, int c, const float* __restrict__ scale,
                                                const float* __restrict__ shift, float* __restrict__ out, int ld_out, unsigned int* range) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q4 = c / 4;
  const long long r = t / q4;
  const int ch = (int)(t % q4) * 4;
  float mx = 0.0f;
  if (r < n) {
    const float4 s = *reinterpret_cast<const float4*>(scale + ch), b = *reinterpret_cast<const float4*>(shift + ch);
    float4 v = SPLIT ? split16_load4(in + r * ld_in, ch) : *reinterpret_cast<const float4*>(in + r * ld_in + ch);
    v.x = fmaf(v.x, s.x, b.x); v.y = fmaf(v.y, s.y, b.y); v.z = fmaf(v.z, s.z, b.z); v.w = fmaf(v.w, s.w, b.w);
    if (SPLIT) { split16_track(mx, v); split16_store4(out + r * ld_out, ch, v); }
    else *reinterpret_cast<float4*>(out + r * ld_out + ch) = v;
  }
  if (SPLIT) {
    for (int o = 32; o; o >>= 1) mx = split16_merge(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) split16_report(range, mx);
  }
}

int launch_affine(const float* in, int ld_in, int n, int c, const float* scale, const float* shift, float* out, int ld_out, bool split,
                  unsigned int* range, hipStream_t st) {
  EYOC_REQUIRE(c % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && (!split || (c % 32 == 0 && ld_in % 32 == 0 && ld_out % 32 == 0)),
               EYOC_ERR_INVALID, "model: stand-alone norm over %d channels (rows of %d -> %d floats)", c, ld_in, ld_out);
  if (!n) return EYOC_OK;
  const dim3 grid((unsigned)cdiv((long long)n * (c / 4), 256));
  if (split) hipLaunchKernelGGL(k_affine<true>, grid, dim3(256), 0, st, in, ld_in, n, c, scale, shift, out, ld_out, range);
  else hipLaunchKernelGGL(k_affine<false>, grid, dim3(256), 0, st, in, ld_in, n, c, scale, shift, out, ld_out, range);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

size_t plan_blob_floats(const std::vector<LayerPlan>& L) {
  size_t end = 0;
  for (auto& p : L) {
    end = std::max(end, p.b_off + pad64(p.cout));
    if (!is_norm_layer(p.map)) end = std::max(end, p.s_off + 64);
  }
  return end;
}

const eyoc_layer_params* find_layer(const eyoc_layer_params* layers, int n, const std::string& name) {
  for (int i = 0; i < n; ++i)
    if (layers[i].name && name == layers[i].name) return &layers[i];
  return nullptr;
}

int check_desc(const eyoc_model_desc* d) {
  EYOC_REQUIRE(d, EYOC_ERR_INVALID, "model: NULL desc");
  EYOC_REQUIRE(d->in_channels >= 1 && d->in_channels <= 64, EYOC_ERR_INVALID, "model: in_channels %d", d->in_channels);
  EYOC_REQUIRE(d->expanded == 0 || d->expanded == 1, EYOC_ERR_INVALID, "model: expanded %d not in {0, 1}", d->expanded);
  EYOC_REQUIRE(d->out_channels == 32 || d->out_channels == 64 || d->out_channels == 128, EYOC_ERR_INVALID,
               "model: out_channels %d not in {32,64,128}", d->out_channels);
  EYOC_REQUIRE(d->conv1_kernel_size == 1 || d->conv1_kernel_size == 3 || d->conv1_kernel_size == 5 ||
               d->conv1_kernel_size == 7, EYOC_ERR_INVALID, "model: conv1_kernel_size %d", d->conv1_kernel_size);
  for (int i = 1; i <= 4; ++i) {
    const int c = d->channels[i], t = d->tr_channels[i];
    EYOC_REQUIRE(c == 32 || c == 64 || c == 128 || c == 256, EYOC_ERR_INVALID, "model: CHANNELS[%d] = %d", i, c);
    EYOC_REQUIRE(t == 32 || t == 64 || t == 128 || t == 256, EYOC_ERR_INVALID, "model: TR_CHANNELS[%d] = %d", i, t);
  }
  EYOC_REQUIRE(d->channels[1] <= 128, EYOC_ERR_INVALID, "model: CHANNELS[1] = %d > 128", d->channels[1]);
  return EYOC_OK;
}

int check_block_norm(const eyoc_model_desc* d, int block_norm) {
  EYOC_REQUIRE(block_norm == 0 || block_norm == 1, EYOC_ERR_INVALID, "model: block_norm %d not in {0 (batch norm), 1 (instance norm)}", block_norm);
  EYOC_REQUIRE(!(block_norm == 1 && d->expanded), EYOC_ERR_INVALID, "model: no instance-norm plan for the expanded network");
  return EYOC_OK;
}

// an instance norm's parameters as eyoc_layer_params carries them: weight and bias, no statistics
const eyoc_layer_params* find_inorm(const eyoc_layer_params* layers, int n, const LayerPlan& p) {
  const eyoc_layer_params* nm = find_layer(layers, n, p.norm);
  if (!(nm && nm->bn_weight && nm->bn_bias && !nm->bn_mean && !nm->bn_var && nm->cout == p.cout)) {
    set_error("eyoc_model_create: instance norm '%s' missing or wrong width (weight and bias of %d channels, no statistics)", p.norm.c_str(), p.cout);
    return nullptr;
  }
  return nm;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Device-side re-pack (eyoc_model_repack_device): the arithmetic of eyoc_model_pack_host, eyoc_spconv_pack_weights and
// eyoc_spconv_pack_weights_split16 restated as four launches over ALL layers of the plan - fold, fp32 pack + layer maximum, layer
// scales, split16 pack.  The blob must come out bit for bit as the host writes it, so every float operation below is the host's, in the
// host's order, unfused (the host is plain x86-64: no FMA), and a NaN an operation produces or passes on is the one SSE gives.
// Per-layer descriptors travel as kernel arguments (2.7 KB at most): nothing is uploaded, nothing allocated.
constexpr int RP_MAXL = 48;        // layers of the largest plan (expanded: 46)
constexpr int RP_CH = 256;         // channels of the widest layer (check_desc)

struct RpFoldLayer {
  const float *g, *b, *m, *v, *bias;   // the norm folded into the layer (all NULL: none), the convolution's bias (NULL: none)
  uint32_t b_off, w_off;               // float offsets into the blob: shifts; M_AFFINE's scales
  uint32_t cout, affine;               // affine 1: M_AFFINE (the folded scale goes to w_off); 2: M_INORM (weight -> w_off, bias -> b_off, as they are)
};
struct RpFoldArgs { RpFoldLayer L[RP_MAXL]; };

struct RpPackLayer {
  const float* kernel;                 // NULL: M_AFFINE (no weights)
  uint32_t w_off, w16_off, s_off;
  uint32_t K, cin, cout, conv1;
};
struct RpPackArgs {
  RpPackLayer L[RP_MAXL];
  uint32_t blk[RP_MAXL + 1];           // prefix of 256-thread blocks per layer: a block works inside one layer
  int n;
};

struct RpWs {                          // the workspace
  float scale[RP_MAXL][RP_CH];         // folded scale per layer and channel (1 for a layer without a norm)
  uint32_t maxbits[RP_MAXL];           // bits of max |w * scale| per layer (integer order = float order for non-negative floats)
  float up[RP_MAXL];                   // 2^sh of the split16 layers
};

// what SSE's mulss / subss / addss / divss return where the IEEE result r of (a op b) is a NaN: the first NaN operand, quieted, else
// the default NaN, which is NEGATIVE on x86 (the device's is positive).  (Two NaN operands: the host compiler chooses the order of a
// commutative operation's operands - such a product is not pinned.)
__device__ inline float rp_nan(float r, float a, float b) {
  if (r == r) return r;
  if (a != a) return __uint_as_float(__float_as_uint(a) | 0x00400000u);
  if (b != b) return __uint_as_float(__float_as_uint(b) | 0x00400000u);
  return __uint_as_float(0xffc00000u);
}

__device__ inline float rp_mul(float a, float b) {
#pragma clang fp contract(off)
  return rp_nan(a * b, a, b);
}

// float -> fp16 as the host's _Float16 conversion: round to nearest even, subnormals kept; a NaN keeps its sign and the top of its payload
__device__ inline uint16_t rp_half_bits(float v) {
  if (v != v) {
    const uint32_t u = __float_as_uint(v);
    return (uint16_t)(((u >> 16) & 0x8000u) | 0x7e00u | ((u >> 13) & 0x1ffu));
  }
  const _Float16 h = (_Float16)v;
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  return b;
}

__device__ inline float rp_half_float(uint16_t b) {
  _Float16 h;
  __builtin_memcpy(&h, &b, 2);
  return (float)h;
}

// wmax = f 2^e with f in [0.5, 1) (frexp) from the bits of a positive finite float
__device__ inline int rp_frexp_e(uint32_t bits) {
  const int E = (int)(bits >> 23);
  return E ? E - 126 : (31 - __clz((int)bits)) - 148;
}

__device__ inline float rp_pow2(int sh) { return __uint_as_float((uint32_t)(127 + sh) << 23); }   // sh in [-24, 24]

__device__ inline int rp_find_layer(const uint32_t* blk, int n, uint32_t b) {   // the layer li with blk[li] <= b < blk[li + 1]
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// one block per layer, one thread per channel: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ bias)
__global__ void __launch_bounds__(RP_CH) k_repack_fold(RpFoldArgs a, float eps, float* __restrict__ blob, RpWs* __restrict__ ws) {
#pragma clang fp contract(off)
  const int li = blockIdx.x, c = threadIdx.x;
  const RpFoldLayer& L = a.L[li];
  if (c == 0) ws->maxbits[li] = 0u;
  const int pc = (int)((L.cout + 63u) / 64u * 64u);
  if (c >= pc) return;
  float s = 1.0f, sh = 0.0f;
  if (c < (int)L.cout) {
    if (L.affine == 2) {
      s = L.g[c];
      sh = L.b[c];
    } else if (L.g) {
      const float var = L.v[c], g = L.g[c], mu = L.m[c], be = L.b[c];
      const float ve = rp_nan(var + eps, var, eps);
      float rt = sqrtf(ve);
      if (rt != rt) rt = ve != ve ? __uint_as_float(__float_as_uint(ve) | 0x00400000u) : __uint_as_float(0xffc00000u);
      s = rp_nan(g / rt, g, rt);
      const float ms = rp_mul(mu, s);
      sh = rp_nan(be - ms, be, ms);
    }
    if (L.bias) { const float bi = L.bias[c]; sh = rp_nan(sh + bi, sh, bi); }
  } else {
    s = 0.0f;                                                             // the blob's padding
  }
  blob[L.b_off + c] = sh;
  if (L.affine) blob[L.w_off + c] = s;
  else if (c < (int)L.cout) ws->scale[li][c] = s;
}

// the fp32 half: one thread per 16-byte fragment of eyoc_spconv_pack_weights' order (the first convolution: plain [K][cin][cout]),
// and the layer's max |w * scale| by integer atomicMax (a maximum does not depend on the order)
__global__ void __launch_bounds__(256) k_repack_f32(RpPackArgs a, float* __restrict__ blob, RpWs* __restrict__ ws) {
  __shared__ uint32_t wave_max[4];
  const int li = rp_find_layer(a.blk, a.n, blockIdx.x);
  const RpPackLayer& L = a.L[li];
  const uint32_t f = (blockIdx.x - a.blk[li]) * 256u + threadIdx.x;      // fragment of the layer
  const uint32_t elems = L.K * L.cin * L.cout;
  const float* __restrict__ sc = ws->scale[li];
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  bool live = false;
  if (L.conv1) {
    live = f < (elems + 63u) / 64u * 16u;                                  // with the padding behind the last float
    const uint32_t i = f * 4u;
    if (i + 0 < elems) o.x = rp_mul(L.kernel[i + 0], sc[(i + 0) % L.cout]);
    if (i + 1 < elems) o.y = rp_mul(L.kernel[i + 1], sc[(i + 1) % L.cout]);
    if (i + 2 < elems) o.z = rp_mul(L.kernel[i + 2], sc[(i + 2) % L.cout]);
    if (i + 3 < elems) o.w = rp_mul(L.kernel[i + 3], sc[(i + 3) % L.cout]);
  } else if (f < elems / 4u) {
    live = true;
    const uint32_t CT = L.cout >= 128u ? 128u : L.cout, CC = L.cin % 64u == 0u ? 64u : 32u;   // spconv_ct, spconv_cc
    const uint32_t NS = L.cout / CT, NCC = L.cin / CC, NT = CT / 16u, JQ = CC / 16u;
    const uint32_t lane = f & 63u;
    uint32_t r = f >> 6;
    const uint32_t jq = r % JQ; r /= JQ;
    const uint32_t nt = r % NT; r /= NT;
    const uint32_t cc = r % NCC; r /= NCC;
    const uint32_t s = r % NS, k = r / NS;
    const uint32_t ci = cc * CC + (jq * 4u + (lane >> 4)) * 4u, co = s * CT + nt * 16u + (lane & 15u);
    const float* __restrict__ w = L.kernel + ((size_t)k * L.cin + ci) * L.cout + co;
    const float scv = sc[co];
    o.x = rp_mul(w[0], scv);
    o.y = rp_mul(w[L.cout], scv);
    o.z = rp_mul(w[2 * (size_t)L.cout], scv);
    o.w = rp_mul(w[3 * (size_t)L.cout], scv);
  }
  if (live) *reinterpret_cast<float4*>(blob + L.w_off + (size_t)f * 4u) = o;
  // the first convolution counts finite values only, the split16 layers everything but NaN (inf included)
  const uint32_t lim = L.conv1 ? 0x7f7fffffu : 0x7f800000u;
  uint32_t mx = 0u;
  {
    const uint32_t b0 = __float_as_uint(o.x) & 0x7fffffffu, b1 = __float_as_uint(o.y) & 0x7fffffffu;
    const uint32_t b2 = __float_as_uint(o.z) & 0x7fffffffu, b3 = __float_as_uint(o.w) & 0x7fffffffu;
    if (b0 <= lim) mx = b0;
    if (b1 <= lim && b1 > mx) mx = b1;
    if (b2 <= lim && b2 > mx) mx = b2;
    if (b3 <= lim && b3 > mx) mx = b3;
  }
  for (int d = 32; d; d >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)mx, d); mx = t > mx ? t : mx; }
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
    if (mx) atomicMax(&ws->maxbits[li], mx);
  }
}

// one wave per layer: sh from the layer's maximum (the two host rules), the blob's 64 scale words, 2^sh for the split16 pack
__global__ void __launch_bounds__(64) k_repack_scales(RpPackArgs a, float* __restrict__ blob, RpWs* __restrict__ ws) {
  const int li = blockIdx.x, lane = threadIdx.x;
  const RpPackLayer& L = a.L[li];
  if (!L.kernel) return;
  const uint32_t mb = ws->maxbits[li];
  float v = 0.0f;
  if (L.conv1) {                                                           // e = 1 for an all-zero kernel: sh = 8
    const int e = mb ? rp_frexp_e(mb) : 1;
    const int sh = min(24, max(-6, 9 - e));
    v = lane == 0 ? rp_pow2(sh) : lane == 1 ? rp_pow2(-sh) : 0.0f;
  } else {                                                                 // a zero or non-finite maximum: sh = 0
    int sh = 0;
    if (mb && mb < 0x7f800000u) sh = min(24, max(-6, 9 - rp_frexp_e(mb)));
    if (lane == 0) { v = rp_pow2(-sh); ws->up[li] = rp_pow2(sh); }
  }
  blob[L.s_off + lane] = v;
}

// the split16 half: one thread per PAIR of 16-byte fragments - the hi halves (fragment jq = 2 q) and the lo halves (jq = 2 q + 1, 64
// fragments further) of the same eight weights, which are read once
__global__ void __launch_bounds__(256) k_repack_split16(RpPackArgs a, float* __restrict__ blob, const RpWs* __restrict__ ws) {
#pragma clang fp contract(off)
  const int li = rp_find_layer(a.blk, a.n, blockIdx.x);
  const RpPackLayer& L = a.L[li];
  const uint32_t g = (blockIdx.x - a.blk[li]) * 256u + threadIdx.x;
  if (g >= L.K * L.cin * L.cout / 8u) return;                              // a thread packs eight weights
  const uint32_t CT = L.cout >= 128u ? 128u : L.cout, CC = L.cin % 64u == 0u ? 64u : 32u;
  const uint32_t NS = L.cout / CT, NCC = L.cin / CC, NT = CT / 16u, JQ = CC / 16u;
  const uint32_t lane = g & 63u;
  uint32_t r = g >> 6;
  const uint32_t q = r % (JQ / 2u); r /= JQ / 2u;
  const size_t f_hi = ((size_t)r * JQ + 2u * q) * 64u + lane;              // r = ((k * NS + s) * NCC + cc) * NT + nt
  const uint32_t nt = r % NT; r /= NT;
  const uint32_t cc = r % NCC; r /= NCC;
  const uint32_t s = r % NS, k = r / NS;
  const uint32_t ci = cc * CC + q * 32u + (lane >> 4) * 8u, co = s * CT + nt * 16u + (lane & 15u);
  const float* __restrict__ w = L.kernel + ((size_t)k * L.cin + ci) * L.cout + co;
  const float scv = ws->scale[li][co], up = ws->up[li];
  uint32_t hi[4], lo[4];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = rp_mul(rp_mul(w[(size_t)e * L.cout], scv), up);
    const uint16_t hb = rp_half_bits(v);
    const float hf = rp_half_float(hb);
    const uint16_t lb = rp_half_bits(rp_nan(v - hf, v, hf));
    if (e & 1) { hi[e >> 1] |= (uint32_t)hb << 16; lo[e >> 1] |= (uint32_t)lb << 16; }
    else { hi[e >> 1] = hb; lo[e >> 1] = lb; }
  }
  uint4* out = reinterpret_cast<uint4*>(blob + L.w16_off);
  out[f_hi] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  out[f_hi + 64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

}  // namespace

extern "C" {

size_t eyoc_model_repack_workspace_bytes(const eyoc_model* m) { return m ? align_up(sizeof(RpWs)) : 0; }

int eyoc_model_repack_device(eyoc_ctx* ctx, eyoc_model* m, const eyoc_layer_params* layers, int n_layers, void* ws_dev,
                             size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx && m && layers && ws_dev, EYOC_ERR_INVALID, "eyoc_model_repack_device: NULL argument");
  EYOC_REQUIRE(ws_bytes >= eyoc_model_repack_workspace_bytes(m), EYOC_ERR_WORKSPACE,
               "eyoc_model_repack_device: workspace %zu < required %zu bytes", ws_bytes, eyoc_model_repack_workspace_bytes(m));
  EYOC_REQUIRE(((uintptr_t)ws_dev & 255) == 0, EYOC_ERR_INVALID, "eyoc_model_repack_device: workspace must be 256-byte aligned");
  const int n = (int)m->layers.size();
  EYOC_REQUIRE(n <= RP_MAXL, EYOC_ERR_INVALID, "eyoc_model_repack_device: plan of %d layers (at most %d)", n, RP_MAXL);
  // everything that can be wrong with `layers` is found here, from the plan, before the first launch (the checks and messages of
  // eyoc_model_pack_host)
  RpFoldArgs fa;
  RpPackArgs p32, p16;
  memset(&fa, 0, sizeof(fa));
  memset(&p32, 0, sizeof(p32));
  uint32_t b32 = 0, b16 = 0;
  uint32_t blk16[RP_MAXL + 1];
  for (int li = 0; li < n; ++li) {
    const LayerPlan& p = m->layers[li];
    RpFoldLayer& F = fa.L[li];
    RpPackLayer& P = p32.L[li];
    p32.blk[li] = b32;
    blk16[li] = b16;
    F.b_off = (uint32_t)p.b_off; F.w_off = (uint32_t)p.w_off; F.cout = (uint32_t)p.cout; F.affine = p.map == M_AFFINE ? 1 : p.map == M_INORM ? 2 : 0;
    EYOC_REQUIRE(p.cout <= RP_CH, EYOC_ERR_INVALID, "eyoc_model_repack_device: layer '%s' has %d channels", p.name.c_str(), p.cout);
    const eyoc_layer_params* cv = nullptr;
    if (p.map == M_INORM) {
      const eyoc_layer_params* nm = find_inorm(layers, n_layers, p);
      if (!nm) return EYOC_ERR_INVALID;
      F.g = nm->bn_weight; F.b = nm->bn_bias;
      continue;
    }
    if (p.map != M_AFFINE) {
      cv = find_layer(layers, n_layers, p.name);
      EYOC_REQUIRE(cv && cv->kernel && cv->K == p.K && cv->cin == p.cin && cv->cout == p.cout, EYOC_ERR_INVALID,
                   "eyoc_model_create: layer '%s' missing or shape mismatch (expected K=%d cin=%d cout=%d, got %d %d %d)",
                   p.name.c_str(), p.K, p.cin, p.cout, cv ? cv->K : -1, cv ? cv->cin : -1, cv ? cv->cout : -1);
      EYOC_REQUIRE(p.map == M_CONV1 || (p.cin > 0 && p.cin % 32 == 0 && (p.cout == 32 || p.cout == 64 || p.cout == 128 || p.cout == 256)),
                   EYOC_ERR_INVALID, "pack_weights: unsupported shape C_in %d C_out %d", p.cin, p.cout);
    }
    if (!p.norm.empty()) {
      const eyoc_layer_params* bn = find_layer(layers, n_layers, p.norm);
      EYOC_REQUIRE(bn && bn->bn_weight && bn->bn_bias && bn->bn_mean && bn->bn_var && bn->cout == p.cout, EYOC_ERR_INVALID,
                   "eyoc_model_create: norm '%s' missing or wrong width", p.norm.c_str());
      F.g = bn->bn_weight; F.b = bn->bn_bias; F.m = bn->bn_mean; F.v = bn->bn_var;
    }
    if (!cv) continue;
    if (p.has_bias && cv->bias) F.bias = cv->bias;
    const size_t elems = (size_t)p.K * p.cin * p.cout;
    P.kernel = cv->kernel; P.w_off = (uint32_t)p.w_off; P.w16_off = (uint32_t)p.w16_off; P.s_off = (uint32_t)p.s_off;
    P.K = (uint32_t)p.K; P.cin = (uint32_t)p.cin; P.cout = (uint32_t)p.cout; P.conv1 = p.map == M_CONV1;
    b32 += (uint32_t)cdiv((long long)(pad64(elems) / 4), 256);
    if (p.map != M_CONV1) b16 += (uint32_t)cdiv((long long)(elems / 8), 256);
  }
  p32.blk[n] = b32; blk16[n] = b16;
  p32.n = n;
  p16 = p32;
  memcpy(p16.blk, blk16, sizeof(uint32_t) * (n + 1));
  EYOC_REQUIRE(m->blob_floats <= 0xffffffffu, EYOC_ERR_INVALID, "eyoc_model_repack_device: blob of %zu floats", m->blob_floats);
  hipStream_t st = (hipStream_t)stream;
  RpWs* ws = (RpWs*)ws_dev;
  hipLaunchKernelGGL(k_repack_fold, dim3(n), dim3(RP_CH), 0, st, fa, m->desc.bn_eps, m->blob, ws);
  hipLaunchKernelGGL(k_repack_f32, dim3(b32), dim3(256), 0, st, p32, m->blob, ws);
  hipLaunchKernelGGL(k_repack_scales, dim3(n), dim3(64), 0, st, p32, m->blob, ws);
  if (b16) hipLaunchKernelGGL(k_repack_split16, dim3(b16), dim3(256), 0, st, p16, m->blob, (const RpWs*)ws);
  EYOC_CHECK_HIP(hipGetLastError());
  return EYOC_OK;
}

size_t eyoc_model_blob_floats_in(const eyoc_model_desc* desc, int block_norm) {
  if (check_desc(desc) != EYOC_OK || check_block_norm(desc, block_norm) != EYOC_OK) return 0;
  std::vector<LayerPlan> L;
  BufPlan bufs[B_COUNT];
  build_plan(*desc, block_norm, L, bufs);
  return plan_blob_floats(L);
}

size_t eyoc_model_blob_floats(const eyoc_model_desc* desc) { return eyoc_model_blob_floats_in(desc, 0); }

// Folds batch norm into every convolution and writes the packed blob (fp32 fragment order + split16 packing + shifts) into
// HOST memory.  Pure host code: no device is touched, so a rank can build (or verify) the blob it broadcasts without a GPU.
int eyoc_model_pack_host(const eyoc_model_desc* desc, const eyoc_layer_params* layers, int n_layers, float* blob_host,
                         size_t blob_floats) {
  return eyoc_model_pack_host_in(desc, layers, n_layers, blob_host, blob_floats, 0);
}

// block_norm 1: the residual blocks' convolutions are packed as they are (scale 1, shift 0), every block norm is a layer of its own
// holding its weight at w_off and its bias at b_off
int eyoc_model_pack_host_in(const eyoc_model_desc* desc, const eyoc_layer_params* layers, int n_layers, float* blob_host,
                            size_t blob_floats, int block_norm) {
  EYOC_REQUIRE(layers && blob_host, EYOC_ERR_INVALID, "eyoc_model_pack_host: NULL argument");
  int rc = check_desc(desc);
  if (!rc) rc = check_block_norm(desc, block_norm);
  if (rc) return rc;
  std::vector<LayerPlan> plan;
  BufPlan bufs[B_COUNT];
  build_plan(*desc, block_norm, plan, bufs);
  const size_t need = plan_blob_floats(plan);
  EYOC_REQUIRE(blob_floats >= need, EYOC_ERR_INVALID, "eyoc_model_pack_host: blob of %zu floats required, got %zu", need, blob_floats);
  std::fill(blob_host, blob_host + need, 0.0f);
  for (auto& p : plan) {
    if (p.map == M_INORM) {
      const eyoc_layer_params* nm = find_inorm(layers, n_layers, p);
      if (!nm) return EYOC_ERR_INVALID;
      memcpy(blob_host + p.w_off, nm->bn_weight, p.cout * sizeof(float));
      memcpy(blob_host + p.b_off, nm->bn_bias, p.cout * sizeof(float));
      continue;
    }
    if (p.map == M_AFFINE) {                                            // scale / shift of a norm that stands alone (the same fold as below)
      const eyoc_layer_params* bn = find_layer(layers, n_layers, p.norm);
      EYOC_REQUIRE(bn && bn->bn_weight && bn->bn_bias && bn->bn_mean && bn->bn_var && bn->cout == p.cout, EYOC_ERR_INVALID,
                   "eyoc_model_create: norm '%s' missing or wrong width", p.norm.c_str());
      for (int c = 0; c < p.cout; ++c) {
        const float s = bn->bn_weight[c] / std::sqrt(bn->bn_var[c] + desc->bn_eps);
        blob_host[p.w_off + c] = s;
        blob_host[p.b_off + c] = bn->bn_bias[c] - bn->bn_mean[c] * s;
      }
      continue;
    }
    const eyoc_layer_params* cv = find_layer(layers, n_layers, p.name);
    EYOC_REQUIRE(cv && cv->kernel && cv->K == p.K && cv->cin == p.cin && cv->cout == p.cout, EYOC_ERR_INVALID,
                 "eyoc_model_create: layer '%s' missing or shape mismatch (expected K=%d cin=%d cout=%d, got %d %d %d)",
                 p.name.c_str(), p.K, p.cin, p.cout, cv ? cv->K : -1, cv ? cv->cin : -1, cv ? cv->cout : -1);
    std::vector<float> scale(p.cout, 1.0f), shift(p.cout, 0.0f);
    if (!p.norm.empty()) {
      const eyoc_layer_params* bn = find_layer(layers, n_layers, p.norm);
      EYOC_REQUIRE(bn && bn->bn_weight && bn->bn_bias && bn->bn_mean && bn->bn_var && bn->cout == p.cout, EYOC_ERR_INVALID,
                   "eyoc_model_create: norm '%s' missing or wrong width", p.norm.c_str());
      for (int c = 0; c < p.cout; ++c) {
        const float s = bn->bn_weight[c] / std::sqrt(bn->bn_var[c] + desc->bn_eps);
        scale[c] = s;
        shift[c] = bn->bn_bias[c] - bn->bn_mean[c] * s;
      }
    }
    if (p.has_bias && cv->bias)
      for (int c = 0; c < p.cout; ++c) shift[c] += cv->bias[c];
    float* w = blob_host + p.w_off;
    if (p.map == M_CONV1) {  // plain [K][cin][cout] with the scale folded in
      float wmax = 0.0f;
      for (size_t i = 0; i < (size_t)p.K * p.cin * p.cout; ++i) {
        w[i] = cv->kernel[i] * scale[i % p.cout];
        if (std::isfinite(w[i])) wmax = std::max(wmax, std::fabs(w[i]));
      }
      int e = 1;                                        // wmax = f 2^e, f in [0.5, 1): wmax 2^(9 - e) lies in [256, 512)
      if (wmax > 0.0f) (void)std::frexp(wmax, &e);
      const int sh = std::min(24, std::max(-6, 9 - e));   // same clamp as eyoc_spconv_pack_weights_split16
      blob_host[p.s_off] = std::ldexp(1.0f, sh);
      blob_host[p.s_off + 1] = std::ldexp(1.0f, -sh);
    } else {
      rc = eyoc_spconv_pack_weights(cv->kernel, scale.data(), p.K, p.cin, p.cout, w);
      if (!rc) rc = eyoc_spconv_pack_weights_split16(cv->kernel, scale.data(), p.K, p.cin, p.cout, blob_host + p.w16_off,
                                                     blob_host + p.s_off);
      if (rc) return rc;
    }
    memcpy(blob_host + p.b_off, shift.data(), p.cout * sizeof(float));
  }
  return EYOC_OK;
}

int eyoc_model_create(eyoc_ctx* ctx, const eyoc_model_desc* desc, const eyoc_layer_params* layers, int n_layers,
                      float* blob_dev, size_t blob_floats, eyoc_model** out) {
  return eyoc_model_create_in(ctx, desc, layers, n_layers, blob_dev, blob_floats, 0, out);
}

int eyoc_model_create_in(eyoc_ctx* ctx, const eyoc_model_desc* desc, const eyoc_layer_params* layers, int n_layers,
                         float* blob_dev, size_t blob_floats, int block_norm, eyoc_model** out) {
  EYOC_REQUIRE(ctx && out && blob_dev, EYOC_ERR_INVALID, "eyoc_model_create: NULL argument");
  int rc = check_desc(desc);
  if (!rc) rc = check_block_norm(desc, block_norm);
  if (rc) return rc;
  eyoc_model* m = new eyoc_model();
  m->desc = *desc;
  m->block_norm = block_norm;
  build_plan(*desc, block_norm, m->layers, m->bufs);
  m->blob = blob_dev;
  m->blob_floats = plan_blob_floats(m->layers);
  if (blob_floats < m->blob_floats || ((uintptr_t)blob_dev & 255) != 0) {
    set_error("eyoc_model_create: blob of %zu floats (256-byte aligned) required, got %zu at %p", m->blob_floats,
              blob_floats, (void*)blob_dev);
    delete m;
    return EYOC_ERR_INVALID;
  }
  if (layers) {
    std::vector<float> host(m->blob_floats, 0.0f);
    rc = eyoc_model_pack_host_in(desc, layers, n_layers, host.data(), host.size(), block_norm);
    if (rc) { delete m; return rc; }
    hipError_t e = hipMemcpy(blob_dev, host.data(), m->blob_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      set_error("eyoc_model_create: weight upload failed: %s", hipGetErrorString(e));
      delete m;
      return EYOC_ERR_HIP;
    }
  }
  {   // the SPLIT16 range-guard words (16 bytes; part of the handle like the timing events)
    hipError_t e = hipMalloc((void**)&m->range, 32);                    // words 0..3 as documented; words 4, 5: overflow in the output of the layer that carries the fused tail / in that tail's intermediate
    if (e == hipSuccess) e = hipMemset(m->range, 0, 32);
    if (e != hipSuccess) {
      set_error("eyoc_model_create: range-guard allocation failed: %s", hipGetErrorString(e));
      if (m->range) (void)hipFree(m->range);
      delete m;
      return EYOC_ERR_HIP;
    }
  }
  *out = m;
  return EYOC_OK;
}

int eyoc_model_destroy(eyoc_model* m) {
  if (!m) return EYOC_OK;
  for (auto e : m->events) (void)hipEventDestroy(e);
  if (m->range) (void)hipFree(m->range);
  delete m;
  return EYOC_OK;
}

int eyoc_model_fuse_tail(eyoc_ctx* ctx, int on) {
  if (!ctx) return -1;
  const int prev = ctx->knobs.fuse_tail;
  if (on >= 0 && on <= 2) ctx->knobs.fuse_tail = on;
  return prev;
}

int eyoc_model_set_probe(eyoc_model* m, int on) {
  EYOC_REQUIRE(m, EYOC_ERR_INVALID, "eyoc_model_set_probe: NULL model");
  const unsigned int words[2] = {0u, on ? 1u : 0u};                   // max |x| reset, probe switch
  EYOC_CHECK_HIP(hipMemcpy(m->range + 1, words, 8, hipMemcpyHostToDevice));
  m->probe = on ? 1 : 0;
  return EYOC_OK;
}

int eyoc_model_range_check(eyoc_model* m, void* stream, float* max_abs) {
  EYOC_REQUIRE(m, EYOC_ERR_INVALID, "eyoc_model_range_check: NULL model");
  unsigned int words[4] = {0, 0, 0, 0};
  hipStream_t st = (hipStream_t)stream;
  EYOC_CHECK_HIP(hipMemcpyAsync(words, m->range, 16, hipMemcpyDeviceToHost, st));
  EYOC_CHECK_HIP(hipStreamSynchronize(st));
  float mx;
  memcpy(&mx, &words[1], 4);
  if (max_abs) *max_abs = m->probe ? mx : -1.0f;
  if (words[3]) {
    EYOC_CHECK_HIP(hipMemsetAsync(m->range + 3, 0, 4, st));            // reported once; word 0 is per forward (cleared when one starts)
    set_error("split16 arithmetic overflowed: an activation reached %g (fp16 hi halves end at 65504) in a forward since the last "
              "check - the features of every such forward are NaN; run the model with spconv math \"fp32\"", (double)SPLIT16_LIMIT);
    return EYOC_ERR_RANGE;
  }
  return EYOC_OK;
}

int eyoc_model_range_snapshot(eyoc_model* m, uint32_t* words_host, void* stream) {
  EYOC_REQUIRE(m && words_host, EYOC_ERR_INVALID, "eyoc_model_range_snapshot: NULL argument");
  EYOC_CHECK_HIP(hipMemcpyAsync(words_host, m->range, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return EYOC_OK;
}

// split-K scratch of the staged kernel (spconv_st.hip, launch_spconv_st): only stride-1 layers with >= 4 input blocks whose
// 32-channel workgroups fit KS_MAX_SLOTS partial-sum slots can split - a batch whose smallest such layer is larger (the bench: 571
// tiles x 8 channel groups at level 3) and a model that is pinned to fp32 products need none of the 32 MiB
static size_t ks_part_bytes(const eyoc_model* m, const eyoc_maps* maps) {
  if (m->math == 0) return 0;
  for (const LayerPlan& p : m->layers)
    if (p.map == M_S1 && p.cin >= 128 && p.cout >= 64 && p.cout <= 256 &&
        (long long)cdiv(maps->rows[p.level], ST_TILE) * (p.cout / 32) <= KS_MAX_SLOTS)
      return KS_PART_BYTES;
  return 0;
}

// the instance-norm layers' scratch (partial sums, statistics): the largest layer's, shared by all of them; 0 for a batch-norm model
static size_t in_ws_bytes(const eyoc_model* m, const eyoc_maps* maps) {
  size_t b = 0;
  for (const LayerPlan& p : m->layers)
    if (p.map == M_INORM && maps->rows[p.out_level] > 0) b = std::max(b, in_layer_workspace_bytes(maps->rows[p.out_level], p.cout));
  return b;
}

size_t eyoc_model_workspace_bytes(const eyoc_model* m, const eyoc_maps* maps) {
  if (!m || !maps) return 0;
  size_t b = 0;
  for (int i = B_X1; i < B_OUT; ++i) b += align_up((size_t)maps->rows[m->bufs[i].level] * m->bufs[i].width * sizeof(float));
  b += align_up(ks_part_bytes(m, maps));
  b += align_up(in_ws_bytes(m, maps));
  return b + 256;
}

// eyoc_model_forward_rows: floats it needs beside the full forward's buffers - the compact rows [n_rows, 96] (sampled tail) or the
// full output [N, out_channels] (fallback), whichever is larger.  Both live in B_X1 when they fit: the first block's input is dead
// long before the last layer runs.  0 = they fit.
static size_t rows_region_floats(const eyoc_model* m, const eyoc_maps* maps, int n_rows) {
  return std::max((size_t)n_rows * 96, (size_t)maps->rows[0] * m->desc.out_channels);
}
static size_t rows_extra_floats(const eyoc_model* m, const eyoc_maps* maps, int n_rows) {
  const size_t need = rows_region_floats(m, maps, n_rows);
  return need <= (size_t)maps->rows[0] * m->bufs[B_X1].width ? 0 : need;
}

size_t eyoc_model_workspace_bytes_rows(const eyoc_model* m, const eyoc_maps* maps, int n_rows) {
  if (!m || !maps || n_rows < 0) return 0;
  return eyoc_model_workspace_bytes(m, maps) + align_up(rows_extra_floats(m, maps, n_rows) * sizeof(float)) +
         align_up(spconv_rows_scratch_bytes(maps->rows[0], n_rows));
}

int eyoc_model_sampled_tail(eyoc_ctx* ctx, int on) {
  if (!ctx) return -1;
  const int prev = ctx->knobs.sampled_tail;
  if (on == 0 || on == 1) ctx->knobs.sampled_tail = on;
  return prev;
}

int eyoc_model_num_layers(const eyoc_model* m) { return m ? (int)m->layers.size() : 0; }

int eyoc_model_set_math(eyoc_model* m, int mode) {
  EYOC_REQUIRE(m && mode >= -1 && mode <= 1, EYOC_ERR_INVALID, "eyoc_model_set_math: mode %d not in {-1, 0, 1}", mode);
  const int prev = m->math;
  m->math = mode;
  return prev + 1 ? prev + 2 : 1;   // previous mode + 2 (so that every valid answer is positive): 1 = auto, 2 = fp32, 3 = split16
}

int eyoc_model_last_math(const eyoc_model* m) { return m ? m->last.math : -1; }

int eyoc_model_set_timing(eyoc_model* m, int on) {
  EYOC_REQUIRE(m, EYOC_ERR_INVALID, "eyoc_model_set_timing: NULL model");
  m->timing = on ? 1 : 0;
  m->last.events_valid[0] = m->last.events_valid[1] = 0;
  if (on && m->events.empty()) {
    m->events.resize(2 * (m->layers.size() + 1));
    for (auto& e : m->events) EYOC_CHECK_HIP(hipEventCreate(&e));
  }
  return EYOC_OK;
}

int eyoc_model_timing_slot(eyoc_model* m, int slot) {
  EYOC_REQUIRE(m && (slot == 0 || slot == 1), EYOC_ERR_INVALID, "eyoc_model_timing_slot: slot %d", slot);
  m->slot = slot;
  return EYOC_OK;
}

int eyoc_model_layer_ms(eyoc_model* m, float* ms) {
  EYOC_REQUIRE(m && ms, EYOC_ERR_INVALID, "eyoc_model_layer_ms: NULL argument");
  EYOC_REQUIRE(m->timing && m->last.events_valid[m->slot], EYOC_ERR_INVALID, "eyoc_model_layer_ms: no timed forward recorded in slot %d", m->slot);
  const hipEvent_t* ev = m->events.data() + (size_t)m->slot * (m->layers.size() + 1);
  EYOC_CHECK_HIP(hipEventSynchronize(ev[m->layers.size()]));
  for (size_t i = 0; i < m->layers.size(); ++i) EYOC_CHECK_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
  return EYOC_OK;
}

}  // extern "C"

// ---- The forward: carve the workspace, RESOLVE the launch schedule (host decisions only: which launch every layer becomes and what
// must be ready in front of it - eyoc_model_forward_steps returns them as data), then RUN it.  eyoc_model_forward (rows_dev == NULL:
// out_dev is [N, out_channels]) and eyoc_model_forward_rows (out_dev is [n_rows, out_channels], row i = the network's output row
// rows_dev[i]) are one schedule.  With rows, the last 3^3 layer and the 1x1 tail run on the listed rows only where the full forward
// would fuse them (spconv_rows.hip); otherwise the full output goes to the workspace and its rows are taken.
namespace {

struct Bufs {                          // the carved workspace of one forward
  float* buf[B_COUNT];                 // B_OUT of a forward with a row list: rows_region (the full output, whose rows are taken at the end)
  float* ks_part = nullptr;            // split-K scratch of the staged kernel (ks_part_bytes)
  void* in_ws = nullptr;               // the instance-norm layers' scratch (in_ws_bytes)
  float* rows_region = nullptr;        // a row list: the compact rows [n_rows, 96] (sampled tail) or the full output (fallback)
  void* rows_scratch = nullptr;        // ... and the rows kernel's scratch
  float* out = nullptr;                // the caller's out_dev
};

Bufs carve(const eyoc_model* m, const eyoc_maps* maps, const float* feats_dev, float* out_dev, void* ws, size_t ws_bytes,
           const int64_t* rows_dev, int n_rows) {
  Bufs b;
  Carver cv(ws, ws_bytes);
  b.buf[B_IN] = const_cast<float*>(feats_dev);
  b.buf[B_OUT] = b.out = out_dev;
  for (int i = B_X1; i < B_OUT; ++i) b.buf[i] = cv.take<float>((size_t)maps->rows[m->bufs[i].level] * m->bufs[i].width);
  if (const size_t ks_bytes = ks_part_bytes(m, maps)) b.ks_part = cv.take<float>(ks_bytes / 4);
  if (const size_t in_bytes = in_ws_bytes(m, maps)) b.in_ws = cv.take<unsigned char>(in_bytes);
  if (rows_dev) {
    const size_t extra = rows_extra_floats(m, maps, n_rows);
    b.rows_region = extra ? cv.take<float>(extra) : b.buf[B_X1];
    b.rows_scratch = cv.take<unsigned char>(spconv_rows_scratch_bytes(maps->rows[0], n_rows));
    b.buf[B_OUT] = b.rows_region;
  }
  return b;
}

// arithmetic of the sparse convolutions: SPLIT16 needs the wave-private kernel for EVERY layer (only it reads and
// writes the format), which round 1 measured to pay off once the finest level alone fills the chip (>= 4096 wave tiles ~ 4 KITTI
// pairs); small batches stay on fp32, where the launcher picks the workgroup-tiled kernel per layer
int forward_math(const eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, bool* split) {
  const int want = m->math;
  const bool split_ok = ctx->knobs.spconv_kernel != 0 && !(m->desc.normalize_feature && m->desc.out_channels > 64) &&
                        m->desc.channels[1] % 32 == 0;
  *split = split_ok && (want == 1 || (want < 0 && maps->rows[0] >= 8192));   // = the Z-order threshold of eyoc_maps_build
  EYOC_REQUIRE(want != 1 || *split, EYOC_ERR_INVALID,
               "eyoc_model_forward: split16 arithmetic is not available for this model / kernel selection");
  return EYOC_OK;
}

enum StepKind { S_INORM, S_AFFINE, S_CONV1, S_SPCONV, S_TAIL, S_SPCONV_TAIL, S_ROWS_TAIL, S_TAKE_ROWS };   // eyoc_hip.h lists them

struct Step {
  StepKind kind;
  int first, count = 1;                // the layers [first, first + count) it covers; the time of a step is booked on its first layer
  int path = -1;                       // S_SPCONV, S_SPCONV_TAIL, S_ROWS_TAIL: spconv_record_path of `a`
  SpconvArgs a;                        // ... the layer (S_SPCONV_TAIL: with a.tail, the 1x1 pair in its epilogue)
  Conv1Args c1;                        // S_CONV1
  // made ready in front of the launch, in this order
  int in_plan_level = -1;              // maps_ensure_in_plan
  int table_kind = -1, table_level = 0;   // maps_ensure_table: a lazily skipped [27][n] table that a gathering kernel reads
  const float* permute_src = nullptr;  // S_CONV1 on Z-ordered maps: the caller's features, copied in internal order to c1.in
  bool table0 = false;                 // maps_build_table0: the first convolution probes the hash table
};
constexpr int MAX_STEPS = RP_MAXL + 1;   // one per layer and the row gather

// layers li, li + 1 are the 1x1 pair the tail kernels take (spconv_tail.hip): conv1_tr -> [ReLU] -> final (+ bias) -> [row normalisation]
bool is_tail_pair(const eyoc_model* m, size_t li) {
  if (li + 2 > m->layers.size()) return false;
  const LayerPlan &q1 = m->layers[li], &q2 = m->layers[li + 1];
  return q1.map == M_IDENT && q1.K == 1 && q1.res_buf < 0 && q2.map == M_IDENT && q2.K == 1 && q2.in_buf == q1.out_buf && q2.res_buf < 0 &&
         !q2.relu && q2.out_buf == B_OUT && q1.out_col == 0 && tail_fusable(q1.cin, q1.cout, q2.cout);
}

int launch_tail(const eyoc_model* m, size_t li, const float* in, int ld_in, int n, float* out, int ld_out, const int32_t* out_perm,
                hipStream_t st) {
  const LayerPlan &q1 = m->layers[li], &q2 = m->layers[li + 1];
  return launch_tail_fused(in, ld_in, n, m->blob + q1.w16_off, m->blob + q1.s_off, m->blob + q1.b_off, q1.relu, m->blob + q2.w16_off,
                           m->blob + q2.s_off, m->blob + q2.b_off, q2.l2norm, out, ld_out, out_perm, m->range, st);
}

// a sparse-convolution layer's arguments.  A split16 layer is handed every tile-record family its table kind and widths admit - one
// rule per family; which of them takes the layer is spconv_record_path's decision
SpconvArgs fill_spconv(eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, const Bufs& b, bool split, const LayerPlan& p) {
  SpconvArgs a;
  a.nbr = p.map == M_S1 ? maps->nbr_s1[p.level] : p.map == M_DOWN ? maps->nbr_down[p.level]
          : p.map == M_UP ? maps->nbr_up[p.level] : nullptr;
  a.K = p.K; a.n_out = maps->rows[p.out_level];
  a.n_in = maps->rows[m->bufs[p.in_buf].level];
  a.in = b.buf[p.in_buf] + p.in_col; a.ld_in = m->bufs[p.in_buf].width; a.cin = p.cin;
  a.w = m->blob + p.w_off; a.cout = p.cout; a.bias = m->blob + p.b_off;
  a.res = p.res_buf >= 0 ? b.buf[p.res_buf] : nullptr; a.ld_res = p.res_buf >= 0 ? m->bufs[p.res_buf].width : 0;
  a.relu = p.relu; a.l2norm = p.l2norm;
  a.out = b.buf[p.out_buf] + p.out_col; a.ld_out = m->bufs[p.out_buf].width;
  a.ctx = ctx;
  if (split) {
    a.math = 1;
    a.w = m->blob + p.w16_off;
    a.out_scale = m->blob + p.s_off;
    a.out_split = p.out_buf != B_OUT;
    a.range = m->range;
    const bool blocks = p.cin % 32 == 0;
    if (p.map == M_S1 && blocks && p.cin >= 32) { a.local = maps->local_s1[p.level]; a.ks_part = b.ks_part; }   // spconv_st.hip, Z-ordered rows
    if (p.map == M_S1 && blocks && p.cout % 128 == 0 && ctx->knobs.s1_wide) a.local128 = maps->local_s1w[p.level];
    if (p.map == M_DOWN && blocks && p.cout % 64 == 0) a.local_down = maps->local_down[p.level];                 // spconv_st.hip on 128-row tiles
    if (p.map == M_UP && blocks && p.cout % 64 == 0) { a.local_up = maps->local_up[p.level]; a.local_upc = maps->local_upc[p.level]; }   // spconv_up.hip; spconv_upc.hip (class-major tiles)
  }
  if (p.out_buf == B_OUT) a.out_perm = maps->row_perm;   // the network output goes back to the caller's row order
  a.perm = p.map == M_UP ? maps->perm_up[p.level] : p.map == M_S1 ? maps->perm_s1[p.level]
           : p.map == M_DOWN ? maps->perm_down[p.level] : nullptr;
  return a;
}

void fill_conv1(eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, const Bufs& b, bool split, const LayerPlan& p, Step& s) {
  Conv1Args& a = s.c1;
  a.coords = maps->coords[0]; a.n = maps->rows[p.out_level]; a.table = maps->table[0]; a.ks = m->desc.conv1_kernel_size;
  a.in = b.buf[p.in_buf]; a.cin = p.cin; a.w = m->blob + p.w_off; a.bias = m->blob + p.b_off; a.cout = p.cout;
  a.out = b.buf[p.out_buf] + p.out_col; a.ld_out = m->bufs[p.out_buf].width;
  a.out_split = split ? 1 : 0;
  a.ctx = ctx;
  a.range = split ? m->range : nullptr;
  a.wscale = m->blob + p.s_off;
  a.in_perm = maps->row_perm;                        // Z-ordered maps: the caller's features are read through the permutation
  if (a.in_perm) {
    // ... once: a copy in internal order in a buffer nothing uses yet (an indirection per probed neighbour cost the
    // 5^3 first convolution 0.4 of its 2.0 ms on the 64-pair batch)
    int best = -1;
    size_t best_sz = 0;
    for (int i = B_X1; i < B_OUT; ++i) {
      const size_t sz = (size_t)maps->rows[m->bufs[i].level] * m->bufs[i].width;
      if (i != p.out_buf && sz > best_sz) { best = i; best_sz = sz; }
    }
    if (best >= 0 && best_sz >= (size_t)a.n * p.cin) {
      s.permute_src = a.in;
      a.in = b.buf[best];
      a.in_perm = nullptr;
    }
  }
  a.parent = maps->parent[0]; a.children = maps->children[0]; a.s1c = maps->nbr_s1[1]; a.nc = maps->rows[1];
  a.local1 = maps->row_perm ? maps->local_s1[1] : nullptr;          // Z-ordered maps: the level-1 tile rulebooks (256-parent tiles)
  s.table0 = conv1_path(a) == Conv1Path::Probe;
}

// -> the number of steps.  Reads the plan, the maps' host fields and the ctx's knobs; launches and writes nothing
int resolve_schedule(eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, const Bufs& b, bool split, const int64_t* rows_dev,
                     Step* steps) {
  const size_t nl = m->layers.size();
  EYOC_REQUIRE(nl >= 1 && nl < MAX_STEPS, EYOC_ERR_INVALID, "eyoc_model_forward: a plan of %zu layers", nl);
  const bool want_rows = rows_dev && ctx->knobs.sampled_tail;
  int ns = 0;
  for (size_t li = 0; li < nl; li += steps[ns].count, ++ns) {
    const LayerPlan& p = m->layers[li];
    Step& s = steps[ns];
    s.first = (int)li;
    if (p.map == M_INORM) {
      s.kind = S_INORM; s.in_plan_level = p.out_level;   // built on the first instance-norm forward over these maps, without a read-back
    } else if (p.map == M_AFFINE) {
      s.kind = S_AFFINE;
    } else if (p.map == M_CONV1) {
      s.kind = S_CONV1; fill_conv1(ctx, m, maps, b, split, p, s);
    } else if (split && ctx->knobs.fuse_tail != 0 && li + 2 == nl && is_tail_pair(m, li)) {
      s.kind = S_TAIL; s.count = 2;   // conv1_tr -> ReLU -> final (+ bias) -> row normalisation in one kernel: the [N, 64] intermediate stays in registers
    } else {
      s.kind = S_SPCONV;
      s.a = fill_spconv(ctx, m, maps, b, split, p);
      s.path = spconv_record_path(s.a);
      // lazy tables (common.h eyoc_maps): a layer that no tile-record kernel takes reads its [27][n] table - filled on first use
      if ((p.map == M_S1 || p.map == M_UP) && s.path == 0) { s.table_kind = p.map == M_S1 ? EYOC_MAP_S1 : EYOC_MAP_UP; s.table_level = p.level; }
      // the 1x1 tail behind the last staged layer (eyoc_model_fuse_tail 2, the default): block2_tr.conv2 writes the 64 decoder channels
      // the tail reads next to the 32 skip channels.  (A row list does not ask for the 256-row kernel: small inputs, whose full forward
      // runs the tail as a kernel of its own - the same bits -, take the sampled path too)
      if (split && ctx->knobs.fuse_tail == 2 && li + 3 == nl && p.map == M_S1 && p.cout == 64 && is_tail_pair(m, li + 1)) {
        const LayerPlan &q1 = m->layers[li + 1], &q2 = m->layers[li + 2];
        if (q1.in_buf == p.out_buf && q1.in_col == p.out_col && q1.cin == p.cout + 32 && s.path == 1 &&
            (spconv_st_can_fuse_tail(s.a) || want_rows)) {
          if (want_rows && maps->row_perm && spconv_rows_supported(s.a)) {
            // this layer for the listed rows only (compact [n_rows, 96] split16 rows: its 64 channels + the 32 skip channels), then the
            // tail as a kernel of its own on them - the bits of the fused epilogue
            s.kind = S_ROWS_TAIL; s.count = 3;
          } else if (spconv_st_can_fuse_tail(s.a)) {
            // in the layer's epilogue: with the tail riding there the 64 channels never reach memory
            s.kind = S_SPCONV_TAIL; s.count = 3;
            TailFuse& t = s.a.tail;
            t.skip = b.buf[q1.in_buf] + q1.in_col + p.cout; t.ld_skip = m->bufs[q1.in_buf].width;
            t.w1 = m->blob + q1.w16_off; t.s1 = m->blob + q1.s_off; t.b1 = m->blob + q1.b_off; t.relu1 = q1.relu;
            t.w2 = m->blob + q2.w16_off; t.s2 = m->blob + q2.s_off; t.b2 = m->blob + q2.b_off; t.l2norm = q2.l2norm;
            t.out = b.buf[q2.out_buf] + q2.out_col; t.ld_out = m->bufs[q2.out_buf].width; t.out_perm = maps->row_perm;
          }
        }
      }
    }
  }
  if (rows_dev && steps[ns - 1].kind != S_ROWS_TAIL) steps[ns++] = Step{S_TAKE_ROWS, (int)nl, 0};   // the fallback: the rows of the full output
  return ns;
}

int run_schedule(const eyoc_model* m, const eyoc_maps* maps_c, const Bufs& b, bool split, const int64_t* rows_dev, int n_rows,
                 const Step* steps, int ns, hipStream_t st) {
  eyoc_maps* maps = const_cast<eyoc_maps*>(maps_c);                      // what a step needs ready is filled on first use (common.h eyoc_maps)
  const hipEvent_t* ev = m->timing ? m->events.data() + (size_t)m->slot * (m->layers.size() + 1) : nullptr;
  if (ev) EYOC_CHECK_HIP(hipEventRecord(ev[0], st));
  bool progress_recorded = m->progress_event == nullptr;
  for (int si = 0; si < ns; ++si) {
    const Step& s = steps[si];
    const LayerPlan* p = m->layers.data() + s.first;                     // p[0 .. count): the covered layers
    // in front of the first step that begins at or behind the layer: a layer inside a multi-layer step has no launch of its own
    if (!progress_recorded && s.first >= m->progress_layer) { EYOC_CHECK_HIP(hipEventRecord(m->progress_event, st)); progress_recorded = true; }
    int rc = EYOC_OK;
    if (s.in_plan_level >= 0) rc = maps_ensure_in_plan(maps, s.in_plan_level, st);
    if (!rc && s.table_kind >= 0) rc = maps_ensure_table(maps, s.table_kind, s.table_level, st);
    if (!rc && s.permute_src) rc = launch_permute_rows(s.permute_src, maps->row_perm, s.c1.n, s.c1.cin, const_cast<float*>(s.c1.in), st);
    if (!rc && s.table0) rc = maps_build_table0(maps, st);
    if (rc) return rc;
    const int n_out = s.count ? maps->rows[p->out_level] : 0;
    switch (s.kind) {
      case S_INORM:
        if (n_out)
          rc = launch_in_layer(b.buf[p->in_buf] + p->in_col, m->bufs[p->in_buf].width, n_out, p->cout, maps->in_plan[p->out_level],
                               m->blob + p->w_off, m->blob + p->b_off, IN_EPS, p->relu, p->res_buf >= 0 ? b.buf[p->res_buf] : nullptr,
                               p->res_buf >= 0 ? m->bufs[p->res_buf].width : 0, b.buf[p->out_buf] + p->out_col, m->bufs[p->out_buf].width,
                               split, split ? m->range : nullptr, b.in_ws, st);
        break;
      case S_AFFINE:
        rc = launch_affine(b.buf[p->in_buf] + p->in_col, m->bufs[p->in_buf].width, n_out, p->cout, m->blob + p->w_off, m->blob + p->b_off,
                           b.buf[p->out_buf] + p->out_col, m->bufs[p->out_buf].width, split, split ? m->range : nullptr, st);
        break;
      case S_CONV1: rc = launch_conv1(s.c1, st); break;
      case S_SPCONV:
      case S_SPCONV_TAIL: rc = launch_spconv(s.a, s.path, st); break;
      case S_TAIL:
        rc = launch_tail(m, s.first, b.buf[p->in_buf] + p->in_col, m->bufs[p->in_buf].width, n_out, b.buf[p[1].out_buf] + p[1].out_col,
                         m->bufs[p[1].out_buf].width, maps->row_perm, st);
        break;
      case S_ROWS_TAIL:
        EYOC_CHECK_HIP(hipMemsetAsync(m->range + 6, 0, 4, st));          // word 6: the (row, offset) pairs the rows kernel multiplies
        rc = launch_spconv_rows(s.a, s.a.local, maps->row_perm, rows_dev, n_rows, b.buf[p[1].in_buf] + p[1].in_col + p->cout,
                                m->bufs[p[1].in_buf].width, b.rows_region, b.rows_scratch, m->range + 6, st);
        if (!rc) rc = launch_tail(m, s.first + 1, b.rows_region, 96, n_rows, b.out, m->desc.out_channels, nullptr, st);
        break;
      case S_TAKE_ROWS: rc = launch_take_rows(b.rows_region, maps->rows[0], m->desc.out_channels, rows_dev, n_rows, b.out, st); break;
    }
    if (rc) return rc;
    for (int e = 1; ev && e <= s.count; ++e) EYOC_CHECK_HIP(hipEventRecord(ev[s.first + e], st));   // the other covered layers read 0
  }
  if (!progress_recorded) EYOC_CHECK_HIP(hipEventRecord(m->progress_event, st));
  return EYOC_OK;
}

int forward_impl(eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, const float* feats_dev, float* out_dev, void* ws,
                 size_t ws_bytes, void* stream, const int64_t* rows_dev, int n_rows) {
  hipStream_t st = (hipStream_t)stream;
  bool split;
  if (int rc = forward_math(ctx, m, maps, &split)) return rc;
  const Bufs b = carve(m, maps, feats_dev, out_dev, ws, ws_bytes, rows_dev, n_rows);
  Step steps[MAX_STEPS];
  const int ns = resolve_schedule(ctx, m, maps, b, split, rows_dev, steps);
  if (ns < 0) return ns;
  eyoc_model::Last& last = const_cast<eyoc_model*>(m)->last;             // the one thing a forward writes to its model: what it was
  const bool sampled = steps[ns - 1].kind == S_ROWS_TAIL;                // (it covers the last three layers, so it is the last step)
  last.math = split ? 1 : 0;
  last.sampled_layer = sampled ? steps[ns - 1].first : -1;
  last.sampled_rows = sampled ? n_rows : 0;
  // the overflow flag of THIS forward (the sticky copy is word 3).  Cleared by every forward, fp32 ones included: after an
  // overflow switched a model to fp32 MFMAs, eyoc_model_range_snapshot must not keep reporting the old verdict for forwards
  // that cannot overflow
  EYOC_CHECK_HIP(hipMemsetAsync(m->range, 0, 4, st));
  EYOC_CHECK_HIP(hipMemsetAsync(m->range + 4, 0, 8, st));             // words 4, 5: the fused tail's own verdicts (spconv_st.hip TAILF)
  if (int rc = run_schedule(m, maps, b, split, rows_dev, n_rows, steps, ns, st)) return rc;
  if (m->timing) last.events_valid[m->slot] = 1;
  return EYOC_OK;
}

}  // namespace

extern "C" {

int eyoc_model_forward(eyoc_ctx* ctx, const eyoc_model* mc, const eyoc_maps* maps, const float* feats_dev, float* out_dev,
                       void* ws, size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx && mc && maps && feats_dev && out_dev && ws, EYOC_ERR_INVALID, "eyoc_model_forward: NULL argument");
  EYOC_REQUIRE(ws_bytes >= eyoc_model_workspace_bytes(mc, maps), EYOC_ERR_WORKSPACE,
               "eyoc_model_forward: workspace %zu < required %zu bytes", ws_bytes, eyoc_model_workspace_bytes(mc, maps));
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "eyoc_model_forward: workspace must be 256-byte aligned");
  return forward_impl(ctx, mc, maps, feats_dev, out_dev, ws, ws_bytes, stream, nullptr, 0);
}

int eyoc_model_forward_rows(eyoc_ctx* ctx, const eyoc_model* mc, const eyoc_maps* maps, const float* feats_dev, const int64_t* rows_dev,
                            int n_rows, float* out_dev, void* ws, size_t ws_bytes, void* stream) {
  EYOC_REQUIRE(ctx && mc && maps && feats_dev && ws && n_rows >= 0 && (n_rows == 0 || (rows_dev && out_dev)), EYOC_ERR_INVALID,
               "eyoc_model_forward_rows: NULL argument");
  EYOC_REQUIRE(mc->desc.out_channels % 4 == 0, EYOC_ERR_INVALID, "eyoc_model_forward_rows: %d output channels", mc->desc.out_channels);
  EYOC_REQUIRE(ws_bytes >= eyoc_model_workspace_bytes_rows(mc, maps, n_rows), EYOC_ERR_WORKSPACE,
               "eyoc_model_forward_rows: workspace %zu < required %zu bytes", ws_bytes, eyoc_model_workspace_bytes_rows(mc, maps, n_rows));
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "eyoc_model_forward_rows: workspace must be 256-byte aligned");
  if (n_rows == 0) return EYOC_OK;                                       // nothing is read: nothing is launched
  return forward_impl(ctx, mc, maps, feats_dev, out_dev, ws, ws_bytes, stream, rows_dev, n_rows);
}

int eyoc_model_forward_steps(eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, const int64_t* rows_dev, int n_rows, void* ws,
                             size_t ws_bytes, int32_t* step_of_layer, int32_t* kind_of_layer, int32_t* path_of_layer) {
  EYOC_REQUIRE(ctx && m && maps && ws && step_of_layer && kind_of_layer && path_of_layer && (!rows_dev || n_rows >= 1), EYOC_ERR_INVALID,
               "eyoc_model_forward_steps: NULL argument");
  const size_t need = rows_dev ? eyoc_model_workspace_bytes_rows(m, maps, n_rows) : eyoc_model_workspace_bytes(m, maps);
  EYOC_REQUIRE(ws_bytes >= need, EYOC_ERR_WORKSPACE, "eyoc_model_forward_steps: workspace %zu < required %zu bytes", ws_bytes, need);
  EYOC_REQUIRE(((uintptr_t)ws & 255) == 0, EYOC_ERR_INVALID, "eyoc_model_forward_steps: workspace must be 256-byte aligned");
  bool split;
  if (int rc = forward_math(ctx, m, maps, &split)) return rc;
  // the caller's features and output take no part in any decision: a residual or an output permutation does, hence the real carve
  const Bufs b = carve(m, maps, nullptr, nullptr, ws, ws_bytes, rows_dev, n_rows);
  Step steps[MAX_STEPS];
  const int ns = resolve_schedule(ctx, m, maps, b, split, rows_dev, steps);
  for (int si = 0; si < ns; ++si)
    for (int l = steps[si].first; l < steps[si].first + steps[si].count; ++l) { step_of_layer[l] = si; kind_of_layer[l] = steps[si].kind; path_of_layer[l] = steps[si].path; }
  return ns;
}

int eyoc_model_set_progress_event(eyoc_model* m, int layer, void* hip_event) {
  EYOC_REQUIRE(m, EYOC_ERR_INVALID, "eyoc_model_set_progress_event: NULL model");
  const int n = (int)m->layers.size();
  if (layer < 0) layer += n;                                             // -1 = in front of the last layer
  EYOC_REQUIRE(!hip_event || (layer >= 0 && layer <= n), EYOC_ERR_INVALID, "eyoc_model_set_progress_event: layer %d of %d", layer, n);
  m->progress_event = (hipEvent_t)hip_event;
  m->progress_layer = layer;
  return EYOC_OK;
}

int eyoc_model_layer_work(eyoc_ctx* ctx, const eyoc_model* m, const eyoc_maps* maps, void* stream, const char** names,
                          int64_t* pairs, double* flops, double* gather_bytes, double* compulsory_bytes) {
  EYOC_REQUIRE(ctx && m && maps, EYOC_ERR_INVALID, "eyoc_model_layer_work: NULL argument");
  eyoc_maps_info_t info;
  int rc = eyoc_maps_info(ctx, maps, m->desc.conv1_kernel_size, stream, &info);
  if (rc) return rc;
  // the handle's most recent forward computed its last three layers for a row list (eyoc_model_forward_rows): their work is what
  // that forward multiplied - the pairs its rows kernel counted (range word 6), the listed rows for the two 1x1 layers
  unsigned int sampled_pairs = 0;
  if (m->last.sampled_layer >= 0) {
    EYOC_CHECK_HIP(hipMemcpyAsync(&sampled_pairs, m->range + 6, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    EYOC_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  for (size_t li = 0; li < m->layers.size(); ++li) {
    const LayerPlan& p = m->layers[li];
    const bool sampled = m->last.sampled_layer >= 0 && (int)li >= m->last.sampled_layer && (int)li <= m->last.sampled_layer + 2;
    const double n_out = sampled ? m->last.sampled_rows : maps->rows[p.out_level];
    double n_in = n_out, pr = 0;
    if (sampled) {
      pr = (int)li == m->last.sampled_layer ? (double)sampled_pairs : n_out;
    } else
    switch (p.map) {
      case M_CONV1: pr = (double)info.pairs_conv1; break;
      case M_S1: pr = (double)info.pairs_s1[p.level]; break;
      case M_DOWN: pr = (double)info.pairs_down[p.level]; n_in = maps->rows[p.level]; break;
      case M_UP: pr = (double)info.pairs_up[p.level]; n_in = maps->rows[p.level + 1]; break;
      case M_IDENT: pr = n_out; break;
      case M_AFFINE: break;
      case M_INORM: break;
    }
    if (is_norm_layer(p.map)) {                                             // no products: one read and one write of the rows
      if (names) names[li] = p.name.c_str();
      if (pairs) pairs[li] = 0;
      if (flops) flops[li] = 2.0 * n_out * p.cout;
      if (gather_bytes) gather_bytes[li] = 8.0 * n_out * p.cout;
      if (compulsory_bytes) compulsory_bytes[li] = 8.0 * n_out * p.cout;
      continue;
    }
    const double wbytes = 4.0 * p.K * p.cin * p.cout;
    if (names) names[li] = p.name.c_str();
    if (pairs) pairs[li] = (int64_t)pr;
    if (flops) flops[li] = 2.0 * pr * p.cin * p.cout;
    if (gather_bytes) gather_bytes[li] = pr * (4.0 * p.cin + 8.0) + 4.0 * n_out * p.cout + wbytes;
    if (compulsory_bytes) compulsory_bytes[li] = 4.0 * (n_in * p.cin + n_out * p.cout) + 8.0 * pr + wbytes;
  }
  return EYOC_OK;
}

}  // extern "C"
