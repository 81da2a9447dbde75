// The neural colour model (the reference's ColorModel: LayerNorm, a GLU-MLP for the diffuse colour and an SH-modulated
// GLU-MLP for the specular colour) as fused kernels on f16 MFMA.  Row maths in gsr_color.h.
//
// Layout.  A wave works on 16 rows at a time, row = lane & 15, lane group g = lane >> 4.  A feature vector of length n
// (padded to 32 KS) sits in a row's four lanes as KS blocks of 8: element j of block s in group g is feature
//   phi(s, g, j) = 32 s + 16 (j >> 2) + 4 g + (j & 3).
// Every Linear is y^T = W x^T on v_mfma_f32_16x16x32_f16: A = 16 output rows of W (the pack kernel's fragments), B = the
// row vectors (k slot 8 g + j of B holds feature phi(s, g, j), and A's k slots are packed in the same order), C = 16
// outputs x 16 rows with output 16 t + 4 g + r in register r of group g.  That is phi(t >> 1, g, 4 (t & 1) + r): an
// output tile pair is the next layer's B block with no data movement, and GLU, x * a + b and every activation are
// lane-local.  The encoder's a and b halves are packed as separate tile ranges so that a_f, b_f and x_f meet in one lane.
// Numerics: each Linear's input and weight are rounded once to f16 (RNE), products accumulate in fp32 on top of the fp32
// bias; everything elementwise is fp32.
//
// Backward.  One kernel recomputes the forward of each 16-row tile and walks it back.  The data path dx = W^T dy runs on
// the same MFMA with the pack kernel's transposed fragments; dy enters as f16 times 2^k, k per wave and layer so that
// max |dy| lands in [2^14, 2^15) (gradients of 1e-7 do not underflow), and the fp32 product is scaled back exactly.
// Weight gradients: the four waves of a workgroup stage dy (scaled f16) and the layer input (f16) as [feature][16 rows]
// in LDS; wave w then owns dW tiles w, w+4, ... of the layer and sums all four waves' rows with v_mfma_f32_16x16x16_f16
// (k = the 16 rows of one wave, so one scale per product), unscaling each product into fp32 accumulators that live for
// the whole grid-stride loop.  Bias gradients are fixed-order row sums of the staged dy.  Each workgroup writes one
// fixed-size slot; cm_finish_kernel sums the slots in workgroup order.  The grid depends on M only and there are no float
// atomics: every result is bit-reproducible.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "gsr_color.h"
#include "gsr_host.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int CM_BLOCK = 256;              // 4 waves
constexpr int CM_ROWS = 64;                // rows per workgroup step (16 per wave)
constexpr int CM_FWD_MAX_WG = 2048;
constexpr int CM_BWD_MAX_WG = 256;
constexpr int CM_H = 32;
constexpr int CM_MAX_FEATURES = 64;

// forces compile-time evaluation of a constexpr offset
#define CM_C(x) (std::integral_constant<int, (x)>::value)

// Packed layers, in this order: 0 base.0, 1 base.1, 2 base.out, 3 encode, 4 dir.0, 5 dir.1, 6 dir.out (1 and 5 only for
// L = 2).  T = output tiles of 16, KS = input blocks of 32.  KF = input blocks of the F features, KSH = of the SH basis.
template <int S>
constexpr int cm_ksh() { return (S + 1) * (S + 1) > 32 ? 2 : 1; }

template <int L, int KF, int S>
struct CmShape {
  static constexpr int KSH = cm_ksh<S>();
  static constexpr int T[7] = {4, L == 2 ? 4 : 0, 1, 4 * KF, 4, L == 2 ? 4 : 0, 1};
  static constexpr int KS[7] = {KF, 1, 1, KSH, KF, 1, 1};
  // input tiles of 16 of the weight gradient (the SH basis is not padded to a whole block)
  static constexpr int TQ[7] = {2 * KF, 2, 2, ((S + 1) * (S + 1) + 15) / 16, 2 * KF, 2, 2};
  // transposed fragments (dx = W^T dy): output tiles = input blocks x 2, input blocks = output tiles / 2 (rounded up)
  static constexpr int TT(int l) { return 2 * KS[l]; }
  static constexpr int KT(int l) { return (T[l] + 1) / 2; }
  static constexpr int frags(int l) { return T[l] * KS[l]; }
  static constexpr int frag_off(int l) { return l == 0 ? 0 : frag_off(l - 1) + frags(l - 1); }
  static constexpr int FWD_FRAGS = frag_off(7);
  static constexpr int tfrag_off(int l) { return l == 0 ? FWD_FRAGS : tfrag_off(l - 1) + (T[l - 1] ? TT(l - 1) * KT(l - 1) : 0); }
  static constexpr int ALL_FRAGS = tfrag_off(7);
  static constexpr int bias_off(int l) { return l == 0 ? 0 : bias_off(l - 1) + 16 * T[l - 1]; }
  static constexpr int BIAS = bias_off(7);
  static constexpr int PACK_BYTES = ALL_FRAGS * 64 * 16 + BIAS * 4;
  // per-workgroup gradient slot: dW tiles (T x TQ of 16 x 16, C layout), then biases, then d_glo, then d_cam_pos
  static constexpr int dw_tiles(int l) { return T[l] * TQ[l]; }
  static constexpr int dw_off(int l) { return l == 0 ? 0 : dw_off(l - 1) + 256 * dw_tiles(l - 1); }
  static constexpr int SLOT_BIAS = dw_off(7);
  static constexpr int SLOT_GLO = SLOT_BIAS + BIAS;
  static constexpr int SLOT_CAM = SLOT_GLO + CM_MAX_FEATURES;
  static constexpr int SLOT = SLOT_CAM + 4;
};
template <int L, int KF, int S> constexpr int CmShape<L, KF, S>::T[7];
template <int L, int KF, int S> constexpr int CmShape<L, KF, S>::KS[7];
template <int L, int KF, int S> constexpr int CmShape<L, KF, S>::TQ[7];

struct CmDims {
  int P, G, F, S, n_sh;
  int out_dim[7], in_dim[7];
};

CmDims cm_dims(const GsrColorModel& m) {
  CmDims d;
  d.P = m.P; d.G = m.G; d.F = m.P + m.G; d.S = m.S; d.n_sh = (m.S + 1) * (m.S + 1);
  const int outs[7] = {2 * CM_H, 2 * CM_H, 4, 2 * d.F, 2 * CM_H, 2 * CM_H, 4};
  const int ins[7] = {d.F, CM_H, CM_H, d.n_sh, d.F, CM_H, CM_H};
  for (int l = 0; l < 7; ++l) { d.out_dim[l] = outs[l]; d.in_dim[l] = ins[l]; }
  return d;
}

// Source row of packed output row p of layer l (-1: padding).  The encoder's a rows are packed at [0, 32 KF), its b rows
// (source rows F ..) at [32 KF, 64 KF).
__host__ __device__ inline int cm_row(int l, int p, int F, int out_dim, int KF) {
  if (l == 3) {
    const int half = 32 * KF;
    if (p < half) return p < F ? p : -1;
    return p - half < F ? F + p - half : -1;
  }
  return p < out_dim ? p : -1;
}

__device__ __forceinline__ int cm_phi(int s, int g, int j) { return 32 * s + 16 * (j >> 2) + 4 * g + (j & 3); }

struct CmPackArgs {
  const float* w[7];
  const float* b[7];
  int T[7], KS[7], frag_off[7], tfrag_off[7], bias_off[7], out_dim[7], in_dim[7];
  int F, KF, total_frag_halves, total_bias;
};

// One thread per fragment lane (8 halves): forward fragments, transposed fragments, then one thread per bias float.
__global__ void __launch_bounds__(256) cm_pack_kernel(CmPackArgs a, uint4* __restrict__ frags, float* __restrict__ bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_lanes = a.total_frag_halves / 8;
  if (i < n_lanes) {
    const int frag = i >> 6, lane = i & 63, g = lane >> 4;
    for (int l = 0; l < 7; ++l) {
      if (!a.T[l]) continue;
      const int nf = a.T[l] * a.KS[l];
      const int TT = 2 * a.KS[l], KT = (a.T[l] + 1) / 2;
      const float* W = a.w[l];
      const int in_dim = a.in_dim[l];
      half8 v;
      if (frag >= a.frag_off[l] && frag < a.frag_off[l] + nf) {
        const int t = (frag - a.frag_off[l]) / a.KS[l], s = (frag - a.frag_off[l]) % a.KS[l];
        const int src = cm_row(l, 16 * t + (lane & 15), a.F, a.out_dim[l], a.KF);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int q = cm_phi(s, g, j);
          v[j] = (src >= 0 && q < in_dim) ? (_Float16)W[(int64_t)src * in_dim + q] : (_Float16)0.f;
        }
        frags[i] = *reinterpret_cast<uint4*>(&v);
        return;
      }
      if (frag >= a.tfrag_off[l] && frag < a.tfrag_off[l] + TT * KT) {
        const int t = (frag - a.tfrag_off[l]) / KT, s = (frag - a.tfrag_off[l]) % KT;
        const int q = 16 * t + (lane & 15);                 // forward input feature = output of the transpose
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int p = cm_phi(s, g, j);                    // forward packed output row = k slot of the transpose
          const int src = p < 16 * a.T[l] ? cm_row(l, p, a.F, a.out_dim[l], a.KF) : -1;
          v[j] = (src >= 0 && q < in_dim) ? (_Float16)W[(int64_t)src * in_dim + q] : (_Float16)0.f;
        }
        frags[i] = *reinterpret_cast<uint4*>(&v);
        return;
      }
    }
    return;
  }
  const int k = i - n_lanes;
  if (k >= a.total_bias) return;
  for (int l = 0; l < 7; ++l) {
    if (!a.T[l] || k < a.bias_off[l] || k >= a.bias_off[l] + 16 * a.T[l]) continue;
    const int src = cm_row(l, k - a.bias_off[l], a.F, a.out_dim[l], a.KF);
    bias[k] = src >= 0 ? a.b[l][src] : 0.f;
  }
}

// ---- per-wave building blocks -----------------------------------------------------------------------------------

template <int KS>
__device__ __forceinline__ void cm_to_half(const float (&x)[KS][8], half8 (&b)[KS], float scale) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) b[s][j] = (_Float16)(x[s][j] * scale);
}

// y[t] = init[t] + sum_s A(t, s) B(s) on v_mfma_f32_16x16x32_f16.  frags: [(t KS + s) 64 + lane] (LDS or global).
template <int T, int KS>
__device__ __forceinline__ void cm_mm(const uint4* frags, const half8 (&b)[KS], f4 (&y)[T], int lane) {
  // A volatile asm is a scheduling boundary: the fragment loads of this product are not hoisted above the previous
  // one, so the fragments of only one layer are in registers at a time.
  int opaque = 0;
  asm volatile("" : "+s"(opaque));
  frags += opaque;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const uint4 w = frags[(t * KS + s) * 64 + lane];
      y[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const half8*>(&w), b[s], y[t], 0, 0, 0);
    }
}

template <int T>
__device__ __forceinline__ void cm_bias(const float* bias, f4 (&y)[T], int g) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) y[t][r] = bias[16 * t + 4 * g + r];
}

// output tiles as row vector blocks (tile 2s -> elements 0..3 of block s, tile 2s+1 -> 4..7)
template <int T, int KS>
__device__ __forceinline__ void cm_tiles_to_blocks(const f4 (&y)[T], float (&x)[KS][8]) {
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = 2 * s + (j >> 2);
      x[s][j] = t < T ? y[t][j & 3] : 0.f;
    }
}

__device__ __forceinline__ float cm_group_sum(float v) {      // over the 4 lanes of a row
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float cm_row_sum(float v) {        // over the 16 rows of a lane group
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}
__device__ __forceinline__ float cm_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Power-of-two scale putting the wave's largest |dy| into [2^14, 2^15): no f16 overflow, no underflow of the large ones.
__device__ __forceinline__ float cm_scale_for(float amax) {
  if (!(amax > 0.f) || !(amax < INFINITY)) return 1.f;
  int e;
  frexpf(amax, &e);
  int k = 15 - e;
  k = k > 120 ? 120 : (k < -120 ? -120 : k);
  return ldexpf(1.f, k);
}

template <int T>
__device__ __forceinline__ float cm_tiles_absmax(const f4 (&y)[T]) {
  float m = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(y[t][r]));
  return cm_wave_max(m);
}

// The MLP of one branch: y0 = W0 x + b0, h0 = GLU(y0) [, y1 = W1 h0 + b1, h1 = GLU(y1)], o = Wout h + bout.
template <int L, int KF>
struct CmMlpAct {
  f4 y0[4], y1[4];
  float h0[1][8], h1[1][8];
  f4 o[1];
};

template <int T>
__device__ __forceinline__ void cm_glu(const f4 (&y)[T], float (&h)[1][8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) h[0][j] = gsr_cm_glu(y[j >> 2][j & 3], y[2 + (j >> 2)][j & 3]);
}

// weights: forward fragments of the layers l0, l0+1, l0+2 at frag offsets; biases at bias offsets
template <int L, int KF, typename Sh, int LB>
__device__ __forceinline__ void cm_mlp_fwd(const uint4* frags, const float* bias, const float (&x)[KF][8],
                                           CmMlpAct<L, KF>& a, int lane) {
  const int g = lane >> 4;
  half8 b[KF];
  cm_to_half(x, b, 1.f);
  cm_bias(bias + CM_C(Sh::bias_off(LB)), a.y0, g);
  cm_mm<4, KF>(frags + 64 * CM_C(Sh::frag_off(LB)), b, a.y0, lane);
  cm_glu(a.y0, a.h0);
  half8 bh[1];
  if constexpr (L == 2) {
    cm_to_half(a.h0, bh, 1.f);
    cm_bias(bias + CM_C(Sh::bias_off(LB + 1)), a.y1, g);
    cm_mm<4, 1>(frags + 64 * CM_C(Sh::frag_off(LB + 1)), bh, a.y1, lane);
    cm_glu(a.y1, a.h1);
    cm_to_half(a.h1, bh, 1.f);
  } else {
    cm_to_half(a.h0, bh, 1.f);
  }
  cm_bias(bias + CM_C(Sh::bias_off(LB + 2)), a.o, g);
  cm_mm<1, 1>(frags + 64 * CM_C(Sh::frag_off(LB + 2)), bh, a.o, lane);
}

// Everything the forward computes for a 16-row tile.
template <int L, int KF, int KSH>
struct CmTile {
  float x[KF][8];          // LayerNorm output
  float rstd;
  float sh[KSH][8];
  f4 e[4 * KF];            // encoder: a tiles [0, 2KF), b tiles [2KF, 4KF)
  float z[KF][8];
  CmMlpAct<L, KF> base, dir;
  float d[3], inv_norm;
  bool clamped;
};

// Loads row `row` (< M, else zeros) and normalises it: t.x, t.rstd.
template <int L, int KF, int S>
__device__ __forceinline__ void cm_ln_fwd(const float* __restrict__ pf, const float* __restrict__ glo, int64_t row,
                                          int64_t M, int P, int F, CmTile<L, KF, cm_ksh<S>()>& t, int lane) {
  const int g = lane >> 4;
  const bool valid = row < M;
  // input row: [point_features, glo], LayerNorm over F
  float u[KF][8];
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < KF; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = cm_phi(s, g, j);
      float v = 0.f;
      if (f < P) v = valid ? pf[row * P + f] : 0.f;
      else if (f < F) v = glo[f - P];
      u[s][j] = v;
      sum += v;
    }
  const float mean = cm_group_sum(sum) / (float)F;
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < KF; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dv = cm_phi(s, g, j) < F ? u[s][j] - mean : 0.f;
      u[s][j] = dv;
      ss += dv * dv;
    }
  t.rstd = gsr_cm_ln_rstd(cm_group_sum(ss), F);
#pragma unroll
  for (int s = 0; s < KF; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) t.x[s][j] = u[s][j] * t.rstd;

}

// The specular branch's forward from t.x: direction, SH basis, encoder, x a + b, MLP.
template <int L, int KF, int S>
__device__ __forceinline__ void cm_dir_fwd(const uint4* frags, const float* bias, const float* __restrict__ pos,
                                           const float* __restrict__ cam, int64_t row, int64_t M,
                                           CmTile<L, KF, cm_ksh<S>()>& t, int lane) {
  constexpr int KSH = cm_ksh<S>();
  using Sh = CmShape<L, KF, S>;
  const int g = lane >> 4;
  const bool valid = row < M;
  float v[3] = {0.f, 0.f, 0.f};
  if (valid)
    for (int k = 0; k < 3; ++k) v[k] = pos[row * 3 + k] - cam[k];
  gsr_cm_normalize(v, t.d, t.inv_norm, t.clamped);
#pragma unroll
  for (int s = 0; s < KSH; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) t.sh[s][j] = 0.f;
  gsr_cm_rsh<S>(t.d[0], t.d[1], t.d[2], [&](int c, float val) {
    const int w = c & 31;
    float& dst = t.sh[c >> 5][4 * (w >> 4) + (w & 3)];
    dst = ((w >> 2) & 3) == g ? val : dst;               // a select, not a branch: the array stays in registers
  });
  half8 bsh[KSH];
  cm_to_half(t.sh, bsh, 1.f);
  cm_bias(bias + CM_C(Sh::bias_off(3)), t.e, g);
  cm_mm<4 * KF, KSH>(frags + 64 * CM_C(Sh::frag_off(3)), bsh, t.e, lane);
#pragma unroll
  for (int s = 0; s < KF; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ta = 2 * s + (j >> 2);
      t.z[s][j] = fmaf(t.x[s][j], t.e[ta][j & 3], t.e[2 * KF + ta][j & 3]);
    }
  cm_mlp_fwd<L, KF, Sh, 4>(frags, bias, t.z, t.dir, lane);
}

template <int L, int KF, int S>
__global__ void __launch_bounds__(CM_BLOCK) cm_forward_kernel(const uint4* __restrict__ gfrags,
                                                              const float* __restrict__ gbias,
                                                              const float* __restrict__ pf, const float* __restrict__ pos,
                                                              const float* __restrict__ cam, const float* __restrict__ glo,
                                                              int64_t M, int P, int F, float* __restrict__ diffuse,
                                                              float* __restrict__ specular) {
  constexpr int KSH = cm_ksh<S>();
  using Sh = CmShape<L, KF, S>;
  __shared__ uint4 sfrags[Sh::FWD_FRAGS * 64];
  __shared__ float sbias[Sh::BIAS];
  for (int i = threadIdx.x; i < Sh::FWD_FRAGS * 64; i += CM_BLOCK) sfrags[i] = gfrags[i];
  for (int i = threadIdx.x; i < Sh::BIAS; i += CM_BLOCK) sbias[i] = gbias[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const int64_t steps = (M + CM_ROWS - 1) / CM_ROWS;
  for (int64_t st = blockIdx.x; st < steps; st += gridDim.x) {
    const int64_t row = st * CM_ROWS + 16 * wave + (lane & 15);
    // an offset the compiler cannot see through, so that the weight fragments are re-read from LDS in every step
    // instead of being hoisted out of the loop into registers
    int opaque = 0;
    asm volatile("" : "+s"(opaque));
    CmTile<L, KF, KSH> t;
    cm_ln_fwd<L, KF, S>(pf, glo, row, M, P, F, t, lane);
    cm_mlp_fwd<L, KF, Sh, 0>(sfrags + opaque, sbias + opaque, t.x, t.base, lane);
    cm_dir_fwd<L, KF, S>(sfrags + opaque, sbias + opaque, pos, cam, row, M, t, lane);
    if (g == 0 && row < M) {
      float o[4], out[3];
      for (int r = 0; r < 4; ++r) o[r] = t.base.o[0][r];
      gsr_cm_lum(o, 0.f, out);
      for (int c = 0; c < 3; ++c) diffuse[row * 3 + c] = out[c];
      for (int r = 0; r < 4; ++r) o[r] = t.dir.o[0][r];
      gsr_cm_lum(o, GSR_CM_SPEC_BIAS, out);
      for (int c = 0; c < 3; ++c) specular[row * 3 + c] = out[c];
    }
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------

constexpr int CM_STAGE_DY = 128;      // staged dy features per wave (the encoder's 4 KF tiles at most)
constexpr int CM_STAGE_X = 64;        // staged input features per wave

struct CmStage {
  _Float16 dy[4][CM_STAGE_DY][16];
  _Float16 x[4][CM_STAGE_X][16];
  float scale[4];
  float glo[4][CM_MAX_FEATURES];
  float cam[4][4];
};

// dW accumulators of one layer: wave w owns tiles w, w + 4, ... of the T x TQ tiles.
template <int T, int TQ>
struct CmAcc {
  static constexpr int N = (T * TQ + 3) / 4;
  f4 a[N > 0 ? N : 1];
  float bias;
};

template <int T, int TQ>
__device__ __forceinline__ void cm_acc_init(CmAcc<T, TQ>& acc) {
#pragma unroll
  for (int i = 0; i < CmAcc<T, TQ>::N; ++i) acc.a[i] = f4{0.f, 0.f, 0.f, 0.f};
  acc.bias = 0.f;
}

// Stage this wave's dy (output tiles, times `scale`) and layer input (KS blocks), then, after the barrier, add the
// workgroup's 64 rows into the owned dW tiles and the bias sums.  Every wave of the block calls this in step.
template <int T, int KS, int TQ = 2 * KS>
__device__ __forceinline__ void cm_dw(CmStage& st, CmAcc<T, TQ>& acc, const f4 (&dy)[T], const float (&x)[KS][8],
                                      float scale, int lane, int wave) {
  const int g = lane >> 4, r16 = lane & 15;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) st.dy[wave][16 * t + 4 * g + r][r16] = (_Float16)(dy[t][r] * scale);
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) st.x[wave][cm_phi(s, g, j)][r16] = (_Float16)x[s][j];
  if (lane == 0) st.scale[wave] = scale;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CmAcc<T, TQ>::N; ++i) {
    const int tile = wave + 4 * i;
    if (tile < T * TQ) {
      const int tp = tile / TQ, tq = tile % TQ;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const half4 A = *reinterpret_cast<const half4*>(&st.dy[w][16 * tp + r16][4 * g]);
        const half4 B = *reinterpret_cast<const half4*>(&st.x[w][16 * tq + r16][4 * g]);
        const f4 p = __builtin_amdgcn_mfma_f32_16x16x16f16(A, B, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const float inv = 1.f / st.scale[w];
        acc.a[i] += p * inv;
      }
    }
  }
  const int p = threadIdx.x;
  if (p < 16 * T) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += (float)st.dy[w][p][r];
      acc.bias += s / st.scale[w];
    }
  }
  __syncthreads();
}

template <int T, int TQ>
__device__ __forceinline__ void cm_acc_store(const CmAcc<T, TQ>& acc, float* slot, int dw_off, int bias_off, int lane,
                                             int wave) {
#pragma unroll
  for (int i = 0; i < CmAcc<T, TQ>::N; ++i) {
    const int tile = wave + 4 * i;
    if (tile < T * TQ) reinterpret_cast<f4*>(slot + dw_off + 256 * tile)[lane] = acc.a[i];
  }
  if ((int)threadIdx.x < 16 * T) slot[bias_off + threadIdx.x] = acc.bias;
}

// dx blocks (KO blocks of 32 outputs) = W^T dy, with dy scaled into f16 and the product scaled back.
template <int T, int KO>
__device__ __forceinline__ void cm_dx(const uint4* tfrags, const f4 (&dy)[T], float scale, float (&dx)[KO][8], int lane) {
  constexpr int KT = (T + 1) / 2;
  float blocks[KT][8];
  cm_tiles_to_blocks<T, KT>(dy, blocks);
  half8 b[KT];
  cm_to_half(blocks, b, scale);
  f4 y[2 * KO];
#pragma unroll
  for (int t = 0; t < 2 * KO; ++t) y[t] = f4{0.f, 0.f, 0.f, 0.f};
  cm_mm<2 * KO, KT>(tfrags, b, y, lane);
  const float inv = 1.f / scale;
#pragma unroll
  for (int t = 0; t < 2 * KO; ++t) y[t] *= inv;
  cm_tiles_to_blocks<2 * KO, KO>(y, dx);
}

template <int L, int KF>
struct CmMlpAccs {
  CmAcc<4, 2 * KF> l0;
  CmAcc<L == 2 ? 4 : 0, 2> l1;
  CmAcc<1, 2> out;
};

template <int L, int KF>
__device__ __forceinline__ void cm_mlp_accs_init(CmMlpAccs<L, KF>& a) {
  cm_acc_init(a.l0);
  cm_acc_init(a.l1);
  cm_acc_init(a.out);
}

// Back through a GLU: dh (one block) -> dy of the 4 pre-activation tiles
__device__ __forceinline__ void cm_glu_bwd(const f4 (&y)[4], const float (&dh)[1][8], f4 (&dy)[4]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float da, db;
    gsr_cm_glu_bwd(y[j >> 2][j & 3], y[2 + (j >> 2)][j & 3], dh[0][j], da, db);
    dy[j >> 2][j & 3] = da;
    dy[2 + (j >> 2)][j & 3] = db;
  }
}

// Back through one branch's MLP from d_o (out tile, group 0 holds outputs 0..3): dW into accs, returns dx of its input.
template <int L, int KF, typename Sh, int LB>
__device__ __forceinline__ void cm_mlp_bwd(const uint4* gfrags, const CmMlpAct<L, KF>& a, const float (&x)[KF][8],
                                           const f4 (&d_o)[1], CmMlpAccs<L, KF>& acc, CmStage& st, float (&dx)[KF][8],
                                           int lane, int wave) {
  // output layer
  float s = cm_scale_for(cm_tiles_absmax(d_o));
  cm_dw<1, 1>(st, acc.out, d_o, L == 2 ? a.h1 : a.h0, s, lane, wave);
  float dh[1][8];
  cm_dx<1, 1>(gfrags + 64 * CM_C(Sh::tfrag_off(LB + 2)), d_o, s, dh, lane);
  f4 dy[4];
  if constexpr (L == 2) {
    cm_glu_bwd(a.y1, dh, dy);
    s = cm_scale_for(cm_tiles_absmax(dy));
    cm_dw<4, 1>(st, acc.l1, dy, a.h0, s, lane, wave);
    cm_dx<4, 1>(gfrags + 64 * CM_C(Sh::tfrag_off(LB + 1)), dy, s, dh, lane);
  }
  cm_glu_bwd(a.y0, dh, dy);
  s = cm_scale_for(cm_tiles_absmax(dy));
  cm_dw<4, KF>(st, acc.l0, dy, x, s, lane, wave);
  cm_dx<4, KF>(gfrags + 64 * CM_C(Sh::tfrag_off(LB)), dy, s, dx, lane);
}

template <int L, int KF, typename Sh, int LB>
__device__ __forceinline__ void cm_mlp_accs_store(const CmMlpAccs<L, KF>& a, float* slot, int lane, int wave) {
  cm_acc_store(a.l0, slot, CM_C(Sh::dw_off(LB)), Sh::SLOT_BIAS + CM_C(Sh::bias_off(LB)), lane, wave);
  if constexpr (L == 2) cm_acc_store(a.l1, slot, CM_C(Sh::dw_off(LB + 1)), Sh::SLOT_BIAS + CM_C(Sh::bias_off(LB + 1)), lane, wave);
  cm_acc_store(a.out, slot, CM_C(Sh::dw_off(LB + 2)), Sh::SLOT_BIAS + CM_C(Sh::bias_off(LB + 2)), lane, wave);
}

template <int L, int KF, int S>
__global__ void __launch_bounds__(CM_BLOCK) cm_backward_kernel(
    const uint4* __restrict__ gfrags, const float* __restrict__ gbias, const float* __restrict__ pf,
    const float* __restrict__ pos, const float* __restrict__ cam, const float* __restrict__ glo, int64_t M, int P, int F,
    const float* __restrict__ d_diffuse, const float* __restrict__ d_specular, int want_cam,
    float* __restrict__ d_pf, float* __restrict__ slots) {
  constexpr int KSH = cm_ksh<S>();
  using Sh = CmShape<L, KF, S>;
  __shared__ CmStage st;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, r16 = lane & 15;
  const bool has_d = d_diffuse != nullptr, has_s = d_specular != nullptr;
  const bool cam_grad = has_s && want_cam;
  CmMlpAccs<L, KF> acc_base, acc_dir;
  CmAcc<4 * KF, Sh::TQ[3]> acc_enc;
  cm_mlp_accs_init(acc_base);
  cm_mlp_accs_init(acc_dir);
  cm_acc_init(acc_enc);
  float acc_glo = 0.f, acc_cam[3] = {0.f, 0.f, 0.f};

  const int64_t steps = (M + CM_ROWS - 1) / CM_ROWS;
  for (int64_t stp = blockIdx.x; stp < steps; stp += gridDim.x) {
    const int64_t row = stp * CM_ROWS + 16 * wave + r16;
    const bool valid = row < M;
    int opaque = 0;                        // as in cm_forward_kernel: no hoisting of the fragment loads
    asm volatile("" : "+s"(opaque));
    const uint4* frags = gfrags + opaque;
    CmTile<L, KF, KSH> t;
    cm_ln_fwd<L, KF, S>(pf, glo, row, M, P, F, t, lane);
    float dx[KF][8];
#pragma unroll
    for (int s = 0; s < KF; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) dx[s][j] = 0.f;

    if (has_d) {
      cm_mlp_fwd<L, KF, Sh, 0>(frags, gbias + opaque, t.x, t.base, lane);
      f4 d_o[1] = {f4{0.f, 0.f, 0.f, 0.f}};
      if (g == 0 && valid) {
        float o[4], dout[3], dq[4];
        for (int r = 0; r < 4; ++r) o[r] = t.base.o[0][r];
        for (int c = 0; c < 3; ++c) dout[c] = d_diffuse[row * 3 + c];
        gsr_cm_lum_bwd(o, 0.f, dout, dq);
        for (int r = 0; r < 4; ++r) d_o[0][r] = dq[r];
      }
      float dxb[KF][8];
      cm_mlp_bwd<L, KF, Sh, 0>(frags, t.base, t.x, d_o, acc_base, st, dxb, lane, wave);
#pragma unroll
      for (int s = 0; s < KF; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) dx[s][j] += dxb[s][j];
    }
    if (has_s) {
      cm_dir_fwd<L, KF, S>(frags, gbias + opaque, pos, cam, row, M, t, lane);
      f4 d_o[1] = {f4{0.f, 0.f, 0.f, 0.f}};
      if (g == 0 && valid) {
        float o[4], dout[3], dq[4];
        for (int r = 0; r < 4; ++r) o[r] = t.dir.o[0][r];
        for (int c = 0; c < 3; ++c) dout[c] = d_specular[row * 3 + c];
        gsr_cm_lum_bwd(o, GSR_CM_SPEC_BIAS, dout, dq);
        for (int r = 0; r < 4; ++r) d_o[0][r] = dq[r];
      }
      float dz[KF][8];
      cm_mlp_bwd<L, KF, Sh, 4>(frags, t.dir, t.z, d_o, acc_dir, st, dz, lane, wave);
      // z = x a + b
      f4 de[4 * KF];
#pragma unroll
      for (int s = 0; s < KF; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ta = 2 * s + (j >> 2);
          dx[s][j] += dz[s][j] * t.e[ta][j & 3];
          de[ta][j & 3] = dz[s][j] * t.x[s][j];
          de[2 * KF + ta][j & 3] = dz[s][j];
        }
      const float se = cm_scale_for(cm_tiles_absmax(de));
      cm_dw<4 * KF, KSH, Sh::TQ[3]>(st, acc_enc, de, t.sh, se, lane, wave);
      if (cam_grad) {
        float dsh[KSH][8];
        cm_dx<4 * KF, KSH>(frags + 64 * CM_C(Sh::tfrag_off(3)), de, se, dsh, lane);
        float dd[3] = {0.f, 0.f, 0.f};
        asm volatile("");                   // scheduling boundary: the SH derivative is not interleaved with the MFMAs
        gsr_cm_rsh<S>(GsrDual3{t.d[0], 1.f, 0.f, 0.f}, GsrDual3{t.d[1], 0.f, 1.f, 0.f}, GsrDual3{t.d[2], 0.f, 0.f, 1.f},
                      [&](int c, GsrDual3 val) {
                        const int w = c & 31;
                        const float k = ((w >> 2) & 3) == g ? dsh[c >> 5][4 * (w >> 4) + (w & 3)] : 0.f;
                        dd[0] += k * val.dx;
                        dd[1] += k * val.dy;
                        dd[2] += k * val.dz;
                      });
        for (int k = 0; k < 3; ++k) dd[k] = cm_group_sum(dd[k]);
        float dv[3];
        gsr_cm_normalize_bwd(t.d, t.inv_norm, t.clamped, dd, dv);
        for (int k = 0; k < 3; ++k) acc_cam[k] -= cm_row_sum(valid ? dv[k] : 0.f);
      }
    }
    // LayerNorm backward
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int s = 0; s < KF; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) { s1 += dx[s][j]; s2 += dx[s][j] * t.x[s][j]; }
    s1 = cm_group_sum(s1);
    s2 = cm_group_sum(s2);
#pragma unroll
    for (int s = 0; s < KF; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int f = cm_phi(s, g, j);
        const float du = valid ? gsr_cm_ln_bwd(t.x[s][j], dx[s][j], t.rstd, s1, s2, F) : 0.f;
        if (f < P && valid) d_pf[row * P + f] = du;
        const float gs = cm_row_sum(f >= P && f < F ? du : 0.f);
        if (r16 == 8 * s + j) acc_glo += gs;
      }
  }

  // the workgroup's slot
  float* slot = slots + (int64_t)blockIdx.x * Sh::SLOT;
  cm_mlp_accs_store<L, KF, Sh, 0>(acc_base, slot, lane, wave);
  cm_acc_store(acc_enc, slot, CM_C(Sh::dw_off(3)), Sh::SLOT_BIAS + CM_C(Sh::bias_off(3)), lane, wave);
  cm_mlp_accs_store<L, KF, Sh, 4>(acc_dir, slot, lane, wave);
  if (r16 < 8 * KF) st.glo[wave][cm_phi(r16 >> 3, g, r16 & 7)] = acc_glo;
  if (r16 >= 8 * KF)
    for (int s = KF; s < 2; ++s) st.glo[wave][cm_phi(s, g, r16 & 7)] = 0.f;
  if (lane == 0)
    for (int k = 0; k < 3; ++k) st.cam[wave][k] = acc_cam[k];
  __syncthreads();
  if (threadIdx.x < CM_MAX_FEATURES) {
    float s = 0.f;
    for (int w = 0; w < 4; ++w) s += st.glo[w][threadIdx.x];
    slot[Sh::SLOT_GLO + threadIdx.x] = s;
  }
  if (threadIdx.x < 4) {
    float s = 0.f;
    if (threadIdx.x < 3)
      for (int w = 0; w < 4; ++w) s += st.cam[w][threadIdx.x];
    slot[Sh::SLOT_CAM + threadIdx.x] = s;
  }
}

struct CmOut {
  float* dw[7];
  float* db[7];
  float* d_glo;
  float* d_cam;
  int out_dim[7], in_dim[7];
  int F, P, KF;
};

// One thread per slot float: the sum over workgroups 0 .. n_wg-1 in order, written to its parameter's gradient.
template <int L, int KF, int S>
__global__ void __launch_bounds__(256) cm_finish_kernel(const float* __restrict__ slots, int n_wg, CmOut o) {
  using Sh = CmShape<L, KF, S>;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Sh::SLOT) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int w = 0;
  for (; w + 4 <= n_wg; w += 4)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += slots[(int64_t)(w + k) * Sh::SLOT + e];
  for (int k = 0; w < n_wg; ++w, ++k) acc[k] += slots[(int64_t)w * Sh::SLOT + e];
  const float v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (e < Sh::SLOT_BIAS) {
    for (int l = 0; l < 7; ++l) {
      if (!Sh::T[l] || e < Sh::dw_off(l) || e >= Sh::dw_off(l) + 256 * Sh::dw_tiles(l)) continue;
      const int rel = e - Sh::dw_off(l), tile = rel >> 8, within = rel & 255, lane = within >> 2, r = within & 3;
      const int TQ = Sh::TQ[l];
      const int p = 16 * (tile / TQ) + 4 * (lane >> 4) + r, q = 16 * (tile % TQ) + (lane & 15);
      const int src = cm_row(l, p, o.F, o.out_dim[l], o.KF);
      if (src >= 0 && q < o.in_dim[l]) o.dw[l][(int64_t)src * o.in_dim[l] + q] = v;
    }
  } else if (e < Sh::SLOT_GLO) {
    const int k = e - Sh::SLOT_BIAS;
    for (int l = 0; l < 7; ++l) {
      if (!Sh::T[l] || k < Sh::bias_off(l) || k >= Sh::bias_off(l) + 16 * Sh::T[l]) continue;
      const int src = cm_row(l, k - Sh::bias_off(l), o.F, o.out_dim[l], o.KF);
      if (src >= 0) o.db[l][src] = v;
    }
  } else if (e < Sh::SLOT_CAM) {
    const int f = e - Sh::SLOT_GLO;
    if (f >= o.P && f < o.F) o.d_glo[f - o.P] = v;
  } else {
    const int k = e - Sh::SLOT_CAM;
    if (k < 3 && o.d_cam) o.d_cam[k] = v;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------

bool cm_supported(const GsrColorModel* m) {
  return m && m->H == CM_H && (m->L == 1 || m->L == 2) && m->S >= 2 && m->S <= 5 && m->P >= 0 && m->G >= 0 &&
         m->P + m->G >= 1 && m->P + m->G <= CM_MAX_FEATURES && m->color_channels == 3;
}

bool cm_params_present(const GsrColorModel* m) {
  for (int l = 0; l < 7; ++l) {
    const bool need = m->L == 2 || (l != 1 && l != 5);
    if (need && (!m->weight[l] || !m->bias[l])) return false;
  }
  return true;
}

template <int L, int KF, int S>
CmPackArgs cm_pack_args(const GsrColorModel& m) {
  using Sh = CmShape<L, KF, S>;
  const CmDims d = cm_dims(m);
  CmPackArgs a{};
  for (int l = 0; l < 7; ++l) {
    a.w[l] = m.weight[l];
    a.b[l] = m.bias[l];
    a.T[l] = Sh::T[l];
    a.KS[l] = Sh::KS[l];
    a.frag_off[l] = Sh::frag_off(l);
    a.tfrag_off[l] = Sh::tfrag_off(l);
    a.bias_off[l] = Sh::bias_off(l);
    a.out_dim[l] = d.out_dim[l];
    a.in_dim[l] = d.in_dim[l];
  }
  a.F = d.F;
  a.KF = KF;
  a.total_frag_halves = Sh::ALL_FRAGS * 64 * 8;
  a.total_bias = Sh::BIAS;
  return a;
}

template <int L, int KF, int S>
int cm_pack(const GsrColorModel& m, void* packed, hipStream_t stream) {
  using Sh = CmShape<L, KF, S>;
  const CmPackArgs a = cm_pack_args<L, KF, S>(m);
  uint4* frags = reinterpret_cast<uint4*>(packed);
  float* bias = reinterpret_cast<float*>(frags + Sh::ALL_FRAGS * 64);
  const int n = Sh::ALL_FRAGS * 64 + Sh::BIAS;
  cm_pack_kernel<<<grid_for(n, 256), 256, 0, stream>>>(a, frags, bias);
  return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_LAUNCH_FAILED;
}

int64_t cm_bwd_wg(int64_t M) {
  const int64_t steps = (M + CM_ROWS - 1) / CM_ROWS;
  return steps < CM_BWD_MAX_WG ? steps : CM_BWD_MAX_WG;
}

struct CmCall {
  const GsrColorModel* m;
  const float *pf, *pos, *cam, *glo;
  int64_t M;
  float *diffuse, *specular;
  const float *d_diffuse, *d_specular;
  float* d_pf;
  const GsrColorGrads* grads;
  void* ws;
  size_t ws_bytes;
  hipStream_t stream;
};

template <int L, int KF, int S>
int cm_forward_t(const CmCall& c) {
  constexpr int KSH = cm_ksh<S>();
  using Sh = CmShape<L, KF, S>;
  if (c.ws_bytes < (size_t)Sh::PACK_BYTES) return GSR_ERR_WORKSPACE_TOO_SMALL;
  int rc = cm_pack<L, KF, S>(*c.m, c.ws, c.stream);
  if (rc) return rc;
  if (c.M == 0) return GSR_OK;
  const uint4* frags = reinterpret_cast<const uint4*>(c.ws);
  const float* bias = reinterpret_cast<const float*>(frags + Sh::ALL_FRAGS * 64);
  const int64_t steps = (c.M + CM_ROWS - 1) / CM_ROWS;
  const unsigned grid = (unsigned)(steps < CM_FWD_MAX_WG ? steps : CM_FWD_MAX_WG);
  cm_forward_kernel<L, KF, S><<<grid, CM_BLOCK, 0, c.stream>>>(frags, bias, c.pf, c.pos, c.cam, c.glo, c.M, c.m->P,
                                                               c.m->P + c.m->G, c.diffuse, c.specular);
  return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_LAUNCH_FAILED;
}

template <int L, int KF, int S>
size_t cm_bwd_ws_t(int64_t M) {
  constexpr int KSH = cm_ksh<S>();
  using Sh = CmShape<L, KF, S>;
  return (size_t)Sh::PACK_BYTES + sizeof(float) * (size_t)Sh::SLOT * (size_t)cm_bwd_wg(M);
}

template <int L, int KF, int S>
int cm_backward_t(const CmCall& c) {
  constexpr int KSH = cm_ksh<S>();
  using Sh = CmShape<L, KF, S>;
  if (c.ws_bytes < cm_bwd_ws_t<L, KF, S>(c.M)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  int rc = cm_pack<L, KF, S>(*c.m, c.ws, c.stream);
  if (rc) return rc;
  const uint4* frags = reinterpret_cast<const uint4*>(c.ws);
  const float* bias = reinterpret_cast<const float*>(frags + Sh::ALL_FRAGS * 64);
  float* slots = reinterpret_cast<float*>(reinterpret_cast<char*>(c.ws) + Sh::PACK_BYTES);
  const int64_t wg = cm_bwd_wg(c.M);
  const int want_cam = c.grads->d_cam_pos != nullptr;
  if (wg > 0) {
    cm_backward_kernel<L, KF, S><<<(unsigned)wg, CM_BLOCK, 0, c.stream>>>(
        frags, bias, c.pf, c.pos, c.cam, c.glo, c.M, c.m->P, c.m->P + c.m->G, c.d_diffuse, c.d_specular, want_cam, c.d_pf,
        slots);
    GSR_CHECK_LAUNCH();
  }
  const CmDims d = cm_dims(*c.m);
  CmOut o{};
  for (int l = 0; l < 7; ++l) {
    o.dw[l] = c.grads->d_weight[l];
    o.db[l] = c.grads->d_bias[l];
    o.out_dim[l] = d.out_dim[l];
    o.in_dim[l] = d.in_dim[l];
  }
  o.d_glo = c.grads->d_glo;
  o.d_cam = c.grads->d_cam_pos;
  o.F = d.F;
  o.P = d.P;
  o.KF = KF;
  cm_finish_kernel<L, KF, S><<<grid_for(Sh::SLOT, 256), 256, 0, c.stream>>>(slots, (int)wg, o);
  return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_LAUNCH_FAILED;
}

// dispatch on (L, KF, S): f(l, kf, s) gets the model's shape as three std::integral_constant
template <class F>
void cm_dispatch(const GsrColorModel* m, F&& f) {
  gsr_pick<1, 2>(m->L, [&](auto l) {
    gsr_pick<1, 2>(m->P + m->G <= 32 ? 1 : 2, [&](auto kf) {
      gsr_pick<2, 3, 4, 5>(m->S, [&](auto s) { f(l, kf, s); });
    });
  });
}

}  // namespace

extern "C" {

int64_t gsr_color_struct_bytes(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(GsrColorModel);
    case 1: return (int64_t)sizeof(GsrColorGrads);
    default: return -1;
  }
}

int gsr_color_supported(const GsrColorModel* m) { return cm_supported(m) ? GSR_OK : GSR_ERR_UNSUPPORTED; }

size_t gsr_color_forward_workspace_bytes(const GsrColorModel* m) {
  if (!cm_supported(m)) return 0;
  size_t bytes = 0;
  cm_dispatch(m, [&](auto l, auto kf, auto s) {
    bytes = (size_t)CmShape<decltype(l)::value, decltype(kf)::value, decltype(s)::value>::PACK_BYTES;
  });
  return bytes;
}

size_t gsr_color_backward_workspace_bytes(const GsrColorModel* m, int64_t M) {
  if (!cm_supported(m) || M < 0) return 0;
  size_t bytes = 0;
  cm_dispatch(m, [&](auto l, auto kf, auto s) {
    bytes = cm_bwd_ws_t<decltype(l)::value, decltype(kf)::value, decltype(s)::value>(M);
  });
  return bytes;
}

int gsr_color_forward(const GsrColorModel* m, const float* point_features, const float* positions, const float* cam_pos,
                      const float* glo_feature, int64_t M, float* diffuse_out, float* specular_out, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!cm_supported(m)) return GSR_ERR_UNSUPPORTED;
  if (M < 0 || !cm_params_present(m) || !cam_pos || (m->G > 0 && !glo_feature) || !workspace) return GSR_ERR_INVALID_ARGUMENT;
  if (M > 0 && ((m->P > 0 && !point_features) || !positions || !diffuse_out || !specular_out)) return GSR_ERR_INVALID_ARGUMENT;
  CmCall c{m, point_features, positions, cam_pos, glo_feature, M, diffuse_out, specular_out, nullptr, nullptr, nullptr,
           nullptr, workspace, workspace_bytes, gsr_stream(stream)};
  int rc = GSR_OK;
  cm_dispatch(m, [&](auto l, auto kf, auto s) {
    rc = cm_forward_t<decltype(l)::value, decltype(kf)::value, decltype(s)::value>(c);
  });
  return rc;
}

int gsr_color_backward(const GsrColorModel* m, const float* point_features, const float* positions, const float* cam_pos,
                       const float* glo_feature, int64_t M, const float* d_diffuse, const float* d_specular,
                       float* d_point_features, const GsrColorGrads* grads, void* workspace, size_t workspace_bytes,
                       void* stream) {
  if (!cm_supported(m)) return GSR_ERR_UNSUPPORTED;
  if (M < 0 || !cm_params_present(m) || !cam_pos || (m->G > 0 && (!glo_feature || !grads || !grads->d_glo)) || !grads ||
      !workspace)
    return GSR_ERR_INVALID_ARGUMENT;
  for (int l = 0; l < 7; ++l) {
    const bool need = m->L == 2 || (l != 1 && l != 5);
    if (need && (!grads->d_weight[l] || !grads->d_bias[l])) return GSR_ERR_INVALID_ARGUMENT;
  }
  if (M > 0 && ((m->P > 0 && (!point_features || !d_point_features)) || !positions)) return GSR_ERR_INVALID_ARGUMENT;
  CmCall c{m, point_features, positions, cam_pos, glo_feature, M, nullptr, nullptr, d_diffuse, d_specular,
           d_point_features, grads, workspace, workspace_bytes, gsr_stream(stream)};
  int rc = GSR_OK;
  cm_dispatch(m, [&](auto l, auto kf, auto s) {
    rc = cm_backward_t<decltype(l)::value, decltype(kf)::value, decltype(s)::value>(c);
  });
  return rc;
}

}  // extern "C"
