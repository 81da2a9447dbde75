// Scene regulariser (the reference's MLPScene.compute_reg / reg_loss, mlp_scene.py:246-288) and the scene's post-step
// projection (mlp_scene.py:236-237).
//
// Regulariser, per row i of the M culled points (j = idx[i] is its row of the N-row log_scaling):
//   s = exp(log_scaling[j]); norm = (s . s) / depth^2; aspect = max(s) / min(s); op = (1 - exp(-4 opacity))^2 norm;
//   spec = |specular_0| + |specular_1| + |specular_2| (0 without a specular tensor); w = visibility (or 1)
//   term_k = sum over rows with visibility > 0 of {norm, op, aspect, spec}_k w / count;  loss = sum_k weight_k term_k,
// a zero weight dropping its term.  The mask visibility > 0 is applied here, over all M rows: nothing is compacted and
// the count never leaves the device.  count = 0 gives terms 0, loss 0 and zero gradients.
//   forward:  reg_fwd_kernel, a grid fixed by M alone, each block writing one slot of 4 float sums + the row count
//             (rows of a thread in ascending order, DPP row sums, the block's 16 rows in order); reg_finish_kernel, one
//             block, adds the slots (thread t: t, t + 256, ...; then the same block sum).  No float atomics: two runs
//             give the same bits.
//   backward: reg_bwd_kernel, one thread per row: d_opacity, d_depths, d_specular written for every row (zero where
//             masked) and the log_scaling term added into row idx[i] of the N-row gradient (rows of idx are unique: a
//             plain read-modify-write).  visibility is a constant.
#include "gsr_device.h"
#include "gsr_dpp_reduce.h"
#include "gsr_host.h"

namespace {

constexpr int REG_BLOCK = 256;
constexpr int REG_MAX_BLOCKS = 1024;             // 4 per CU
constexpr int REG_SLOT = 5;                      // 4 sums + the count (stored as its bit pattern)

struct RegRow {
  float norm, aspect, sat, e4, s2[3], spec, w;
  int k_max, k_min;
};

// the row's terms; first largest / first smallest scale take the aspect term's gradient
__device__ __forceinline__ RegRow reg_row(const GsrReg& a, int64_t i, float vis) {
  RegRow r;
  const int64_t j = a.idx[i];
  const float* ls = a.log_scaling + 3 * j;
  const float s0 = expf(ls[0]), s1 = expf(ls[1]), s2 = expf(ls[2]);
  r.s2[0] = s0 * s0; r.s2[1] = s1 * s1; r.s2[2] = s2 * s2;
  const float depth = a.depths[i];
  r.norm = (r.s2[0] + r.s2[1] + r.s2[2]) / (depth * depth);
  float smax = s0, smin = s0;
  r.k_max = 0; r.k_min = 0;
  if (s1 > smax) { smax = s1; r.k_max = 1; }
  if (s2 > smax) { smax = s2; r.k_max = 2; }
  if (s1 < smin) { smin = s1; r.k_min = 1; }
  if (s2 < smin) { smin = s2; r.k_min = 2; }
  r.aspect = smax / smin;
  r.e4 = expf(-4.f * a.opacity[i]);
  r.sat = 1.f - r.e4;
  r.spec = 0.f;
  if (a.specular) {
    const float* sp = a.specular + 3 * i;
    r.spec = fabsf(sp[0]) + fabsf(sp[1]) + fabsf(sp[2]);
  }
  r.w = a.visibility_weighted ? vis : 1.f;
  return r;
}

// block sum in a fixed order: DPP row sums (gsr_dpp_reduce.h), then the block's 16 rows of 16 lanes in order through
// LDS; valid in thread 0.  The four sums of a kernel share one hand-off array: the barrier keeps a publish off the
// previous sum's reads.
__device__ __forceinline__ float reg_rows_sum(float v) {
  const float row[1] = {gsr_row_sum_to_lane15(v)};
  __syncthreads();
  const GsrRows<1>& s_rows = gsr_block_rows_handoff(row);
  return threadIdx.x == 0 ? gsr_rows_sum(s_rows, 0) : 0.f;
}

__device__ __forceinline__ uint32_t reg_count(uint32_t v) {      // the block's count; valid in thread 0
  v = gsr_wave_sum_u32(v);
  __syncthreads();
  const GsrWaves<uint32_t>& s_wave = gsr_block_handoff(v);
  return threadIdx.x == 0 ? s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3] : 0u;
}

__global__ __launch_bounds__(REG_BLOCK) void reg_fwd_kernel(GsrReg a, float* __restrict__ slots) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t n = 0;
  for (int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x; i < a.M; i += (int64_t)gridDim.x * REG_BLOCK) {
    const float vis = a.visibility[i];
    if (!(vis > 0.f) || (uint64_t)a.idx[i] >= (uint64_t)a.N) continue;     // (a row outside log_scaling counts as masked)
    const RegRow r = reg_row(a, i, vis);
    acc[0] += r.norm * r.w;
    acc[1] += r.sat * r.sat * r.norm * r.w;
    acc[2] += r.aspect * r.w;
    acc[3] += r.spec * r.w;
    ++n;
  }
  float* slot = slots + (int64_t)blockIdx.x * REG_SLOT;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t = reg_rows_sum(acc[k]);
    if (threadIdx.x == 0) slot[k] = t;
  }
  const uint32_t c = reg_count(n);
  if (threadIdx.x == 0) slot[4] = __uint_as_float(c);
}

// terms_out: scale, opacity, aspect, specular (unweighted means) and the count as a float
__global__ __launch_bounds__(REG_BLOCK) void reg_finish_kernel(const float* __restrict__ slots, int n_slots, GsrReg a,
                                                                float* __restrict__ loss_out,
                                                                float* __restrict__ terms_out) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t n = 0;
  for (int b = threadIdx.x; b < n_slots; b += REG_BLOCK) {
    const float* slot = slots + (int64_t)b * REG_SLOT;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += slot[k];
    n += __float_as_uint(slot[4]);
  }
  float total[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) total[k] = reg_rows_sum(acc[k]);
  const uint32_t count = reg_count(n);
  if (threadIdx.x == 0) {
    float loss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float term = count ? total[k] / (float)count : 0.f;
      terms_out[k] = term;
      if (a.weight[k] != 0.f) loss += a.weight[k] * term;
    }
    terms_out[4] = (float)count;
    loss_out[0] = loss;
  }
}

__global__ __launch_bounds__(REG_BLOCK) void reg_bwd_kernel(GsrReg a, const float* __restrict__ terms,
                                                             const float* __restrict__ d_loss,
                                                             float* __restrict__ d_opacity, float* __restrict__ d_depths,
                                                             float* __restrict__ d_specular,
                                                             float* __restrict__ d_log_scaling) {
  const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
  if (i >= a.M) return;
  const float vis = a.visibility[i];
  const float count = terms[4];
  float d_op = 0.f, d_dep = 0.f, d_sp[3] = {0.f, 0.f, 0.f};
  if (vis > 0.f && count > 0.f && (uint64_t)a.idx[i] < (uint64_t)a.N) {
    const RegRow r = reg_row(a, i, vis);
    const float c = r.w * (d_loss[0] / count);
    const float w_scale = a.weight[0] != 0.f ? a.weight[0] * c : 0.f;
    const float w_op = a.weight[1] != 0.f ? a.weight[1] * c : 0.f;
    const float w_aspect = a.weight[2] != 0.f ? a.weight[2] * c : 0.f;
    const float w_spec = a.weight[3] != 0.f ? a.weight[3] * c : 0.f;
    const float d_norm = w_scale + w_op * r.sat * r.sat;
    d_op = w_op * r.norm * 8.f * r.sat * r.e4;
    const float depth = a.depths[i];
    d_dep = -2.f * d_norm * r.norm / depth;
    if (d_log_scaling) {
      const float inv_d2 = 1.f / (depth * depth);
      const float da = w_aspect * r.aspect;
      float* g = d_log_scaling + 3 * a.idx[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float d = 2.f * d_norm * r.s2[k] * inv_d2;
        if (k == r.k_max) d += da;
        if (k == r.k_min) d -= da;
        g[k] += d;
      }
    }
    if (a.specular && d_specular) {
      const float* sp = a.specular + 3 * i;
#pragma unroll
      for (int k = 0; k < 3; ++k) d_sp[k] = sp[k] > 0.f ? w_spec : (sp[k] < 0.f ? -w_spec : 0.f);
    }
  }
  if (d_opacity) d_opacity[i] = d_op;
  if (d_depths) d_depths[i] = d_dep;
  if (d_specular) {
#pragma unroll
    for (int k = 0; k < 3; ++k) d_specular[3 * i + k] = d_sp[k];
  }
}

// rotation row -> F.normalize(dim=1, eps): v / max(|v|, eps); the row's three log-scales -> clamp(lo, hi), NaN kept
__global__ __launch_bounds__(REG_BLOCK) void scene_post_step_kernel(float4* __restrict__ rotation,
                                                                     float* __restrict__ log_scaling, int64_t N,
                                                                     float eps, float lo, float hi) {
  const int64_t i = (int64_t)blockIdx.x * REG_BLOCK + threadIdx.x;
  if (i >= N) return;
  float4 q = rotation[i];
  const float d = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), eps);
  q.x /= d; q.y /= d; q.z /= d; q.w /= d;
  rotation[i] = q;
  float* ls = log_scaling + 3 * i;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v = ls[k];
    ls[k] = v != v ? v : fminf(fmaxf(v, lo), hi);
  }
}

int reg_blocks(int64_t M) {
  const int64_t b = (M + REG_BLOCK - 1) / REG_BLOCK;
  return (int)(b < REG_MAX_BLOCKS ? b : REG_MAX_BLOCKS);
}

bool reg_args_ok(const GsrReg* a) {
  if (!a || a->M < 0 || a->N < 0) return false;
  return a->M == 0 || (a->idx && a->log_scaling && a->depths && a->opacity && a->visibility && a->N > 0);
}

}  // namespace

extern "C" {

int64_t gsr_reg_struct_bytes(void) { return (int64_t)sizeof(GsrReg); }

size_t gsr_reg_workspace_bytes(int64_t M) {
  return M < 0 ? 0 : sizeof(float) * REG_SLOT * (size_t)(reg_blocks(M) > 0 ? reg_blocks(M) : 1);
}

int gsr_reg_forward(const GsrReg* args, float* loss_out, float* terms_out, void* workspace, size_t workspace_bytes,
                    void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!reg_args_ok(args) || !loss_out || !terms_out) return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < gsr_reg_workspace_bytes(args->M)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  const int blocks = reg_blocks(args->M);
  float* slots = static_cast<float*>(workspace);
  if (blocks > 0) {
    reg_fwd_kernel<<<blocks, REG_BLOCK, 0, stream>>>(*args, slots);
    GSR_CHECK_LAUNCH();
  }
  reg_finish_kernel<<<1, REG_BLOCK, 0, stream>>>(slots, blocks, *args, loss_out, terms_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_reg_backward(const GsrReg* args, const float* terms, const float* d_loss, float* d_opacity, float* d_depths,
                     float* d_specular, float* d_log_scaling, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!reg_args_ok(args) || !terms || !d_loss) return GSR_ERR_INVALID_ARGUMENT;
  if (args->M == 0) return GSR_OK;
  reg_bwd_kernel<<<grid_for(args->M, REG_BLOCK), REG_BLOCK, 0, stream>>>(
      *args, terms, d_loss, d_opacity, d_depths, d_specular, d_log_scaling);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_scene_post_step(float* rotation_xyzw, float* log_scaling, int64_t N, float eps, float lo, float hi,
                        void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (N < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (N == 0) return GSR_OK;
  if (!rotation_xyzw || !log_scaling || (reinterpret_cast<uintptr_t>(rotation_xyzw) & 15)) return GSR_ERR_INVALID_ARGUMENT;
  scene_post_step_kernel<<<grid_for(N, REG_BLOCK), REG_BLOCK, 0, stream>>>(
      reinterpret_cast<float4*>(rotation_xyzw), log_scaling, N, eps, lo, hi);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
