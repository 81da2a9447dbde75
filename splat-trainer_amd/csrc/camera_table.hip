// Pose tables: rows of (unit quaternion, translation) to 4x4 rigid transforms and back, one launch per direction.  Per-row
// maths and the order of every operation in gsr_camera_table.h.  No float atomics, no LDS, no scratch.
//
// pose_forward_kernel   one lane per image: its row (or its two rows, for a rig) to T[b], stored as four float4.
// pose_backward_kernel  one lane per table row, the left table's rows first: the lane walks the batch in increasing
//                       position, adds the terms of the images that select its row and chains the sum through the row,
//                       so every row is written (zeros when no image selects it) and a sum has one order.  The batch's
//                       indices are the same for every lane of a wave.  (A + A') B compares; B is a batch of images.
// An index outside its table reads row 0 and ORs 1 into the caller's status word (an integer atomic, on that path only).
#include "gsr_device.h"
#include "gsr_camera_table.h"
#include "gsr_host.h"

namespace {

constexpr int PT_BLOCK = 256;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(PT_BLOCK) void pose_forward_kernel(const float* __restrict__ q_left,
                                                                 const float* __restrict__ t_left, int64_t A_left,
                                                                 const int64_t* __restrict__ idx_left,
                                                                 const float* __restrict__ q_right,
                                                                 const float* __restrict__ t_right, int64_t A_right,
                                                                 const int64_t* __restrict__ idx_right, int64_t B,
                                                                 float* __restrict__ T_out, int32_t* __restrict__ status) {
  const int64_t b = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (b >= B) return;
  bool bad = false;
  const int64_t l = gsr_pose_index(idx_left[b], A_left, &bad);
  float ql[4], tl[3], qr[4], tr[3], T[16];
#pragma unroll
  for (int k = 0; k < 4; ++k) ql[k] = q_left[4 * l + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tl[k] = t_left[3 * l + k];
  if (q_right) {
    const int64_t r = gsr_pose_index(idx_right[b], A_right, &bad);
#pragma unroll
    for (int k = 0; k < 4; ++k) qr[k] = q_right[4 * r + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tr[k] = t_right[3 * r + k];
    gsr_pose_forward_image(ql, tl, qr, tr, T);
  } else {
    gsr_pose_forward_image(ql, tl, nullptr, nullptr, T);
  }
  float4* out = reinterpret_cast<float4*>(T_out + 16 * b);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = make_float4(T[4 * i], T[4 * i + 1], T[4 * i + 2], T[4 * i + 3]);
  if (bad) atomicOr(status, 1);
}

__global__ __launch_bounds__(PT_BLOCK) void pose_backward_kernel(const float* __restrict__ q_left,
                                                                  const float* __restrict__ t_left, int64_t A_left,
                                                                  const int64_t* __restrict__ idx_left,
                                                                  const float* __restrict__ q_right,
                                                                  const float* __restrict__ t_right, int64_t A_right,
                                                                  const int64_t* __restrict__ idx_right, int64_t B,
                                                                  const float* __restrict__ G, float* __restrict__ d_q_left,
                                                                  float* __restrict__ d_t_left, float* __restrict__ d_q_right,
                                                                  float* __restrict__ d_t_right,
                                                                  int32_t* __restrict__ status) {
  const int64_t row = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  const bool left = row < A_left;
  const int64_t a = left ? row : row - A_left;
  if (!left && (!q_right || a >= A_right)) return;
  float* d_q = left ? d_q_left : d_q_right;
  float* d_t = left ? d_t_left : d_t_right;
  if (!d_q) return;                                   // this table's gradient is not asked for
  float dq[4], dt[3];
  const bool bad = left ? gsr_pose_backward_row(true, a, q_left, A_left, idx_left, q_right, t_right, A_right, idx_right, B, G, dq, dt)
                        : gsr_pose_backward_row(false, a, q_right, A_right, idx_right, q_left, t_left, A_left, idx_left, B, G, dq, dt);
#pragma unroll
  for (int k = 0; k < 4; ++k) d_q[4 * a + k] = dq[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) d_t[3 * a + k] = dt[k];
  if (bad) atomicOr(status, 1);
}

// The arguments both entry points share.
int check_tables(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left, const float* q_right,
                 const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B, const int32_t* status) {
  if (!q_left || !t_left || A_left < 1 || A_left > GSR_POSE_MAX_ROWS || B < 0 || B > GSR_POSE_MAX_ROWS || !status)
    return GSR_ERR_INVALID_ARGUMENT;
  if (B > 0 && !idx_left) return GSR_ERR_INVALID_ARGUMENT;
  if (q_right) {
    if (!t_right || A_right < 1 || A_right > GSR_POSE_MAX_ROWS || (B > 0 && !idx_right)) return GSR_ERR_INVALID_ARGUMENT;
  } else if (t_right || idx_right) {
    return GSR_ERR_INVALID_ARGUMENT;
  }
  return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_pose_forward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                     const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                     float* T_out, int32_t* status, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  const int rc = check_tables(q_left, t_left, A_left, idx_left, q_right, t_right, A_right, idx_right, B, status);
  if (rc != GSR_OK) return rc;
  if (B == 0) return GSR_OK;
  if (!T_out || !aligned16(T_out)) return GSR_ERR_INVALID_ARGUMENT;
  pose_forward_kernel<<<grid_for(B, PT_BLOCK), PT_BLOCK, 0, stream>>>(q_left, t_left, A_left, idx_left, q_right, t_right,
                                                                      A_right, idx_right, B, T_out, status);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_pose_backward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                      const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                      const float* d_T, float* d_q_left, float* d_t_left, float* d_q_right, float* d_t_right,
                      int32_t* status, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  const int rc = check_tables(q_left, t_left, A_left, idx_left, q_right, t_right, A_right, idx_right, B, status);
  if (rc != GSR_OK) return rc;
  if ((B > 0 && !d_T) || !d_q_left != !d_t_left || !d_q_right != !d_t_right || (!q_right && d_q_right) ||
      (!d_q_left && !d_q_right))
    return GSR_ERR_INVALID_ARGUMENT;
  const int64_t rows = A_left + (q_right ? A_right : 0);
  pose_backward_kernel<<<grid_for(rows, PT_BLOCK), PT_BLOCK, 0, stream>>>(
      q_left, t_left, A_left, idx_left, q_right, t_right, A_right, idx_right, B, d_T, d_q_left, d_t_left, d_q_right,
      d_t_right, status);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_pose_block_size(void) { return PT_BLOCK; }

}  // extern "C"
