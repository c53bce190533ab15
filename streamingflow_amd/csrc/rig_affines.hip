// The camera rig's affines on the device for gfx950: what LiftSplat.rig_affines states with ~20 small torch launches
// and a synchronising torch.inverse, in one launch that a graph can record.
//   sf_rig_affines_fwd   affine[b*s*n][12] = the 3x4 that takes (u*d, v*d, d, 1) of a camera's frustum to the final ego frame:
//     R_cam * K^-1 | t_cam  (get_geometry, streamingflow.py:277-292), then the left-multiplications ego[t], t = own frame .. s-2, in that
//     order (projection_to_birds_eye_view, :386-396), ego = pose_vec2mat(future_egomotion) = [xmat * ymat * zmat | translation]
//     (utils/geometry.py:124-172).
// All arithmetic is fp64 on the fp32 inputs promoted first (sin / cos of the promoted angles too), every operation rounded on its own (the
// compiler's contraction is off, so the figures do not depend on the build); the one rounding to fp32 is at the store.  K is a general
// 3x3: inverted by cofactors over the determinant.  One thread per (frame, camera), no LDS, no scratch; the chain loop is bounded by s.
// A camera whose determinant is zero (cancelled down to the rounding noise of its own terms) or non-finite, or whose inputs hold a
// non-finite value, gets twelve NaNs and ORs SF_RIG_BAD_CAMERA into the flag word: the lift's quantiser sends a NaN position to the
// sentinel cell, so such a camera feeds no BEV cell, and nothing raises at enqueue.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sfnative.h"

namespace sf {
namespace {

constexpr int RIG_THREADS = 64;

__device__ __forceinline__ bool finite64(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }      // false for NaN, +-inf

// utils/geometry.py:124-172 for one pose (tx, ty, tz, rx, ry, rz): R = xmat * ymat * zmat, the products taken left to right as bmm does
__device__ __forceinline__ void pose_mat(const float* __restrict__ v, double R[3][3], double T[3]) {
#pragma clang fp contract(off)
  const double ax = (double)v[3], ay = (double)v[4], az = (double)v[5];
  const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
  const double X[3][3] = {{1.0, 0.0, 0.0}, {0.0, cx, -sx}, {0.0, sx, cx}};
  const double Y[3][3] = {{cy, 0.0, sy}, {0.0, 1.0, 0.0}, {-sy, 0.0, cy}};
  const double Z[3][3] = {{cz, -sz, 0.0}, {sz, cz, 0.0}, {0.0, 0.0, 1.0}};
  double XY[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) XY[i][j] = X[i][0] * Y[0][j] + X[i][1] * Y[1][j] + X[i][2] * Y[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = XY[i][0] * Z[0][j] + XY[i][1] * Z[1][j] + XY[i][2] * Z[2][j];
  T[0] = (double)v[0]; T[1] = (double)v[1]; T[2] = (double)v[2];
}

__global__ __launch_bounds__(RIG_THREADS) void rig_affines_kernel(const float* __restrict__ intrinsics, const float* __restrict__ extrinsics,
                                                                  const float* __restrict__ egomotion, int total, int s, int n_cam,
                                                                  float* __restrict__ affine, int* __restrict__ flags) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * RIG_THREADS + threadIdx.x;      // (sample, frame, camera), camera fastest
  if (i >= total) return;
  const int frame = i / n_cam, b = frame / s, own = frame - b * s;
  const float* __restrict__ Kp = intrinsics + 9 * (size_t)i;
  const float* __restrict__ Ep = extrinsics + 16 * (size_t)i;
  bool ok = true;
  double K[3][3], A[3][4];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      K[r][c] = (double)Kp[3 * r + c];
      ok = ok && finite64(K[r][c]);
    }
  double Rc[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Rc[r][c] = (double)Ep[4 * r + c];
      ok = ok && finite64(Rc[r][c]);
    }
    A[r][3] = (double)Ep[4 * r + 3];
    ok = ok && finite64(A[r][3]);
  }
  // cofactors of K (the transpose of the cofactor matrix is the adjugate) and the determinant along the first row
  const double c00 = K[1][1] * K[2][2] - K[1][2] * K[2][1], c01 = K[1][2] * K[2][0] - K[1][0] * K[2][2], c02 = K[1][0] * K[2][1] - K[1][1] * K[2][0];
  const double c10 = K[0][2] * K[2][1] - K[0][1] * K[2][2], c11 = K[0][0] * K[2][2] - K[0][2] * K[2][0], c12 = K[0][1] * K[2][0] - K[0][0] * K[2][1];
  const double c20 = K[0][1] * K[1][2] - K[0][2] * K[1][1], c21 = K[0][2] * K[1][0] - K[0][0] * K[1][2], c22 = K[0][0] * K[1][1] - K[0][1] * K[1][0];
  const double det = K[0][0] * c00 + K[0][1] * c01 + K[0][2] * c02;
  // what the six products of the determinant sum to in magnitude: a determinant below 2^-44 of it is the rounding noise of a singular
  // matrix (fp64 leaves about 2^-51 of it), which two equal rows produce without summing to an exact zero
  const double mass = __builtin_fabs(K[0][0]) * (__builtin_fabs(K[1][1] * K[2][2]) + __builtin_fabs(K[1][2] * K[2][1])) +
                      __builtin_fabs(K[0][1]) * (__builtin_fabs(K[1][2] * K[2][0]) + __builtin_fabs(K[1][0] * K[2][2])) +
                      __builtin_fabs(K[0][2]) * (__builtin_fabs(K[1][0] * K[2][1]) + __builtin_fabs(K[1][1] * K[2][0]));
  ok = ok && finite64(det) && __builtin_fabs(det) > mass * 0x1p-44;
  const double Ki[3][3] = {{c00 / det, c10 / det, c20 / det}, {c01 / det, c11 / det, c21 / det}, {c02 / det, c12 / det, c22 / det}};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) A[r][c] = Rc[r][0] * Ki[0][c] + Rc[r][1] * Ki[1][c] + Rc[r][2] * Ki[2][c];
  // frames 0..t are moved by pose t, t = 0..s-2: this frame meets the poses own .. s-2, in that order
  const float* __restrict__ ego = egomotion + 6 * (size_t)b * s;
  for (int t = own; t < s - 1; ++t) {
    const float* __restrict__ v = ego + 6 * (size_t)t;
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && finite64((double)v[k]);
    double R[3][3], T[3], N[3][4];
    pose_mat(v, R, T);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) N[r][c] = R[r][0] * A[0][c] + R[r][1] * A[1][c] + R[r][2] * A[2][c];
      N[r][3] = R[r][0] * A[0][3] + R[r][1] * A[1][3] + R[r][2] * A[2][3] + T[r];      // the fourth row of A is (0, 0, 0, 1)
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) A[r][c] = N[r][c];
  }
  float* __restrict__ o = affine + 12 * (size_t)i;
  const float bad = __builtin_nanf("");
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) o[4 * r + c] = ok ? (float)A[r][c] : bad;
  if (!ok) atomicOr(flags, SF_RIG_BAD_CAMERA);
}

}  // namespace
}  // namespace sf

extern "C" int sf_rig_affines_fwd(const float* intrinsics, const float* extrinsics, const float* future_egomotion, int b, int s, int n_cam,
                                  float* affine, int32_t* flags, void* stream) {
  if (!intrinsics || !extrinsics || !future_egomotion || !affine || !flags || b <= 0 || s <= 0 || n_cam <= 0) return SF_ERR_INVALID;
  const long total = (long)b * s * n_cam;
  if (total >= (1L << 31) / 16) return SF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sf::rig_affines_kernel, dim3((unsigned)((total + sf::RIG_THREADS - 1) / sf::RIG_THREADS)), dim3(sf::RIG_THREADS), 0,
                     static_cast<hipStream_t>(stream), intrinsics, extrinsics, future_egomotion, (int)total, s, n_cam, affine,
                     reinterpret_cast<int*>(flags));
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}
