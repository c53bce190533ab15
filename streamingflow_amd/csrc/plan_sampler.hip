// The planner's trajectory sampler for gfx950: streamingflow/utils/sampler.py::sample with the decimation of
// NuscenesData.get_trajectory_sampling, per sample of a batch, from fed uniforms.
//   sf_fresnel_fwd        the Fresnel integrals S(z), C(z) in fp64 (test entry around the device function below)
//   sf_plan_sample_fwd    M rows (lines, circles, clothoids) of n_t kept stamps, ordered by x at the key stamp (stable), fp32 [B][M][n_t][3]
// All arithmetic is fp64 in the reference's operation order without contraction; the cast to fp32 happens at the store.
//
// Fresnel method (tables: tools/gen_fresnel_tables.py).  |z| <= 1.6: Maclaurin series in z^4.  Beyond: C = 1/2 + f sin(p) - g cos(p),
// S = 1/2 - f cos(p) - g sin(p) with p = pi z^2 / 2 reduced exactly (fmod(z^2, 4)) and f = F(t) / (pi z), g = G(t) / (pi^2 z^3),
// F and G Chebyshev expansions in t = 1 / z^2 on three pieces of [0, 1 / 1.6^2].  The tables live in constant memory and are read
// through a pointer: no per-thread array.
//
// Launch shapes (profiles/samplebench.json).  One launch: a workgroup of 512 threads per sample forms the M keys in LDS, ranks them
// and writes each row to its rank.  Two launches: keys over (M / 256, B) workgroups into the workspace, then every workgroup of a second
// grid, in which up to 16 threads share a row (one kept stamp each), loads its sample's keys to LDS, ranks its rows and writes them.
// Either way rank(i) = #{j : k_j < k_i, or k_j == k_i and j < i}: stable, no atomics, < M whatever the keys hold (NaN included).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "../../include/sfnative.h"
#include "fresnel_tables.h"

namespace sf {
namespace {

constexpr int SAMPLE_MAX_M = 4096;      // keys of one sample in LDS: 32 KB
constexpr int WG_THREADS = 512;         // one-launch shape: 256 vector registers per thread, which the fp64 sincos / fmod chains need
constexpr int ROW_THREADS = 256;        // two-launch shape
constexpr double PI = 3.141592653589793;

__constant__ double c_fresnel_f[3 * SF_FRESNEL_NCHEB] = {SF_FRESNEL_F};
__constant__ double c_fresnel_g[3 * SF_FRESNEL_NCHEB] = {SF_FRESNEL_G};
__constant__ double c_fresnel_s[SF_FRESNEL_NSERIES] = {SF_FRESNEL_S};
__constant__ double c_fresnel_c[SF_FRESNEL_NSERIES] = {SF_FRESNEL_C};

// S(z), C(z) = int_0^z sin / cos(pi t^2 / 2) dt (scipy.special.fresnel's convention); odd in z; NaN -> NaN; +-1/2 beyond 1e100
__device__ __noinline__ double2 fresnel(double z) {
  const double az = fabs(z);
  double s, c;
  if (az <= SF_FRESNEL_Z0) {
    double x = az * az;
    x *= x;
    double hs = c_fresnel_s[SF_FRESNEL_NSERIES - 1], hc = c_fresnel_c[SF_FRESNEL_NSERIES - 1];
    for (int n = SF_FRESNEL_NSERIES - 2; n >= 0; --n) {
      hs = hs * x + c_fresnel_s[n];
      hc = hc * x + c_fresnel_c[n];
    }
    s = az * az * az * hs;
    c = az * hc;
  } else if (az < 1e100) {
    const double z2 = az * az;
    const double t = 1.0 / z2;
    const int piece = (t > SF_FRESNEL_T1 ? 1 : 0) + (t > SF_FRESNEL_T2 ? 1 : 0);
    const double lo = piece == 0 ? 0.0 : (piece == 1 ? SF_FRESNEL_T1 : SF_FRESNEL_T2);
    const double hi = piece == 0 ? SF_FRESNEL_T1 : (piece == 1 ? SF_FRESNEL_T2 : SF_FRESNEL_T3);
    const double x2 = 2.0 * ((2.0 * t - lo - hi) / (hi - lo));
    const double* cf = c_fresnel_f + piece * SF_FRESNEL_NCHEB;
    const double* cg = c_fresnel_g + piece * SF_FRESNEL_NCHEB;
    double f1 = 0.0, f2 = 0.0, g1 = 0.0, g2 = 0.0;      // Clenshaw
    for (int k = SF_FRESNEL_NCHEB - 1; k >= 1; --k) {
      const double f0 = cf[k] + x2 * f1 - f2, g0 = cg[k] + x2 * g1 - g2;
      f2 = f1, f1 = f0, g2 = g1, g1 = g0;
    }
    const double F = cf[0] + 0.5 * x2 * f1 - f2, G = cg[0] + 0.5 * x2 * g1 - g2;
    const double f = F / (PI * az), g = G / (PI * PI * az * z2);
    double sn, cs;
    sincospi(0.5 * fmod(z2, 4.0), &sn, &cs);
    c = 0.5 + f * sn - g * cs;
    s = 0.5 - f * cs - g * sn;
  } else {
    s = c = az != az ? az : 0.5;
  }
  return make_double2(z < 0.0 ? -s : s, z < 0.0 ? -c : c);
}

// one body of the fp64 sincos (its large-argument reduction is long) for the circles and the clothoids' rotation
__device__ __noinline__ double2 sin_cos(double x) {
  double sn, cs;
  sincos(x, &sn, &cs);
  return make_double2(sn, cs);
}

__global__ __launch_bounds__(ROW_THREADS) void fresnel_kernel(const double* __restrict__ z, long n, double* __restrict__ S, double* __restrict__ C) {
  const long i = (long)blockIdx.x * ROW_THREADS + threadIdx.x;
  if (i >= n) return;
  const double2 sc = fresnel(z[i]);
  S[i] = sc.x;
  C[i] = sc.y;
}

struct PlanSampleArgs {
  const double* v0;
  const double* kappa;
  const double* t0;
  const double* n0;
  const double* tt;
  const double* uniforms;
  double t_key;
  int n_straight, n_left, n_right, M, n_t;
  float* out;
  int32_t* order;
  double* keys;      // two-launch shape: [B][M]
};

// (a + pi) % (2 pi) - pi with Python's %: the remainder has the divisor's sign
__device__ __noinline__ double wrap(double a) {
  double r = fmod(a + PI, 2.0 * PI);
  if (r < 0.0) r += 2.0 * PI;
  return r - PI;
}

// What is fixed for one sample, and for one row of it (pre-sort position p)
struct SampleFrame {
  double kappa, t0x, t0y, n0x, n0y, radius, cx, xi0, sgn;
  bool krappa_pos;
};
struct Row {
  double v, a, alpha, theta0, rc, rs, x0, y0;
  int kind;      // 0 line, 1 circle, 2 clothoid
  bool mirror;
};

__device__ __forceinline__ SampleFrame sample_frame(const PlanSampleArgs& a, int b) {
#pragma clang fp contract(off)
  SampleFrame f;
  f.kappa = a.kappa[b];
  f.t0x = a.t0[2 * b], f.t0y = a.t0[2 * b + 1], f.n0x = a.n0[2 * b], f.n0y = a.n0[2 * b + 1];
  const double krappa = f.kappa <= 0.0 ? fmin(-0.01, f.kappa) : fmax(0.01, f.kappa);
  f.radius = fabs(1.0 / krappa);
  f.cx = -1.0 / krappa;
  f.krappa_pos = krappa >= 0.0;
  f.xi0 = fabs(f.kappa) / PI;
  f.sgn = f.kappa > 0.0 ? 1.0 : (f.kappa < 0.0 ? -1.0 : 0.0);
  return f;
}

// Row p of sample b before the sort.  kappa > 0: [curves 0 .. left), lines, curves [left, left + right) mirrored];
// otherwise [curves [left, left + right) mirrored, lines, curves 0 .. left)].
__device__ __forceinline__ Row row_setup(const PlanSampleArgs& a, const SampleFrame& f, int b, int p) {
#pragma clang fp contract(off)
  Row r;
  const int first = f.kappa > 0.0 ? a.n_left : a.n_right;
  int j = 0, g;
  r.mirror = false;
  if (p >= first && p < first + a.n_straight) {
    r.kind = 0;
    g = p - first;
  } else {
    if (f.kappa > 0.0) {
      j = p < first ? p : p - a.n_straight;
      r.mirror = p >= first;
    } else {
      j = p < first ? a.n_left + p : p - first - a.n_straight;
      r.mirror = p < first;
    }
    g = a.n_straight + j;
    r.kind = 2;
  }
  const double* u = a.uniforms + (size_t)b * 5 * a.M;
  r.a = 10.0 * (u[g] - 0.5) + 2.0;
  r.v = u[2 * a.M + g] >= 0.2 ? 15.0 * u[a.M + g] : a.v0[b];
  r.alpha = r.theta0 = r.x0 = r.y0 = 0.0;
  r.rc = 1.0, r.rs = 0.0;
  if (r.kind) {
    r.alpha = (80 - 6) * u[3 * a.M + j] + 6.0;
    if (u[4 * a.M + j] < 0.2) {
      r.kind = 1;
    } else {
      const double q = f.kappa / PI / r.alpha;
      r.theta0 = 0.5 * PI * (q * q);
      const double2 rot = sin_cos(r.theta0 * f.sgn);
      r.rs = rot.x, r.rc = rot.y;
    }
  }
  return r;
}

// Row p at the key stamp alone (o == nullptr; returns its x) or at the kept stamps s0, s0 + step, ... < n_t (written to o as fp32).  A
// clothoid's first pass is the first stamp, whose point it is shifted by; one loop, so the Fresnel code exists once.
__device__ __forceinline__ double row_eval(const PlanSampleArgs& a, const SampleFrame& f, int b, int p, float* o, int s0, int step) {
#pragma clang fp contract(off)
  Row r = row_setup(a, f, b, p);
  const int n = o ? a.n_t : 1;
  double key = 0.0;
  bool base = r.kind == 2;
  int s = s0;
  while (base || s < n) {
    const double t = base ? a.tt[0] : (o ? a.tt[s] : a.t_key);
    const double L = r.v * t + r.a * (t * t) / 2.0;
    double x, y, th;
    if (r.kind == 0) {
      x = L * f.t0x, y = L * f.t0y, th = 0.0;
    } else if (r.kind == 1) {
      const double phi = f.krappa_pos ? L / f.radius : PI - L / f.radius;
      const double2 sc = sin_cos(phi);
      x = f.cx + f.radius * sc.y;
      y = 0.0 + f.radius * sc.x;
      th = wrap(f.krappa_pos ? L / f.radius : -L / f.radius);
    } else {
      const double z = (f.xi0 + L) / r.alpha;
      const double2 sc = fresnel(z);
      const double S = sc.x, C = sc.y;
      const double px = r.alpha * (C * f.t0x + S * f.n0x), py = r.alpha * (C * f.t0y + S * f.n0y);
      if (base) {
        r.x0 = px, r.y0 = py;
        base = false;
        continue;
      }
      const double X = px - r.x0, Y = py - r.y0;
      x = r.rc * X + r.rs * Y;
      y = -r.rs * X + r.rc * Y;
      th = wrap((0.5 * PI * (z * z) - r.theta0) * f.sgn);
    }
    if (r.mirror) x = -x, th = -th;
    if (o)
      o[3 * s] = (float)x, o[3 * s + 1] = (float)y, o[3 * s + 2] = (float)th;
    else
      key = x;
    s += step;
  }
  return key;
}

// rank of row p among the M keys in LDS, the part of it over j = j0, j0 + step, ...: the whole is < M whatever the keys hold
__device__ __forceinline__ int row_rank(const double* keys, int M, int p, int j0, int step) {
  const double k = keys[p];
  int rank = 0;
  for (int j = j0; j < M; j += step) {
    const double kj = keys[j];
    rank += (kj < k || (kj == k && j < p)) ? 1 : 0;
  }
  return rank;
}

__global__ __launch_bounds__(WG_THREADS) void plan_sample_wg_kernel(PlanSampleArgs a) {
  extern __shared__ double keys[];
  __shared__ SampleFrame frame;      // read back into vector registers: this kernel's scalar registers are taken by its three loop levels
  const int b = blockIdx.x;
  if (threadIdx.x == 0) frame = sample_frame(a, b);
  __syncthreads();
  const SampleFrame f = frame;
#pragma clang loop unroll(disable)
  for (int phase = 0; phase < 2; ++phase) {      // keys, barrier, rows: one body, so the row code exists once
    for (int p = threadIdx.x; p < a.M; p += WG_THREADS) {
      float* o = nullptr;
      if (phase) {
        const int rank = row_rank(keys, a.M, p, 0, 1);
        o = a.out + ((size_t)b * a.M + rank) * a.n_t * 3;
        if (a.order) a.order[(size_t)b * a.M + rank] = p;
      }
      const double k = row_eval(a, f, b, p, o, 0, 1);
      if (!phase) keys[p] = k;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(ROW_THREADS) void plan_sample_keys_kernel(PlanSampleArgs a) {
  const int b = blockIdx.y, p = blockIdx.x * ROW_THREADS + threadIdx.x;
  if (p >= a.M) return;
  const SampleFrame f = sample_frame(a, b);
  a.keys[(size_t)b * a.M + p] = row_eval(a, f, b, p, nullptr, 0, 1);
}

// tpr (a power of two <= 16: never across a wavefront) threads share a row: each takes every tpr-th key of the rank count and every
// tpr-th kept stamp, so the chain of dependent fp64 operations a thread runs is one or two stamps long instead of n_t
__global__ __launch_bounds__(ROW_THREADS) void plan_sample_rows_kernel(PlanSampleArgs a, int tpr) {
  extern __shared__ double keys[];
  const int b = blockIdx.y, sub = threadIdx.x & (tpr - 1), p = blockIdx.x * (ROW_THREADS / tpr) + threadIdx.x / tpr;
  for (int j = threadIdx.x; j < a.M; j += ROW_THREADS) keys[j] = a.keys[(size_t)b * a.M + j];
  __syncthreads();
  if (p >= a.M) return;      // all tpr threads of a row alike
  const SampleFrame f = sample_frame(a, b);
  int rank = row_rank(keys, a.M, p, sub, tpr);
  for (int o = tpr >> 1; o; o >>= 1) rank += __shfl_xor(rank, o);
  if (a.order && sub == 0) a.order[(size_t)b * a.M + rank] = p;
  row_eval(a, f, b, p, a.out + ((size_t)b * a.M + rank) * a.n_t * 3, sub, tpr);
}

}  // namespace
}  // namespace sf

using namespace sf;

extern "C" {

int sf_fresnel_fwd(const double* z, long n, double* S, double* C, void* stream) {
  if (!z || !S || !C || n < 0 || n >= (1L << 31) * ROW_THREADS) return SF_ERR_INVALID;
  if (n == 0) return SF_OK;
  hipLaunchKernelGGL(fresnel_kernel, dim3((unsigned)((n + ROW_THREADS - 1) / ROW_THREADS)), dim3(ROW_THREADS), 0, static_cast<hipStream_t>(stream), z, n,
                     S, C);
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

size_t sf_plan_sample_ws_bytes(int B, int M, int n_t) {
  (void)n_t;
  return B < 1 || M < 1 ? 0 : (size_t)B * M * sizeof(double);
}

int sf_plan_sample_fwd(const double* v0, const double* kappa, const double* t0, const double* n0, const double* tt_kept, double t_key,
                       const double* uniforms, int n_straight, int n_left, int n_right, int B, int M, int n_t, float* out, int32_t* order,
                       void* ws, size_t ws_bytes, void* stream) {
  if (!v0 || !kappa || !t0 || !n0 || !tt_kept || !uniforms || !out || !ws) return SF_ERR_INVALID;
  if (B < 1 || M < 1 || n_t < 1 || B > 65535 || n_straight < 0 || n_left < 0 || n_right < 0 || (long)n_straight + n_left + n_right != M)
    return SF_ERR_INVALID;
  if (M > SAMPLE_MAX_M) return SF_ERR_UNSUPPORTED;
  if (ws_bytes < sf_plan_sample_ws_bytes(B, M, n_t)) return SF_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  PlanSampleArgs a;
  a.v0 = v0, a.kappa = kappa, a.t0 = t0, a.n0 = n0, a.tt = tt_kept, a.uniforms = uniforms, a.t_key = t_key;
  a.n_straight = n_straight, a.n_left = n_left, a.n_right = n_right, a.M = M, a.n_t = n_t;
  a.out = out, a.order = order, a.keys = static_cast<double*>(ws);
  const size_t lds = (size_t)M * sizeof(double);
  const char* e = getenv("SF_PLAN_SAMPLE_LAUNCHES");      // measurement switch (tools/samplebench.py): 1 or 2; unset: the default below
  const int launches = e && (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 2;
  if (launches == 1) {
    hipLaunchKernelGGL(plan_sample_wg_kernel, dim3((unsigned)B), dim3(WG_THREADS), lds, st, a);
  } else {
    const dim3 grid((unsigned)((M + ROW_THREADS - 1) / ROW_THREADS), (unsigned)B);
    hipLaunchKernelGGL(plan_sample_keys_kernel, grid, dim3(ROW_THREADS), 0, st, a);
    int tpr = 1;
    while (tpr < n_t && tpr < 16) tpr <<= 1;
    const dim3 rows((unsigned)((M + ROW_THREADS / tpr - 1) / (ROW_THREADS / tpr)), (unsigned)B);
    hipLaunchKernelGGL(plan_sample_rows_kernel, rows, dim3(ROW_THREADS), lds, st, a, tpr);
  }
  return hipGetLastError() == hipSuccess ? SF_OK : SF_ERR_LAUNCH;
}

}  // extern "C"
