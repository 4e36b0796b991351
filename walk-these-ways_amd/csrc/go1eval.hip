// go1eval.hip — evaluation metrics of a policy rollout on the device (include/go1eval.h), gfx950.
//
// eval_accumulate_kernel: one thread per environment.  Every input is a row of an SoA buffer ([k][N]), so the 64 lanes of a
// wavefront read 64 consecutive floats (256 contiguous bytes) per load, and the accumulators ([metric][N]) are read and written
// the same way.  Each accumulator element has one writer: no atomics, no cross-lane traffic, nothing depends on scheduling.
// eval_reduce_kernel: one workgroup per (group, row of the result table).  Thread t combines environments t, t + T, ... in
// ascending order in fp64, then a binary tree in LDS with a fixed shape; thread 0 writes the row with vector stores.
// tests/eval_ref.py restates both in fp64 numpy from the header's text.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/go1eval.h"

namespace {

constexpr int ACC_THREADS = 256;
constexpr int NM = GO1EVAL_NUM_METRICS, NF = GO1EVAL_NUM_FIELDS, RT = GO1EVAL_REDUCE_THREADS;

struct EvalArgs {
  Go1EvalConfig c;
  Go1EvalBuffers b;
};

__device__ __forceinline__ void fold(const Go1EvalBuffers& b, int m, int N, int e, float v) {
  const size_t i = (size_t)m * N + e;
  if (!isfinite(v)) { b.nonfinite[i] += 1u; return; }
  b.count[i] += 1u;
  b.sum[i] += (double)v;
  b.sumsq[i] += (double)v * (double)v;
  b.min[i] = fminf(b.min[i], v);
  b.max[i] = fmaxf(b.max[i], v);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) eval_clear_kernel(const EvalArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1EvalBuffers& b = A.b;
  for (int m = 0; m < NM; m++) {
    const size_t i = (size_t)m * N + e;
    b.count[i] = 0u; b.nonfinite[i] = 0u; b.sum[i] = 0.0; b.sumsq[i] = 0.0; b.min[i] = INFINITY; b.max[i] = -INFINITY;
  }
  b.steps[e] = 0u; b.episodes_terminated[e] = 0u; b.episodes_timed_out[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) eval_accumulate_kernel(const EvalArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1EvalBuffers& b = A.b;
  b.steps[e] += 1u;
  if (b.reset_buf[e]) {
    if (b.time_out_buf[e]) b.episodes_timed_out[e] += 1u; else b.episodes_terminated[e] += 1u;
    fold(b, GO1EVAL_TERMINATION, N, e, 1.0f);
    return;
  }
  if (b.episode_length_buf[e] <= A.c.warmup_steps) return;

  const float vx = b.base_lin_vel[e], vy = b.base_lin_vel[N + e], wz = b.base_ang_vel[2 * N + e];
  const float dv = vx - b.commands[e], dw = wz - b.commands[2 * N + e];
  fold(b, GO1EVAL_LIN_VEL_RMSD, N, e, sqrtf(dv * dv));
  fold(b, GO1EVAL_ANG_VEL_RMSD, N, e, sqrtf(dw * dw));
  fold(b, GO1EVAL_LIN_VEL_X, N, e, vx);
  fold(b, GO1EVAL_ANG_VEL_YAW, N, e, wz);

  const float z = b.root_states[2 * N + e];
  float height = z;                                   // measured_heights = NULL: mean of (z - 0) over one point
  if (b.measured_heights) {
    double s = 0.0;                                   // (fp64 carry, one rounding: see the header)
    for (int p = 0; p < A.c.num_height_points; p++) s += (double)(z - b.measured_heights[(size_t)p * N + e]);
    height = (float)s / (float)A.c.num_height_points;
  }
  fold(b, GO1EVAL_BASE_HEIGHT, N, e, height);

  float tmax = 0.f;
  double psum = 0.0;
  for (int j = 0; j < 12; j++) {
    const float tq = b.torques[j * N + e];
    tmax = fmaxf(tmax, fabsf(tq));
    psum += (double)(tq * b.dof_vel[j * N + e]);
  }
  const float power = (float)psum;
  fold(b, GO1EVAL_MAX_TORQUES, N, e, tmax);
  fold(b, GO1EVAL_POWER_CONSUMPTION, N, e, power);

  const float mass = A.c.default_body_mass + b.payloads[e];
  const float speed = sqrtf(vx * vx + vy * vy);
  fold(b, GO1EVAL_COT, N, e, power / (mass * (float)GO1EVAL_GRAVITY * speed));
  fold(b, GO1EVAL_FROUDE_NUMBER, N, e, vx * vx / (float)(GO1EVAL_GRAVITY * GO1EVAL_FROUDE_HEIGHT));
  fold(b, GO1EVAL_TERMINATION, N, e, 0.0f);
}

extern "C" __global__ void __launch_bounds__(RT) eval_reduce_kernel(const EvalArgs A) {
  __shared__ double lds[NF][RT];
  const int N = A.c.num_envs;
  const int t = (int)threadIdx.x;
  const int g = (int)blockIdx.x / (NM + 1), m = (int)blockIdx.x % (NM + 1);
  const bool group_row = m == NM;
  const Go1EvalBuffers& b = A.b;
  // metric row: a0 count, a1 nonfinite, a2 sum, a3 sumsq, a4 min, a5 max.  group row: a0 envs, a1 steps, a2 terminated, a3 timed out, a4 fallen envs
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = group_row ? 0.0 : (double)INFINITY, a5 = group_row ? 0.0 : -(double)INFINITY;
  for (int e = t; e < N; e += RT) {
    if (b.group[e] != g) continue;
    if (group_row) {
      a0 += 1.0; a1 += (double)b.steps[e]; a2 += (double)b.episodes_terminated[e]; a3 += (double)b.episodes_timed_out[e];
      a4 += b.episodes_terminated[e] > 0u ? 1.0 : 0.0;
    } else {
      const size_t i = (size_t)m * N + e;
      a0 += (double)b.count[i]; a1 += (double)b.nonfinite[i]; a2 += b.sum[i]; a3 += b.sumsq[i];
      if (b.count[i] > 0u) { a4 = fmin(a4, (double)b.min[i]); a5 = fmax(a5, (double)b.max[i]); }
    }
  }
  lds[0][t] = a0; lds[1][t] = a1; lds[2][t] = a2; lds[3][t] = a3; lds[4][t] = a4; lds[5][t] = a5;
  __syncthreads();
  for (int s = RT / 2; s > 0; s >>= 1) {
    if (t < s) {
      for (int f = 0; f < 4; f++) lds[f][t] += lds[f][t + s];
      if (group_row) { lds[4][t] += lds[4][t + s]; }
      else { lds[4][t] = fmin(lds[4][t], lds[4][t + s]); lds[5][t] = fmax(lds[5][t], lds[5][t + s]); }
    }
    __syncthreads();
  }
  if (t != 0) return;
  double* out = b.results + ((size_t)g * (NM + 1) + m) * NF;
  const double nan = (double)NAN;
  if (group_row) {
    out[GO1EVAL_G_ENVS] = lds[0][0]; out[GO1EVAL_G_STEPS] = lds[1][0]; out[GO1EVAL_G_TERMINATED] = lds[2][0];
    out[GO1EVAL_G_TIMED_OUT] = lds[3][0]; out[GO1EVAL_G_FALL_RATE] = lds[0][0] > 0.0 ? lds[4][0] / lds[0][0] : nan; out[5] = 0.0;
  } else {
    const double n = lds[0][0];
    const double mean = n > 0.0 ? lds[2][0] / n : nan;
    const double var = n > 0.0 ? lds[3][0] / n - mean * mean : nan;
    out[GO1EVAL_F_COUNT] = n; out[GO1EVAL_F_MEAN] = mean; out[GO1EVAL_F_STD] = n > 0.0 ? sqrt(fmax(var, 0.0)) : nan;
    out[GO1EVAL_F_MIN] = n > 0.0 ? lds[4][0] : nan; out[GO1EVAL_F_MAX] = n > 0.0 ? lds[5][0] : nan; out[GO1EVAL_F_NONFINITE] = lds[1][0];
  }
}

namespace {
int check(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!buf->count || !buf->sum || !buf->sumsq || !buf->min || !buf->max || !buf->nonfinite || !buf->steps || !buf->episodes_terminated ||
      !buf->episodes_timed_out) return -2;
  return 0;
}
EvalArgs args_of(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf) { EvalArgs A; A.c = *cfg; A.b = *buf; return A; }
dim3 env_grid(int n) { return dim3((unsigned)((n + ACC_THREADS - 1) / ACC_THREADS)); }
}  // namespace

extern "C" int go1eval_clear(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  const EvalArgs A = args_of(cfg, buf);
  hipLaunchKernelGGL(eval_clear_kernel, env_grid(cfg->num_envs), dim3(ACC_THREADS), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

extern "C" int go1eval_accumulate(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->base_lin_vel || !buf->base_ang_vel || !buf->commands || !buf->root_states || !buf->torques || !buf->dof_vel || !buf->payloads ||
      !buf->reset_buf || !buf->time_out_buf || !buf->episode_length_buf) return -3;
  if (buf->measured_heights && cfg->num_height_points <= 0) return -4;
  const EvalArgs A = args_of(cfg, buf);
  hipLaunchKernelGGL(eval_accumulate_kernel, env_grid(cfg->num_envs), dim3(ACC_THREADS), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

extern "C" int go1eval_reduce(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (cfg->num_groups <= 0 || !buf->group || !buf->results) return -5;
  const EvalArgs A = args_of(cfg, buf);
  hipLaunchKernelGGL(eval_reduce_kernel, dim3((unsigned)(cfg->num_groups * (NM + 1))), dim3(RT), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1eval_version(void) { return "go1eval 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
