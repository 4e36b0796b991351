// go1feet.hip — per-foot ground reaction forces of a policy rollout on the device (include/go1feet.h), gfx950.
//
// feet_accumulate_kernel: one thread per (foot, environment) in a one-dimensional launch whose blocks each belong to one foot, so every
// row access of a wavefront is one contiguous run of 64 floats (the profile word alone is scattered: its bin differs from lane to lane).
// Each word has one writer: no atomics, no LDS, nothing depends on scheduling.  The rows of an event (touchdown, lift-off) and the
// profile word are read and written only on the steps that fold into them.
// feet_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, foot) for the profile.  Thread t
// combines environments t, t + 256, ... in ascending order in fp64, then a binary tree of fixed shape in LDS.
// tests/feet_ref.py restates both in numpy from the header's text.
//
// The library shares no source with libgo1eval (its surface and stamp stay as they are): the fold of a value into the six
// accumulators, the clear, the reduction tree and the validation and launch helpers are restated here by go1eval.hip's rules.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/go1feet.h"

namespace {

constexpr int ACC_THREADS = 256;
constexpr int NM = GO1FEET_NUM, FEET = GO1FEET_NUM_FEET, BINS = GO1FEET_PHASE_BINS, NF = GO1FEET_NUM_FIELDS, RT = GO1FEET_REDUCE_THREADS;
constexpr int SLICES = RT / BINS;
static_assert(RT == 256 && BINS == 16, "feet_reduce_kernel: sixteen slices of environments per profile bin");

// a kernel's one argument: the caller's config and buffers, by value
struct FeetArgs {
  Go1FeetConfig c;
  Go1FeetBuffers b;
};

// rows first_row ... first_row + rows - 1 of the accumulators of environment e: nothing folded yet
__device__ __forceinline__ void clear_rows(const Go1FeetBuffers& b, int first_row, int rows, int N, int e) {
  for (int m = 0; m < rows; m++) {
    const size_t i = (size_t)(first_row + m) * N + e;
    b.count[i] = 0u; b.nonfinite[i] = 0u; b.sum[i] = 0.0; b.sumsq[i] = 0.0; b.min[i] = INFINITY; b.max[i] = -INFINITY;
  }
}

__device__ __forceinline__ void fold(const Go1FeetBuffers& b, int m, int N, int e, float v) {
  const size_t i = (size_t)m * N + e;
  if (!isfinite(v)) { b.nonfinite[i] += 1u; return; }
  b.count[i] += 1u;
  b.sum[i] += (double)v;
  b.sumsq[i] += (double)v * (double)v;
  b.min[i] = fminf(b.min[i], v);
  b.max[i] = fmaxf(b.max[i], v);
}

// the binary tree of fixed shape over the partial results of a workgroup of RT threads, thread t's in lds[f][t]: sums in rows
// 0 ... F - 1 and, with MinMax, a minimum in row F and a maximum in row F + 1.  Afterwards lds[f][0] holds the workgroup's.
template <int F, bool MinMax = false>
__device__ __forceinline__ void tree_reduce(double (*lds)[RT], int t) {
  __syncthreads();
  for (int s = RT / 2; s > 0; s >>= 1) {
    if (t < s) {
      for (int f = 0; f < F; f++) lds[f][t] += lds[f][t + s];
      if (MinMax) { lds[F][t] = fmin(lds[F][t], lds[F][t + s]); lds[F + 1][t] = fmax(lds[F + 1][t], lds[F + 1][t + s]); }
    }
    __syncthreads();
  }
}

// one metric row of the result table, by one workgroup of RT threads: thread t combines the group's environments t, t + RT, ... in
// ascending order, then the tree; thread 0 writes the six fields.  a0 count, a1 nonfinite, a2 sum, a3 sumsq, a4 min, a5 max
__device__ __forceinline__ void reduce_metric_row(const Go1FeetBuffers& b, int g, int m, int N, double (*lds)[RT], double* out) {
  const int t = (int)threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = (double)INFINITY, a5 = -(double)INFINITY;
  for (int e = t; e < N; e += RT) {
    if (b.group[e] != g) continue;
    const size_t i = (size_t)m * N + e;
    a0 += (double)b.count[i]; a1 += (double)b.nonfinite[i]; a2 += b.sum[i]; a3 += b.sumsq[i];
    if (b.count[i] > 0u) { a4 = fmin(a4, (double)b.min[i]); a5 = fmax(a5, (double)b.max[i]); }
  }
  lds[0][t] = a0; lds[1][t] = a1; lds[2][t] = a2; lds[3][t] = a3; lds[4][t] = a4; lds[5][t] = a5;
  tree_reduce<4, true>(lds, t);
  if (t != 0) return;
  const double nan = (double)NAN;
  const double n = lds[0][0];
  const double mean = n > 0.0 ? lds[2][0] / n : nan;
  const double var = n > 0.0 ? lds[3][0] / n - mean * mean : nan;
  out[GO1FEET_F_COUNT] = n; out[GO1FEET_F_MEAN] = mean; out[GO1FEET_F_STD] = n > 0.0 ? sqrt(fmax(var, 0.0)) : nan;
  out[GO1FEET_F_MIN] = n > 0.0 ? lds[4][0] : nan; out[GO1FEET_F_MAX] = n > 0.0 ? lds[5][0] : nan; out[GO1FEET_F_NONFINITE] = lds[1][0];
}

// the launch of one thread per (foot, environment): block k is foot k / blocks_per_foot, its lanes consecutive environments
__device__ __forceinline__ bool foot_thread(int N, int* f, int* e) {
  const int per_foot = (N + ACC_THREADS - 1) / ACC_THREADS;
  *f = (int)blockIdx.x / per_foot;
  *e = ((int)blockIdx.x % per_foot) * ACC_THREADS + (int)threadIdx.x;
  return *f < FEET && *e < N;
}

// the profile bin of the finite phase ph: clamped as a float, then converted (see the header)
__device__ __forceinline__ int phase_bin(float ph) {
  const float b = floorf(ph * (float)BINS), last = (float)(BINS - 1);
  return (int)(b > last ? last : (b > 0.0f ? b : 0.0f));
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) feet_clear_kernel(const FeetArgs A) {
  const int N = A.c.num_envs;
  int f, e;
  if (!foot_thread(N, &f, &e)) return;
  const Go1FeetBuffers& b = A.b;
  const size_t i = (size_t)f * N + e;
  clear_rows(b, f * NM, NM, N, e);
  for (int bin = 0; bin < BINS; bin++) {
    const size_t w = (size_t)(f * BINS + bin) * N + e;
    b.profile_sum[w] = 0.0; b.profile_count[w] = 0u;
  }
  b.prev_contact[i] = 2; b.stance_valid[i] = 0; b.stance_steps[i] = 0;
  b.stance_peak[i] = 0.0f; b.stance_impulse[i] = 0.0f; b.stance_slip[i] = 0.0f;
  if (f == 0) { b.steps[e] = 0u; b.resets[e] = 0u; }
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) feet_accumulate_kernel(const FeetArgs A) {
  const Go1FeetConfig& c = A.c;
  const int N = c.num_envs;
  int f, e;
  if (!foot_thread(N, &f, &e)) return;
  const Go1FeetBuffers& b = A.b;
  const size_t i = (size_t)f * N + e;
  const bool reset = b.reset_buf[e] != 0;
  if (f == 0) {
    b.steps[e] += 1u;
    if (reset) b.resets[e] += 1u;
  }
  if (reset || b.episode_length_buf[e] <= c.warmup_steps) {                // nothing folded, the foot's state unknown
    b.prev_contact[i] = 2; b.stance_valid[i] = 0;
    return;
  }
  const size_t body = (size_t)(12 * (f + 1)) * N + e, vel = (size_t)(3 * f) * N + e;
  const float fx = b.contact_forces[body], fy = b.contact_forces[body + N], fz = b.contact_forces[body + 2 * (size_t)N];
  const float vx = b.foot_velocities[vel], vy = b.foot_velocities[vel + N], pvz = b.prev_foot_velocities[vel + 2 * (size_t)N];
  const float ph = b.foot_indices[i];
  const float mu = 0.5f * (b.friction_coeffs[e] + c.terrain_friction);
  const int prev = (int)b.prev_contact[i];
  const bool valid = b.stance_valid[i] != 0;

  const bool contact = fz > (float)GO1FEET_CONTACT_FORCE;
  const float hh = fx * fx + fy * fy;
  const float fn = sqrtf(hh + fz * fz), ft = sqrtf(hh), s = sqrtf(vx * vx + vy * vy);
  const float d = fn - c.max_contact_force;
  float excess = d > 0.0f ? d : 0.0f;
  if (d != d) excess = d;                                                  // (the select would drop the NaN)
  const float m = pvz < -100.0f ? -100.0f : (pvz > 0.0f ? 0.0f : pvz);
  const int row = f * NM;
  fold(b, row + GO1FEET_CONTACT, N, e, contact ? 1.0f : 0.0f);
  if (contact) {
    fold(b, row + GO1FEET_FORCE_NORMAL, N, e, fz);
    fold(b, row + GO1FEET_FORCE_TANGENT, N, e, ft);
    fold(b, row + GO1FEET_FRICTION_USE, N, e, ft / (mu * fz));
  }
  fold(b, row + GO1FEET_FORCE_EXCESS, N, e, excess);
  fold(b, row + GO1FEET_IMPACT_VEL_SQ, N, e, fn > 1.0f ? m * m : 0.0f);

  if (contact) {
    if (prev == 0) {                                                       // touchdown: a stance seen from its first step
      fold(b, row + GO1FEET_TOUCHDOWN_SPEED, N, e, pvz < 0.0f ? -pvz : 0.0f);
      fold(b, row + GO1FEET_TOUCHDOWN_FORCE, N, e, fz);
    }
  } else if (prev == 1 && valid) {                                         // lift-off: the stance is complete
    fold(b, row + GO1FEET_STANCE_PEAK_FORCE, N, e, b.stance_peak[i]);
    fold(b, row + GO1FEET_STANCE_IMPULSE, N, e, b.stance_impulse[i]);
    fold(b, row + GO1FEET_STANCE_SLIP, N, e, b.stance_slip[i]);
    fold(b, row + GO1FEET_STANCE_TIME, N, e, (float)b.stance_steps[i] * c.dt);
  }

  if (isfinite(ph) && isfinite(fz)) {
    const size_t w = (size_t)(f * BINS + phase_bin(ph)) * N + e;           // the bin is clamped: in [0, BINS)
    b.profile_sum[w] += (double)fz;
    b.profile_count[w] += 1u;
  }

  if (contact) {
    if (prev == 0) {
      b.stance_valid[i] = 1; b.stance_steps[i] = 1;
      b.stance_peak[i] = fz; b.stance_impulse[i] = fz * c.dt; b.stance_slip[i] = s * c.dt;
    } else if (prev == 1 && valid) {
      b.stance_steps[i] += 1;
      b.stance_peak[i] = fmaxf(b.stance_peak[i], fz);
      b.stance_impulse[i] += fz * c.dt;
      b.stance_slip[i] += s * c.dt;
    }                                                                      // (prev == 2: began unobserved; stance_valid is 0 already)
  } else if (valid) {
    b.stance_valid[i] = 0;
  }
  b.prev_contact[i] = contact ? 1 : 0;
}

extern "C" __global__ void __launch_bounds__(RT) feet_reduce_kernel(const FeetArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = FEET * NM + 1;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1FeetBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m != rows - 1) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: environments, steps, resets
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int e = t; e < N; e += RT) {
      if (b.group[e] != g) continue;
      a0 += 1.0; a1 += (double)b.steps[e]; a2 += (double)b.resets[e];
    }
    lds[0][t] = a0; lds[1][t] = a1; lds[2][t] = a2;
    tree_reduce<3>(lds, t);
    if (t != 0) return;
    out[GO1FEET_G_ENVS] = lds[0][0]; out[GO1FEET_G_STEPS] = lds[1][0]; out[GO1FEET_G_RESETS] = lds[2][0];
    out[3] = 0.0; out[4] = 0.0; out[5] = 0.0;
    return;
  }
  // the profile of (group, foot): thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
  const int k = (int)blockIdx.x - G * rows;
  const int g = k / FEET, f = k % FEET, bin = t % BINS;
  const size_t w = (size_t)(f * BINS + bin) * N;
  double sum = 0.0, count = 0.0;
  for (int e = t / BINS; e < N; e += SLICES) {
    if (b.group[e] != g) continue;
    sum += b.profile_sum[w + e]; count += (double)b.profile_count[w + e];
  }
  lds[0][t] = sum; lds[1][t] = count;
  __syncthreads();
  for (int s = RT / 2; s >= BINS; s >>= 1) {
    if (t < s) { lds[0][t] += lds[0][t + s]; lds[1][t] += lds[1][t + s]; }
    __syncthreads();
  }
  if (t < BINS) {
    double* out = b.profile_results + (((size_t)g * FEET + f) * BINS + t) * 2;
    out[0] = lds[0][t]; out[1] = lds[1][t];
  }
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
dim3 foot_grid(int n) { return dim3((unsigned)(FEET * ((n + ACC_THREADS - 1) / ACC_THREADS))); }

int launch(void (*kernel)(FeetArgs), dim3 grid, int block, void* stream, const Go1FeetConfig* cfg, const Go1FeetBuffers* buf) {
  FeetArgs A; A.c = *cfg; A.b = *buf;
  hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

bool finite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }        // (a NaN fails both)

// what every entry point asks first: -1, -2
int check(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!buf->count || !buf->sum || !buf->sumsq || !buf->min || !buf->max || !buf->nonfinite || !buf->prev_contact || !buf->stance_valid ||
      !buf->stance_steps || !buf->stance_peak || !buf->stance_impulse || !buf->stance_slip || !buf->steps || !buf->resets ||
      !buf->profile_sum || !buf->profile_count) return -2;
  return 0;
}
}  // namespace

extern "C" int go1feet_clear(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(feet_clear_kernel, foot_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1feet_accumulate(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->contact_forces || !buf->foot_velocities || !buf->prev_foot_velocities || !buf->foot_indices || !buf->friction_coeffs ||
      !buf->reset_buf || !buf->episode_length_buf) return -3;
  if (!(finite(cfg->dt) && cfg->dt > 0.0f && finite(cfg->terrain_friction) && cfg->terrain_friction >= 0.0f && finite(cfg->max_contact_force)))
    return -12;
  return launch(feet_accumulate_kernel, foot_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1feet_reduce(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (cfg->num_groups <= 0 || !buf->group || !buf->results || !buf->profile_results) return -5;
  return launch(feet_reduce_kernel, dim3((unsigned)(cfg->num_groups * (FEET * NM + 1 + FEET))), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1feet_version(void) { return "go1feet 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
