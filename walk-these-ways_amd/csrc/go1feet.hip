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
// The fold of a value into the six accumulators, the clear, the launch of one thread per (row, environment), the fixed-order reductions
// (a metric row, the sums of a group row, the sums per bin of the profile) and the validation and launch helpers are go1_tables.h's,
// shared with the evaluation and trunk libraries.  The library's surface, symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1feet.h"
#include "go1_tables.h"

namespace {

constexpr int NM = GO1FEET_NUM, FEET = GO1FEET_NUM_FEET;
GO1_TABLES_MATCH(GO1FEET);
static_assert(GO1FEET_PHASE_BINS == BINS, "feet_reduce_kernel: the profile's bins are bin_sums'");

using FeetArgs = Args<Go1FeetConfig, Go1FeetBuffers>;

// the profile bin of the finite phase ph: clamped as a float, then converted (see the header)
__device__ __forceinline__ int phase_bin(float ph) {
  const float b = floorf(ph * (float)BINS), last = (float)(BINS - 1);
  return (int)(b > last ? last : (b > 0.0f ? b : 0.0f));
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) feet_clear_kernel(const FeetArgs A) {
  const int N = A.c.num_envs;
  int f, e;
  if (!row_thread(N, FEET, &f, &e)) return;                               // (block k is foot k / blocks_per_foot)
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
  if (!row_thread(N, FEET, &f, &e)) return;                               // (block k is foot k / blocks_per_foot)
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
    // the group's own row: a[0] envs, a[1] steps, a[2] resets
    group_sums<3>(b.group, g, N, lds, [&b](int e, double* a) { a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.resets[e]; });
    if (t != 0) return;
    out[GO1FEET_G_ENVS] = lds[0][0]; out[GO1FEET_G_STEPS] = lds[1][0]; out[GO1FEET_G_RESETS] = lds[2][0];
    out[3] = 0.0; out[4] = 0.0; out[5] = 0.0;
    return;
  }
  // the profile of (group, foot): thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
  const int k = (int)blockIdx.x - G * rows;
  const int g = k / FEET, f = k % FEET;
  const size_t w = (size_t)(f * BINS + t % BINS) * N;
  bin_sums<2>(b.group, g, N, lds, [&b, w](int e, double* a) { a[0] += b.profile_sum[w + e]; a[1] += (double)b.profile_count[w + e]; });
  if (t < BINS) {
    double* out = b.profile_results + (((size_t)g * FEET + f) * BINS + t) * 2;
    out[0] = lds[0][t]; out[1] = lds[1][t];
  }
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev_contact || !buf->stance_valid || !buf->stance_steps || !buf->stance_peak || !buf->stance_impulse ||
      !buf->stance_slip || !buf->steps || !buf->resets || !buf->profile_sum || !buf->profile_count) return -2;
  return 0;
}
}  // namespace

extern "C" int go1feet_clear(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(feet_clear_kernel, row_grid(FEET, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1feet_accumulate(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->contact_forces || !buf->foot_velocities || !buf->prev_foot_velocities || !buf->foot_indices || !buf->friction_coeffs ||
      !buf->reset_buf || !buf->episode_length_buf) return -3;
  if (!(finite(cfg->dt) && cfg->dt > 0.0f && finite(cfg->terrain_friction) && cfg->terrain_friction >= 0.0f && finite(cfg->max_contact_force)))
    return -12;
  return launch(feet_accumulate_kernel, row_grid(FEET, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1feet_reduce(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->profile_results) return -5;
  return launch(feet_reduce_kernel, table_grid(cfg->num_groups, FEET * NM + 1 + FEET), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1feet_version(void) { return "go1feet 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
