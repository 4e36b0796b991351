// go1sens.hip — the robustness of a policy rollout against the randomised dynamics on the device (include/go1sens.h), gfx950: per
// dynamics parameter and bin of its value the exposure, falls, time-outs, reward, tracking errors and power, charged to the value that
// was in force during the step.
//
// sens_accumulate_kernel: one thread per (row, environment) through row_thread, rows 0 .. 8 the parameters and row 9 the pair; lanes on
// consecutive environments, so every row access of a wavefront is one contiguous run of 64 words (the words of a bin alone are scattered:
// the bin differs from lane to lane).  Each word has one writer: no atomics, no LDS, nothing depends on scheduling.  The ten threads of
// an environment compute the step's outcomes with the same operations on the same inputs.
// sens_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, parameter) for the curves, one per
// (group, parameter) for the three counts, and four per group for the pair map.
// tests/sens_ref.py restates all of it in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear, the fixed-order reductions (a metric row, the sums of a group row, the sums
// per bin) and the validation and launch helpers are go1_tables.h's, shared with the other table libraries.  The library's surface,
// symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1sens.h"
#include "go1_tables.h"

namespace {

constexpr int NP = GO1SENS_NUM, NQ = GO1SENS_NUM_QUANT, NC = GO1SENS_NUM_COUNTS, CELLS = GO1SENS_PAIR_CELLS, PQ = GO1SENS_PAIR_QUANT;
constexpr int SIDE = GO1SENS_PAIR_SIDE, PAIR_GROUPS = CELLS / GO1SENS_BINS;
GO1_TABLES_MATCH(GO1SENS);
static_assert(GO1SENS_BINS == BINS, "sens_reduce_kernel: the curves' bins are bin_sums'");
static_assert(GO1SENS_KD_FACTOR == NP - 1 && NP == 9, "sens_accumulate_kernel: nine parameters");
static_assert(SIDE * SIDE == CELLS && 2 * SIDE == BINS && PAIR_GROUPS * BINS == CELLS, "the pair map: two bins per side step, sixteen cells per workgroup");
static_assert(NQ == 8 && PQ == 4 && NC == 3, "sens_reduce_kernel: eight quantities per bin, four per cell, three counts");

using SensArgs = Args<Go1SensConfig, Go1SensBuffers>;

// the simulator's value of parameter p (in [0, NP)) for environment e at this moment
__device__ __forceinline__ float now(const Go1SensBuffers& b, int p, size_t n, int e) {
  switch (p) {
    case GO1SENS_FRICTION: return b.friction_coeffs[e];
    case GO1SENS_RESTITUTION: return b.restitutions[e];
    case GO1SENS_PAYLOAD: return b.payloads[e];
    case GO1SENS_COM_X: return b.com_displacements[e];
    case GO1SENS_COM_Y: return b.com_displacements[n + e];
    case GO1SENS_COM_Z: return b.com_displacements[2 * n + e];
    case GO1SENS_MOTOR_STRENGTH: return b.motor_strengths[e];
    case GO1SENS_KP_FACTOR: return b.Kp_factors[e];
    default: return b.Kd_factors[e];
  }
}

// the bin of a value: -1 for none, else in [0, BINS)
__device__ __forceinline__ int bin_of(float v, float lo, float scale) {
  if (!isfinite(v)) return -1;
  float t = (v - lo) * scale;
  t = fminf(fmaxf(t, 0.0f), (float)(BINS - 1));
  return (int)t;
}

// both indices name a parameter (the entry points refuse half a pair; the kernels index with nothing else)
__device__ __forceinline__ bool has_pair(const Go1SensConfig& c) { return c.pair_a >= 0 && c.pair_a < NP && c.pair_b >= 0 && c.pair_b < NP; }

struct Outcomes {
  float lin_err, yaw_err, power;
  bool finite;
};

// the three outcomes of the step just taken by environment e
__device__ __forceinline__ Outcomes outcomes(const Go1SensBuffers& b, size_t n, int e) {
  Outcomes o;
  const float ex = b.base_lin_vel[e] - b.commands[e], ey = b.base_lin_vel[n + e] - b.commands[n + e];
  o.lin_err = sqrtf(ex * ex + ey * ey);
  o.yaw_err = fabsf(b.base_ang_vel[2 * n + e] - b.commands[2 * n + e]);
  double psum = 0.0;
  for (int j = 0; j < 12; j++) psum += (double)(b.torques[j * n + e] * b.dof_vel[j * n + e]);
  o.power = (float)psum;
  o.finite = isfinite(o.lin_err) && isfinite(o.yaw_err) && isfinite(o.power);
  return o;
}

// cur and pair_cur of environment e from the simulator's buffers
__device__ __forceinline__ void take(const Go1SensConfig& c, const Go1SensBuffers& b, size_t n, int e) {
  for (int p = 0; p < NP; p++) b.cur[p * n + e] = now(b, p, n, e);
  const bool pair = has_pair(c);
  b.pair_cur[e] = pair ? now(b, c.pair_a, n, e) : 0.0f;
  b.pair_cur[n + e] = pair ? now(b, c.pair_b, n, e) : 0.0f;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) sens_clear_kernel(const SensArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1SensBuffers& b = A.b;
  const size_t n = (size_t)N;
  clear_rows(b, 0, NP, N, e);
  for (int k = 0; k < NP * BINS; k++) {
    const size_t i = k * n + e;
    b.steps[i] = 0u; b.measured[i] = 0u; b.falls[i] = 0u; b.timeouts[i] = 0u;
    b.reward_sum[i] = 0.0; b.lin_err_sum[i] = 0.0; b.yaw_err_sum[i] = 0.0; b.power_sum[i] = 0.0;
  }
  for (int p = 0; p < NP; p++) { b.unbinned[p * n + e] = 0u; b.redraws[p * n + e] = 0u; b.bad[p * n + e] = 0u; }
  b.launches[e] = 0u;
  for (int k = 0; k < CELLS; k++) {
    const size_t i = k * n + e;
    b.pair_steps[i] = 0u; b.pair_falls[i] = 0u; b.pair_measured[i] = 0u; b.pair_lin_err_sum[i] = 0.0;
  }
  take(A.c, b, n, e);
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) sens_snapshot_kernel(const SensArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  take(A.c, A.b, (size_t)N, e);
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) sens_accumulate_kernel(const SensArgs A) {
  const Go1SensConfig& c = A.c;
  const int N = c.num_envs;
  int p, e;
  if (!row_thread(N, NP + 1, &p, &e)) return;
  const Go1SensBuffers& b = A.b;
  const size_t n = (size_t)N;
  const bool reset = b.reset_buf[e] != 0;
  const bool live = !reset && b.episode_length_buf[e] > c.warmup_steps;

  if (p == NP) {                                                           // the pair thread
    b.launches[e] += 1u;
    if (!has_pair(c)) return;
    const int pa = c.pair_a, pb = c.pair_b;
    const int ba = bin_of(b.pair_cur[e], c.lo[pa], c.scale[pa]), bb = bin_of(b.pair_cur[n + e], c.lo[pb], c.scale[pb]);
    if (ba >= 0 && bb >= 0) {
      const size_t i = (size_t)(SIDE * (ba >> 1) + (bb >> 1)) * n + e;      // both bins are clamped: the cell is in [0, CELLS)
      b.pair_steps[i] += 1u;
      if (reset) {
        if (b.time_out_buf[e] == 0) b.pair_falls[i] += 1u;
      } else if (live) {
        const Outcomes o = outcomes(b, n, e);
        if (o.finite) { b.pair_measured[i] += 1u; b.pair_lin_err_sum[i] += (double)o.lin_err; }
      }
    }
    b.pair_cur[e] = now(b, pa, n, e);
    b.pair_cur[n + e] = now(b, pb, n, e);
    return;
  }

  if (c.active[p] == 0) return;
  const size_t row = (size_t)p * n + e;
  const float v = b.cur[row];
  const int bin = bin_of(v, c.lo[p], c.scale[p]);
  fold(b, p, N, e, v);                                                     // 1
  if (bin < 0) {
    b.unbinned[row] += 1u;                                                 // 2
  } else {
    const size_t i = ((size_t)p * BINS + bin) * n + e;                     // the bin is clamped: in [0, BINS)
    const float r = b.rew_buf[e];
    b.steps[i] += 1u;                                                      // 3
    if (isfinite(r)) b.reward_sum[i] += (double)r;
    else b.bad[row] += 1u;
    if (reset) {                                                           // 4
      if (b.time_out_buf[e] != 0) b.timeouts[i] += 1u;
      else b.falls[i] += 1u;
    } else if (live) {                                                     // 5
      const Outcomes o = outcomes(b, n, e);
      if (o.finite) {
        b.measured[i] += 1u;
        b.lin_err_sum[i] += (double)o.lin_err; b.yaw_err_sum[i] += (double)o.yaw_err; b.power_sum[i] += (double)o.power;
      } else {
        b.bad[row] += 1u;
      }
    }
  }
  const float w = now(b, p, n, e);                                         // 6
  if (__float_as_int(w) != __float_as_int(v)) b.redraws[row] += 1u;
  b.cur[row] = w;
}

extern "C" __global__ void __launch_bounds__(RT) sens_reduce_kernel(const SensArgs A) {
  __shared__ double lds[NQ][RT];
  static_assert(NQ >= NF, "the metric rows need six slices");
  constexpr int rows = NP + 1;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1SensBuffers& b = A.b;
  const size_t n = (size_t)N;
  int k = (int)blockIdx.x;
  if (k < G * rows) {
    const int g = k / rows, m = k % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m < NP) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: a[0] envs, a[1] launches
    group_sums<2>(b.group, g, N, lds, [&b](int e, double* a) { a[0] += 1.0; a[1] += (double)b.launches[e]; });
    if (t != 0) return;
    out[GO1SENS_G_ENVS] = lds[0][0]; out[GO1SENS_G_LAUNCHES] = lds[1][0];
    out[2] = 0.0; out[3] = 0.0; out[4] = 0.0; out[5] = 0.0;
    return;
  }
  k -= G * rows;
  if (k < G * NP) {
    // the curves of (group, parameter): thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
    const int g = k / NP, p = k % NP;
    const size_t w = ((size_t)p * BINS + t % BINS) * n;
    bin_sums<NQ>(b.group, g, N, lds, [&b, w](int e, double* a) {
      const size_t i = w + e;
      a[GO1SENS_Q_STEPS] += (double)b.steps[i]; a[GO1SENS_Q_MEASURED] += (double)b.measured[i]; a[GO1SENS_Q_FALLS] += (double)b.falls[i];
      a[GO1SENS_Q_TIMEOUTS] += (double)b.timeouts[i]; a[GO1SENS_Q_REWARD_SUM] += b.reward_sum[i]; a[GO1SENS_Q_LIN_ERR_SUM] += b.lin_err_sum[i];
      a[GO1SENS_Q_YAW_ERR_SUM] += b.yaw_err_sum[i]; a[GO1SENS_Q_POWER_SUM] += b.power_sum[i];
    });
    if (t < BINS) {
      double* out = b.curves + ((size_t)g * NP + p) * NQ * BINS;
      for (int q = 0; q < NQ; q++) out[q * BINS + t] = lds[q][t];
    }
    return;
  }
  k -= G * NP;
  if (k < G * NP) {
    // the three counts of (group, parameter): a[0] unbinned, a[1] redraws, a[2] bad
    const int g = k / NP, p = k % NP;
    const size_t w = (size_t)p * n;
    group_sums<NC>(b.group, g, N, lds, [&b, w](int e, double* a) {
      a[GO1SENS_C_UNBINNED] += (double)b.unbinned[w + e]; a[GO1SENS_C_REDRAWS] += (double)b.redraws[w + e]; a[GO1SENS_C_BAD] += (double)b.bad[w + e];
    });
    if (t != 0) return;
    double* out = b.counts + ((size_t)g * NP + p) * NC;
    out[GO1SENS_C_UNBINNED] = lds[0][0]; out[GO1SENS_C_REDRAWS] = lds[1][0]; out[GO1SENS_C_BAD] = lds[2][0];
    return;
  }
  k -= G * NP;
  // sixteen cells of a group's pair map: thread t owns cell 16 * part + t % 16
  const int g = k / PAIR_GROUPS, part = k % PAIR_GROUPS;
  const int cell = part * BINS + t % BINS;
  const size_t w = (size_t)cell * n;
  bin_sums<PQ>(b.group, g, N, lds, [&b, w](int e, double* a) {
    const size_t i = w + e;
    a[GO1SENS_P_STEPS] += (double)b.pair_steps[i]; a[GO1SENS_P_FALLS] += (double)b.pair_falls[i]; a[GO1SENS_P_MEASURED] += (double)b.pair_measured[i];
    a[GO1SENS_P_LIN_ERR_SUM] += b.pair_lin_err_sum[i];
  });
  if (t < BINS) {
    double* out = b.pair_results + (size_t)g * PQ * CELLS;
    for (int q = 0; q < PQ; q++) out[q * CELLS + cell] = lds[q][t];
  }
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1SensConfig* cfg, const Go1SensBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->cur || !buf->pair_cur || !buf->steps || !buf->measured || !buf->falls || !buf->timeouts || !buf->reward_sum ||
      !buf->lin_err_sum || !buf->yaw_err_sum || !buf->power_sum || !buf->unbinned || !buf->redraws || !buf->bad || !buf->launches || !buf->pair_steps ||
      !buf->pair_falls || !buf->pair_measured || !buf->pair_lin_err_sum) return -2;
  return 0;
}

bool has_parameters(const Go1SensBuffers* buf) {
  return buf->friction_coeffs && buf->restitutions && buf->payloads && buf->com_displacements && buf->motor_strengths && buf->Kp_factors && buf->Kd_factors;
}

// -12: the bins of an active parameter, and the pair
bool good_config(const Go1SensConfig* cfg) {
  for (int p = 0; p < NP; p++)
    if (cfg->active[p] != 0 && (!positive(cfg->scale[p]) || !finite(cfg->lo[p]))) return false;
  const int a = cfg->pair_a, b = cfg->pair_b;
  if (a < -1 || a >= NP || b < -1 || b >= NP) return false;
  if (a == -1 && b == -1) return true;
  if (a == -1 || b == -1 || a == b) return false;
  return cfg->active[a] != 0 && cfg->active[b] != 0;
}
}  // namespace

extern "C" int go1sens_clear(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_parameters(buf)) return -3;
  return launch(sens_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1sens_snapshot(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_parameters(buf)) return -3;
  return launch(sens_snapshot_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1sens_accumulate(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->reset_buf || !buf->time_out_buf || !buf->episode_length_buf || !buf->rew_buf || !buf->base_lin_vel || !buf->base_ang_vel || !buf->commands ||
      !buf->torques || !buf->dof_vel || !has_parameters(buf)) return -3;
  if (!good_config(cfg)) return -12;
  return launch(sens_accumulate_kernel, row_grid(NP + 1, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1sens_reduce(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->curves || !buf->counts || !buf->pair_results) return -5;
  return launch(sens_reduce_kernel, table_grid(cfg->num_groups, NP + 1 + NP + NP + PAIR_GROUPS), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1sens_version(void) { return "go1sens 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
