/* go1eval.h — C-ABI of the policy-evaluation metrics (libgo1eval.so).
 *
 * Replaces the per-step host evaluation of the reference's go1_gym_learn/eval_metrics/metrics.py (METRICS_FNS, each a torch
 * expression followed by .cpu()): one launch after a simulator step folds ten scalar metrics of every environment into
 * per-environment accumulators on the device, and one launch at the end of a sweep reduces them per group of environments.
 * The step loop never waits for the host.
 *
 * Conventions (as include/go1sim.h, include/go1render.h)
 *   - plain C; every pointer in Go1EvalBuffers is a DEVICE pointer owned by the caller.  The library never allocates, never
 *     copies between host and device and never synchronises the stream.  Return value 0 = ok, < 0 = error code.
 *   - inputs are the simulator's SoA buffers: component c of environment e at index c*N + e.
 *
 * Metrics (fp32, the reference's formulas; index = Go1EvalMetric):
 *   lin_vel_rmsd       sqrt((base_lin_vel[0] - commands[0])^2)
 *   ang_vel_rmsd       sqrt((base_ang_vel[2] - commands[2])^2)
 *   lin_vel_x          base_lin_vel[0]
 *   ang_vel_yaw        base_ang_vel[2]
 *   base_height        mean over the height points of (root_states[2] - measured_heights[p]); measured_heights = NULL: root_states[2]
 *   max_torques        max over the 12 joints of |torques[j]|
 *   power_consumption  sum over the 12 joints of torques[j] * dof_vel[j]
 *   CoT                power_consumption / ((default_body_mass + payloads) * 9.8 * |base_lin_vel[0:2]|)
 *   froude_number      base_lin_vel[0]^2 / (9.8 * 0.30)
 *   termination        reset_buf (1 on a step that ended an episode, by termination or by time-out; else 0)
 *   Every term and every result is an fp32 value, as in the reference.  The two long sums (base_height over the height points,
 *   power_consumption over the joints) add their fp32 terms in an fp64 carry and round to fp32 once: torch fixes no order for an
 *   fp32 sum, and this result lies within the rounding bound of every order.  Consequence: a step's base_height and
 *   power_consumption (and CoT, which divides it) need not be bit-equal to what METRICS_FNS gives on the same device, so their
 *   minima and maxima may differ from torch's in the last bit; the other metrics' per-step values are the same fp32 operations.
 *
 * go1eval_accumulate, per environment e (one thread each, no atomics, no cross-lane traffic: every accumulator has exactly
 * one writer, so the result does not depend on scheduling), in this order:
 *   1. steps[e] += 1.
 *   2. reset_buf[e] != 0: the step ended an episode.  episodes_timed_out[e] += 1 if time_out_buf[e] != 0, else
 *      episodes_terminated[e] += 1; the value 1 is folded into `termination`; NOTHING else is touched (the buffers then mix the
 *      old episode's velocities with the new episode's pose).
 *   3. otherwise, episode_length_buf[e] <= warmup_steps: nothing more (the drop from the spawn height does not pollute the
 *      tracking error).  episode_length_buf == warmup_steps is excluded, warmup_steps + 1 is the first step that counts.
 *   4. otherwise all ten metrics are folded (termination with the value 0).
 *   Folding a value v into metric m:  v not finite (CoT of a robot that stands still divides by zero): nonfinite[m][e] += 1 and
 *   nothing else.  Otherwise count[m][e] += 1, sum[m][e] += (double)v, sumsq[m][e] += (double)v * (double)v,
 *   min[m][e] = min(min, v), max[m][e] = max(max, v).
 *
 * go1eval_reduce, per group g in [0, num_groups) (group[e] == g; -1 or any id outside the range = not evaluated) and metric m,
 * over the group's environments, fp64:
 *   count = sum of count[m][e];  nonfinite = sum of nonfinite[m][e];  S = sum of sum[m][e];  Q = sum of sumsq[m][e]
 *   mean = S / count;  std = sqrt(max(Q / count - mean^2, 0))  (population, over every folded step of every environment);
 *   min / max over the environments with count[m][e] > 0.  count == 0: mean, std, min, max are NaN.
 *   Row GO1EVAL_NUM_METRICS of a group holds the group's own figures (Go1EvalGroupField): environments, steps (sum of steps[e]),
 *   episodes_terminated, episodes_timed_out, fall_rate = environments with episodes_terminated[e] > 0 / environments (NaN for an
 *   empty group; the definition of tools/play_eval.py), 0.
 *   Fixed combination order: thread t of GO1EVAL_REDUCE_THREADS combines environments t, t + T, t + 2T, ... in ascending order,
 *   then a binary tree over the threads (stride T/2, T/4, ... 1: thread t takes thread t + stride).  Same inputs, same bits.
 */
#ifndef GO1EVAL_H_INCLUDED
#define GO1EVAL_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1EVAL_NUM_METRICS 10
#define GO1EVAL_NUM_FIELDS 6
#define GO1EVAL_REDUCE_THREADS 256
#define GO1EVAL_GRAVITY 9.8          /* the reference's g; fp32 where it meets an fp32 value */
#define GO1EVAL_FROUDE_HEIGHT 0.30   /* the reference's leg length h; g * h is formed in double, then rounded to fp32 */

enum Go1EvalMetric {
  GO1EVAL_LIN_VEL_RMSD = 0, GO1EVAL_ANG_VEL_RMSD = 1, GO1EVAL_LIN_VEL_X = 2, GO1EVAL_ANG_VEL_YAW = 3, GO1EVAL_BASE_HEIGHT = 4,
  GO1EVAL_MAX_TORQUES = 5, GO1EVAL_POWER_CONSUMPTION = 6, GO1EVAL_COT = 7, GO1EVAL_FROUDE_NUMBER = 8, GO1EVAL_TERMINATION = 9
};
/* columns of a metric row of the result table */
enum Go1EvalField { GO1EVAL_F_COUNT = 0, GO1EVAL_F_MEAN = 1, GO1EVAL_F_STD = 2, GO1EVAL_F_MIN = 3, GO1EVAL_F_MAX = 4, GO1EVAL_F_NONFINITE = 5 };
/* columns of a group's own row (row GO1EVAL_NUM_METRICS) */
enum Go1EvalGroupField { GO1EVAL_G_ENVS = 0, GO1EVAL_G_STEPS = 1, GO1EVAL_G_TERMINATED = 2, GO1EVAL_G_TIMED_OUT = 3, GO1EVAL_G_FALL_RATE = 4 };

typedef struct Go1EvalConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t num_height_points;   /* rows of measured_heights (ignored when it is NULL) */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold no metric */
  int32_t num_groups;          /* G of the result table */
  float default_body_mass;     /* kg, the reference's env.default_body_mass */
} Go1EvalConfig;

typedef struct Go1EvalBuffers {
  /* read by go1eval_accumulate */
  const float* base_lin_vel;          /* [3][N] */
  const float* base_ang_vel;          /* [3][N] */
  const float* commands;              /* [>= 3][N] */
  const float* root_states;           /* [13][N]; row 2 is read */
  const float* measured_heights;      /* [num_height_points][N] or NULL (the ground is 0) */
  const float* torques;               /* [12][N] */
  const float* dof_vel;               /* [12][N] */
  const float* payloads;              /* [N] */
  const uint8_t* reset_buf;           /* [N] */
  const uint8_t* time_out_buf;        /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* accumulators, [GO1EVAL_NUM_METRICS][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* [N] */
  uint32_t* steps;
  uint32_t* episodes_terminated;
  uint32_t* episodes_timed_out;
  /* go1eval_reduce */
  const int32_t* group;               /* [N] */
  double* results;                    /* [num_groups][GO1EVAL_NUM_METRICS + 1][GO1EVAL_NUM_FIELDS] */
} Go1EvalBuffers;

/* empty accumulators: counts 0, sums 0, min = +inf, max = -inf.  One launch. */
int go1eval_clear(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream);

/* after a simulator step: fold the step into the accumulators.  One launch, one thread per environment. */
int go1eval_accumulate(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream);

/* at the end: the result table from the accumulators (which it leaves as they are).  One launch. */
int go1eval_reduce(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream);

/* "go1eval <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1eval_version(void);

#ifdef __cplusplus
}
#endif

#endif
