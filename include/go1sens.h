/* go1sens.h — C-ABI of libgo1sens.so: the robustness of a policy rollout against the randomised dynamics, measured on the device (HIP,
 * gfx950): per dynamics parameter and per bin of its value, the exposure, the falls and time-outs, the reward, the two tracking errors and
 * the mechanical power.
 *
 * The other families reduce a rollout by command cell.  This one reduces it by what the evaluation presets vary: friction, restitution,
 * payload, the displacement of the centre of mass and the motor strength (and the two gain factors).  The parameters move during a
 * rollout inside the step kernel (a reset re-draws the motor parameters, the randomisation interval re-draws them all), and on the step
 * of a fall the simulator's buffers already hold the respawned robot's values.  So the values IN FORCE are carried here from step to
 * step, and a fall is charged to the bin of the carried value.  It is a library of its own, as the episode library is: no other binary,
 * stamp or parity result depends on it.  The accumulators, the folding rule, the fixed-order reductions and the numbering of the return
 * codes are go1eval.h's, restated here (the device helpers are csrc/go1_tables.h's, shared with those libraries and covered by this
 * library's stamp).  This header is the specification: tests/sens_ref.py is written from its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).
 *
 * Nine parameters (index = Go1SensParam); now(p, e) is the simulator's value of parameter p for environment e at this moment:
 *   friction        friction_coeffs[e]                 com_y           row 1 of com_displacements [3][N]
 *   restitution     restitutions[e]                    com_z           row 2 of com_displacements
 *   payload         payloads[e]                        motor_strength  row 0 of motor_strengths [12][N]
 *   com_x           row 0 of com_displacements         Kp_factor       row 0 of Kp_factors [12][N]
 *                                                      Kd_factor       row 0 of Kd_factors [12][N]
 * The simulator draws one value for all twelve joints, so row 0 stands for them (a caller who wrote per-joint values gets joint 0's).
 *
 * The config carries per parameter active[p], lo[p] and scale[p] = 16 / (hi - lo) (computed by the host in fp64 and rounded to fp32
 * once), and the pair (pair_a, pair_b): two parameter indices, or -1 and -1 for no pair.
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off).  Only + - *,
 * sqrtf, fabsf, fminf, fmaxf, conversions and comparisons are used.
 *
 * bin(p, v), the bin of a value v of parameter p:  none if v is not finite;  otherwise t = (v - lo[p]) * scale[p], then
 *   t = fminf(fmaxf(t, 0), 15), and the bin is (int)t.  A finite value outside [lo, hi) lands in an end bin; the `value` row's min and
 *   max show it.
 *
 * Per environment e, the inputs of a step (read after the simulator's step):
 *   r        rew_buf;  reset_buf, time_out_buf, episode_length_buf (elb below)
 *   vx, vy   rows 0 and 1 of base_lin_vel [3][N];  wz  row 2 of base_ang_vel [3][N];  cx, cy, cz  rows 0, 1 and 2 of commands
 *   torques [12][N], dof_vel [12][N], and the seven parameter buffers
 * The three outcomes of a step:
 *   lin_err = sqrtf(ex * ex + ey * ey), ex = vx - cx, ey = vy - cy
 *   yaw_err = fabsf(wz - cz)
 *   power   = go1eval.h's power_consumption: the twelve fp32 products torques[j] * dof_vel[j], added in ascending j in an fp64 carry,
 *             the carry rounded to fp32 once
 *
 * State per environment: cur [9][N] (float: the parameter values in force during the step that is about to be, or has just been, taken);
 * pair_cur [2][N] (float: a private copy of the pair's two values for the pair thread, because the parameter threads overwrite cur in
 * the same launch); per (parameter, bin): steps, measured, falls, timeouts (uint32 [9][16][N]) and reward_sum, lin_err_sum, yaw_err_sum,
 * power_sum (double [9][16][N]); per parameter: unbinned, redraws, bad (uint32 [9][N]); launches (uint32 [N]); the pair map:
 * pair_steps, pair_falls, pair_measured (uint32 [64][N]) and pair_lin_err_sum (double [64][N]), cell = 8 * row + column.
 * The accumulators ([9][N], row = parameter) are the `value` rows: the realised distribution of each parameter.
 *
 * go1sens_accumulate: ONE launch of one thread per (row, environment), 10 * ceil(N / 256) blocks of 256 threads, block k on row
 * k / ceil(N / 256): rows 0 .. 8 are the parameters, row 9 is the pair.  Every thread that needs them computes the step's outcomes with
 * the same operations, so they are the same bits in all ten.  No atomics, no LDS, every word has one writer.
 *   Parameter thread (p, e).  If active[p] == 0 it returns at once.  Otherwise, in this order:
 *   1. v = cur[p][e], b = bin(p, v).  v is folded into accumulator row p with the folding rule: a non-finite value adds 1 to
 *      nonfinite[p][e] and enters nothing else; a finite one adds 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and
 *      enters min by fminf and max by fmaxf.
 *   2. If b is none: unbinned[p][e] += 1, and steps 3 to 5 are skipped.
 *   3. steps[p][b][e] += 1.  If r is finite reward_sum[p][b][e] += (double)r, else bad[p][e] += 1.
 *   4. If reset_buf[e] != 0 (a reset step): timeouts[p][b][e] += 1 if time_out_buf[e] != 0, else falls[p][b][e] += 1.  Nothing else: the
 *      velocities and commands already belong to the respawned robot.  The fall is charged to the bin of the CARRIED value.
 *   5. Otherwise, if elb > warmup_steps: if lin_err, yaw_err and power are all finite, measured[p][b][e] += 1 and
 *      lin_err_sum, yaw_err_sum, power_sum [p][b][e] += (double) of each; else bad[p][e] += 1.
 *   6. On every step, binned or not: w = now(p, e).  If the bits of w differ from the bits of v, redraws[p][e] += 1.  cur[p][e] = w.
 *   Pair thread (row 9, e).  launches[e] += 1.  Without a pair (pair_a < 0 or pair_b < 0) nothing else.  Otherwise
 *   ba = bin(pair_a, pair_cur[0][e]), bb = bin(pair_b, pair_cur[1][e]); if both are bins, cell = 8 * (ba >> 1) + (bb >> 1) and:
 *   pair_steps[cell][e] += 1;  on a reset step pair_falls[cell][e] += 1 unless time_out_buf[e] != 0;  on any other step with
 *   elb > warmup_steps and all three outcomes finite pair_measured[cell][e] += 1 and pair_lin_err_sum[cell][e] += (double)lin_err.
 *   Then, with or without a cell, pair_cur[0][e] = now(pair_a, e) and pair_cur[1][e] = now(pair_b, e).
 *
 * go1sens_clear: one launch, one thread per environment: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0,
 *   min = +inf, max = -inf), every counter, sum and map word 0, cur[p][e] = now(p, e) for all nine parameters, and pair_cur from the
 *   pair's two (0 and 0 without a pair).
 * go1sens_snapshot: the same launch shape; takes cur and pair_cur again and touches nothing else.  For a reset from outside the step
 *   (reset_idx re-draws the motor parameters): what is in force from now is what the buffers hold.
 * go1sens_reduce: ONE launch of GO1SENS_REDUCE_THREADS-thread workgroups, which writes four tables and leaves what it reads as it is:
 *   num_groups * (GO1SENS_NUM + 1) workgroups write results[num_groups][GO1SENS_NUM + 1][GO1SENS_NUM_FIELDS].
 *     Rows 0 .. 8: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's environments
 *     e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments with
 *     count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields (index =
 *     Go1SensField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with count = 0
 *     the four in the middle are NaN.
 *     Row 9 (index = Go1SensGroupField): environments, launches (the sum of launches[e]), then 0, 0, 0, 0, in the same order.
 *   num_groups * GO1SENS_NUM further workgroups write curves[num_groups][GO1SENS_NUM][GO1SENS_NUM_QUANT][GO1SENS_BINS] as doubles, the
 *     quantities in the order of Go1SensQuantity: steps, measured, falls, timeouts, reward_sum, lin_err_sum, yaw_err_sum, power_sum.  In
 *     the workgroup of a (group, parameter) thread t owns bin t % 16 and adds, as doubles, its bin's eight words of the group's
 *     environments e = t / 16, t / 16 + 16, ... in ascending order; then a fixed tree over the 16 slices (thread t takes thread
 *     t + 128, then + 64, + 32, + 16) and threads 0 .. 15 write their bin: the foot library's profile order.
 *   num_groups * GO1SENS_NUM further workgroups write counts[num_groups][GO1SENS_NUM][GO1SENS_NUM_COUNTS] as doubles (index =
 *     Go1SensCount: unbinned, redraws, bad), summed as the group row is.
 *   num_groups * 4 further workgroups write pair_results[num_groups][GO1SENS_PAIR_QUANT][GO1SENS_PAIR_CELLS] as doubles (index =
 *     Go1SensPairQuantity: steps, falls, measured, lin_err_sum): workgroup k of a group owns the cells 16 k .. 16 k + 15, thread t the
 *     cell 16 k + t % 16, in the order of the curves.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator or a state array is missing
 *   -3   an input is missing (go1sens_accumulate: any; go1sens_clear and go1sens_snapshot: one of the seven parameter buffers;
 *        go1sens_reduce reads none)
 *   -5   no group, no table of the four, or num_groups <= 0 (go1sens_reduce only)
 *   -12  (go1sens_accumulate only) an active parameter whose scale is not positive and finite or whose lo is not finite; a pair index
 *        outside [-1, 8]; one index -1 and the other not; a pair of equal indices; an inactive pair member
 *   -20  the launch itself failed
 *
 * What the figures are not.  A value outside its range counts in an end bin.  A re-draw in the callback of step t takes effect at step
 * t + 1, and that is how it is charged.  The curves are marginal: inside a bin of one parameter the others vary freely; only the one
 * pair map shows an interaction.  motor_offsets (twelve independent draws), the lag and gravity (global) are not measured.  redraws
 * counts changes of the bits: a re-draw that lands on the same value is not seen.
 */
#ifndef GO1SENS_H
#define GO1SENS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1SENS_NUM 9
#define GO1SENS_BINS 16
#define GO1SENS_NUM_QUANT 8
#define GO1SENS_NUM_COUNTS 3
#define GO1SENS_PAIR_SIDE 8
#define GO1SENS_PAIR_CELLS 64
#define GO1SENS_PAIR_QUANT 4
#define GO1SENS_NUM_FIELDS 6
#define GO1SENS_REDUCE_THREADS 256

enum Go1SensParam {
  GO1SENS_FRICTION = 0, GO1SENS_RESTITUTION = 1, GO1SENS_PAYLOAD = 2, GO1SENS_COM_X = 3, GO1SENS_COM_Y = 4, GO1SENS_COM_Z = 5,
  GO1SENS_MOTOR_STRENGTH = 6, GO1SENS_KP_FACTOR = 7, GO1SENS_KD_FACTOR = 8
};
/* columns of a `value` row */
enum Go1SensField { GO1SENS_F_COUNT = 0, GO1SENS_F_MEAN = 1, GO1SENS_F_STD = 2, GO1SENS_F_MIN = 3, GO1SENS_F_MAX = 4, GO1SENS_F_NONFINITE = 5 };
/* columns of a group's own row (row GO1SENS_NUM) */
enum Go1SensGroupField { GO1SENS_G_ENVS = 0, GO1SENS_G_LAUNCHES = 1 };
/* the eight quantities of a curve */
enum Go1SensQuantity {
  GO1SENS_Q_STEPS = 0, GO1SENS_Q_MEASURED = 1, GO1SENS_Q_FALLS = 2, GO1SENS_Q_TIMEOUTS = 3, GO1SENS_Q_REWARD_SUM = 4,
  GO1SENS_Q_LIN_ERR_SUM = 5, GO1SENS_Q_YAW_ERR_SUM = 6, GO1SENS_Q_POWER_SUM = 7
};
/* the three counts per (group, parameter) */
enum Go1SensCount { GO1SENS_C_UNBINNED = 0, GO1SENS_C_REDRAWS = 1, GO1SENS_C_BAD = 2 };
/* the four quantities of the pair map */
enum Go1SensPairQuantity { GO1SENS_P_STEPS = 0, GO1SENS_P_FALLS = 1, GO1SENS_P_MEASURED = 2, GO1SENS_P_LIN_ERR_SUM = 3 };

typedef struct Go1SensConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps enter no outcome */
  int32_t num_groups;          /* G of the result tables */
  int32_t pair_a;              /* the pair map's row parameter, -1: no pair */
  int32_t pair_b;              /* the pair map's column parameter, -1: no pair */
  int32_t active[GO1SENS_NUM]; /* != 0: the parameter is measured */
  float lo[GO1SENS_NUM];       /* the lower edge of bin 0 */
  float scale[GO1SENS_NUM];    /* 16 / (hi - lo) */
} Go1SensConfig;

typedef struct Go1SensBuffers {
  /* read by go1sens_accumulate */
  const uint8_t* reset_buf;           /* [N] */
  const uint8_t* time_out_buf;        /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  const float* rew_buf;               /* [N] */
  const float* base_lin_vel;          /* [3][N] */
  const float* base_ang_vel;          /* [3][N] */
  const float* commands;              /* [num_commands][N] */
  const float* torques;               /* [12][N] */
  const float* dof_vel;               /* [12][N] */
  /* the seven parameter buffers: read by go1sens_accumulate, go1sens_clear and go1sens_snapshot */
  const float* friction_coeffs;       /* [N] */
  const float* restitutions;          /* [N] */
  const float* payloads;              /* [N] */
  const float* com_displacements;     /* [3][N] */
  const float* motor_strengths;       /* [12][N] */
  const float* Kp_factors;            /* [12][N] */
  const float* Kd_factors;            /* [12][N] */
  /* accumulators, [GO1SENS_NUM][N]: the `value` rows */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  float* cur;                         /* [GO1SENS_NUM][N]: the values in force */
  float* pair_cur;                    /* [2][N]: the pair thread's copy of its two */
  uint32_t* steps;                    /* [GO1SENS_NUM][GO1SENS_BINS][N]: launches spent in the bin */
  uint32_t* measured;                 /* [GO1SENS_NUM][GO1SENS_BINS][N]: of those, steps that entered the three outcome sums */
  uint32_t* falls;                    /* [GO1SENS_NUM][GO1SENS_BINS][N]: reset steps without time_out_buf */
  uint32_t* timeouts;                 /* [GO1SENS_NUM][GO1SENS_BINS][N]: reset steps with time_out_buf */
  double* reward_sum;                 /* [GO1SENS_NUM][GO1SENS_BINS][N] */
  double* lin_err_sum;                /* [GO1SENS_NUM][GO1SENS_BINS][N] */
  double* yaw_err_sum;                /* [GO1SENS_NUM][GO1SENS_BINS][N] */
  double* power_sum;                  /* [GO1SENS_NUM][GO1SENS_BINS][N] */
  uint32_t* unbinned;                 /* [GO1SENS_NUM][N]: launches with a value that has no bin */
  uint32_t* redraws;                  /* [GO1SENS_NUM][N]: launches after which the buffer held other bits */
  uint32_t* bad;                      /* [GO1SENS_NUM][N]: non-finite rewards and non-finite outcomes, not summed */
  uint32_t* launches;                 /* [N]: accumulate launches since the clear */
  uint32_t* pair_steps;               /* [GO1SENS_PAIR_CELLS][N] */
  uint32_t* pair_falls;               /* [GO1SENS_PAIR_CELLS][N] */
  uint32_t* pair_measured;            /* [GO1SENS_PAIR_CELLS][N] */
  double* pair_lin_err_sum;           /* [GO1SENS_PAIR_CELLS][N] */
  /* go1sens_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][GO1SENS_NUM + 1][GO1SENS_NUM_FIELDS] */
  double* curves;                     /* [num_groups][GO1SENS_NUM][GO1SENS_NUM_QUANT][GO1SENS_BINS] */
  double* counts;                     /* [num_groups][GO1SENS_NUM][GO1SENS_NUM_COUNTS] */
  double* pair_results;               /* [num_groups][GO1SENS_PAIR_QUANT][GO1SENS_PAIR_CELLS] */
} Go1SensBuffers;

/* empty accumulators, bins and maps; the values in force taken from the simulator's buffers.  One launch, one thread per environment. */
int go1sens_clear(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream);

/* the values in force taken again from the simulator's buffers, nothing cleared.  One launch, one thread per environment. */
int go1sens_snapshot(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream);

/* after a simulator step: fold the step of every environment.  One launch, one thread per (row, environment). */
int go1sens_accumulate(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream);

/* at the end: the four result tables from the accumulators and the state (which it leaves as they are).  One launch. */
int go1sens_reduce(const Go1SensConfig* cfg, const Go1SensBuffers* buf, void* stream);

/* "go1sens <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1sens_version(void);

#ifdef __cplusplus
}
#endif

#endif
