/* go1obs.h — C-ABI of libgo1obs.so: the distribution of what the policy is fed, measured on the device (HIP, gfx950): per column of
 * obs_buf (and, when asked, of privileged_obs_buf) the moments and range, a sixteen-bin histogram with two tails, the steps at the
 * observation clip, and the moments of the change from one step to the next.
 *
 * The other families describe what the robot does.  This one describes the sim-to-real interface: obs_buf holds scaled velocities,
 * gravity, commands, joint positions and rates, actions, clock and contact columns, with noise added and clipped at clip_observations.
 * On a reset step obs_buf already holds the respawned robot's observation, so the change from step to step needs the previous value
 * carried on the device, and a reset step folds none.  It is a library of its own, as the sensitivity library is: no other binary, stamp
 * or parity result depends on it.  The accumulators, the folding rule, the fixed-order reductions and the numbering of the return codes
 * are go1eval.h's, restated here (the device helpers are csrc/go1_tables.h's, shared with those libraries and covered by this library's
 * stamp).  This header is the specification: tests/obs_ref.py is written from its text.
 *
 * Channels: C = num_obs + (privileged != 0 ? num_privileged_obs : 0), at most GO1OBS_MAX_CHANNELS.  value(c, e), the value of channel c
 * of environment e after the simulator's step:
 *   c < num_obs   obs_buf[e * num_obs + c]                              (environment-major, as the simulator keeps it)
 *   otherwise     privileged_obs_buf[e * num_privileged_obs + (c - num_obs)]
 * Every buffer of this library is SoA, [k][N] with the environment last.
 *
 * The config carries by value, per channel, lo[c] and scale[c] = 16 / (hi - lo) (computed by the host in fp32: 16.0f / (hi - lo) on
 * fp32 hi and lo), one clip (the simulator's clip_observations) and warmup_steps.
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off).  Only + - *,
 * fabsf, fminf, fmaxf, conversions and comparisons are used.
 *
 * State per (channel, environment): prev [C][N] (float: the channel's value after the previous launch), age [C][N] (uint32: launches
 * since the clear or the last break), hist [C][16][N], below, above, at_clip [C][N] (uint32); per environment: launches, resets
 * (uint32 [N]).  The accumulators ([2 C][N]): row c is the `value` row of channel c, row C + c its `delta` row.
 *
 * go1obs_accumulate: ONE launch of one thread per (channel, environment), C * ceil(N / 256) blocks of 256 threads, block k on channel
 * k / ceil(N / 256).  No atomics, no LDS, no scratch; every thread owns every state word it reads or writes, and no thread reads a word
 * that another thread of the launch writes.  Thread (c, e), with v = value(c, e), in this order:
 *   0. Channel 0's thread: launches[e] += 1.
 *   1. a = age[c][e] + 1; age[c][e] = a.  Steps with a <= warmup_steps enter nothing: prev[c][e] = v, and the thread returns.
 *   2. v is folded into accumulator row c with the folding rule: a non-finite value adds 1 to nonfinite[c][e] and enters nothing else;
 *      a finite one adds 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.
 *   3. A non-finite v has no bin.  Otherwise t = (v - lo[c]) * scale[c] (a subtract, then a multiply):  t < 0: below[c][e] += 1;
 *      0 <= t < 16: hist[c][(int)t][e] += 1;  anything else: above[c][e] += 1.  A value equal to hi is above.
 *   4. If fabsf(v) >= clip: at_clip[c][e] += 1 (an infinity counts, a NaN does not).
 *   5. If reset_buf[e] != 0 (a reset step): channel 0's thread adds 1 to resets[e]; no change is folded: prev belongs to the robot that
 *      fell.  Otherwise, if a - 1 > warmup_steps (the previous launch was measured too): fabsf(v - prev[c][e]) is folded into
 *      accumulator row C + c with the folding rule.  The first measured step folds none.
 *   6. prev[c][e] = v.
 *
 * go1obs_clear: one launch, one thread per (channel, environment): accumulator rows c and C + c as go1eval_clear (count = nonfinite = 0,
 *   sum = sumsq = 0, min = +inf, max = -inf), every counter 0, prev = 0, age = 0; channel 0's thread: launches[e] = resets[e] = 0.
 * go1obs_break: one launch, one thread per (channel, k), k < num_break: e = break_ids ? break_ids[k] : k; an e outside [0, N) is left
 *   alone; age[c][e] = min(age[c][e], warmup_steps) (0 for a negative warmup_steps); channel 0's thread adds 1 to resets[e]; nothing
 *   else.  The next launch of e is then a first measured step: it folds no change.  For a reset from outside the step (reset_idx): the
 *   robot was put elsewhere between two launches.  With break_ids NULL num_break is taken as N.  The ids must be distinct (each word
 *   keeps one writer).
 * go1obs_reduce: ONE launch of GO1OBS_REDUCE_THREADS-thread workgroups, which writes three tables and leaves what it reads as it is:
 *   num_groups * (2 C + 1) workgroups write results[num_groups][2 C + 1][GO1OBS_NUM_FIELDS].
 *     Rows 0 .. 2 C - 1: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's environments
 *     e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments with
 *     count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields (index =
 *     Go1ObsField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with count = 0
 *     the four in the middle are NaN.
 *     Row 2 C (index = Go1ObsGroupField), from channel 0: environments, launches (the sum of launches[e]), measured (the sum of
 *     count[0][e] + nonfinite[0][e]: the env-steps that entered a value row), resets (the sum of resets[e]: measured reset steps and
 *     breaks), then 0, 0; summed in the same order.
 *   num_groups * C further workgroups write hist_results[num_groups][C][GO1OBS_BINS] as doubles: in the workgroup of a (group, channel)
 *     thread t owns bin t % 16 and adds, as doubles, its bin's word of the group's environments e = t / 16, t / 16 + 16, ... in ascending
 *     order; then a fixed tree over the 16 slices (thread t takes thread t + 128, then + 64, + 32, + 16) and threads 0 .. 15 write their
 *     bin: the foot library's profile order.
 *   num_groups * C further workgroups write tails[num_groups][C][GO1OBS_NUM_TAILS] as doubles (index = Go1ObsTail: below, above,
 *     at_clip), summed as the group row is.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator or a state array is missing
 *   -3   an input is missing (go1obs_accumulate only: obs_buf, reset_buf, or privileged_obs_buf with privileged != 0)
 *   -5   no group, no table of the three, or num_groups <= 0 (go1obs_reduce only)
 *   -12  num_obs < 1, num_privileged_obs < 0 with privileged != 0, or C > GO1OBS_MAX_CHANNELS (every entry point: C sizes every launch);
 *        (go1obs_accumulate only) a channel whose scale is not positive and finite or whose lo is not finite, or a clip that is a NaN;
 *        (go1obs_break only) break_ids with num_break < 0 (with num_break = 0 there is nothing to launch: 0)
 *   -20  the launch itself failed
 *
 * What the figures are not.  The observation of a reset step is the respawned robot's, and it is measured.  The policy sees the history
 * of observations, of which this is the newest row.  A value outside [lo, hi) counts in a tail, not in a bin; the `value` row's min and
 * max show how far out.  `delta` includes the injected noise: two draws of it per difference.  Channels are measured one by one: nothing
 * here says how two of them move together.
 */
#ifndef GO1OBS_H
#define GO1OBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1OBS_MAX_CHANNELS 160       /* GO1_MAX_OBS + GO1_MAX_PRIV_OBS of go1sim.h */
#define GO1OBS_BINS 16
#define GO1OBS_NUM_TAILS 3
#define GO1OBS_NUM_FIELDS 6
#define GO1OBS_REDUCE_THREADS 256

/* columns of a `value` or `delta` row */
enum Go1ObsField { GO1OBS_F_COUNT = 0, GO1OBS_F_MEAN = 1, GO1OBS_F_STD = 2, GO1OBS_F_MIN = 3, GO1OBS_F_MAX = 4, GO1OBS_F_NONFINITE = 5 };
/* columns of a group's own row (row 2 C) */
enum Go1ObsGroupField { GO1OBS_G_ENVS = 0, GO1OBS_G_LAUNCHES = 1, GO1OBS_G_MEASURED = 2, GO1OBS_G_RESETS = 3 };
/* the three counts per (group, channel) beside the bins */
enum Go1ObsTail { GO1OBS_T_BELOW = 0, GO1OBS_T_ABOVE = 1, GO1OBS_T_AT_CLIP = 2 };

typedef struct Go1ObsConfig {
  int32_t num_envs;                  /* N */
  int32_t warmup_steps;              /* launches with age <= warmup_steps enter nothing */
  int32_t num_groups;                /* G of the result tables */
  int32_t num_obs;                   /* columns of obs_buf */
  int32_t num_privileged_obs;        /* columns of privileged_obs_buf */
  int32_t privileged;                /* != 0: the privileged columns are channels too */
  int32_t num_break;                 /* go1obs_break: the environments named by break_ids */
  float clip;                        /* the simulator's clip_observations */
  float lo[GO1OBS_MAX_CHANNELS];     /* the lower edge of bin 0 */
  float scale[GO1OBS_MAX_CHANNELS];  /* 16 / (hi - lo) */
} Go1ObsConfig;

typedef struct Go1ObsBuffers {
  /* read by go1obs_accumulate */
  const float* obs_buf;               /* [N][num_obs] */
  const float* privileged_obs_buf;    /* [N][num_privileged_obs] */
  const uint8_t* reset_buf;           /* [N] */
  /* accumulators, [2 C][N]: the `value` rows, then the `delta` rows */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  float* prev;                        /* [C][N]: the value after the previous launch */
  uint32_t* age;                      /* [C][N]: launches since the clear or the last break */
  uint32_t* hist;                     /* [C][GO1OBS_BINS][N] */
  uint32_t* below;                    /* [C][N]: finite values under lo */
  uint32_t* above;                    /* [C][N]: finite values at or over hi */
  uint32_t* at_clip;                  /* [C][N]: values with fabsf(v) >= clip */
  uint32_t* launches;                 /* [N]: accumulate launches since the clear */
  uint32_t* resets;                   /* [N]: measured reset steps, and breaks */
  /* go1obs_break */
  const int64_t* break_ids;           /* [num_break] distinct environments, or NULL: all */
  /* go1obs_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][2 C + 1][GO1OBS_NUM_FIELDS] */
  double* hist_results;               /* [num_groups][C][GO1OBS_BINS] */
  double* tails;                      /* [num_groups][C][GO1OBS_NUM_TAILS] */
} Go1ObsBuffers;

/* empty accumulators, bins, tails and state.  One launch, one thread per (channel, environment). */
int go1obs_clear(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream);

/* the next launch of the named environments folds no change; nothing is cleared.  One launch, one thread per (channel, id). */
int go1obs_break(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream);

/* after a simulator step: fold the observation of every environment.  One launch, one thread per (channel, environment). */
int go1obs_accumulate(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream);

/* at the end: the three result tables from the accumulators and the state (which it leaves as they are).  One launch. */
int go1obs_reduce(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream);

/* "go1obs <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1obs_version(void);

#ifdef __cplusplus
}
#endif

#endif
