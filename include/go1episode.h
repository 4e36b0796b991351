/* go1episode.h — C-ABI of libgo1episode.so: whole episodes of a policy rollout, measured on the device (HIP, gfx950): returns, lengths,
 * the distance covered, the tracking error over an episode, and the histograms a survival curve is made of.
 *
 * The other families reduce a rollout per step or per stride.  This one reduces it per EPISODE: what return the policy collects, how long
 * it stays up, how far it gets, and, because an evaluation window is usually shorter than an episode, how many episodes are still open at
 * its end and how old they are (the right-censored observations of a Kaplan-Meier estimate, taken on the host).  Per-step families cannot
 * reconstruct this afterwards: on the step of a reset the simulator's buffers already hold the respawned robot, and the reset clears
 * episode_sums inside the step kernel; only rew_buf, reset_buf and time_out_buf of that step still belong to the old episode.  So the
 * state of the open episode is carried here from step to step.  It is a library of its own, as the gait library is: no other binary,
 * stamp or parity result depends on it.  The accumulators, the folding rule, the fixed-order reductions and the numbering of the return
 * codes are go1eval.h's, restated here (the device helpers are csrc/go1_tables.h's, shared with those libraries and covered by this
 * library's stamp).  This header is the specification: tests/episode_ref.py is written from its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).
 *
 * Per environment e, the inputs of a step (read after the simulator's step):
 *   r        rew_buf: the step's reward; on a reset step the terminal reward of the episode that ended
 *   reset_buf, time_out_buf, episode_length_buf (elb below)
 *   x, y     rows 0 and 1 of root_states [13][N]: the base position (world); on a reset step the respawn pose
 *   vx, vy   rows 0 and 1 of base_lin_vel [3][N];  wz  row 2 of base_ang_vel [3][N]
 *   cx, cy, cz   rows 0, 1 and 2 of commands: the commanded forward, lateral and yaw velocity
 *   total    row return_row (the simulator's num_rewards: the "total" row) of episode_sums: on a step without a reset the sum of the
 *            open episode's rewards, this step's included (the step kernel adds r to it in fp32, one addition per step)
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off).  Only + - * /,
 * sqrtf, fabsf, conversions from integers and comparisons are used.
 *
 * Eleven rows (index = Go1EpisodeMetric, accumulator row = metric):
 *   step_reward         every launch                              r
 *   length              at an episode's close                     (float) L, L the episode's steps
 *   fell                at a close                                time_out_buf != 0 ? 0 : 1
 *   length_fell         at a close without time_out_buf           (float) L
 *   return              at a close                                ret
 *   reward_rate         at a close                                ret / (float) L
 *   lin_vel_err         at a close, if track_steps > 0            lin_err / (float) track_steps
 *   yaw_vel_err         at a close, if track_steps > 0            yaw_err / (float) track_steps
 *   discounted_return   at the close of a whole episode           disc_ret
 *   displacement        at the close of a whole episode           sqrtf(dx * dx + dy * dy), dx = prev_x - first_x, dy = prev_y - first_y
 *   path_length         at the close of a whole episode           path
 * The folding rule is go1eval_accumulate's: a non-finite value adds 1 to nonfinite[row][e] and enters nothing else; a finite value v adds
 * 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.
 *
 * State per environment: age (int32: the steps of the open episode seen so far, -1: unknown, as after a clear); whole (uint8: the open
 * episode was seen from its first step); ret, disc_ret, disc_w (float: the running return, the running discounted return and the weight
 * of the next reward); first_pos [2] and prev_pos [2] (float: x, y where the episode was first seen and on the previous step); path
 * (float); lin_err, yaw_err (float: the sums of the two tracking errors) and track_steps (int32: their terms); steps, closed, fell,
 * timed_out, cut, unseen (uint32); fall_hist [16] and timeout_hist [16] (uint32: closed episodes per length bin).
 *
 * go1episode_accumulate: one thread per environment, ceil(N / 256) blocks of 256 threads; no atomics, no LDS, every word has one writer,
 * and every load and store of a row is one contiguous run over a wavefront (the histogram words alone are scattered: their bin differs
 * from lane to lane).  The rows of an episode's close are touched only on the steps that close one.  Per e, in this order:
 *   1. steps[e] += 1, and step_reward = r is folded.
 *   2. If reset_buf[e] != 0 (a reset step):
 *      (a) if age >= 0, an episode of L = age + 1 steps closes (the reset step is its last).  Its reward is the terminal reward:
 *            ret = ret + r;  disc_ret = disc_ret + disc_w * r.  Nothing else of this step belongs to the old episode.
 *          With timed = time_out_buf[e] != 0, folded in this order: length, fell, length_fell (if !timed), return, reward_rate;
 *          if track_steps > 0: lin_vel_err, yaw_vel_err;  if whole: discounted_return, displacement, path_length.
 *          bin = min((L - 1) / bin_steps, 15) (integer division);  timeout_hist[bin][e] += 1 if timed, else fall_hist[bin][e] += 1.
 *          closed += 1, and timed_out += 1 if timed, else fell += 1.
 *      (b) otherwise (the age is unknown) unseen += 1: an episode ended of which nothing was seen.
 *      (c) in both cases a whole episode opens at the respawn pose: age = 0, whole = 1, ret = 0, disc_ret = 0, disc_w = 1,
 *          first_pos = prev_pos = (x, y), path = 0, lin_err = yaw_err = 0, track_steps = 0.  Nothing else happens on this step.
 *   3. Otherwise, consistency: if age >= 0 and elb != age + 1, the episode was cut from outside (reset_idx, place_on_terrain, a manual
 *      reset(): none of them sets reset_buf).  cut += 1, what was carried is dropped without being folded, and the step is a first sight.
 *   4. A first sight (age < 0, or a cut): age = elb, whole = (elb == 1), ret = total (it holds this step's reward already, so the return
 *      of an episode begun before arming is still exact), disc_ret = r and disc_w = gamma (discounting starts here; only a whole episode
 *      folds it), first_pos = prev_pos = (x, y), path = 0, lin_err = yaw_err = 0, track_steps = 0.
 *   5. Otherwise a step inside the episode: age = elb;  ret = ret + r;  disc_ret = disc_ret + disc_w * r, then disc_w = disc_w * gamma;
 *      dx = x - prev_x, dy = y - prev_y, path = path + sqrtf(dx * dx + dy * dy);  prev_pos = (x, y).
 *   6. After 4 or 5, if elb > warmup_steps: ex = vx - cx, ey = vy - cy, lin_err = lin_err + sqrtf(ex * ex + ey * ey);
 *      yaw_err = yaw_err + fabsf(wz - cz);  track_steps += 1.
 *
 * go1episode_clear: one launch of the same shape: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0, min = +inf,
 *   max = -inf), both histograms and the six counters 0, age = -1, whole = 0, ret = disc_ret = 0, disc_w = 1, first_pos = prev_pos = 0,
 *   path = lin_err = yaw_err = 0, track_steps = 0.
 * go1episode_reduce: ONE launch of GO1EPISODE_REDUCE_THREADS-thread workgroups, which writes two tables and leaves what it reads as it is:
 *   num_groups * (GO1EPISODE_NUM + 2) workgroups write results[num_groups][GO1EPISODE_NUM + 2][GO1EPISODE_NUM_FIELDS].
 *     Rows 0 .. GO1EPISODE_NUM - 1: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's
 *     environments e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments
 *     with count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields
 *     (index = Go1EpisodeField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with
 *     count = 0 the four in the middle are NaN.
 *     Row GO1EPISODE_NUM (index = Go1EpisodeGroupField): environments, steps (sum of steps[e]), closed, fell, timed_out, open (the
 *     environments with age >= 0), in the same order.
 *     Row GO1EPISODE_NUM + 1 (index = Go1EpisodeGroupField2): cut, unseen, open_steps (the sum of the ages that are >= 0), then 0, 0, 0.
 *   num_groups * GO1EPISODE_NUM_HISTS further workgroups write hist_results[num_groups][GO1EPISODE_NUM_HISTS][GO1EPISODE_BINS] as doubles:
 *     histogram 0 is fall_hist, histogram 1 timeout_hist, histogram 2 comes from the state: an environment with age >= 0 counts 1 in bin
 *     min(age / bin_steps, 15): an open episode of age a has at least a + 1 steps, so it is censored in the bin an episode of a + 1 steps
 *     closes in.  In the workgroup of a (group, histogram) thread t owns bin t % 16 and adds, as doubles, its bin's word (or its 0 or 1)
 *     of the group's environments e = t / 16, t / 16 + 16, ... in ascending order; then a fixed tree over the 16 slices (thread t takes
 *     thread t + 128, then + 64, + 32, + 16) and threads 0 .. 15 write their bin: the foot library's profile order.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator, a histogram or a state array is missing
 *   -3   an input is missing (go1episode_accumulate only: go1episode_clear and go1episode_reduce read none)
 *   -5   no group, no table, no histogram table, or num_groups <= 0 (go1episode_reduce only)
 *   -12  gamma not finite or not in (0, 1], bin_steps < 1 or return_row < 0 (go1episode_accumulate; go1episode_reduce tests bin_steps alone)
 *   -20  the launch itself failed
 *
 * What the figures are not.  The terminal step contributes only its reward: its pose, velocities and commands are the next episode's.
 * An episode first seen at elb == 1 is whole, but its distances start from the pose AFTER that step, not from the spawn pose (an episode
 * opened by a reset step seen here starts from the respawn pose itself).  An episode begun before the clear has an exact length and
 * return, enters the histograms as if it had been observed from its start, and folds no discounted return and no distance.  A reset
 * from outside within one step of a reset step (elb == age + 1 all the same) is not seen as a cut.  There are sixteen bins, the last one
 * open-ended.  The only cause of an end this library knows is time_out_buf or not.
 */
#ifndef GO1EPISODE_H
#define GO1EPISODE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1EPISODE_NUM 11
#define GO1EPISODE_BINS 16
#define GO1EPISODE_NUM_HISTS 3
#define GO1EPISODE_NUM_FIELDS 6
#define GO1EPISODE_REDUCE_THREADS 256

enum Go1EpisodeMetric {
  GO1EPISODE_STEP_REWARD = 0, GO1EPISODE_LENGTH = 1, GO1EPISODE_FELL = 2, GO1EPISODE_LENGTH_FELL = 3, GO1EPISODE_RETURN = 4,
  GO1EPISODE_REWARD_RATE = 5, GO1EPISODE_LIN_VEL_ERR = 6, GO1EPISODE_YAW_VEL_ERR = 7, GO1EPISODE_DISCOUNTED_RETURN = 8,
  GO1EPISODE_DISPLACEMENT = 9, GO1EPISODE_PATH_LENGTH = 10
};
/* columns of a metric row */
enum Go1EpisodeField { GO1EPISODE_F_COUNT = 0, GO1EPISODE_F_MEAN = 1, GO1EPISODE_F_STD = 2, GO1EPISODE_F_MIN = 3, GO1EPISODE_F_MAX = 4, GO1EPISODE_F_NONFINITE = 5 };
/* columns of a group's first own row (row GO1EPISODE_NUM) */
enum Go1EpisodeGroupField { GO1EPISODE_G_ENVS = 0, GO1EPISODE_G_STEPS = 1, GO1EPISODE_G_CLOSED = 2, GO1EPISODE_G_FELL = 3, GO1EPISODE_G_TIMED_OUT = 4, GO1EPISODE_G_OPEN = 5 };
/* columns of a group's second own row (row GO1EPISODE_NUM + 1) */
enum Go1EpisodeGroupField2 { GO1EPISODE_H_CUT = 0, GO1EPISODE_H_UNSEEN = 1, GO1EPISODE_H_OPEN_STEPS = 2 };

typedef struct Go1EpisodeConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps enter no tracking error */
  int32_t num_groups;          /* G of the result tables */
  int32_t return_row;          /* the row of episode_sums that holds the episode's total: the simulator's num_rewards */
  float gamma;                 /* the discount of discounted_return, in (0, 1] */
  int32_t bin_steps;           /* the width of a length bin in steps; the sixteenth bin is open-ended */
} Go1EpisodeConfig;

typedef struct Go1EpisodeBuffers {
  /* read by go1episode_accumulate */
  const float* rew_buf;               /* [N] */
  const uint8_t* reset_buf;           /* [N] */
  const uint8_t* time_out_buf;        /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  const float* root_states;           /* [13][N] */
  const float* base_lin_vel;          /* [3][N] */
  const float* base_ang_vel;          /* [3][N] */
  const float* commands;              /* [num_commands][N] */
  const float* episode_sums;          /* [return_row + 1][N] */
  /* accumulators, [GO1EPISODE_NUM][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  int32_t* age;                       /* [N]: steps of the open episode seen so far; -1: unknown */
  uint8_t* whole;                     /* [N]: the open episode was seen from its first step */
  float* ret;                         /* [N]: the running return */
  float* disc_ret;                    /* [N]: the running discounted return */
  float* disc_w;                      /* [N]: the weight of the next reward */
  float* first_pos;                   /* [2][N]: x, y where the episode was first seen */
  float* prev_pos;                    /* [2][N]: x, y on the previous step */
  float* path;                        /* [N]: the length of the path so far */
  float* lin_err;                     /* [N]: the sum of the linear-velocity errors */
  float* yaw_err;                     /* [N]: the sum of the yaw-rate errors */
  int32_t* track_steps;               /* [N]: the terms of the two sums */
  uint32_t* steps;                    /* [N]: accumulate launches since the clear */
  uint32_t* closed;                   /* [N]: episodes closed */
  uint32_t* fell;                     /* [N]: of those, without time_out_buf */
  uint32_t* timed_out;                /* [N]: of those, with time_out_buf */
  uint32_t* cut;                      /* [N]: episodes cut from outside and dropped */
  uint32_t* unseen;                   /* [N]: reset steps that ended an episode of unknown age */
  uint32_t* fall_hist;                /* [GO1EPISODE_BINS][N]: episodes that fell per length bin */
  uint32_t* timeout_hist;             /* [GO1EPISODE_BINS][N]: episodes that timed out per length bin */
  /* go1episode_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][GO1EPISODE_NUM + 2][GO1EPISODE_NUM_FIELDS] */
  double* hist_results;               /* [num_groups][GO1EPISODE_NUM_HISTS][GO1EPISODE_BINS] */
} Go1EpisodeBuffers;

/* empty accumulators and histograms, every environment's episode unknown.  One launch, one thread per environment. */
int go1episode_clear(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf, void* stream);

/* after a simulator step: fold the step of every environment.  One launch, one thread per environment. */
int go1episode_accumulate(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf, void* stream);

/* at the end: the two result tables from the accumulators, the histograms and the state (which it leaves as they are).  One launch. */
int go1episode_reduce(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf, void* stream);

/* "go1episode <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1episode_version(void);

#ifdef __cplusplus
}
#endif

#endif
