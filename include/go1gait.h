/* go1gait.h — C-ABI of libgo1gait.so: inter-leg coordination and the realised gait of a policy rollout, measured on the device
 * (HIP, gfx950).
 *
 * The behaviour table (go1eval.h) says how often each foot's contact agrees with its own commanded schedule, the foot library
 * (go1feet.h) what each foot puts into the ground over its own phase, and the trunk library (go1trunk.h) counts the supporting feet.
 * None of them relates one foot to another: which legs move together, at which phase of one leg's stride the others touch down, and how
 * the time divides among flight, a diagonal pair, a lateral pair, three and four feet.  These are the quantities of gait analysis, and
 * they tell a trot that is a little late from a pace.  This library is that family.  It is a library of its own, as the evaluation,
 * foot and trunk libraries are: no other binary, stamp or parity result depends on it.  The accumulators, the folding rule, the
 * fixed-order reduction and the numbering of the return codes are go1eval.h's, restated here (the device helpers are csrc/go1_tables.h's,
 * shared with those libraries and covered by this library's stamp).  This header is the specification: tests/gait_ref.py is written from
 * its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).  Foot f (0 FL, 1 FR, 2 RL, 3 RR) is
 * body 4 (f + 1) of contact_forces [17 * 3][N]; its vertical force is row 12 (f + 1) + 2.
 *
 * Per environment e, the inputs of a step (read after the simulator's step):
 *   fz_f     row 12 (f + 1) + 2 of contact_forces, foot f (N, world; the net force of the LAST SUBSTEP)
 *   fi_f     row f of foot_indices [4][N]: the gait clock of foot f in cycles, in [0, 1)
 *   reset_buf, episode_length_buf
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off).  Only + - /,
 * *, floorf, fabsf, conversions from integers and comparisons are used: no trigonometric function runs on the device; circular means are
 * taken on the host from the phase histograms.
 *
 * FL (foot 0) is the reference foot: a reference stride runs from one touchdown of FL to the next, and the other three feet's
 * touchdowns are placed within it.
 *
 * Fifteen rows (index = Go1GaitMetric, accumulator row = metric):
 *   sync_FL_FR, sync_FL_RL, sync_FL_RR, sync_FR_RL, sync_FR_RR, sync_RL_RR
 *                          every folded step         c_i == c_j ? 1 : 0 for the pair (i, j): the share of steps on which the two feet are
 *                                                    both on the ground or both in the air
 *   phase_err_FR, _RL, _RR        at a stride's close, if the foot touched down in it    err (below): realised minus commanded
 *                                                    touchdown phase, wrapped to [-0.5, 0.5)
 *   phase_abs_err_FR, _RL, _RR    with phase_err     fabsf(err)
 *   touchdowns_FR, _RL, _RR       at a stride's close    (float) td_count[f]: the foot's touchdowns within the stride
 * The folding rule is go1eval_accumulate's: a non-finite value adds 1 to nonfinite[row][e] and enters nothing else; a finite value v adds
 * 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.
 *
 * State per environment: prev_contact [4] (uint8: 0 in the air, 1 on the ground, 2 unknown); ref_steps (int32: the steps since the
 * reference stride opened, -1 while none is open); last_td [3] and td_count [3] (int32, index f - 1 for f = 1 .. 3: the step within the
 * stride of the foot's latest touchdown, -1 for none, and the number of its touchdowns in the stride); steps, resets, strides and
 * strides_dropped (uint32); support_hist [16] (uint32: steps per support pattern) and phase_hist [3][16] (uint32: closed strides per
 * touchdown-phase bin of foot f = 1 .. 3).
 *
 * go1gait_accumulate: one thread per environment, ceil(N / 256) blocks of 256 threads; no atomics, no LDS, every word has one writer,
 * and every load and store of a row is one contiguous run over a wavefront (the histogram words alone are scattered: their bin differs
 * from lane to lane).  The rows of a stride's close are touched only on the steps that close one.  Per e, in this order:
 *   1. steps[e] += 1, and resets[e] += 1 if reset_buf[e] != 0.
 *   2. If reset_buf[e] != 0 or episode_length_buf[e] <= warmup_steps: prev_contact[0 .. 3] = 2 and ref_steps = -1.  Nothing is folded and
 *      nothing else happens on this step.  An open stride ended this way is forgotten, not counted as dropped (last_td and td_count keep
 *      what they hold: nothing reads them before a stride opens and writes them again).
 *   3. Contact and support pattern: c_f = fz_f > GO1GAIT_CONTACT_FORCE, the foot family's rule (a NaN compares false: in the air).
 *      mask = sum over f of c_f << f.  The six sync rows are folded in the order of the enum.  support_hist[mask][e] += 1.
 *   4. td_f = c_f && prev_contact[f] == 0: a touchdown is a step on the ground after a step seen in the air.
 *   5. If ref_steps >= 0: ref_steps += 1; if now ref_steps > max_stride_steps, the stride is dropped: ref_steps = -1 and
 *      strides_dropped += 1.
 *   6. If td_0:
 *      (a) if ref_steps >= min_stride_steps, a reference stride of L = ref_steps steps closes.  For f = 1, 2, 3 in this order:
 *            touchdowns_f = (float) td_count[f] is folded;
 *            if td_count[f] >= 1:
 *              p = (float) last_td[f] / (float) L                  the realised touchdown phase, in [0, 1)
 *              d = fi_0 - fi_f, cmd = d - floorf(d)                the commanded one (see below)
 *              err = p - cmd, then err = err - floorf(err + 0.5f)  wrapped to [-0.5, 0.5)
 *              phase_err_f = err and phase_abs_err_f = fabsf(err) are folded (a non-finite foot index gives a NaN: counted in nonfinite)
 *              b = floorf(p * 16.0f + 0.5f); a b that is not in [1, 15] (so 16, which is phase 1 = phase 0) becomes 0, AS A FLOAT and
 *              only then converted to an integer: the bins are centred on k / 16, bin 0 covers [31/32, 1) and [0, 1/32)
 *              phase_hist[f - 1][b][e] += 1 (whether err is finite or not: p always is)
 *          then strides += 1 and the stride is opened again as in (c).
 *      (b) otherwise, if ref_steps >= 0: a touchdown of FL within min_stride_steps of the stride's opening is chatter.  It is ignored as a
 *          reference event: the stride goes on.
 *      (c) otherwise a stride opens: ref_steps = 0, td_count[1 .. 3] = 0, last_td[1 .. 3] = -1.
 *   7. For f = 1, 2, 3: if td_f and ref_steps >= 0: last_td[f] = ref_steps and td_count[f] += 1.  This runs after 6, so a touchdown on
 *      the step that opens a stride belongs to the new stride, at phase 0.
 *   8. prev_contact[f] = c_f for the four feet.
 *
 * The sign of the commanded phase.  The simulator advances every foot's clock at one frequency, foot_indices[f] = (gait_index + offset_f)
 * mod 1, and a foot touches down where its clock wraps to 0.  A foot whose clock is AHEAD of FL's by a wraps, and touches down, a cycles
 * EARLIER: seen from FL's touchdown at phase 0, at phase 1 - a.  So the commanded touchdown phase of foot f within FL's stride is
 * frac(fi_FL - fi_f): FL minus f, not f minus FL.  The clocks are read, not commands[5:8]: pacing_offset and the like are in them already.
 * They are read on the closing step, so a command changed within a stride is judged by what it is at the stride's end.
 *
 * go1gait_clear: one launch of the same shape: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0, min = +inf,
 *   max = -inf), both histograms and the four counters 0, prev_contact = 2, ref_steps = -1, last_td = -1, td_count = 0.
 * go1gait_reduce: ONE launch of GO1GAIT_REDUCE_THREADS-thread workgroups, which writes two tables and leaves what it reads as it is:
 *   num_groups * (GO1GAIT_NUM + 1) workgroups write results[num_groups][GO1GAIT_NUM + 1][GO1GAIT_NUM_FIELDS].
 *     Rows 0 .. GO1GAIT_NUM - 1: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's environments
 *     e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments with
 *     count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields
 *     (index = Go1GaitField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with
 *     count = 0 the four in the middle are NaN.
 *     The last row of a group (index = Go1GaitGroupField): environments, steps (sum of steps[e]), resets, strides, strides_dropped, then
 *     0, in the same order.
 *   num_groups * GO1GAIT_NUM_HISTS further workgroups write hist_results[num_groups][GO1GAIT_NUM_HISTS][GO1GAIT_BINS] as doubles:
 *     histogram 0 is the support pattern (bin = mask), histograms 1 .. 3 the touchdown phases of FR, RL, RR.  In the workgroup of a
 *     (group, histogram) thread t owns bin t % 16 and adds, as doubles, the histogram's word [t % 16][e] of the group's environments
 *     e = t / 16, t / 16 + 16, ... in ascending order; then a fixed tree over the 16 slices (thread t takes thread t + 128, then + 64,
 *     + 32, + 16) and threads 0 .. 15 write their bin: the foot library's profile order.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator, a histogram or a state array is missing
 *   -3   an input is missing (go1gait_accumulate only: go1gait_clear and go1gait_reduce read none)
 *   -5   no group, no table, no histogram table, or num_groups <= 0 (go1gait_reduce only)
 *   -12  min_stride_steps < 1 or max_stride_steps < min_stride_steps (go1gait_accumulate only)
 *   -20  the launch itself failed
 *
 * What the figures are not.  Contact is fz > 1 N of the last substep, not a debounced contact sensor: with min_stride_steps = 1 (the
 * default, as everywhere else) a foot that bounces closes a stride at every bounce.  FL is the reference: a robot whose FL never lifts
 * yields no stride and no phase, only the synchronies and the support pattern.  The phase resolution is one policy step in L.  A stride
 * longer than max_stride_steps is dropped whole.
 */
#ifndef GO1GAIT_H
#define GO1GAIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1GAIT_NUM 15
#define GO1GAIT_BINS 16
#define GO1GAIT_NUM_HISTS 4
#define GO1GAIT_NUM_FIELDS 6
#define GO1GAIT_REDUCE_THREADS 256
#define GO1GAIT_CONTACT_FORCE 1.0

enum Go1GaitMetric {
  GO1GAIT_SYNC_FL_FR = 0, GO1GAIT_SYNC_FL_RL = 1, GO1GAIT_SYNC_FL_RR = 2, GO1GAIT_SYNC_FR_RL = 3, GO1GAIT_SYNC_FR_RR = 4, GO1GAIT_SYNC_RL_RR = 5,
  GO1GAIT_PHASE_ERR_FR = 6, GO1GAIT_PHASE_ERR_RL = 7, GO1GAIT_PHASE_ERR_RR = 8,
  GO1GAIT_PHASE_ABS_ERR_FR = 9, GO1GAIT_PHASE_ABS_ERR_RL = 10, GO1GAIT_PHASE_ABS_ERR_RR = 11,
  GO1GAIT_TOUCHDOWNS_FR = 12, GO1GAIT_TOUCHDOWNS_RL = 13, GO1GAIT_TOUCHDOWNS_RR = 14
};
/* columns of a metric row */
enum Go1GaitField { GO1GAIT_F_COUNT = 0, GO1GAIT_F_MEAN = 1, GO1GAIT_F_STD = 2, GO1GAIT_F_MIN = 3, GO1GAIT_F_MAX = 4, GO1GAIT_F_NONFINITE = 5 };
/* columns of a group's own row (row GO1GAIT_NUM) */
enum Go1GaitGroupField { GO1GAIT_G_ENVS = 0, GO1GAIT_G_STEPS = 1, GO1GAIT_G_RESETS = 2, GO1GAIT_G_STRIDES = 3, GO1GAIT_G_STRIDES_DROPPED = 4 };

typedef struct Go1GaitConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing */
  int32_t num_groups;          /* G of the result tables */
  int32_t min_stride_steps;    /* a touchdown of FL sooner after the stride's opening is chatter; 1: no debounce */
  int32_t max_stride_steps;    /* a stride that grows beyond it is dropped; 100 is 2 s at a 0.02 s policy step */
} Go1GaitConfig;

typedef struct Go1GaitBuffers {
  /* read by go1gait_accumulate */
  const float* contact_forces;        /* [17 * 3][N] */
  const float* foot_indices;          /* [4][N] */
  const uint8_t* reset_buf;           /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* accumulators, [GO1GAIT_NUM][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  uint8_t* prev_contact;              /* [4][N]: 0 in the air, 1 on the ground, 2 unknown */
  int32_t* ref_steps;                 /* [N]: steps since the reference stride opened; -1: none open */
  int32_t* last_td;                   /* [3][N]: FR, RL, RR: the step within the stride of the latest touchdown; -1: none */
  int32_t* td_count;                  /* [3][N]: FR, RL, RR: touchdowns within the stride */
  uint32_t* steps;                    /* [N]: accumulate launches since the clear */
  uint32_t* resets;                   /* [N]: of those, the steps that reset the environment */
  uint32_t* strides;                  /* [N]: reference strides closed */
  uint32_t* strides_dropped;          /* [N]: reference strides that outgrew max_stride_steps */
  uint32_t* support_hist;             /* [GO1GAIT_BINS][N]: steps per support pattern (bin = mask) */
  uint32_t* phase_hist;               /* [3][GO1GAIT_BINS][N]: FR, RL, RR: closed strides per touchdown-phase bin */
  /* go1gait_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][GO1GAIT_NUM + 1][GO1GAIT_NUM_FIELDS] */
  double* hist_results;               /* [num_groups][GO1GAIT_NUM_HISTS][GO1GAIT_BINS] */
} Go1GaitBuffers;

/* empty accumulators and histograms, every foot's contact unknown, no open stride.  One launch, one thread per environment. */
int go1gait_clear(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf, void* stream);

/* after a simulator step: fold the step of every environment.  One launch, one thread per environment. */
int go1gait_accumulate(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf, void* stream);

/* at the end: the two result tables from the accumulators, the histograms and the state (which it leaves as they are).  One launch. */
int go1gait_reduce(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf, void* stream);

/* "go1gait <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1gait_version(void);

#ifdef __cplusplus
}
#endif

#endif
