/* go1feet.h — C-ABI of libgo1feet.so: per-foot ground reaction forces of a policy rollout, measured on the device (HIP, gfx950).
 *
 * The evaluation library (go1eval.h) measures the robot as a whole, its gait timing and its joints.  None of its tables looks at what
 * the feet put into the ground: how hard a foot lands, the peak vertical load of a stance, how much of the available friction the gait
 * uses, how far a loaded foot slides, how the load is shared between the feet, and the ground-reaction-force (GRF) curve over the
 * commanded gait cycle.  This library is that family.  It is a library of its own, as the renderer and the evaluation library are: no
 * other binary, stamp or parity result depends on it, and libgo1eval's surface stays as it is.  The accumulators, the folding rule, the
 * fixed-order reduction and the numbering of the return codes are go1eval.h's, restated here (csrc/go1feet.hip restates the few device
 * helpers as well; the two libraries share no header).  This header is the specification: tests/feet_ref.py is written from its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).  Foot f (0 FL, 1 FR, 2 RL, 3 RR) is
 * body 4 (f + 1) of contact_forces [17 * 3][N]: its rows are 12 (f + 1), 12 (f + 1) + 1, 12 (f + 1) + 2.
 *
 * Per foot f and environment e, the inputs of a step (read after the simulator's step):
 *   fx, fy, fz   the foot body's three rows of contact_forces (N, world frame; the net force of the LAST SUBSTEP)
 *   vx, vy       rows 3 f, 3 f + 1 of foot_velocities (m/s, world frame)
 *   pvz          row 3 f + 2 of prev_foot_velocities: the foot's vertical velocity at the start of the step, the operand of the
 *                reference's impact term
 *   ph           foot_indices[f][e]: the foot's place in the commanded gait cycle, [0, 1)
 *   mu           0.5f * (friction_coeffs[e] + terrain_friction): the solver's static coefficient of the contact
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off: a rounding
 * after every multiply, add, division and square root):
 *   c  = fz > GO1FEET_CONTACT_FORCE      the foot is on the ground: the behaviour table's contact (go1eval.h), so duty factors are
 *                                        comparable.  A NaN compares false: in the air.
 *   fn = sqrtf((fx * fx + fy * fy) + fz * fz)
 *   ft = sqrtf(fx * fx + fy * fy)
 *   s  = sqrtf(vx * vx + vy * vy)
 *
 * Twelve rows per foot (index = Go1FeetMetric), accumulator row f * GO1FEET_NUM + metric:
 *   contact            every folded step   c ? 1 : 0.  Its mean is the foot's realised duty factor.
 *   force_normal       when c              fz
 *   force_tangent      when c              ft
 *   friction_use       when c              ft / (mu * fz) (one multiply, one division).  1 is the edge of the static cone.  A non-finite
 *                                          value (mu = 0) is counted in nonfinite, as everywhere.
 *   force_excess       every folded step   d > 0 ? d : +0 with d = fn - max_contact_force; a NaN d is handed on (and counted in
 *                                          nonfinite), as the reference's clip hands it on.  Summed over the feet it is the reference's
 *                                          _reward_feet_contact_forces.
 *   impact_vel_sq      every folded step   fn > 1.0f ? m * m : +0 with m = pvz < -100 ? -100 : (pvz > 0 ? +0 : pvz) (a NaN pvz stays a
 *                                          NaN).  Summed over the feet it is the reference's _reward_feet_impact_vel.
 *   touchdown_speed    at a touchdown      pvz < 0 ? -pvz : +0: how fast the foot was coming down (a NaN pvz gives 0)
 *   touchdown_force    at a touchdown      fz
 *   stance_peak_force  at a lift-off       the largest fz of the stance (fmaxf over its steps)
 *   stance_impulse     at a lift-off       the sum of fz * dt over the stance's steps, accumulated in fp32 in step order (each product
 *                                          rounded, then added)
 *   stance_slip        at a lift-off       the sum of s * dt over the stance's steps, likewise: metres slid while loaded
 *   stance_time        at a lift-off       (float)stance_steps * dt
 * The folding rule is go1eval_accumulate's: a non-finite value adds 1 to nonfinite[row][e] and enters nothing else; a finite value v adds
 * 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.
 *
 * State per (foot, environment): prev_contact (uint8: 0 in the air, 1 on the ground, 2 unknown), stance_valid (uint8: the stance now under
 * way was seen from its touchdown), stance_steps (int32), stance_peak, stance_impulse, stance_slip (fp32).  State per environment:
 * steps and resets, written by the thread of foot 0.
 *   A TOUCHDOWN is c with prev_contact == 0.  It folds touchdown_speed and touchdown_force and opens a valid stance with this step's
 *     values: stance_valid = 1, stance_steps = 1, stance_peak = fz, stance_impulse = fz * dt, stance_slip = s * dt.
 *   A further stance step is c with prev_contact == 1 and stance_valid: stance_steps += 1, stance_peak = fmaxf(stance_peak, fz),
 *     stance_impulse += fz * dt, stance_slip += s * dt.
 *   A LIFT-OFF is !c with prev_contact == 1 and stance_valid.  It folds the four stance rows from the state and closes the stance.
 *   Every step with !c leaves stance_valid = 0.  A stance that began unobserved (c with prev_contact == 2) is never valid, so it is
 *     never folded: whatever makes prev_contact 2 (the clear, a reset step, a warm-up step) has set stance_valid = 0, and only a
 *     touchdown sets it again.
 *   Then prev_contact = c ? 1 : 0.  There is no debounce: one step in the air ends a stance.
 *
 * The GRF profile has GO1FEET_PHASE_BINS bins over the gait phase.  On every folded step on which ph and fz are both finite the bin is
 * b = floorf(ph * 16.0f), clamped to [0, 15] AS A FLOAT and only then converted to an integer (the terrain and joint families' rule: no
 * value outside an int's range is ever converted), and profile_sum[f][b][e] += (double)fz, profile_count[f][b][e] += 1.  A foot in the
 * air contributes its 0, so sum / count is the mean vertical force at that phase of the commanded cycle.
 *
 * go1feet_accumulate: one thread per (foot, environment); no atomics, no LDS, every word has one writer.  The launch is
 * one-dimensional: 4 * ceil(N / 256) blocks of 256 threads, block k works on foot k / ceil(N / 256) and its lanes on consecutive
 * environments, so every load and store of a row is one contiguous run over a wavefront (the one exception: the profile word, whose bin
 * differs from lane to lane).  The rows of an event (touchdown, lift-off) and the profile word are touched only on the steps that fold
 * into them.  Per (f, e), in this order:
 *   1. the thread of foot 0: steps[e] += 1, and resets[e] += 1 if reset_buf[e] != 0.
 *   2. reset_buf[e] != 0: the step reset the environment.  Nothing is folded; prev_contact = 2, stance_valid = 0 (the four other state
 *      words keep what they hold: nothing reads them before a touchdown has written them again).
 *   3. otherwise, episode_length_buf[e] <= warmup_steps: the same.  (The behaviour table's rule: a warm-up breaks every stride.)
 *   4. otherwise the rows are folded (the six per-step rows, then a touchdown's two or a lift-off's four), then the profile sample, then
 *      the state advances as above.
 * go1feet_clear: one launch of the same shape: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0, min = +inf,
 *   max = -inf), the profile 0, prev_contact = 2, stance_valid = 0, stance_steps = 0, the three stance floats 0, steps = resets = 0.
 * go1feet_reduce: ONE launch of GO1FEET_REDUCE_THREADS-thread workgroups, which writes three tables and leaves what it reads as it is:
 *   num_groups * (4 * GO1FEET_NUM + 1) workgroups write results[num_groups][4 * GO1FEET_NUM + 1][GO1FEET_NUM_FIELDS].
 *     Rows f * GO1FEET_NUM + metric: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's
 *     environments e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments
 *     with count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields
 *     (index = Go1FeetField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with
 *     count = 0 the four in the middle are NaN.
 *     The last row of a group (index = Go1FeetGroupField): environments, steps (sum of steps[e]), resets, then 0, 0, 0, in the same order.
 *   num_groups * 4 further workgroups write profile_results[num_groups][4][GO1FEET_PHASE_BINS][2] as doubles: sum, then count.  In the
 *     workgroup of (group, foot) thread t owns bin t % 16 and adds profile_sum[f][t % 16][e] (and, as doubles, profile_count) of the
 *     group's environments e = t / 16, t / 16 + 16, ... in ascending order; then a fixed tree over the 16 slices (thread t takes thread
 *     t + 128, then + 64, + 32, + 16) and threads 0 .. 15 write their bin.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator, the profile or a state array is missing
 *   -3   an input is missing (go1feet_accumulate only: go1feet_clear and go1feet_reduce read none)
 *   -5   no group, no table, no profile table, or num_groups <= 0 (go1feet_reduce only)
 *   -12  dt not finite and positive, terrain_friction not finite or negative, or max_contact_force not finite (go1feet_accumulate only)
 *   -20  the launch itself failed
 *
 * What the figures are not.  contact_forces is the last substep's net force on the body: the impulse and the profile sample one substep
 * in four.  Contact is fz > 1 N and "normal" / "tangent" are world z / horizontal: friction_use is exact on flat ground only; on relief
 * it mixes in the slope, and a foot pressed against a wall reads as in the air.  mu is the STATIC coefficient: a sliding contact sits
 * at the dynamic one, so at or below 1.
 */
#ifndef GO1FEET_H
#define GO1FEET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1FEET_NUM 12
#define GO1FEET_NUM_FEET 4
#define GO1FEET_PHASE_BINS 16
#define GO1FEET_NUM_FIELDS 6
#define GO1FEET_REDUCE_THREADS 256
#define GO1FEET_CONTACT_FORCE 1.0

enum Go1FeetMetric {
  GO1FEET_CONTACT = 0, GO1FEET_FORCE_NORMAL = 1, GO1FEET_FORCE_TANGENT = 2, GO1FEET_FRICTION_USE = 3, GO1FEET_FORCE_EXCESS = 4,
  GO1FEET_IMPACT_VEL_SQ = 5, GO1FEET_TOUCHDOWN_SPEED = 6, GO1FEET_TOUCHDOWN_FORCE = 7, GO1FEET_STANCE_PEAK_FORCE = 8,
  GO1FEET_STANCE_IMPULSE = 9, GO1FEET_STANCE_SLIP = 10, GO1FEET_STANCE_TIME = 11
};
/* columns of a metric row */
enum Go1FeetField { GO1FEET_F_COUNT = 0, GO1FEET_F_MEAN = 1, GO1FEET_F_STD = 2, GO1FEET_F_MIN = 3, GO1FEET_F_MAX = 4, GO1FEET_F_NONFINITE = 5 };
/* columns of a group's own row (row 4 * GO1FEET_NUM) */
enum Go1FeetGroupField { GO1FEET_G_ENVS = 0, GO1FEET_G_STEPS = 1, GO1FEET_G_RESETS = 2 };

typedef struct Go1FeetConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing */
  int32_t num_groups;          /* G of the result tables */
  float dt;                    /* s, the policy step: impulse, slip and stance time multiply by it */
  float terrain_friction;      /* the ground's static coefficient (Go1SimConfig.terrain_friction) */
  float max_contact_force;     /* N: force_excess counts what lies beyond it (Go1SimConfig.max_contact_force) */
} Go1FeetConfig;

typedef struct Go1FeetBuffers {
  /* read by go1feet_accumulate */
  const float* contact_forces;        /* [17 * 3][N] */
  const float* foot_velocities;       /* [4 * 3][N] */
  const float* prev_foot_velocities;  /* [4 * 3][N] */
  const float* foot_indices;          /* [4][N] */
  const float* friction_coeffs;       /* [N] */
  const uint8_t* reset_buf;           /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* accumulators, [4 * GO1FEET_NUM][N]: row f * GO1FEET_NUM + metric */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  uint8_t* prev_contact;              /* [4][N]: 0 air, 1 ground, 2 unknown */
  uint8_t* stance_valid;              /* [4][N] */
  int32_t* stance_steps;              /* [4][N] */
  float* stance_peak;                 /* [4][N] */
  float* stance_impulse;              /* [4][N] */
  float* stance_slip;                 /* [4][N] */
  uint32_t* steps;                    /* [N]: accumulate launches since the clear */
  uint32_t* resets;                   /* [N]: of those, the steps that reset the environment */
  double* profile_sum;                /* [4][GO1FEET_PHASE_BINS][N] */
  uint32_t* profile_count;            /* [4][GO1FEET_PHASE_BINS][N] */
  /* go1feet_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][4 * GO1FEET_NUM + 1][GO1FEET_NUM_FIELDS] */
  double* profile_results;            /* [num_groups][4][GO1FEET_PHASE_BINS][2]: sum, count */
} Go1FeetBuffers;

/* empty accumulators and profile, every foot's state unknown.  One launch, one thread per (foot, environment). */
int go1feet_clear(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream);

/* after a simulator step: fold the step of every foot.  One launch, one thread per (foot, environment). */
int go1feet_accumulate(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream);

/* at the end: the three result tables from the accumulators, the profile and the state (which it leaves as they are).  One launch. */
int go1feet_reduce(const Go1FeetConfig* cfg, const Go1FeetBuffers* buf, void* stream);

/* "go1feet <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1feet_version(void);

#ifdef __cplusplus
}
#endif

#endif
