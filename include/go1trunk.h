/* go1trunk.h — C-ABI of libgo1trunk.so: trunk motion, support margin and path drift of a policy rollout, measured on the device
 * (HIP, gfx950).
 *
 * The evaluation library (go1eval.h) measures the robot as a whole, its gait timing and its joints, and libgo1feet (go1feet.h) what
 * each foot puts into the ground.  None of them looks at what the trunk does: how far it rolls and pitches and how fast, what
 * acceleration an IMU or a payload on it would see, whether the base is over the polygon of the supporting feet and how close to its
 * edge, and whether the robot walks the straight line it is commanded.  This library is that family.  It is a library of its own, as
 * the renderer, the evaluation library and the foot library are: no other binary, stamp or parity result depends on it.  The
 * accumulators, the folding rule, the fixed-order reduction and the numbering of the return codes are go1eval.h's, restated here
 * (csrc/go1trunk.hip restates the few device helpers as well; the libraries share no header).  This header is the specification:
 * tests/trunk_ref.py is written from its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).  Foot f (0 FL, 1 FR, 2 RL, 3 RR) is
 * body 4 (f + 1) of contact_forces [17 * 3][N]; its vertical force is row 12 (f + 1) + 2.
 *
 * Per environment e, the inputs of a step (read after the simulator's step):
 *   px, py           rows 0, 1 of root_states (m, world)
 *   qx, qy, qz, qw   rows 3 .. 6 of root_states (xyzw)
 *   vx, vy, vz       rows 7 .. 9 of root_states (m/s, world)
 *   wx, wy, wz       rows 10 .. 12 of root_states (rad/s, world)
 *   bvz              row 2 of base_lin_vel (m/s, body frame)
 *   bwx, bwy         rows 0, 1 of base_ang_vel (rad/s, body frame)
 *   gx, gy           rows 0, 1 of projected_gravity (the unit gravity vector in the body frame)
 *   cx, cy, cw       rows 0, 1, 2 of commands (m/s, m/s, rad/s)
 *   fz_f             row 12 (f + 1) + 2 of contact_forces, foot f (N, world; the net force of the LAST SUBSTEP)
 *   x_f, y_f         rows 3 f, 3 f + 1 of foot_positions (m, world)
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off: a rounding
 * after every multiply, add, division and square root).  Only + - * /, sqrtf, floorf, fabsf and comparisons are used: no
 * trigonometric function, so angles are reported as their sines and converted on the host for display only.
 *   heading   h0x = 1 - 2 * (qy * qy + qz * qz), h0y = 2 * (qx * qy + qw * qz): the body's x axis in the world's horizontal plane.
 *             n = sqrtf(h0x * h0x + h0y * h0y), hx = h0x / n, hy = h0y / n.  heading_ok: n is finite and > 0, and px and py are finite.
 *   contact   c_f = fz_f > GO1TRUNK_CONTACT_FORCE: the foot and behaviour families' rule (a NaN compares false: in the air).  n_c is the
 *             number of feet in contact.
 *   tilt      sqrtf(gx * gx + gy * gy): the sine of the angle between the body's z axis and the vertical.
 *   edge distance, for an edge from foot A to foot B and the base P = (px, py):
 *             ex = x_B - x_A, ey = y_B - y_A, d(A, B) = (ex * (py - y_A) - ey * (px - x_A)) / sqrtf(ex * ex + ey * ey).
 *   The cyclic order of the feet is FL, RL, RR, FR (simulator indices 0, 2, 3, 1): counter-clockwise seen from above, so d > 0 means that
 *   the base lies to the inside of the edge.
 *
 * Seventeen rows (index = Go1TrunkMetric, accumulator row = metric):
 *   roll_sin           every folded step    gy
 *   pitch_sin          every folded step    gx
 *   tilt               every folded step    tilt.  Its square is the reference's _reward_orientation.
 *   tilt_exceeded      every folded step    tilt > tilt_limit ? 1 : 0 (a NaN gives 0)
 *   roll_rate          every folded step    bwx
 *   pitch_rate         every folded step    bwy.  bwx * bwx + bwy * bwy is the reference's _reward_ang_vel_xy.
 *   vertical_vel       every folded step    bvz.  Its square is the reference's _reward_lin_vel_z.
 *   accel_horizontal   when prev_valid      sqrtf(ax * ax + ay * ay) with ax = (vx - pvx) / dt, ay = (vy - pvy) / dt
 *   accel_vertical     when prev_valid      (vz - pvz) / dt
 *   ang_accel          when prev_valid      sqrtf((ux * ux + uy * uy) + uz * uz) with u = (w - pw) / dt, component by component
 *   support_feet       every folded step    (float) n_c
 *   support_margin     when n_c >= 3        the smallest d over the consecutive pairs of the feet in contact, taken in the cyclic order and
 *                                           wrapping round (three edges for three feet, four for four).  Starting from the first edge's d, a
 *                                           further edge's d replaces the margin m when d < m or d is a NaN: a NaN edge makes the margin a NaN
 *                                           whatever the others are.  Positive means inside.  It is this formula, not a convex hull: crossed
 *                                           feet give what it gives, and a zero-length edge (0 / 0) gives a NaN, counted in nonfinite.
 *   margin_negative    when n_c >= 3        margin < 0 ? 1 : 0 (a NaN gives 0)
 *   support_line_dist  when n_c == 2        fabsf(d(A, B)), A the first and B the second of the two feet in contact in the cyclic order
 *   lateral_drift      at a segment's close  see below
 *   heading_drift      at a segment's close  see below
 *   progress_err       at a segment's close  see below
 * The folding rule is go1eval_accumulate's: a non-finite value adds 1 to nonfinite[row][e] and enters nothing else; a finite value v adds
 * 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.
 *
 * State per environment: prev_valid (uint8), prev_lin_vel [3] = pv and prev_ang_vel [3] = pw (fp32): the world velocities of the last folded
 * step; seg_valid (uint8: a segment is open), seg_steps (int32), seg_anchor [4] = x0, y0, hx0, hy0 and seg_command [2] = sx, sy (fp32);
 * segments_dropped, steps and resets (uint32).  After the rows of a folded step: pv = v, pw = w, prev_valid = 1.
 *
 * Segments answer "how far off a straight commanded path after segment_steps steps".  They run on a folded step, after the per-step rows,
 * on the state as the step found it:
 *   No open segment (seg_valid == 0): if heading_ok, one is opened: the anchor is this step's (px, py, hx, hy), sx = sy = 0, seg_steps = 0,
 *     seg_valid = 1.  Nothing is folded.  If not heading_ok, nothing happens.
 *   An open segment: if !(cw == 0) (so also a NaN) or !heading_ok, it is dropped: seg_valid = 0 and segments_dropped += 1; no segment is
 *     opened on that step.  Otherwise sx += cx * dt, sy += cy * dt (each product rounded, then added), seg_steps += 1, and when seg_steps
 *     == segment_steps the segment closes:
 *       dx = px - x0, dy = py - y0, along = dx * hx0 + dy * hy0, lateral = dy * hx0 - dx * hy0
 *       lateral_drift = lateral - sy; heading_drift = hx0 * hy - hy0 * hx, the sine of the heading change, positive to the left;
 *       progress_err = along - sx
 *     are folded, and the segment is anchored again at this step's (px, py, hx, hy) with sx = sy = 0, seg_steps = 0 (it stays open).
 *
 * The tilt histogram has GO1TRUNK_TILT_BINS bins of width 1 / 32 (about 1.8 degrees).  On every folded step with a finite tilt the bin is
 * b = floorf(tilt * 32.0f), clamped to [0, 15] AS A FLOAT and only then converted to an integer, and tilt_hist[b][e] += 1.  The last bin
 * holds everything from 0.46875 up.
 *
 * go1trunk_accumulate: one thread per environment, ceil(N / 256) blocks of 256 threads; no atomics, no LDS, every word has one writer,
 * and every load and store of a row is one contiguous run over a wavefront (the one exception: the histogram word, whose bin differs
 * from lane to lane).  The rows of an event (the accelerations, the support rows, a segment's close) are touched only on the steps that
 * fold into them.  Per e, in this order:
 *   1. steps[e] += 1, and resets[e] += 1 if reset_buf[e] != 0.
 *   2. reset_buf[e] != 0: the step reset the environment.  Nothing is folded; prev_valid = 0 and seg_valid = 0 (an open segment is
 *      forgotten, not counted as dropped; the other state words keep what they hold: nothing reads them before they are written again).
 *   3. otherwise, episode_length_buf[e] <= warmup_steps: the same.
 *   4. otherwise the rows are folded in the order of the enum up to support_line_dist, then the histogram sample, then pv, pw and
 *      prev_valid, then the segment.
 * go1trunk_clear: one launch of the same shape: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0, min = +inf,
 *   max = -inf), the histogram 0 and every state word 0 (so prev_valid = seg_valid = 0).
 * go1trunk_reduce: ONE launch of GO1TRUNK_REDUCE_THREADS-thread workgroups, which writes two tables and leaves what it reads as it is:
 *   num_groups * (GO1TRUNK_NUM + 1) workgroups write results[num_groups][GO1TRUNK_NUM + 1][GO1TRUNK_NUM_FIELDS].
 *     Rows 0 .. GO1TRUNK_NUM - 1: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's environments
 *     e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments with
 *     count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields
 *     (index = Go1TrunkField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with
 *     count = 0 the four in the middle are NaN.
 *     The last row of a group (index = Go1TrunkGroupField): environments, steps (sum of steps[e]), resets, segments_dropped, then 0, 0, in
 *     the same order.
 *   num_groups further workgroups write hist_results[num_groups][GO1TRUNK_TILT_BINS] as doubles.  In the workgroup of a group thread t owns
 *     bin t % 16 and adds, as doubles, tilt_hist[t % 16][e] of the group's environments e = t / 16, t / 16 + 16, ... in ascending order;
 *     then a fixed tree over the 16 slices (thread t takes thread t + 128, then + 64, + 32, + 16) and threads 0 .. 15 write their bin.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator, the histogram or a state array is missing
 *   -3   an input is missing (go1trunk_accumulate only: go1trunk_clear and go1trunk_reduce read none)
 *   -5   no group, no table, no histogram table, or num_groups <= 0 (go1trunk_reduce only)
 *   -12  dt not finite and positive, tilt_limit not finite or negative, or segment_steps <= 0 (go1trunk_accumulate only)
 *   -20  the launch itself failed
 *
 * What the figures are not.  The base origin stands in for the centre of mass: com_displacements, the payload and the legs are ignored.
 * The margin is static (the base's projection against the stance polygon), not a zero-moment point.  Contact is fz > 1 N of the last
 * substep.  commands is read after the step, so a resample inside the step is seen one step early.  The accelerations are differences of
 * policy-step velocities: a push between two steps shows up as one step's acceleration, and what happens within a step is averaged.
 * Segments exist only while the yaw command is exactly 0.
 */
#ifndef GO1TRUNK_H
#define GO1TRUNK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1TRUNK_NUM 17
#define GO1TRUNK_TILT_BINS 16
#define GO1TRUNK_NUM_FIELDS 6
#define GO1TRUNK_REDUCE_THREADS 256
#define GO1TRUNK_CONTACT_FORCE 1.0

enum Go1TrunkMetric {
  GO1TRUNK_ROLL_SIN = 0, GO1TRUNK_PITCH_SIN = 1, GO1TRUNK_TILT = 2, GO1TRUNK_TILT_EXCEEDED = 3, GO1TRUNK_ROLL_RATE = 4,
  GO1TRUNK_PITCH_RATE = 5, GO1TRUNK_VERTICAL_VEL = 6, GO1TRUNK_ACCEL_HORIZONTAL = 7, GO1TRUNK_ACCEL_VERTICAL = 8, GO1TRUNK_ANG_ACCEL = 9,
  GO1TRUNK_SUPPORT_FEET = 10, GO1TRUNK_SUPPORT_MARGIN = 11, GO1TRUNK_MARGIN_NEGATIVE = 12, GO1TRUNK_SUPPORT_LINE_DIST = 13,
  GO1TRUNK_LATERAL_DRIFT = 14, GO1TRUNK_HEADING_DRIFT = 15, GO1TRUNK_PROGRESS_ERR = 16
};
/* columns of a metric row */
enum Go1TrunkField { GO1TRUNK_F_COUNT = 0, GO1TRUNK_F_MEAN = 1, GO1TRUNK_F_STD = 2, GO1TRUNK_F_MIN = 3, GO1TRUNK_F_MAX = 4, GO1TRUNK_F_NONFINITE = 5 };
/* columns of a group's own row (row GO1TRUNK_NUM) */
enum Go1TrunkGroupField { GO1TRUNK_G_ENVS = 0, GO1TRUNK_G_STEPS = 1, GO1TRUNK_G_RESETS = 2, GO1TRUNK_G_SEGMENTS_DROPPED = 3 };

typedef struct Go1TrunkConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing */
  int32_t num_groups;          /* G of the result tables */
  int32_t segment_steps;       /* policy steps of a drift segment */
  float dt;                    /* s, the policy step */
  float tilt_limit;            /* tilt_exceeded counts the steps with tilt beyond it (a sine) */
} Go1TrunkConfig;

typedef struct Go1TrunkBuffers {
  /* read by go1trunk_accumulate */
  const float* root_states;           /* [13][N] */
  const float* base_lin_vel;          /* [3][N] */
  const float* base_ang_vel;          /* [3][N] */
  const float* projected_gravity;     /* [3][N] */
  const float* commands;              /* [>= 3][N] */
  const float* contact_forces;        /* [17 * 3][N] */
  const float* foot_positions;        /* [4 * 3][N] */
  const uint8_t* reset_buf;           /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* accumulators, [GO1TRUNK_NUM][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  uint8_t* prev_valid;                /* [N] */
  float* prev_lin_vel;                /* [3][N]: pv */
  float* prev_ang_vel;                /* [3][N]: pw */
  uint8_t* seg_valid;                 /* [N] */
  int32_t* seg_steps;                 /* [N] */
  float* seg_anchor;                  /* [4][N]: x0, y0, hx0, hy0 */
  float* seg_command;                 /* [2][N]: sx, sy */
  uint32_t* segments_dropped;         /* [N] */
  uint32_t* steps;                    /* [N]: accumulate launches since the clear */
  uint32_t* resets;                   /* [N]: of those, the steps that reset the environment */
  uint32_t* tilt_hist;                /* [GO1TRUNK_TILT_BINS][N] */
  /* go1trunk_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][GO1TRUNK_NUM + 1][GO1TRUNK_NUM_FIELDS] */
  double* hist_results;               /* [num_groups][GO1TRUNK_TILT_BINS] */
} Go1TrunkBuffers;

/* empty accumulators and histogram, no previous velocity, no open segment.  One launch, one thread per environment. */
int go1trunk_clear(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf, void* stream);

/* after a simulator step: fold the step of every environment.  One launch, one thread per environment. */
int go1trunk_accumulate(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf, void* stream);

/* at the end: the two result tables from the accumulators, the histogram and the state (which it leaves as they are).  One launch. */
int go1trunk_reduce(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf, void* stream);

/* "go1trunk <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1trunk_version(void);

#ifdef __cplusplus
}
#endif

#endif
