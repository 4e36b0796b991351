/* go1place.h — C-ABI of libgo1place.so: foot placement and stride geometry of a policy rollout, measured on the device (HIP, gfx950).
 *
 * The command vector asks for a stance width (cmd[12]) and a stance length (cmd[13]); with the forward speed and the step frequency they
 * set where the Raibert heuristic wants each foot.  The behaviour table (go1eval.h) has one figure for all of it, raibert_heuristic:
 * squared, summed over four feet and both axes, in swing and stance alike.  The foot library (go1feet.h) measures forces, the gait
 * library (go1gait.h) timing.  None of them says WHERE a foot lands against its nominal stance point, how far it sweeps under the body in
 * stance, what stride length and track width the robot realises, or how scattered its footprints are.  This library is that family.  It
 * is a library of its own, as the evaluation, foot, trunk and gait libraries are: no other binary, stamp or parity result depends on it.
 * The accumulators, the folding rule, the fixed-order reduction and the numbering of the return codes are go1eval.h's, restated here
 * (the device helpers are csrc/go1_tables.h's, shared with those libraries and covered by this library's stamp).  This header is the
 * specification: tests/place_ref.py is written from its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).  Foot f (0 FL, 1 FR, 2 RL, 3 RR) is
 * body 4 (f + 1) of contact_forces [17 * 3][N]: its vertical force is row 12 (f + 1) + 2; its position is rows 3 f .. 3 f + 2 of
 * foot_positions [4 * 3][N] (m, world).  The PARTNER of foot f is p = f ^ 1: the other foot of the same axle (FL <-> FR, RL <-> RR).
 *
 * Per foot f and environment e, the inputs of a step (read after the simulator's step):
 *   cmd[k]        commands[k][e] for k = 0, 1, 2, 4, and 12 / 13 where num_commands >= 13 / 14
 *   base, q       rows 0 .. 2 (position) and 5, 6 (q.z, q.w of the xyzw quaternion) of root_states
 *   pos, pos_p    the foot's and its partner's three rows of foot_positions
 *   fz            row 12 (f + 1) + 2 of contact_forces (N, world; the net force of the LAST SUBSTEP)
 *   fi            foot_indices[f][e]: the foot's gait clock in cycles, [0, 1)
 *   reset_buf, episode_length_buf
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off: a rounding
 * after every multiply, add, division and square root).  Only + - * /, sqrtf, fabsf, fmaxf, floorf and comparisons are used: no
 * trigonometric function runs on the device.  The quantities are those of the Raibert block of go1eval_behaviour_accumulate, operation
 * for operation:
 *   width  = cmd[12] if num_commands >= 13 else 0.3f;   length = cmd[13] if num_commands >= 14 else 0.45f
 *   yn = fmaxf(sqrtf(q.z * q.z + q.w * q.w), 1e-9f);    yz = -q.z / yn;   yw = q.w / yn        the inverse yaw quaternion (0, 0, yz, yw)
 *   half_period = 0.5f / cmd[4];                        cmd_vy = cmd[2] * length / 2
 *   v = pos - base (three subtractions), and (bx, by) = the x and y of R v = v + yw t + u x t with u = (0, 0, yz), t = 2 (u x v), every
 *     product formed, those by u's zeros included:
 *       cx = 0 * v.z - yz * v.y;   cy = yz * v.x - 0 * v.z;   cz = 0 * v.y - 0 * v.x;   t = (2 cx, 2 cy, 2 cz)
 *       bx = (v.x + yw * t.x) + (0 * t.z - yz * t.y);         by = (v.y + yw * t.y) + (yz * t.x - 0 * t.z)
 *     (so a non-finite v.z makes bx and by NaN, as it does there).  by_p is the partner's by, from pos_p in the same way.
 *   xs = (f < 2 ? 1 : -1) * length / 2;   ys = (f % 2 == 0 ? 1 : -1) * width / 2               the nominal stance point
 *   ph = fabsf(1 - fi * 2) * 1 - 0.5
 *   xo = ph * cmd[0] * half_period;       yo = ph * cmd_vy * half_period, negated for f >= 2   the heuristic's offset
 *   ex = bx - (xs + xo);   ey = by - (ys + yo)      realised minus commanded: ex * ex + ey * ey is the behaviour table's term of the
 *                                                   foot, bit for bit (it squares the same difference with the other sign)
 *   px = bx - xs;          py = by - ys             the foot against its nominal stance point
 *   c  = fz > GO1PLACE_CONTACT_FORCE                the foot is on the ground.  A NaN compares false: in the air.
 *
 * Fourteen rows per foot (index = Go1PlaceMetric), accumulator row f * GO1PLACE_NUM + metric, as go1feet.h lays out its own:
 *   stance_err_x, stance_err_y         every folded step with c       ex, ey
 *   swing_err_x, swing_err_y           every folded step without c    ex, ey
 *   touchdown_x, touchdown_y           at a touchdown                 px, py
 *   touchdown_err_x, touchdown_err_y   at a touchdown                 ex, ey
 *   track_width_err                    at a touchdown                 fabsf(by - by_p) - width
 *   stride_length                      at a touchdown with stride_open    sqrtf(dx * dx + dy * dy), d = the foot's world xy now (pos.x,
 *                                                                     pos.y) minus (td_world_x, td_world_y)
 *   stride_length_err                  with stride_length             stride_length - sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1]) / cmd[4]
 *   liftoff_x, liftoff_y               at a liftoff with stance_open  last_x, last_y: px, py of the last step in contact
 *   stance_sweep                       with liftoff_x, liftoff_y      td_x - last_x: positive when the foot travels backward under the body
 * The folding rule is go1eval_accumulate's: a non-finite value adds 1 to nonfinite[row][e] and enters nothing else; a finite value v adds
 * 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.  cmd[4] = 0 gives non-finite
 * errors, which are counted there.
 *
 * State per (foot, environment): prev_contact (uint8: 0 in the air, 1 on the ground, 2 unknown); stance_open and stride_open (uint8: a
 * touchdown of this stance / an earlier touchdown of this stride was seen); td_x (px at the touchdown), last_x, last_y (px, py of the
 * latest step in contact), td_world_x, td_world_y (the foot's world xy at the touchdown): fp32; touchdowns, liftoffs, strides and
 * map_outside (uint32); map [64] (uint32): the footprint map.  State per environment: steps and resets (uint32), written by the thread
 * of foot 0.
 *
 * The footprint map has GO1PLACE_MAP_SIDE x GO1PLACE_MAP_SIDE cells of map_cell metres around the nominal stance point: with the
 * default 0.03 it spans +-0.12 m.  At a touchdown u = floorf((px + 4.0f * map_cell) / map_cell), and v likewise from py.  If u >= 0,
 * u < 8, v >= 0 and v < 8, tested AS FLOATS (a NaN fails, and no value outside an int's range is ever converted),
 * map[f][8 v + u][e] += 1; otherwise map_outside[f][e] += 1.  So map counts plus map_outside equal touchdowns.
 *
 * go1place_accumulate: one thread per (foot, environment); no atomics, no LDS, no barrier, every word has one writer.  The launch is
 * one-dimensional: 4 * ceil(N / 256) blocks of 256 threads, block k works on foot k / ceil(N / 256) and its lanes on consecutive
 * environments, so every load and store of a row is one contiguous run over a wavefront (the one exception: the map word, whose cell
 * differs from lane to lane).  The rows and state words of an event are touched only on the steps of that event.  Per (f, e), in this
 * order:
 *   1. the thread of foot 0: steps[e] += 1, and resets[e] += 1 if reset_buf[e] != 0.
 *   2. If reset_buf[e] != 0 or episode_length_buf[e] <= warmup_steps: prev_contact = 2, stance_open = stride_open = 0.  Nothing is
 *      folded and nothing else happens: a stance or a stride never spans a reset or the warm-up (the floats keep what they hold: nothing
 *      reads them before a touchdown has written them again).
 *   3. The quantities above; stance_err_x, stance_err_y (with c) or swing_err_x, swing_err_y (without) are folded.
 *   4. TOUCHDOWN, c && prev_contact == 0: touchdown_x, touchdown_y, touchdown_err_x, touchdown_err_y and track_width_err are folded, in
 *      this order; the footprint enters the map or map_outside; if stride_open, stride_length and stride_length_err are folded and
 *      strides += 1; then td_x = px, td_world = (pos.x, pos.y), stance_open = stride_open = 1 and touchdowns += 1.
 *   5. LIFTOFF, !c && prev_contact == 1: if stance_open, liftoff_x, liftoff_y and stance_sweep are folded and liftoffs += 1.  Then
 *      stance_open = 0.  (A stance whose touchdown was not seen, c with prev_contact == 2, is never open: it folds nothing.)
 *   6. If c: last_x = px, last_y = py.
 *   7. prev_contact = c ? 1 : 0.  There is no debounce: one step in the air ends a stance, and a bounce is a stride.
 * go1place_clear: one launch of the same shape: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0, min = +inf,
 *   max = -inf), the map and the six counters 0, prev_contact = 2, stance_open = stride_open = 0, the five floats 0.
 * go1place_reduce: ONE launch of GO1PLACE_REDUCE_THREADS-thread workgroups, which writes two tables and leaves what it reads as it is:
 *   num_groups * (4 * GO1PLACE_NUM + 1) workgroups write results[num_groups][4 * GO1PLACE_NUM + 1][GO1PLACE_NUM_FIELDS].
 *     Rows f * GO1PLACE_NUM + metric: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's
 *     environments e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments
 *     with count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields
 *     (index = Go1PlaceField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with
 *     count = 0 the four in the middle are NaN.
 *     The last row of a group (index = Go1PlaceGroupField): environments, steps (sum of steps[e]), resets, touchdowns, strides,
 *     map_outside, in the same order; the last three add an environment's four words, feet 0 .. 3 in this order, each as a double.
 *   num_groups * 4 * 4 further workgroups write map_results[num_groups][4][64] as doubles.  The workgroup of (group, foot, quarter k)
 *     sums the cells 16 k .. 16 k + 15 in the foot library's profile order: thread t owns cell 16 k + t % 16 and adds, as doubles, the
 *     map's word of the group's environments e = t / 16, t / 16 + 16, ... in ascending order; then a fixed tree over the 16 slices
 *     (thread t takes thread t + 128, then + 64, + 32, + 16) and threads 0 .. 15 write their cell.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator, the map or a state array is missing
 *   -3   an input is missing (go1place_accumulate only: go1place_clear and go1place_reduce read none)
 *   -5   no group, no table, no map table, or num_groups <= 0 (go1place_reduce only)
 *   -12  map_cell not positive and finite, or num_commands < 5 (go1place_accumulate only)
 *   -20  the launch itself failed
 *
 * What the figures are not.  Contact is the last substep's fz > 1 N, not a debounced contact sensor.  Positions are in the YAW-ALIGNED
 * base frame: roll and pitch tilt them, and the base origin stands in for the hip line.  stride_length_err ignores the yaw command: each
 * foot of a turning robot walks an arc of its own.  The partner foot is usually in swing at a touchdown in a trot, so track_width_err
 * compares a landing foot with one in the air.  The map drops what falls outside it and counts it.  map_cell = 0.03 is a placeholder:
 * nothing measured stands behind it.  A float of the state may hold a NaN (px of a foot whose position is not finite); which words are
 * NaN is specified, the sign and payload of such a NaN are the hardware's (IEEE 754 leaves them open).
 */
#ifndef GO1PLACE_H
#define GO1PLACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1PLACE_NUM 14
#define GO1PLACE_NUM_FEET 4
#define GO1PLACE_MAP_SIDE 8
#define GO1PLACE_MAP_CELLS 64
#define GO1PLACE_NUM_FIELDS 6
#define GO1PLACE_REDUCE_THREADS 256
#define GO1PLACE_CONTACT_FORCE 1.0

enum Go1PlaceMetric {
  GO1PLACE_STANCE_ERR_X = 0, GO1PLACE_STANCE_ERR_Y = 1, GO1PLACE_SWING_ERR_X = 2, GO1PLACE_SWING_ERR_Y = 3, GO1PLACE_TOUCHDOWN_X = 4,
  GO1PLACE_TOUCHDOWN_Y = 5, GO1PLACE_TOUCHDOWN_ERR_X = 6, GO1PLACE_TOUCHDOWN_ERR_Y = 7, GO1PLACE_TRACK_WIDTH_ERR = 8,
  GO1PLACE_STRIDE_LENGTH = 9, GO1PLACE_STRIDE_LENGTH_ERR = 10, GO1PLACE_LIFTOFF_X = 11, GO1PLACE_LIFTOFF_Y = 12, GO1PLACE_STANCE_SWEEP = 13
};
/* columns of a metric row */
enum Go1PlaceField { GO1PLACE_F_COUNT = 0, GO1PLACE_F_MEAN = 1, GO1PLACE_F_STD = 2, GO1PLACE_F_MIN = 3, GO1PLACE_F_MAX = 4, GO1PLACE_F_NONFINITE = 5 };
/* columns of a group's own row (row 4 * GO1PLACE_NUM) */
enum Go1PlaceGroupField {
  GO1PLACE_G_ENVS = 0, GO1PLACE_G_STEPS = 1, GO1PLACE_G_RESETS = 2, GO1PLACE_G_TOUCHDOWNS = 3, GO1PLACE_G_STRIDES = 4, GO1PLACE_G_MAP_OUTSIDE = 5
};

typedef struct Go1PlaceConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing */
  int32_t num_groups;          /* G of the result tables */
  int32_t num_commands;        /* entries of the command vector: below 13 / 14 the width / length are the defaults */
  float map_cell;              /* m, the side of a cell of the footprint map; 0.03: the map spans +-0.12 m */
} Go1PlaceConfig;

typedef struct Go1PlaceBuffers {
  /* read by go1place_accumulate */
  const float* commands;              /* [>= num_commands][N] */
  const float* root_states;           /* [13][N] */
  const float* foot_positions;        /* [4 * 3][N] */
  const float* contact_forces;        /* [17 * 3][N] */
  const float* foot_indices;          /* [4][N] */
  const uint8_t* reset_buf;           /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* accumulators, [4 * GO1PLACE_NUM][N]: row f * GO1PLACE_NUM + metric */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  uint8_t* prev_contact;              /* [4][N]: 0 air, 1 ground, 2 unknown */
  uint8_t* stance_open;               /* [4][N] */
  uint8_t* stride_open;               /* [4][N] */
  float* td_x;                        /* [4][N] */
  float* last_x;                      /* [4][N] */
  float* last_y;                      /* [4][N] */
  float* td_world_x;                  /* [4][N] */
  float* td_world_y;                  /* [4][N] */
  uint32_t* touchdowns;               /* [4][N] */
  uint32_t* liftoffs;                 /* [4][N]: liftoffs of stances seen from their touchdown */
  uint32_t* strides;                  /* [4][N] */
  uint32_t* map_outside;              /* [4][N]: touchdowns outside the map */
  uint32_t* map;                      /* [4][GO1PLACE_MAP_CELLS][N]: cell 8 v + u */
  uint32_t* steps;                    /* [N]: accumulate launches since the clear */
  uint32_t* resets;                   /* [N]: of those, the steps that reset the environment */
  /* go1place_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][4 * GO1PLACE_NUM + 1][GO1PLACE_NUM_FIELDS] */
  double* map_results;                /* [num_groups][4][GO1PLACE_MAP_CELLS] */
} Go1PlaceBuffers;

/* empty accumulators and map, every foot's state unknown.  One launch, one thread per (foot, environment). */
int go1place_clear(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf, void* stream);

/* after a simulator step: fold the step of every foot.  One launch, one thread per (foot, environment). */
int go1place_accumulate(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf, void* stream);

/* at the end: the two result tables from the accumulators, the map and the state (which it leaves as they are).  One launch. */
int go1place_reduce(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf, void* stream);

/* "go1place <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1place_version(void);

#ifdef __cplusplus
}
#endif

#endif
