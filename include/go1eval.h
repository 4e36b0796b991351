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
 *
 * ---- the behaviour table (second kernel family; index = Go1BehaviourMetric) --------------------------------------------------
 * The ten metrics above say how well a policy tracks a velocity.  The behaviour table says whether it does what the other
 * commands ask (body height, step frequency, gait, duty factor, foot swing, pitch and roll, stance width and length), from the
 * simulator's SoA buffers after a step, with the same accumulators, the same folding rule and the same reduction.
 *
 * A foot f (0..3) is body 4 + 4 f of contact_forces ([17 * 3][N]) and rows 3 f .. 3 f + 2 of foot_positions / foot_velocities.
 * It is IN CONTACT when its F_z > 1.0 (the reference's threshold).  cmd[k] = commands[k][e].
 *
 * Seven per-step metrics (fp32; a sum over feet or joints adds its fp32 terms in an fp64 carry, feet / joints in ascending
 * order, and rounds to fp32 once, as base_height and power_consumption do above):
 *   contact_match      0.25 * number of feet with [F_z > 1.0] == [desired_contact_states[f] > 0.5]   (tools/play_eval.py's figure)
 *   body_height_err    height - (cmd[3] + base_height_target), signed; height is the metric base_height above (root z minus the
 *                      mean of measured_heights; root z when measured_heights is NULL)
 *   orientation_err    sqrt(dx^2 + dy^2), d = R(q)^T (0, 0, -1) - R(qc)^T (0, 0, -1): q the base quaternion root_states[3..6]
 *                      (xyzw), qc = roll(-cmd[11]) about x  *  pitch(-cmd[10]) about y, the composition of the reference's
 *                      _reward_orientation_control, i.e. qc = (sr cp, cr sp, sr sp, cr cp) with sr, cr = sin, cos(-cmd[11] / 2) and
 *                      sp, cp = sin, cos(-cmd[10] / 2).  R(q)^T v = v + w t + u x t with u = -q.xyz, t = 2 (u x v).  Computed from
 *                      the quaternion and the fixed vector (0, 0, -1), not from projected_gravity: gravity randomisation does not
 *                      show up as an attitude error.
 *   feet_clearance     sum over the feet of (cmd[9] * ph + 0.02 - z_f)^2 * (1 - desired_contact_states[f]),
 *                      ph = 1 - |1 - 2 clip(2 foot_indices[f] - 1, 0, 1)|  (the reference's _reward_feet_clearance_cmd_linear).
 *                      z_f is the foot's WORLD z as there: meaningful on flat ground only.
 *   raibert_heuristic  sum over the feet of (xs + xo - bx)^2 + (ys + yo - by)^2  (the reference's _reward_raibert_heuristic):
 *                      (bx, by) = the foot's position minus the base position, rotated by the inverse yaw of the base, the yaw
 *                      quaternion being (0, 0, -q.z, q.w) / max(sqrt(q.z^2 + q.w^2), 1e-9);
 *                      width = cmd[12] if num_commands >= 13 else 0.3, length = cmd[13] if num_commands >= 14 else 0.45;
 *                      xs = +length / 2 (feet 0, 1), -length / 2 (feet 2, 3);  ys = +width / 2 (feet 0, 2), -width / 2 (feet 1, 3);
 *                      ph = |1 - 2 foot_indices[f]| - 0.5;  xo = ph * cmd[0] * (0.5 / cmd[4]);
 *                      yo = ph * (cmd[2] * length / 2) * (0.5 / cmd[4]), negated for feet 2, 3.  cmd[4] = 0 gives a non-finite value.
 *   feet_slip          sum over the feet IN CONTACT of v_x^2 + v_y^2 (foot_velocities).  The reference's _reward_feet_slip without
 *                      its previous-step filter: it does not depend on last_contacts, which only an active reward term maintains.
 *   action_rate        sum over the 12 joints of (last_actions[j] - last_last_actions[j])^2; after a step last_actions holds this
 *                      step's action and last_last_actions the one before.
 *
 * Three per-stride metrics, folded at a TOUCHDOWN of a foot, not every step.  Per foot the kernel carries prev_contact (0, 1, or
 * 2 = unknown), stride_steps (-1 = no touchdown seen yet), stance_steps and swing_peak.  A touchdown of foot f is: in contact now
 * and prev_contact[f] == 0.  At a touchdown with L = stride_steps[f] >= 0 a stride of L steps has just ended, and with the
 * commands of the touchdown step
 *   step_frequency_err = 1 / (L * dt) - cmd[4]
 *   duty_factor_err    = stance_steps[f] / L - cmd[8]
 *   swing_height_err   = (swing_peak[f] - 0.02) - cmd[9]
 * are folded (L and stance_steps converted to fp32; L >= 2 by construction).  After folding, or after skipping the fold because
 * stride_steps[f] < 0, stride_steps[f] = 0, stance_steps[f] = 0, swing_peak[f] = -inf.  Then, touchdown or not:
 *   stride_steps[f] += 1 if it is >= 0;  stance_steps[f] += 1 if the foot is in contact;
 *   swing_peak[f] = max(swing_peak[f], z_f);  prev_contact[f] = contact.
 * So swing_peak is the largest world z of the foot from the touchdown step to the step before the next touchdown, and 0.02 is
 * the reference's foot radius.  There is NO DEBOUNCE: a chattering contact ends strides of two or three steps and shows up as a
 * high step frequency, which is what it is.
 *
 * go1eval_behaviour_accumulate, per environment e (one thread each; every accumulator and every state word has one writer), in
 * this order:
 *   1. reset_buf[e] != 0, or episode_length_buf[e] <= warmup_steps: nothing is folded; all four feet go to prev_contact = 2,
 *      stride_steps = -1 (stance_steps and swing_peak are left: the next touchdown resets them before they are read).  A stride
 *      never spans a reset or the warm-up.
 *   2. otherwise the seven per-step metrics are folded, then feet 0, 1, 2, 3 are advanced in that order by the rules above: two
 *      touchdowns in one step fold in a fixed order.
 *   Folding is the rule of go1eval_accumulate: a non-finite value is counted in nonfinite and enters nothing else.
 * go1eval_behaviour_clear: accumulators as go1eval_clear; prev_contact = 2, stride_steps = -1, stance_steps = 0, swing_peak = -inf.
 * go1eval_behaviour_reduce: the metric rows of go1eval_reduce, the same fixed combination order (the same device function), into
 * results[num_groups][GO1EVAL_NUM_BEHAVIOUR][GO1EVAL_NUM_FIELDS].  There is no group row; the first table has it.
 *
 * ---- the trace and the step response (third kernel family) --------------------------------------------------------------------
 * The two tables measure steady state.  The trace is a per-step time series of GO1EVAL_NUM_TRACE fp32 channels of K chosen
 * environments, written on the device by one launch per step; the response analysis turns a trace that holds ONE command switch
 * into rise time, overshoot, settling time, steady-state error and integrated error per environment, reduced per group by the
 * tables' fixed-order reduction.  Replaces the per-step host reads of the reference's scripts/play.py (base_lin_vel[0, 0] and
 * dof_pos[0, :] copied to the host after every one of its 250 steps).
 *
 * Channels (index = Go1TraceChannel), the value after a step:
 *    0 lin_vel_x          base_lin_vel[0]                  6 cmd_lin_vel_x    commands[0]
 *    1 lin_vel_y          base_lin_vel[1]                  7 cmd_lin_vel_y    commands[1]
 *    2 ang_vel_yaw        base_ang_vel[2]                  8 cmd_ang_vel_yaw  commands[2]
 *    3 base_height        the metric base_height above     9 cmd_base_height  commands[3] + base_height_target (one fp32 add)
 *    4 contact_match      the behaviour table's           10 max_torques      the metric max_torques above
 *    5 power_consumption  the metric power_consumption    11 reset            reset_buf != 0 ? 1 : 0
 *   12..23 dof_pos_0..11  dof_pos[j]
 *   Channels 3, 5 and 10 are the first table's expressions (the same fp32 terms, the same fp64 carry, rounded once) and channel 4
 *   is the behaviour table's, evaluated on EVERY step: the trace has no warm-up and no reset rule.  A reset step is recorded as
 *   the buffers stand (the old episode's velocities with the new episode's pose); channel 11 marks it.
 *
 * go1eval_trace_record(cfg, buf, row, stream): one launch, one thread per traced environment k in [0, K), K = num_traced.  It
 *   reads environment env_ids[k]; env_ids == NULL means k itself and needs K == N.  It writes trace[(row * 24 + c) * K + k] for
 *   the 24 channels c, so a wavefront's stores of one channel are one contiguous run.  An id outside [0, N) writes NaN to its 24
 *   values.  `row` is a host argument (the caller counts its own launches): row < 0 or row >= capacity is refused before the
 *   launch with a code of its own (-7), and nothing is written.
 *
 * go1eval_response(cfg, buf, stream): one launch, one thread per traced environment, a pure function of the trace.  rows = the
 *   recorded rows, s0 = switch_row (the first row recorded after the command changed: the state one policy step after the
 *   switch), w = smooth, end = rows.  Refused before the launch (-9) unless 1 <= w <= pre + 1, pre <= s0 < rows, hold >= 1,
 *   tail >= 1, max(hold, tail) <= rows - s0, dt > 0 and band > 0; (-10) unless 1 <= num_signals <= GO1EVAL_MAX_SIGNALS, every
 *   y_channel is in [0, 24) and every r_channel is below 24 (negative: none).  c[t] below is channel c of this environment at row t.
 *   Every operation that is not marked fp64 is an fp32 operation on fp32 values; 0.1 and 1e-6 are fp32 constants.
 *   1. Status.  1: some row in [s0 - pre, end) has channel 11 != 0 (the robot fell or timed out inside the window; a NaN, the
 *      trace of an id outside [0, N), is != 0).  Otherwise 2: some signal with r_channel >= 0 has a row t in [s0, end) with
 *      r[t] != r1 = r[s0], or a row t in [s0 - pre, s0) with r[t] != r0 = r[s0 - 1] (the command was not held).  Otherwise 0.
 *      With status != 0 every value of every signal is NaN.
 *   2. Per signal {y_channel, r_channel, fixed_target, fixed_scale}: r1 = r[s0], r0 = r[s0 - 1] (r0 = r1 when s0 == 0);
 *      r_channel < 0: r1 = fixed_target and r0 = r1.  Scale D = fixed_scale if fixed_scale > 0, else |r1 - r0|.  D < 1e-6: all
 *      seven values are NaN (there is no step on this signal).  Direction sgn = +1 if r1 >= r0, else -1.
 *   3. Smoothed signal: ys(t) = the mean of y over rows t - w + 1 .. t: added in an fp64 carry in ascending row order, divided
 *      by (double)w in fp64, rounded to fp32 once.  e(t) = ys(t) - r1.
 *   4. Seven values (index = Go1ResponseMetric), t over [s0, end) in ascending order:
 *      reached           1 if some t has |e(t)| <= 0.1 * D, else 0
 *      rise_time         (float)(t_r - s0 + 1) * dt for the first such t = t_r; NaN when not reached
 *      overshoot         the fold of fmaxf over sgn * e(t) / D, starting from 0: max(0, the largest excursion past the target) / D
 *      settled           t_v = the last t with |e(t)| > band * D, t_s = t_v + 1 (s0 if there is none); 1 if t_s <= end - hold, else 0
 *      settling_time     (float)(t_s - s0 + 1) * dt; NaN when not settled
 *      steady_state_err  the mean over rows [end - tail, end) of the raw y[t] - r1, signed: the fp32 differences added in an
 *                        fp64 carry, divided by (double)tail in fp64, rounded to fp32 once
 *      iae               dt * the sum over [s0, end) of |y[t] - r1|, raw: the fp32 terms added in an fp64 carry, multiplied by
 *                        (double)dt in fp64, rounded to fp32 once
 *      The box filter delays ys by about (w - 1) / 2 rows, and that delay is inside rise_time and settling_time.
 *   5. Outputs: values[(s * 7 + m) * K + k] (fp32) for signal s and value m, and status[k] (int32).  One writer each, no atomics.
 *
 * go1eval_response_reduce(cfg, buf, stream): results[num_groups][num_signals * 7 + 1][GO1EVAL_NUM_FIELDS] over the traced
 *   environments with group[k] == g (-1 or any id outside the range = not evaluated).  Row s * 7 + m is the metric row of
 *   go1eval_reduce (the same device function, the same fixed combination order) over per-environment accumulators that folded the
 *   one value values[s][m][k] by the folding rule above: a non-finite value counts in nonfinite and enters nothing else; a finite
 *   value v has count 1, sum v, sumsq v * v (fp64), min = max = v.  The last row of a group: traced environments, environments
 *   with status 0, with status 1, with status 2, 0, 0 (sums in the same fixed order).
 *
 * ---- the push and the disturbance recovery (fourth kernel family) ----------------------------------------------------------------
 * The response family measures what follows a change of the COMMAND.  This family changes the ROBOT: one launch adds a chosen
 * velocity step to the base of chosen environments between two simulator steps, and the recovery analysis turns a trace that
 * holds ONE such push under constant commands into fall, peak velocity error, recovery time, height drop, yaw-rate deviation and
 * integrated excess error per environment, reduced per group by the tables' fixed-order reduction.  The trace is the third
 * family's, its 24 channels unchanged.  (The reference's _push_robots draws a random planar velocity at a fixed episode
 * interval and REPLACES the base velocity with it; nothing about it is chosen per environment and nothing is measured.)
 *
 * go1eval_push(cfg, buf, stream): one launch, one thread per pushed environment k in [0, K), K = num_pushed.  It pushes
 *   environment env_ids[k]; env_ids == NULL means k itself and needs K == N (-8 otherwise, as go1eval_trace_record).  The four
 *   values of k are push[r * K + k] for the rows r (index = Go1PushRow): forward, left, up velocity step (m/s) and yaw-rate step
 *   (rad/s).  Forward and left are in the robot's HEADING FRAME (the world x-y plane turned by the robot's yaw); up and the yaw
 *   rate are about world z.  Every operation is an fp32 operation; 1e-6 is an fp32 constant; q = root_states rows 3..6 (xyzw):
 *     f = R(q) (1, 0, 0) by R(q) v = v + w t + u x t, u = q.xyz, t = 2 (u x v)      (the body's forward axis in the world)
 *     n = sqrtf(f.x^2 + f.y^2);  heading h = (f.x / n, f.y / n), or (1, 0) when n < 1e-6   (a robot that points straight up or down)
 *     row 7 += dv_forward * h.x - dv_left * h.y;   row 8 += dv_forward * h.y + dv_left * h.x;   row 9 += dv_up;   row 12 += dyaw
 *   There is no trigonometry on the device: a push direction becomes its cosine and sine on the host.  An environment whose four
 *   values all compare equal to zero is NOT WRITTEN (x + 0.0f turns -0.0f into +0.0f, and a zero push leaves every bit as it is).
 *   An id outside [0, N) is skipped.  With env_ids == NULL a wavefront's loads and stores of one row are one contiguous run.  Every
 *   element has one writer PROVIDED no id occurs twice; the kernel does not check that, nor that the table is finite: the host
 *   wrapper (go1eval_host.Go1Push) refuses both before the launch.
 *
 * go1eval_recovery(cfg, buf, stream): one launch, one thread per traced environment, a pure function of the trace.  rows = the
 *   recorded rows, p0 = push_row (the first row recorded AFTER the push: the state one simulator step after it), w = smooth,
 *   end = rows.  Refused before the launch (-11) unless 1 <= pre <= p0, p0 < rows, 1 <= w <= pre + 1, 1 <= hold <= rows - p0,
 *   dt > 0 and band >= 0.  band is an absolute velocity error in m/s.  c[t] below is channel c of this environment at row t; every
 *   operation that is not marked fp64 is an fp32 operation on fp32 values.
 *   1. Status (index = Go1RecoveryStatus), the first rule that applies:
 *      1  some row in [p0 - pre, p0) has channel 11 != 0: the baseline is spoiled (a NaN, the trace of an id outside [0, N), is != 0)
 *      3  some row in [p0, end) has channel 11 != 0: the robot fell (or timed out) after the push
 *      2  channel 6, 7 or 8 has a row t in [p0 - pre, end) with c[t] != c[p0 - pre]: the command was not held
 *      0  otherwise.
 *      The fall is tested BEFORE the command: the row of a reset carries the reset's own command draw, so a fallen robot's commands
 *      always moved as well.  Status 1 and 2: all eight values are NaN.  Status 3: fell = 1 and the other seven are NaN.
 *   2. Signals per row t: e[t] = sqrtf(dx * dx + dy * dy) with dx = c0[t] - c6[t], dy = c1[t] - c7[t] (the planar velocity error);
 *      z[t] = c3[t] (base height); y[t] = c2[t] - c8[t] (the yaw-rate error).  For x in {e, z, y}:
 *      xs(t) = the mean of x over rows t - w + 1 .. t: added in an fp64 carry in ascending row order, divided by (double)w in fp64,
 *              rounded to fp32 once (the response's box filter);
 *      xb    = the mean of the RAW x over rows [p0 - pre, p0): the same carry, divided by (double)pre, rounded to fp32 once.
 *   3. Eight values (index = Go1RecoveryMetric), t over [p0, end) in ascending order:
 *      fell            0 (1 with status 3)
 *      peak_vel_err    es(t_peak) - eb, t_peak = the FIRST t at which es(t) is largest (es(t) > every earlier es)
 *      peak_time       (float)(t_peak - p0 + 1) * dt
 *      recovered       t_s starts at p0 and becomes t + 1 whenever es(t) - eb > band; 1 if t_s <= end - hold, else 0
 *      recovery_time   (float)(t_s - p0) * dt; NaN when not recovered; 0 when the signal never left the band
 *      height_drop     zb - the fold of fminf over zs(t), starting from +inf
 *      yaw_rate_dev    the fold of fmaxf over |ys(t) - yb|, starting from 0
 *      iae_excess      dt * the sum of the RAW e[t] - eb: the fp32 differences added in an fp64 carry, multiplied by (double)dt in
 *                      fp64, rounded to fp32 once.  Negative when the robot tracked better after the push than before it.
 *      The box filter delays xs by about (w - 1) / 2 rows, and that delay is inside peak_time and recovery_time.  Roll and pitch
 *      are no trace channel and are not measured; a fall is seen through the reset flag.
 *   4. Outputs: values[m * K + k] (fp32) for value m, and status[k] (int32).  One writer each, no atomics.
 *
 * go1eval_recovery_reduce(cfg, buf, stream): results[num_groups][GO1EVAL_NUM_RECOVERY + 1][GO1EVAL_NUM_FIELDS] over the traced
 *   environments with group[k] == g.  Row m is the metric row of go1eval_reduce over accumulators that folded the one value
 *   values[m][k], exactly as go1eval_response_reduce forms its rows (a NaN counts in nonfinite).  The last row of a group
 *   (index = Go1RecoveryGroupField): traced environments, environments with status 0, 1, 2, 3, then 0 (sums in the same fixed order).
 *
 * ---- terrain traversal (fifth kernel family; index = Go1TerrainMetric) -------------------------------------------------------------
 * The four families above measure on flat ground.  This one measures a policy on the tile grid of a generated terrain: whether a
 * robot LEAVES THE TILE it was placed on (the criterion of legged_gym-style terrain curricula), falls or times out first, how
 * far it gets, and, while it is under way, how high its base and its feet are ABOVE THE GROUND THEY ARE OVER, how often a foot
 * is pushed sideways and how often a penalised body touches something.  Accumulators, folding rule and reduction are the tables'.
 *
 * Height sample h(x, y): the simulator's own convention for "the ground under a point" (the reference's _get_heights), NOT the
 * bilinear contact surface and not the vertical walls of a trimesh terrain.  Every operation is an fp32 operation:
 *   x or y not finite: h = NaN, tested first: nothing below is evaluated for such a point.
 *   qx = (x + hf_border) / hf_hscale (one add, one division);  px = 0 if not qx > 0, hf_rows - 2 if qx > (float)(hf_rows - 2), else
 *   (long)qx: the truncated index clamped to [0, hf_rows - 2].  The clamp is applied in fp32 BEFORE the conversion: the result
 *   is that of converting first for every qx a long can hold, and no value outside that range is ever converted.
 *   py likewise from y and hf_cols.  h = (float)min(s[px][py], s[px + 1][py], s[px][py + 1]) * hf_vscale: the minimum of three
 *   int16 samples of height_samples ([hf_rows][hf_cols], row-major), converted to fp32, one multiply.  height_samples == NULL: h = 0
 *   for finite x, y (the plane).
 *
 * A foot f is as in the behaviour table (body 4 + 4 f of contact_forces, rows 3 f .. 3 f + 2 of foot_positions); (F_x, F_y, F_z)
 * of body b are rows 3 b .. 3 b + 2 of contact_forces; cmd[k] = commands[k][e]; a_f = z_f - h(x_f, y_f) (one subtraction) is the
 * height of foot f above the ground under it.  Five per-step metrics (fp32; a sum over the feet adds its fp32 terms in an fp64
 * carry, feet in ascending order, and rounds to fp32 once; there is no rounding freedom: same inputs, same bits):
 *   base_height_terrain     root_states[2] - h(root_states[0], root_states[1])
 *   feet_clearance_terrain  sum over the feet of ((cmd[9] * ph + 0.02) - a_f)^2 * (1 - desired_contact_states[f]), ph as in the
 *                           behaviour table's feet_clearance: that expression with z_f replaced by a_f
 *   swing_foot_height       the mean over the feet with desired_contact_states[f] <= 0.5 of a_f - GO1EVAL_FOOT_RADIUS: the fp32
 *                           terms in an fp64 carry, divided by the number of such feet in fp64, rounded to fp32 once.  No such
 *                           foot: NOTHING is folded for this metric on this step (neither count nor nonfinite moves).
 *   stumble                 1 if some foot has sqrtf(F_x * F_x + F_y * F_y) > 5.0f * fabsf(F_z), else 0: legged_gym's feet-stumble
 *                           criterion, a foot pushed sideways by a riser.  The REFERENCE HAS NO SUCH TERM.
 *   collision               the number of bodies b in [0, 17) with bit b set in penalised_body_mask and
 *                           sqrtf((F_x * F_x + F_y * F_y) + F_z * F_z) > 0.1f, as a float (the reference's _reward_collision).  Bits
 *                           17 .. 31 of the mask are ignored.
 *
 * Per environment the family carries status (Go1TerrainStatus), steps, end_step and max_dist.  An environment is measured for
 * its FIRST EPISODE ON ITS HOME TILE only: once its status is not RUNNING no later launch reads or writes anything of it.
 * go1eval_terrain_accumulate, per environment e (one thread each, no atomics, no LDS; every word has one writer), in this order:
 *   1. status[e] != RUNNING: return.
 *   2. reset_buf[e] != 0: status[e] = TIMED_OUT if time_out_buf[e] != 0, else FELL; end_step[e] = steps[e] + 1.  Nothing else: the
 *      buffers already hold the new episode's pose (steps and max_dist stay as the last measured step left them).
 *   3. steps[e] += 1.  dx = root_states[0] - env_origins[0], dy = root_states[1] - env_origins[1] (fp32);
 *      max_dist[e] = fmaxf(max_dist[e], sqrtf(dx * dx + dy * dy)).  If fabsf(dx) > tile_length / 2 or fabsf(dy) > tile_width / 2:
 *      status[e] = TRAVERSED, end_step[e] = steps[e], and nothing is folded.  The comparison is strict (a robot exactly on the edge
 *      is still on its tile), and a dx or dy that is not finite does not traverse: both are tested for finiteness first (a NaN
 *      would fail the comparisons by itself, an infinity would not; fmaxf drops a NaN and keeps an infinity in max_dist).
 *   4. episode_length_buf[e] <= warmup_steps: nothing more.
 *   5. the five per-step metrics are folded in the order of Go1TerrainMetric by the folding rule of go1eval_accumulate: a
 *      non-finite value counts in nonfinite and enters nothing else.
 * go1eval_terrain_clear: accumulators as go1eval_clear; status = RUNNING, steps = 0, end_step = 0, max_dist = 0.
 * go1eval_terrain_reduce: results[num_groups][GO1EVAL_NUM_TERRAIN + GO1EVAL_NUM_OUTCOME + 1][GO1EVAL_NUM_FIELDS].
 *   Rows 0 .. 4: the metric rows of go1eval_reduce (the same device function, the same fixed combination order).
 *   Rows 5 .. 8 (index = GO1EVAL_NUM_TERRAIN + Go1TerrainOutcome): the metric row over accumulators that folded ONE fp32 value per
 *   environment, exactly as go1eval_recovery_reduce forms its rows (a NaN counts in nonfinite):
 *     traversed   1 if TRAVERSED, 0 if FELL or TIMED_OUT, NaN while RUNNING (the window was too short to decide)
 *     fell        1 if FELL, 0 if TRAVERSED or TIMED_OUT, NaN while RUNNING
 *     distance    max_dist[e]: the largest planar distance from the tile's origin over the measured steps
 *     end_time    (float)end_step[e] * dt (one fp32 multiply), NaN while RUNNING
 *   Row 9 (index = Go1TerrainGroupField): environments, environments with status 0, 1, 2, 3 (sums in the same fixed order), then
 *   success_rate = traversed / (traversed + fell + timed_out), one fp64 division, NaN when the denominator is 0.
 * Refused before any launch: -1 no config, no buffers or num_envs <= 0;  -2 an accumulator or a state array is missing;  -3 an
 *   input is missing (height_samples may be NULL);  -5 no group, no table or num_groups <= 0;  -12 the geometry: hf_rows < 2 or
 *   hf_cols < 2 with a height field, hf_hscale <= 0, tile_length <= 0, tile_width <= 0 or dt <= 0 (a NaN is refused as well).
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

/* ---- the behaviour table ---------------------------------------------------------------------------------------------------- */
#define GO1EVAL_NUM_BEHAVIOUR 10
#define GO1EVAL_CONTACT_FORCE 1.0    /* N: a foot is in contact when its F_z exceeds this (the reference's threshold) */
#define GO1EVAL_FOOT_RADIUS 0.02     /* m: the reference's offset between a foot's origin and its sole */

enum Go1BehaviourMetric {
  GO1EVAL_CONTACT_MATCH = 0, GO1EVAL_BODY_HEIGHT_ERR = 1, GO1EVAL_ORIENTATION_ERR = 2, GO1EVAL_FEET_CLEARANCE = 3,
  GO1EVAL_RAIBERT_HEURISTIC = 4, GO1EVAL_FEET_SLIP = 5, GO1EVAL_ACTION_RATE = 6, GO1EVAL_STEP_FREQUENCY_ERR = 7,
  GO1EVAL_DUTY_FACTOR_ERR = 8, GO1EVAL_SWING_HEIGHT_ERR = 9
};

typedef struct Go1BehaviourConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t num_commands;        /* the configuration's command count: below 13 / 14 the stance width / length are the defaults */
  int32_t num_height_points;   /* rows of measured_heights (ignored when it is NULL) */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing and break every stride */
  int32_t num_groups;          /* G of the result table */
  float dt;                    /* s, the policy step (simulation step x decimation) */
  float base_height_target;    /* m, the reference's rewards.base_height_target */
} Go1BehaviourConfig;

typedef struct Go1BehaviourBuffers {
  /* read by go1eval_behaviour_accumulate */
  const float* commands;                /* [>= max(12, min(num_commands, 14))][N] */
  const float* root_states;             /* [13][N]; rows 0..6 are read */
  const float* measured_heights;        /* [num_height_points][N] or NULL (the ground is 0) */
  const float* contact_forces;          /* [17 * 3][N]; the feet are bodies 4, 8, 12, 16 */
  const float* foot_positions;          /* [4 * 3][N], world frame */
  const float* foot_velocities;         /* [4 * 3][N], world frame */
  const float* desired_contact_states;  /* [4][N] */
  const float* foot_indices;            /* [4][N] */
  const float* last_actions;            /* [12][N]: this step's action */
  const float* last_last_actions;       /* [12][N]: the previous step's */
  const uint8_t* reset_buf;             /* [N] */
  const int32_t* episode_length_buf;    /* [N] */
  /* accumulators, [GO1EVAL_NUM_BEHAVIOUR][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* per-foot stride state, [4][N] */
  uint8_t* prev_contact;
  int32_t* stride_steps;
  int32_t* stance_steps;
  float* swing_peak;
  /* go1eval_behaviour_reduce */
  const int32_t* group;                 /* [N] */
  double* results;                      /* [num_groups][GO1EVAL_NUM_BEHAVIOUR][GO1EVAL_NUM_FIELDS] */
} Go1BehaviourBuffers;

/* empty accumulators and unknown stride state.  One launch. */
int go1eval_behaviour_clear(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf, void* stream);

/* after a simulator step: fold the step into the accumulators and advance the stride state.  One launch, one thread per environment.
 * num_commands < 12 (the commanded pitch and roll are rows 10, 11) or dt <= 0 is refused before the launch. */
int go1eval_behaviour_accumulate(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf, void* stream);

/* at the end: the result table from the accumulators (which it leaves as they are).  One launch. */
int go1eval_behaviour_reduce(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf, void* stream);

/* ---- the trace and the step response ------------------------------------------------------------------------------------------ */
#define GO1EVAL_NUM_TRACE 24
#define GO1EVAL_NUM_RESPONSE 7
#define GO1EVAL_MAX_SIGNALS 8

enum Go1TraceChannel {
  GO1TRACE_LIN_VEL_X = 0, GO1TRACE_LIN_VEL_Y = 1, GO1TRACE_ANG_VEL_YAW = 2, GO1TRACE_BASE_HEIGHT = 3, GO1TRACE_CONTACT_MATCH = 4,
  GO1TRACE_POWER_CONSUMPTION = 5, GO1TRACE_CMD_LIN_VEL_X = 6, GO1TRACE_CMD_LIN_VEL_Y = 7, GO1TRACE_CMD_ANG_VEL_YAW = 8,
  GO1TRACE_CMD_BASE_HEIGHT = 9, GO1TRACE_MAX_TORQUES = 10, GO1TRACE_RESET = 11, GO1TRACE_DOF_POS_0 = 12, GO1TRACE_DOF_POS_1 = 13,
  GO1TRACE_DOF_POS_2 = 14, GO1TRACE_DOF_POS_3 = 15, GO1TRACE_DOF_POS_4 = 16, GO1TRACE_DOF_POS_5 = 17, GO1TRACE_DOF_POS_6 = 18,
  GO1TRACE_DOF_POS_7 = 19, GO1TRACE_DOF_POS_8 = 20, GO1TRACE_DOF_POS_9 = 21, GO1TRACE_DOF_POS_10 = 22, GO1TRACE_DOF_POS_11 = 23
};
enum Go1ResponseMetric {
  GO1RESPONSE_REACHED = 0, GO1RESPONSE_RISE_TIME = 1, GO1RESPONSE_OVERSHOOT = 2, GO1RESPONSE_SETTLED = 3, GO1RESPONSE_SETTLING_TIME = 4,
  GO1RESPONSE_STEADY_STATE_ERR = 5, GO1RESPONSE_IAE = 6
};
/* columns of a group's own row (row num_signals * GO1EVAL_NUM_RESPONSE) of the response table */
enum Go1ResponseGroupField { GO1RESPONSE_G_ENVS = 0, GO1RESPONSE_G_OK = 1, GO1RESPONSE_G_RESET = 2, GO1RESPONSE_G_NOT_HELD = 3 };

typedef struct Go1TraceConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t num_traced;          /* K: traced environments (== num_envs when env_ids is NULL) */
  int32_t capacity;            /* rows the trace buffer holds */
  int32_t num_height_points;   /* rows of measured_heights (ignored when it is NULL) */
  float base_height_target;    /* m, the reference's rewards.base_height_target */
} Go1TraceConfig;

typedef struct Go1TraceBuffers {
  const float* base_lin_vel;            /* [3][N] */
  const float* base_ang_vel;            /* [3][N] */
  const float* commands;                /* [>= 4][N] */
  const float* root_states;             /* [13][N]; row 2 is read */
  const float* measured_heights;        /* [num_height_points][N] or NULL (the ground is 0) */
  const float* contact_forces;          /* [17 * 3][N]; the feet are bodies 4, 8, 12, 16 */
  const float* desired_contact_states;  /* [4][N] */
  const float* torques;                 /* [12][N] */
  const float* dof_vel;                 /* [12][N] */
  const float* dof_pos;                 /* [12][N] */
  const uint8_t* reset_buf;             /* [N] */
  const int32_t* env_ids;               /* [K] or NULL (environment k itself) */
  float* trace;                         /* [capacity][GO1EVAL_NUM_TRACE][K] */
} Go1TraceBuffers;

typedef struct Go1ResponseSignal {
  int32_t y_channel;           /* the measured channel */
  int32_t r_channel;           /* the channel that carries its target, or < 0: fixed_target */
  float fixed_target;          /* the target when r_channel < 0 */
  float fixed_scale;           /* > 0: the scale D; otherwise D = |r1 - r0| */
} Go1ResponseSignal;

typedef struct Go1ResponseConfig {
  int32_t num_traced;          /* K of the trace */
  int32_t rows;                /* recorded rows (<= the trace's capacity) */
  int32_t switch_row;          /* s0: the first row recorded after the command changed */
  int32_t pre;                 /* rows before s0 that the status rules cover */
  int32_t smooth;              /* w: rows of the box filter */
  int32_t hold;                /* rows at the end that have to stay inside the band for `settled` */
  int32_t tail;                /* rows at the end that steady_state_err averages */
  float band;                  /* the settling band, as a fraction of D */
  float dt;                    /* s, the policy step */
  int32_t num_signals;         /* S <= GO1EVAL_MAX_SIGNALS */
  int32_t num_groups;          /* G of the result table (go1eval_response_reduce) */
  Go1ResponseSignal signal[GO1EVAL_MAX_SIGNALS];
} Go1ResponseConfig;

typedef struct Go1ResponseBuffers {
  const float* trace;          /* [rows][GO1EVAL_NUM_TRACE][K] */
  float* values;               /* [num_signals][GO1EVAL_NUM_RESPONSE][K] */
  int32_t* status;             /* [K] */
  /* go1eval_response_reduce */
  const int32_t* group;        /* [K] */
  double* results;             /* [num_groups][num_signals * GO1EVAL_NUM_RESPONSE + 1][GO1EVAL_NUM_FIELDS] */
} Go1ResponseBuffers;

/* after a simulator step: row `row` of the trace.  One launch, one thread per traced environment.  row outside [0, capacity): -7,
 * nothing is written.  env_ids == NULL with num_traced != num_envs: -8. */
int go1eval_trace_record(const Go1TraceConfig* cfg, const Go1TraceBuffers* buf, int32_t row, void* stream);

/* the step response of every traced environment from the trace.  One launch.  Window refused: -9; signal refused: -10. */
int go1eval_response(const Go1ResponseConfig* cfg, const Go1ResponseBuffers* buf, void* stream);

/* the response table from values and status (which it leaves as they are).  One launch. */
int go1eval_response_reduce(const Go1ResponseConfig* cfg, const Go1ResponseBuffers* buf, void* stream);

/* ---- the push and the disturbance recovery ------------------------------------------------------------------------------------ */
#define GO1EVAL_NUM_PUSH 4
#define GO1EVAL_NUM_RECOVERY 8

/* rows of the push table */
enum Go1PushRow { GO1PUSH_FORWARD = 0, GO1PUSH_LEFT = 1, GO1PUSH_UP = 2, GO1PUSH_YAW_RATE = 3 };
enum Go1RecoveryMetric {
  GO1RECOVERY_FELL = 0, GO1RECOVERY_PEAK_VEL_ERR = 1, GO1RECOVERY_PEAK_TIME = 2, GO1RECOVERY_RECOVERED = 3, GO1RECOVERY_RECOVERY_TIME = 4,
  GO1RECOVERY_HEIGHT_DROP = 5, GO1RECOVERY_YAW_RATE_DEV = 6, GO1RECOVERY_IAE_EXCESS = 7
};
enum Go1RecoveryStatus { GO1RECOVERY_S_OK = 0, GO1RECOVERY_S_BASELINE_RESET = 1, GO1RECOVERY_S_NOT_HELD = 2, GO1RECOVERY_S_FELL = 3 };
/* columns of a group's own row (row GO1EVAL_NUM_RECOVERY) of the recovery table */
enum Go1RecoveryGroupField {
  GO1RECOVERY_G_ENVS = 0, GO1RECOVERY_G_OK = 1, GO1RECOVERY_G_BASELINE_RESET = 2, GO1RECOVERY_G_NOT_HELD = 3, GO1RECOVERY_G_FELL = 4
};

typedef struct Go1PushConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t num_pushed;          /* K: pushed environments (== num_envs when env_ids is NULL) */
} Go1PushConfig;

typedef struct Go1PushBuffers {
  float* root_states;          /* [13][N]; rows 3..6 are read, rows 7, 8, 9 and 12 are read and written */
  const int32_t* env_ids;      /* [K] or NULL (environment k itself); no id twice */
  const float* push;           /* [GO1EVAL_NUM_PUSH][K], finite */
} Go1PushBuffers;

typedef struct Go1RecoveryConfig {
  int32_t num_traced;          /* K of the trace */
  int32_t rows;                /* recorded rows (<= the trace's capacity) */
  int32_t push_row;            /* p0: the first row recorded after the push */
  int32_t pre;                 /* rows before p0: the baseline, and what the status rules cover */
  int32_t smooth;              /* w: rows of the box filter */
  int32_t hold;                /* rows at the end that have to stay inside the band for `recovered` */
  float band;                  /* the recovery band: m/s of velocity error above the baseline */
  float dt;                    /* s, the policy step */
  int32_t num_groups;          /* G of the result table (go1eval_recovery_reduce) */
} Go1RecoveryConfig;

typedef struct Go1RecoveryBuffers {
  const float* trace;          /* [rows][GO1EVAL_NUM_TRACE][K] */
  float* values;               /* [GO1EVAL_NUM_RECOVERY][K] */
  int32_t* status;             /* [K] */
  /* go1eval_recovery_reduce */
  const int32_t* group;        /* [K] */
  double* results;             /* [num_groups][GO1EVAL_NUM_RECOVERY + 1][GO1EVAL_NUM_FIELDS] */
} Go1RecoveryBuffers;

/* between two simulator steps: add the table's velocity steps to the base of the pushed environments.  One launch, one thread per
 * pushed environment.  No root_states or no table, or num_pushed <= 0: -2.  env_ids == NULL with num_pushed != num_envs: -8. */
int go1eval_push(const Go1PushConfig* cfg, const Go1PushBuffers* buf, void* stream);

/* the recovery of every traced environment from the trace.  One launch.  No outputs: -2; no trace: -3; window refused: -11. */
int go1eval_recovery(const Go1RecoveryConfig* cfg, const Go1RecoveryBuffers* buf, void* stream);

/* the recovery table from values and status (which it leaves as they are).  One launch.  No group, no table or no groups: -5. */
int go1eval_recovery_reduce(const Go1RecoveryConfig* cfg, const Go1RecoveryBuffers* buf, void* stream);

/* ---- terrain traversal ------------------------------------------------------------------------------------------------------------ */
#define GO1EVAL_NUM_TERRAIN 5
#define GO1EVAL_NUM_OUTCOME 4
#define GO1EVAL_STUMBLE_RATIO 5.0    /* a foot stumbles when its horizontal contact force exceeds this many times its vertical one (legged_gym) */
#define GO1EVAL_COLLISION_FORCE 0.1  /* N: a penalised body collides when its contact force exceeds this (the reference's _reward_collision) */

enum Go1TerrainMetric {
  GO1TERRAIN_BASE_HEIGHT_TERRAIN = 0, GO1TERRAIN_FEET_CLEARANCE_TERRAIN = 1, GO1TERRAIN_SWING_FOOT_HEIGHT = 2, GO1TERRAIN_STUMBLE = 3,
  GO1TERRAIN_COLLISION = 4
};
enum Go1TerrainStatus { GO1TERRAIN_S_RUNNING = 0, GO1TERRAIN_S_TRAVERSED = 1, GO1TERRAIN_S_FELL = 2, GO1TERRAIN_S_TIMED_OUT = 3 };
/* rows GO1EVAL_NUM_TERRAIN + Go1TerrainOutcome of the terrain table */
enum Go1TerrainOutcome { GO1TERRAIN_O_TRAVERSED = 0, GO1TERRAIN_O_FELL = 1, GO1TERRAIN_O_DISTANCE = 2, GO1TERRAIN_O_END_TIME = 3 };
/* columns of a group's own row (row GO1EVAL_NUM_TERRAIN + GO1EVAL_NUM_OUTCOME) of the terrain table */
enum Go1TerrainGroupField {
  GO1TERRAIN_G_ENVS = 0, GO1TERRAIN_G_RUNNING = 1, GO1TERRAIN_G_TRAVERSED = 2, GO1TERRAIN_G_FELL = 3, GO1TERRAIN_G_TIMED_OUT = 4,
  GO1TERRAIN_G_SUCCESS_RATE = 5
};

typedef struct Go1TerrainConfig {
  int32_t num_envs;              /* N of the simulator's SoA buffers */
  int32_t warmup_steps;          /* steps with episode_length_buf <= warmup_steps fold no metric (status and distance still advance) */
  int32_t num_groups;            /* G of the result table */
  int32_t hf_rows;               /* the height field's samples along x (ignored when height_samples is NULL) */
  int32_t hf_cols;               /* and along y */
  uint32_t penalised_body_mask;  /* bit b: body b counts towards `collision` */
  float dt;                      /* s, the policy step: end_time = end_step * dt */
  float hf_hscale;               /* m per sample along x and y */
  float hf_vscale;               /* m per int16 unit */
  float hf_border;               /* m: the field starts at world (-hf_border, -hf_border) */
  float tile_length;             /* m: a tile's extent along x */
  float tile_width;              /* m: and along y */
} Go1TerrainConfig;

typedef struct Go1TerrainBuffers {
  /* read by go1eval_terrain_accumulate */
  const float* root_states;             /* [13][N]; rows 0..2 are read */
  const float* commands;                /* [>= 10][N]; row 9 is read */
  const float* contact_forces;          /* [17 * 3][N] */
  const float* foot_positions;          /* [4 * 3][N], world frame */
  const float* desired_contact_states;  /* [4][N] */
  const float* foot_indices;            /* [4][N] */
  const float* env_origins;             /* [3][N]; rows 0, 1: the centre of the environment's home tile */
  const int16_t* height_samples;        /* [hf_rows][hf_cols] or NULL (the plane: the ground is 0) */
  const uint8_t* reset_buf;             /* [N] */
  const uint8_t* time_out_buf;          /* [N] */
  const int32_t* episode_length_buf;    /* [N] */
  /* accumulators, [GO1EVAL_NUM_TERRAIN][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* per-environment state, [N] */
  uint8_t* status;                      /* Go1TerrainStatus */
  uint32_t* steps;                      /* measured steps */
  uint32_t* end_step;                   /* the step at which the status left RUNNING (1 = the first step after the clear) */
  float* max_dist;                      /* m */
  /* go1eval_terrain_reduce */
  const int32_t* group;                 /* [N] */
  double* results;                      /* [num_groups][GO1EVAL_NUM_TERRAIN + GO1EVAL_NUM_OUTCOME + 1][GO1EVAL_NUM_FIELDS] */
} Go1TerrainBuffers;

/* empty accumulators, every environment RUNNING at step 0.  One launch. */
int go1eval_terrain_clear(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf, void* stream);

/* after a simulator step: advance every RUNNING environment and fold its step.  One launch, one thread per environment.
 * Geometry refused: -12. */
int go1eval_terrain_accumulate(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf, void* stream);

/* at the end: the result table from the accumulators and the state (which it leaves as they are).  One launch.  dt <= 0: -12. */
int go1eval_terrain_reduce(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf, void* stream);

/* ---- per-joint actuator usage (sixth kernel family; index = Go1JointMetric) ---------------------------------------------------------
 * The five families above look at the robot as a whole; the only joint-level figure they give is max_torques, one scalar per robot.
 * This family measures every one of the twelve joints by itself: how hard and how fast its motor is driven, how often it sits on the
 * torque clip or on the URDF's speed limit, how much of its power is braking, how far it leans on its soft position limits, and where in
 * the torque-speed plane it operates (a histogram).  Accumulators, folding rule and metric-row reduction are the tables'.  The
 * reference's per-joint reward terms (_reward_torques, _reward_dof_vel, _reward_dof_acc, _reward_dof_pos_limits) are the sums over the
 * joints of rows torque_sq, vel_sq, acc_sq and pos_limit_excess.
 *
 * Joint j of environment e: tau = torques[j][e], qd = dof_vel[j][e], q = dof_pos[j][e], prev = prev_dof_vel[j][e].  Ten values per joint
 * and step, every operation an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off: a
 * rounding after every multiply, add and division):
 *   torque_abs        fabsf(tau)
 *   torque_sq         tau * tau
 *   vel_abs           fabsf(qd)
 *   vel_sq            qd * qd
 *   acc_sq            d * d with d = (prev - qd) / dt  (one subtraction, one division)
 *   power_pos         p > 0 ? p : 0 with p = tau * qd: fmaxf(p, 0) with the sign of a zero fixed (+0; fmaxf leaves it open)
 *   power_neg         p < 0 ? -p : 0: braking, fmaxf(-p, 0) likewise.  As with fmaxf a NaN product folds 0 into both power rows (the NaN
 *                     itself is counted in the nonfinite of torque_abs or vel_abs); an infinite product is counted in nonfinite here.
 *   pos_limit_excess  (lo < 0 ? -lo : 0) + (hi > 0 ? hi : 0) with lo = q - pos_lower[j], hi = q - pos_upper[j]: the reference's
 *                     -min(lo, 0) + max(hi, 0), one add.  A NaN q gives NaN, as the reference's clip hands it on.
 *   torque_saturated  1 if fabsf(tau) >= soft_torque_limit * torque_limit[j] (one multiply), else 0: the limit the SIMULATOR clips at, not
 *                     a motor model.  A NaN compares false: 0.
 *   vel_saturated     1 if fabsf(qd) >= soft_vel_limit * vel_limit[j], else 0
 *
 * The torque-speed histogram of a joint has GO1JOINT_TAU_BINS x GO1JOINT_VEL_BINS cells.  For x with limit L (tau with torque_limit[j],
 * qd with vel_limit[j]; the soft factors play no part) the bin is b = floorf((x / L + 1.0f) * 4.0f), clamped to [0, 7] AS A FLOAT and
 * only then converted to an integer (the terrain family's rule: no value outside an int's range is ever converted).  So x = -L lands
 * in bin 0, x = 0 (of either sign) in bin 4, x >= L in bin 7 and x < -L in bin 0; bin k covers [L (k / 4 - 1), L ((k + 1) / 4 - 1)).
 * (The edges are those of the fp32 expression: x / L + 1 is rounded, so a value within an ulp of 1 of an edge may count in the bin beside it.)
 * The cell is tau_bin * GO1JOINT_VEL_BINS + vel_bin.  A sample enters the histogram on the steps that fold metrics, and only when
 * both tau and qd are finite.
 *
 * go1eval_joint_accumulate: one thread per (joint, environment), no atomics, no LDS; every word has one writer.  The launch is
 * one-dimensional: 12 * ceil(N / 256) blocks of 256 threads, block k works on joint k / ceil(N / 256) and its lanes on consecutive
 * environments, so a joint's limits are uniform per block and every load and store of a row is one contiguous run over a wavefront (the
 * one exception: the histogram word, whose cell differs from lane to lane).  Per (j, e), in this order:
 *   1. the thread of joint 0: steps[e] += 1, and resets[e] += 1 if reset_buf[e] != 0.
 *   2. reset_buf[e] != 0: the step reset the environment; no metric and no histogram sample is folded.
 *   3. otherwise, episode_length_buf[e] <= warmup_steps: nothing is folded (the step counted in steps only).
 *   4. otherwise the ten values are folded in the order of Go1JointMetric into row j * GO1EVAL_NUM_JOINT + metric by the folding rule of
 *      go1eval_accumulate (a non-finite value counts in nonfinite and enters nothing else), then the histogram sample.
 *   5. on EVERY step, folded or not: prev_dof_vel[j][e] = qd.
 *   The previous velocity is the family's own copy: go1eval_joint_clear takes it from dof_vel, and every accumulate leaves the current
 *   dof_vel there.  After a reset step that is the post-reset velocity, which the simulator sets to 0: what the reference's
 *   last_dof_vel[env_ids] = 0 gives.  (The simulator's own last_dof_vel is no use: after a step it already equals dof_vel.)
 * go1eval_joint_clear: one launch of the same shape: accumulators as go1eval_clear, the histogram 0, steps = resets = 0,
 *   prev_dof_vel = dof_vel.
 * go1eval_joint_reduce: ONE launch of GO1EVAL_REDUCE_THREADS-thread workgroups: num_groups * (12 * GO1EVAL_NUM_JOINT + 1) of them
 *   write results[num_groups][12 * GO1EVAL_NUM_JOINT + 1][GO1EVAL_NUM_FIELDS], then num_groups * 12 write
 *   hist_results[num_groups][12][GO1JOINT_TAU_BINS][GO1JOINT_VEL_BINS].
 *   Rows j * GO1EVAL_NUM_JOINT + metric: the metric rows of go1eval_reduce (the same device function, the same fixed combination order).
 *   The last row of a group (index = Go1JointGroupField): environments, steps (sum of steps[e]), resets, then 0, 0, 0 (sums in the same
 *   fixed order).
 *   Histogram, one workgroup per (group, joint): thread t owns cell t % 64 and adds hist[j][t % 64][e] of the group's environments
 *   e = t / 64, t / 64 + 4, t / 64 + 8, ... in ascending order as uint64; then a fixed tree over the four slices (thread t takes
 *   thread t + 128, then thread t + 64) and threads 0 .. 63 write their cell.
 * Refused before any launch: -1 no config, no buffers or num_envs <= 0;  -2 an accumulator, the histogram or a state array is missing;
 *   -3 an input is missing (go1eval_joint_clear reads dof_vel only, go1eval_joint_reduce none);  -5 no group, no table, no histogram
 *   table or num_groups <= 0 (go1eval_joint_reduce);  -12 (go1eval_joint_accumulate) dt, soft_torque_limit, soft_vel_limit, a
 *   torque_limit[j] or a vel_limit[j] that is not finite and positive, or a joint without pos_lower[j] <= pos_upper[j] (a NaN is refused).
 */
#define GO1EVAL_NUM_JOINT 10
#define GO1JOINT_TAU_BINS 8
#define GO1JOINT_VEL_BINS 8

enum Go1JointMetric {
  GO1JOINT_TORQUE_ABS = 0, GO1JOINT_TORQUE_SQ = 1, GO1JOINT_VEL_ABS = 2, GO1JOINT_VEL_SQ = 3, GO1JOINT_ACC_SQ = 4, GO1JOINT_POWER_POS = 5,
  GO1JOINT_POWER_NEG = 6, GO1JOINT_POS_LIMIT_EXCESS = 7, GO1JOINT_TORQUE_SATURATED = 8, GO1JOINT_VEL_SATURATED = 9
};
/* columns of a group's own row (row 12 * GO1EVAL_NUM_JOINT) of the joint table */
enum Go1JointGroupField { GO1JOINT_G_ENVS = 0, GO1JOINT_G_STEPS = 1, GO1JOINT_G_RESETS = 2 };

typedef struct Go1JointConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing */
  int32_t num_groups;          /* G of the result tables */
  float dt;                    /* s, the policy step: acc_sq divides by it */
  float soft_torque_limit;     /* torque_saturated compares with soft_torque_limit * torque_limit[j] */
  float soft_vel_limit;        /* vel_saturated compares with soft_vel_limit * vel_limit[j] */
  float torque_limit[12];      /* N m: the limit the simulator clips the torque at; the histogram's torque scale */
  float vel_limit[12];         /* rad/s: the URDF's speed limit; the histogram's speed scale */
  float pos_lower[12];         /* rad: the simulator's dof_pos_soft_lower */
  float pos_upper[12];         /* rad: the simulator's dof_pos_soft_upper */
} Go1JointConfig;

typedef struct Go1JointBuffers {
  /* read by go1eval_joint_accumulate (go1eval_joint_clear reads dof_vel) */
  const float* torques;               /* [12][N] */
  const float* dof_vel;               /* [12][N] */
  const float* dof_pos;               /* [12][N] */
  const uint8_t* reset_buf;           /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* accumulators, [12 * GO1EVAL_NUM_JOINT][N]: row j * GO1EVAL_NUM_JOINT + metric */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  float* prev_dof_vel;                /* [12][N] */
  uint32_t* steps;                    /* [N]: accumulate launches since the clear */
  uint32_t* resets;                   /* [N]: of those, the steps that reset the environment */
  uint32_t* hist;                     /* [12][GO1JOINT_TAU_BINS * GO1JOINT_VEL_BINS][N] */
  /* go1eval_joint_reduce */
  const int32_t* group;               /* [N] */
  double* results;                    /* [num_groups][12 * GO1EVAL_NUM_JOINT + 1][GO1EVAL_NUM_FIELDS] */
  uint64_t* hist_results;             /* [num_groups][12][GO1JOINT_TAU_BINS][GO1JOINT_VEL_BINS] */
} Go1JointBuffers;

/* empty accumulators and histogram, prev_dof_vel = dof_vel.  One launch, one thread per (joint, environment). */
int go1eval_joint_clear(const Go1JointConfig* cfg, const Go1JointBuffers* buf, void* stream);

/* after a simulator step: fold the step of every joint.  One launch, one thread per (joint, environment).  Limits refused: -12. */
int go1eval_joint_accumulate(const Go1JointConfig* cfg, const Go1JointBuffers* buf, void* stream);

/* at the end: both result tables from the accumulators and the histogram (which it leaves as they are).  One launch. */
int go1eval_joint_reduce(const Go1JointConfig* cfg, const Go1JointBuffers* buf, void* stream);

/* "go1eval <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1eval_version(void);

#ifdef __cplusplus
}
#endif

#endif
