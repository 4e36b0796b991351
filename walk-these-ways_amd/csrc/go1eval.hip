// go1eval.hip — evaluation metrics of a policy rollout on the device (include/go1eval.h), gfx950.
//
// eval_accumulate_kernel: one thread per environment.  Every input is a row of an SoA buffer ([k][N]), so the 64 lanes of a
// wavefront read 64 consecutive floats (256 contiguous bytes) per load, and the accumulators ([metric][N]) are read and written
// the same way.  Each accumulator element has one writer: no atomics, no cross-lane traffic, nothing depends on scheduling.
// eval_reduce_kernel: one workgroup per (group, row of the result table).  Thread t combines environments t, t + T, ... in
// ascending order in fp64, then a binary tree in LDS with a fixed shape; thread 0 writes the row with vector stores.
// tests/eval_ref.py restates both in fp64 numpy from the header's text.
// behaviour_accumulate_kernel / behaviour_reduce_kernel: the second table (gait and behaviour tracking), the same shapes: one
// thread per environment that also carries the per-foot stride state ([4][N], one writer per word), and the metric-row reduction
// shared with eval_reduce_kernel (reduce_metric_row).  tests/behaviour_ref.py is their fp64 model.
// trace_record_kernel / response_kernel / response_reduce_kernel: the trace and the step response, the same shapes again: one
// thread per traced environment; a channel of a trace row is [K] consecutive floats, so both the stores of the record and the
// loads of the analysis (sequential over the rows per thread) are contiguous across a wavefront.  tests/response_ref.py is the model.
// push_kernel / recovery_kernel / recovery_reduce_kernel: the push and the disturbance recovery: one thread per pushed environment
// that adds a velocity step to its rows of root_states, and the response's shapes for the analysis of the trace that follows
// (the same loads, the same reduction through reduce_metric_row and status_row).  tests/recovery_ref.py is the model.
// terrain_accumulate_kernel / terrain_reduce_kernel: terrain traversal, the tables' shapes once more: one thread per environment
// that carries its status, step count and distance ([N], one writer per word) and reads fifteen int16 samples of the height field
// under its base and feet, the family's only scattered loads, issued as one batch; the reduction goes through reduce_metric_row
// (metric rows, and outcome rows over one computed value per environment) and status_row.  tests/terrain_ref.py is the model.
// joint_accumulate_kernel / joint_reduce_kernel: per-joint actuator usage: one thread per (joint, environment) in a one-dimensional
// launch whose blocks each belong to one joint, so the joint's limits are uniform per block and every row access is a contiguous run
// (the histogram word alone is scattered); metric rows through reduce_metric_row, the histogram by its own uint64 sums.  tests/joint_ref.py.
//
// What the six families share with the foot and trunk libraries is written once in go1_tables.h: Args, Row, row_thread, fold and
// clear_rows (the six accumulators of a metric row), tree_reduce, group_sums and reduce_metric_row (the fixed-order reduction), and
// the entry points' env_grid, row_grid, table_grid, launch, has_accumulators, has_table and positive.  What only these families use
// is in the first namespace below: TraceArgs (TraceAt is the trace's Row), Once (one fp32 value per member seen as accumulators that
// folded it once), status_row and values_table_row (the tables of the response and the recovery), and the quaternion helpers.  What
// a family validates beyond the shared checks stays with the family, in the header's order of codes.
#include "../../include/go1eval.h"
#include "go1_tables.h"

namespace {

constexpr int NM = GO1EVAL_NUM_METRICS;
GO1_TABLES_MATCH(GO1EVAL);

using EvalArgs = Args<Go1EvalConfig, Go1EvalBuffers>;
using BehaviourArgs = Args<Go1BehaviourConfig, Go1BehaviourBuffers>;
using ResponseArgs = Args<Go1ResponseConfig, Go1ResponseBuffers>;
using PushArgs = Args<Go1PushConfig, Go1PushBuffers>;
using RecoveryArgs = Args<Go1RecoveryConfig, Go1RecoveryBuffers>;
using TerrainArgs = Args<Go1TerrainConfig, Go1TerrainBuffers>;
using JointArgs = Args<Go1JointConfig, Go1JointBuffers>;
struct TraceArgs {
  Go1TraceConfig c;
  Go1TraceBuffers b;
  int row;
};

// one fp32 value per member, value(i), seen as the accumulators of a member that folded the one value: what reduce_metric_row reads
template <class V>
struct Once {
  struct Count { V v; __device__ uint32_t operator[](size_t i) const { return isfinite(v(i)) ? 1u : 0u; } };
  struct Nonfinite { V v; __device__ uint32_t operator[](size_t i) const { return isfinite(v(i)) ? 0u : 1u; } };
  struct Sum { V v; __device__ double operator[](size_t i) const { const float x = v(i); return isfinite(x) ? (double)x : 0.0; } };
  struct Sumsq { V v; __device__ double operator[](size_t i) const { const float x = v(i); return isfinite(x) ? (double)x * (double)x : 0.0; } };
  struct Value { V v; __device__ float operator[](size_t i) const { return v(i); } };
  const int32_t* group;
  Count count; Nonfinite nonfinite; Sum sum; Sumsq sumsq; Value min, max;
};
template <class V>
__device__ __forceinline__ Once<V> once(const int32_t* group, V v) { return {group, {v}, {v}, {v}, {v}, {v}, {v}}; }
struct Stored { const float* v; __device__ float operator()(size_t i) const { return v[i]; } };       // values[s][m][K], as written

// the last row of a group of the response, recovery and terrain tables, by one workgroup of RT threads in reduce_metric_row's
// combination order: members, members with status 0, 1, 2, 3, then 0 (the response knows no status 3: its count is 0)
template <class Status>
__device__ __forceinline__ void status_row(const Status* status, const int32_t* group, int g, int K, double (*lds)[RT], double* out) {
  group_sums<5>(group, g, K, lds, [status](int e, double* a) {
    const int st = (int)status[e];
    a[0] += 1.0; a[1] += st == 0 ? 1.0 : 0.0; a[2] += st == 1 ? 1.0 : 0.0; a[3] += st == 2 ? 1.0 : 0.0; a[4] += st == 3 ? 1.0 : 0.0;
  });
  if (threadIdx.x != 0) return;
  for (int f = 0; f < 5; f++) out[f] = lds[f][0];
  out[5] = 0.0;
}

// the workgroup's row of a table of `rows` rows per group over values[rows - 1][K] and status[K]: the response's and the recovery's
template <class Buffers>
__device__ __forceinline__ void values_table_row(const Buffers& b, int K, int rows, double (*lds)[RT]) {
  const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
  double* out = b.results + ((size_t)g * rows + m) * NF;
  if (m != rows - 1) { reduce_metric_row(once(b.group, Stored{b.values}), g, m, K, lds, out); return; }
  status_row(b.status, b.group, g, K, lds, out);
}

// ---- the quaternion algebra the behaviour metrics need (xyzw), restated here: this library shares no source with the simulator
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// R(q) v = v + w t + u x t, u = q.xyz, t = 2 (u x v)
__device__ __forceinline__ V3 quat_rotate(float x, float y, float z, float w, V3 v) {
  const V3 u = {x, y, z};
  const V3 c = cross(u, v);
  const V3 t = {2.0f * c.x, 2.0f * c.y, 2.0f * c.z};
  const V3 d = cross(u, t);
  return {v.x + w * t.x + d.x, v.y + w * t.y + d.y, v.z + w * t.z + d.z};
}
__device__ __forceinline__ V3 quat_rotate_inverse(float x, float y, float z, float w, V3 v) { return quat_rotate(-x, -y, -z, w, v); }

// the metric base_height: root z minus the mean of measured_heights (fp64 carry, one rounding: see the header); NULL: root z
__device__ __forceinline__ float height_above_ground(const float* measured_heights, int num_height_points, int N, int e, float z) {
  if (!measured_heights) return z;                    // mean of (z - 0) over one point
  double s = 0.0;
  for (int p = 0; p < num_height_points; p++) s += (double)(z - measured_heights[(size_t)p * N + e]);
  return (float)s / (float)num_height_points;
}

// the metrics max_torques and power_consumption of one environment (power: fp64 carry over the fp32 products, one rounding)
__device__ __forceinline__ void torque_figures(const float* torques, const float* dof_vel, int N, int e, float* tmax, float* power) {
  float m = 0.f;
  double psum = 0.0;
  for (int j = 0; j < 12; j++) {
    const float tq = torques[j * N + e];
    m = fmaxf(m, fabsf(tq));
    psum += (double)(tq * dof_vel[j * N + e]);
  }
  *tmax = m; *power = (float)psum;
}

// foot f touches the ground (the vertical force on its body), and whether that is what the gait wants of it: 1 or 0
__device__ __forceinline__ bool foot_contact(const Row& row, const float* contact_forces, int f) {
  return row(contact_forces, (4 + 4 * f) * 3 + 2) > (float)GO1EVAL_CONTACT_FORCE;
}
__device__ __forceinline__ int contact_match(bool contact, float desired) { return contact == (desired > 0.5f) ? 1 : 0; }

// a foot's term of feet_clearance: how far its height z misses the commanded swing height at its place in the swing phase, squared,
// counted while the gait wants it in the air
__device__ __forceinline__ float clearance_miss(float cmd_swing, float index, float desired, float z) {
  const float swing_phase = 1.0f - fabsf(1.0f - fminf(fmaxf(index * 2.0f - 1.0f, 0.0f), 1.0f) * 2.0f);
  const float miss = cmd_swing * swing_phase + (float)GO1EVAL_FOOT_RADIUS - z;
  return miss * miss * (1.0f - desired);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) eval_clear_kernel(const EvalArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1EvalBuffers& b = A.b;
  clear_rows(b, 0, NM, N, e);
  b.steps[e] = 0u; b.episodes_terminated[e] = 0u; b.episodes_timed_out[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) eval_accumulate_kernel(const EvalArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1EvalBuffers& b = A.b;
  b.steps[e] += 1u;
  if (b.reset_buf[e]) {
    if (b.time_out_buf[e]) b.episodes_timed_out[e] += 1u; else b.episodes_terminated[e] += 1u;
    fold(b, GO1EVAL_TERMINATION, N, e, 1.0f);
    return;
  }
  if (b.episode_length_buf[e] <= A.c.warmup_steps) return;

  const float vx = b.base_lin_vel[e], vy = b.base_lin_vel[N + e], wz = b.base_ang_vel[2 * N + e];
  const float dv = vx - b.commands[e], dw = wz - b.commands[2 * N + e];
  fold(b, GO1EVAL_LIN_VEL_RMSD, N, e, sqrtf(dv * dv));
  fold(b, GO1EVAL_ANG_VEL_RMSD, N, e, sqrtf(dw * dw));
  fold(b, GO1EVAL_LIN_VEL_X, N, e, vx);
  fold(b, GO1EVAL_ANG_VEL_YAW, N, e, wz);

  fold(b, GO1EVAL_BASE_HEIGHT, N, e, height_above_ground(b.measured_heights, A.c.num_height_points, N, e, b.root_states[2 * N + e]));

  float tmax, power;
  torque_figures(b.torques, b.dof_vel, N, e, &tmax, &power);
  fold(b, GO1EVAL_MAX_TORQUES, N, e, tmax);
  fold(b, GO1EVAL_POWER_CONSUMPTION, N, e, power);

  const float mass = A.c.default_body_mass + b.payloads[e];
  const float speed = sqrtf(vx * vx + vy * vy);
  fold(b, GO1EVAL_COT, N, e, power / (mass * (float)GO1EVAL_GRAVITY * speed));
  fold(b, GO1EVAL_FROUDE_NUMBER, N, e, vx * vx / (float)(GO1EVAL_GRAVITY * GO1EVAL_FROUDE_HEIGHT));
  fold(b, GO1EVAL_TERMINATION, N, e, 0.0f);
}

extern "C" __global__ void __launch_bounds__(RT) eval_reduce_kernel(const EvalArgs A) {
  __shared__ double lds[NF][RT];
  const int N = A.c.num_envs;
  const int g = (int)blockIdx.x / (NM + 1), m = (int)blockIdx.x % (NM + 1);
  const Go1EvalBuffers& b = A.b;
  double* out = b.results + ((size_t)g * (NM + 1) + m) * NF;
  if (m != NM) { reduce_metric_row(b, g, m, N, lds, out); return; }
  // the group's own row: a[0] envs, a[1] steps, a[2] terminated, a[3] timed out, a[4] fallen envs
  group_sums<5>(b.group, g, N, lds, [&b](int e, double* a) {
    a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.episodes_terminated[e]; a[3] += (double)b.episodes_timed_out[e];
    a[4] += b.episodes_terminated[e] > 0u ? 1.0 : 0.0;
  });
  if (threadIdx.x != 0) return;
  out[GO1EVAL_G_ENVS] = lds[0][0]; out[GO1EVAL_G_STEPS] = lds[1][0]; out[GO1EVAL_G_TERMINATED] = lds[2][0];
  out[GO1EVAL_G_TIMED_OUT] = lds[3][0]; out[GO1EVAL_G_FALL_RATE] = lds[0][0] > 0.0 ? lds[4][0] / lds[0][0] : (double)NAN; out[5] = 0.0;
}

// ---- the behaviour table --------------------------------------------------------------------------------------------------------
constexpr int NB = GO1EVAL_NUM_BEHAVIOUR;

extern "C" __global__ void __launch_bounds__(ACC_THREADS) behaviour_clear_kernel(const BehaviourArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1BehaviourBuffers& b = A.b;
  clear_rows(b, 0, NB, N, e);
  for (int f = 0; f < 4; f++) {
    const size_t i = (size_t)f * N + e;
    b.prev_contact[i] = 2; b.stride_steps[i] = -1; b.stance_steps[i] = 0; b.swing_peak[i] = -INFINITY;
  }
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) behaviour_accumulate_kernel(const BehaviourArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1BehaviourBuffers& b = A.b;
  if (b.reset_buf[e] || b.episode_length_buf[e] <= A.c.warmup_steps) {      // a stride never spans a reset or the warm-up
    for (int f = 0; f < 4; f++) { b.prev_contact[(size_t)f * N + e] = 2; b.stride_steps[(size_t)f * N + e] = -1; }
    return;
  }
  const Row row = {N, e};
  const float cmd_vx = row(b.commands, 0), cmd_yaw = row(b.commands, 2), cmd_height = row(b.commands, 3), cmd_freq = row(b.commands, 4);
  const float cmd_duty = row(b.commands, 8), cmd_swing = row(b.commands, 9), cmd_pitch = row(b.commands, 10), cmd_roll = row(b.commands, 11);
  const float width = A.c.num_commands >= 13 ? row(b.commands, 12) : 0.3f;
  const float length = A.c.num_commands >= 14 ? row(b.commands, 13) : 0.45f;
  const V3 base = {row(b.root_states, 0), row(b.root_states, 1), row(b.root_states, 2)};
  const float qx = row(b.root_states, 3), qy = row(b.root_states, 4), qz = row(b.root_states, 5), qw = row(b.root_states, 6);

  bool contact[4];
  float foot_z[4];
  int matches = 0;
  double clearance = 0.0, raibert = 0.0, slip = 0.0;          // (fp64 carry over fp32 terms, one rounding: see the header)
  const float yaw_norm = fmaxf(sqrtf(qz * qz + qw * qw), 1e-9f);
  const float yaw_z = -qz / yaw_norm, yaw_w = qw / yaw_norm;
  const float half_period = 0.5f / cmd_freq, cmd_vy = cmd_yaw * length / 2;
  for (int f = 0; f < 4; f++) {
    contact[f] = foot_contact(row, b.contact_forces, f);
    const float desired = row(b.desired_contact_states, f), index = row(b.foot_indices, f);
    matches += contact_match(contact[f], desired);
    const V3 pos = {row(b.foot_positions, 3 * f), row(b.foot_positions, 3 * f + 1), row(b.foot_positions, 3 * f + 2)};
    foot_z[f] = pos.z;

    clearance += (double)clearance_miss(cmd_swing, index, desired, pos.z);

    const V3 rel = quat_rotate(0.0f, 0.0f, yaw_z, yaw_w, V3{pos.x - base.x, pos.y - base.y, pos.z - base.z});
    const float xs = (f < 2 ? 1.0f : -1.0f) * length / 2, ys = (f % 2 == 0 ? 1.0f : -1.0f) * width / 2;
    const float phase = fabsf(1.0f - index * 2.0f) * 1.0f - 0.5f;
    const float xo = phase * cmd_vx * half_period;
    float yo = phase * cmd_vy * half_period;
    if (f >= 2) yo = -yo;
    const float ex = fabsf((xs + xo) - rel.x), ey = fabsf((ys + yo) - rel.y);
    raibert += (double)(ex * ex);
    raibert += (double)(ey * ey);

    const float vx = row(b.foot_velocities, 3 * f), vy = row(b.foot_velocities, 3 * f + 1);
    if (contact[f]) slip += (double)(vx * vx + vy * vy);
  }
  fold(b, GO1EVAL_CONTACT_MATCH, N, e, 0.25f * (float)matches);

  const float height = height_above_ground(b.measured_heights, A.c.num_height_points, N, e, base.z);
  fold(b, GO1EVAL_BODY_HEIGHT_ERR, N, e, height - (cmd_height + A.c.base_height_target));

  float sr, cr, sp, cp;
  sincosf(-cmd_roll * 0.5f, &sr, &cr);
  sincosf(-cmd_pitch * 0.5f, &sp, &cp);
  const V3 down = {0.0f, 0.0f, -1.0f};
  const V3 is = quat_rotate_inverse(qx, qy, qz, qw, down);
  const V3 want = quat_rotate_inverse(sr * cp, cr * sp, sr * sp, cr * cp, down);
  const float dx = is.x - want.x, dy = is.y - want.y;
  fold(b, GO1EVAL_ORIENTATION_ERR, N, e, sqrtf(dx * dx + dy * dy));

  fold(b, GO1EVAL_FEET_CLEARANCE, N, e, (float)clearance);
  fold(b, GO1EVAL_RAIBERT_HEURISTIC, N, e, (float)raibert);
  fold(b, GO1EVAL_FEET_SLIP, N, e, (float)slip);

  double rate = 0.0;
  for (int j = 0; j < 12; j++) {
    const float d = row(b.last_actions, j) - row(b.last_last_actions, j);
    rate += (double)(d * d);
  }
  fold(b, GO1EVAL_ACTION_RATE, N, e, (float)rate);

  for (int f = 0; f < 4; f++) {
    const size_t i = (size_t)f * N + e;
    int stride = b.stride_steps[i], stance = b.stance_steps[i];
    float peak = b.swing_peak[i];
    if (contact[f] && b.prev_contact[i] == 0) {                 // touchdown
      if (stride >= 0) {
        const float L = (float)stride;
        fold(b, GO1EVAL_STEP_FREQUENCY_ERR, N, e, 1.0f / (L * A.c.dt) - cmd_freq);
        fold(b, GO1EVAL_DUTY_FACTOR_ERR, N, e, (float)stance / L - cmd_duty);
        fold(b, GO1EVAL_SWING_HEIGHT_ERR, N, e, (peak - (float)GO1EVAL_FOOT_RADIUS) - cmd_swing);
      }
      stride = 0; stance = 0; peak = -INFINITY;
    }
    if (stride >= 0) stride += 1;
    if (contact[f]) stance += 1;
    b.stride_steps[i] = stride; b.stance_steps[i] = stance; b.swing_peak[i] = fmaxf(peak, foot_z[f]);
    b.prev_contact[i] = contact[f] ? 1 : 0;
  }
}

extern "C" __global__ void __launch_bounds__(RT) behaviour_reduce_kernel(const BehaviourArgs A) {
  __shared__ double lds[NF][RT];
  const int g = (int)blockIdx.x / NB, m = (int)blockIdx.x % NB;
  reduce_metric_row(A.b, g, m, A.c.num_envs, lds, A.b.results + ((size_t)g * NB + m) * NF);
}

// ---- the trace and the step response --------------------------------------------------------------------------------------------
constexpr int NT = GO1EVAL_NUM_TRACE, NR = GO1EVAL_NUM_RESPONSE;

namespace {
// channel ch of row t of the trace at traced environment k: consecutive k, consecutive floats
struct TraceAt {
  const float* trace; int K, k;
  __device__ __forceinline__ float operator()(int t, int ch) const { return trace[((size_t)t * NT + ch) * K + k]; }
};
}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) trace_record_kernel(const TraceArgs A) {
  const int N = A.c.num_envs, K = A.c.num_traced;
  const int k = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (k >= K) return;
  const Go1TraceBuffers& b = A.b;
  float* out = b.trace + (size_t)A.row * NT * K + k;             // channel c at out[c * K]: consecutive k, consecutive floats
  const int e = b.env_ids ? b.env_ids[k] : k;
  if (e < 0 || e >= N) {
    for (int c = 0; c < NT; c++) out[(size_t)c * K] = NAN;
    return;
  }
  const Row row = {N, e};
  out[(size_t)GO1TRACE_LIN_VEL_X * K] = row(b.base_lin_vel, 0);
  out[(size_t)GO1TRACE_LIN_VEL_Y * K] = row(b.base_lin_vel, 1);
  out[(size_t)GO1TRACE_ANG_VEL_YAW * K] = row(b.base_ang_vel, 2);
  out[(size_t)GO1TRACE_BASE_HEIGHT * K] = height_above_ground(b.measured_heights, A.c.num_height_points, N, e, row(b.root_states, 2));
  int matches = 0;
  for (int f = 0; f < 4; f++) {
    matches += contact_match(foot_contact(row, b.contact_forces, f), row(b.desired_contact_states, f));
  }
  out[(size_t)GO1TRACE_CONTACT_MATCH * K] = 0.25f * (float)matches;
  float tmax, power;
  torque_figures(b.torques, b.dof_vel, N, e, &tmax, &power);
  out[(size_t)GO1TRACE_POWER_CONSUMPTION * K] = power;
  out[(size_t)GO1TRACE_CMD_LIN_VEL_X * K] = row(b.commands, 0);
  out[(size_t)GO1TRACE_CMD_LIN_VEL_Y * K] = row(b.commands, 1);
  out[(size_t)GO1TRACE_CMD_ANG_VEL_YAW * K] = row(b.commands, 2);
  out[(size_t)GO1TRACE_CMD_BASE_HEIGHT * K] = row(b.commands, 3) + A.c.base_height_target;
  out[(size_t)GO1TRACE_MAX_TORQUES * K] = tmax;
  out[(size_t)GO1TRACE_RESET * K] = b.reset_buf[e] != 0 ? 1.0f : 0.0f;
  for (int j = 0; j < 12; j++) out[(size_t)(GO1TRACE_DOF_POS_0 + j) * K] = row(b.dof_pos, j);
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) response_kernel(const ResponseArgs A) {
  const Go1ResponseConfig& c = A.c;
  const int K = c.num_traced;
  const int k = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (k >= K) return;
  const TraceAt at = {A.b.trace, K, k};
  const int s0 = c.switch_row, end = c.rows, w = c.smooth;

  int status = 0;
  for (int t = s0 - c.pre; t < end; t++) {
    if (at(t, GO1TRACE_RESET) != 0.0f) status = 1;
  }
  if (status == 0) {
    for (int s = 0; s < c.num_signals; s++) {
      const int rc = c.signal[s].r_channel;
      if (rc < 0) continue;
      const float r1 = at(s0, rc), r0 = s0 > 0 ? at(s0 - 1, rc) : r1;
      for (int t = s0 - c.pre; t < end; t++) {
        if (at(t, rc) != (t < s0 ? r0 : r1)) status = 2;
      }
    }
  }
  A.b.status[k] = status;

  for (int s = 0; s < c.num_signals; s++) {
    float* out = A.b.values + (size_t)s * NR * K + k;
    const Go1ResponseSignal sig = c.signal[s];
    float r1 = sig.fixed_target, r0 = sig.fixed_target;
    if (sig.r_channel >= 0) { r1 = at(s0, sig.r_channel); r0 = s0 > 0 ? at(s0 - 1, sig.r_channel) : r1; }
    const float D = sig.fixed_scale > 0.0f ? sig.fixed_scale : fabsf(r1 - r0);
    if (status != 0 || D < 1e-6f) {
      for (int m = 0; m < NR; m++) out[(size_t)m * K] = NAN;
      continue;
    }
    const float sgn = r1 >= r0 ? 1.0f : -1.0f;
    const float near = 0.1f * D, inside = c.band * D;
    int t_r = -1, t_s = s0;
    float over = 0.0f;
    double tail_sum = 0.0, abs_sum = 0.0;
    for (int t = s0; t < end; t++) {
      double sum = 0.0;
      for (int u = t - w + 1; u <= t; u++) sum += (double)at(u, sig.y_channel);
      const float ys = (float)(sum / (double)w);
      const float err = ys - r1;
      if (t_r < 0 && fabsf(err) <= near) t_r = t;
      over = fmaxf(over, sgn * err / D);
      if (fabsf(err) > inside) t_s = t + 1;
      const float raw = at(t, sig.y_channel) - r1;
      abs_sum += (double)fabsf(raw);
      if (t >= end - c.tail) tail_sum += (double)raw;
    }
    const bool settled = t_s <= end - c.hold;
    out[(size_t)GO1RESPONSE_REACHED * K] = t_r >= 0 ? 1.0f : 0.0f;
    out[(size_t)GO1RESPONSE_RISE_TIME * K] = t_r >= 0 ? (float)(t_r - s0 + 1) * c.dt : NAN;
    out[(size_t)GO1RESPONSE_OVERSHOOT * K] = over;
    out[(size_t)GO1RESPONSE_SETTLED * K] = settled ? 1.0f : 0.0f;
    out[(size_t)GO1RESPONSE_SETTLING_TIME * K] = settled ? (float)(t_s - s0 + 1) * c.dt : NAN;
    out[(size_t)GO1RESPONSE_STEADY_STATE_ERR * K] = (float)(tail_sum / (double)c.tail);
    out[(size_t)GO1RESPONSE_IAE * K] = (float)((double)c.dt * abs_sum);
  }
}

extern "C" __global__ void __launch_bounds__(RT) response_reduce_kernel(const ResponseArgs A) {
  __shared__ double lds[NF][RT];
  values_table_row(A.b, A.c.num_traced, A.c.num_signals * NR + 1, lds);
}

// ---- the push and the disturbance recovery --------------------------------------------------------------------------------------
constexpr int NV = GO1EVAL_NUM_RECOVERY;

extern "C" __global__ void __launch_bounds__(ACC_THREADS) push_kernel(const PushArgs A) {
  const int N = A.c.num_envs, K = A.c.num_pushed;
  const int k = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (k >= K) return;
  const Go1PushBuffers& b = A.b;
  const float forward = b.push[(size_t)GO1PUSH_FORWARD * K + k], left = b.push[(size_t)GO1PUSH_LEFT * K + k];     // consecutive k, consecutive floats
  const float up = b.push[(size_t)GO1PUSH_UP * K + k], dyaw = b.push[(size_t)GO1PUSH_YAW_RATE * K + k];
  if (forward == 0.0f && left == 0.0f && up == 0.0f && dyaw == 0.0f) return;       // a zero push writes nothing: -0.0f stays -0.0f
  const int e = b.env_ids ? b.env_ids[k] : k;
  if (e < 0 || e >= N) return;
  float* root = b.root_states + e;                                                 // row r at root[r * N]
  const V3 f = quat_rotate(root[(size_t)3 * N], root[(size_t)4 * N], root[(size_t)5 * N], root[(size_t)6 * N], V3{1.0f, 0.0f, 0.0f});
  const float n = sqrtf(f.x * f.x + f.y * f.y);
  float hx = 1.0f, hy = 0.0f;
  if (!(n < 1e-6f)) { hx = f.x / n; hy = f.y / n; }
  root[(size_t)7 * N] += forward * hx - left * hy;
  root[(size_t)8 * N] += forward * hy + left * hx;
  root[(size_t)9 * N] += up;
  root[(size_t)12 * N] += dyaw;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) recovery_kernel(const RecoveryArgs A) {
  const Go1RecoveryConfig& c = A.c;
  const int K = c.num_traced;
  const int k = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (k >= K) return;
  const TraceAt at = {A.b.trace, K, k};
  const int p0 = c.push_row, first = c.push_row - c.pre, end = c.rows, w = c.smooth;

  bool spoiled = false, fell = false, moved = false;
  for (int t = first; t < end; t++) {
    if (at(t, GO1TRACE_RESET) != 0.0f) { if (t < p0) spoiled = true; else fell = true; }
    for (int ch = GO1TRACE_CMD_LIN_VEL_X; ch <= GO1TRACE_CMD_ANG_VEL_YAW; ch++) {
      if (at(t, ch) != at(first, ch)) moved = true;
    }
  }
  const int status = spoiled ? GO1RECOVERY_S_BASELINE_RESET : fell ? GO1RECOVERY_S_FELL : moved ? GO1RECOVERY_S_NOT_HELD : GO1RECOVERY_S_OK;
  A.b.status[k] = status;
  float* out = A.b.values + k;
  if (status != GO1RECOVERY_S_OK) {
    for (int m = 0; m < NV; m++) out[(size_t)m * K] = NAN;
    if (status == GO1RECOVERY_S_FELL) out[(size_t)GO1RECOVERY_FELL * K] = 1.0f;
    return;
  }

  // the three signals of a row: planar velocity error, base height, yaw-rate error
  const auto vel_err = [&at](int t) {
    const float dx = at(t, GO1TRACE_LIN_VEL_X) - at(t, GO1TRACE_CMD_LIN_VEL_X), dy = at(t, GO1TRACE_LIN_VEL_Y) - at(t, GO1TRACE_CMD_LIN_VEL_Y);
    return sqrtf(dx * dx + dy * dy);
  };
  const auto height = [&at](int t) { return at(t, GO1TRACE_BASE_HEIGHT); };
  const auto yaw_err = [&at](int t) { return at(t, GO1TRACE_ANG_VEL_YAW) - at(t, GO1TRACE_CMD_ANG_VEL_YAW); };
  // the mean over rows [from, to): fp64 carry in ascending order, rounded once
  const auto mean = [](const auto& x, int from, int to) {
    double sum = 0.0;
    for (int u = from; u < to; u++) sum += (double)x(u);
    return (float)(sum / (double)(to - from));
  };
  const float eb = mean(vel_err, first, p0), zb = mean(height, first, p0), yb = mean(yaw_err, first, p0);

  int t_peak = p0, t_s = p0;
  float peak = -INFINITY, lowest = INFINITY, yaw_dev = 0.0f;
  double excess = 0.0;
  for (int t = p0; t < end; t++) {
    const float es = mean(vel_err, t - w + 1, t + 1);
    if (es > peak) { peak = es; t_peak = t; }
    if (es - eb > c.band) t_s = t + 1;
    lowest = fminf(lowest, mean(height, t - w + 1, t + 1));
    yaw_dev = fmaxf(yaw_dev, fabsf(mean(yaw_err, t - w + 1, t + 1) - yb));
    excess += (double)(vel_err(t) - eb);
  }
  const bool recovered = t_s <= end - c.hold;
  out[(size_t)GO1RECOVERY_FELL * K] = 0.0f;
  out[(size_t)GO1RECOVERY_PEAK_VEL_ERR * K] = peak - eb;
  out[(size_t)GO1RECOVERY_PEAK_TIME * K] = (float)(t_peak - p0 + 1) * c.dt;
  out[(size_t)GO1RECOVERY_RECOVERED * K] = recovered ? 1.0f : 0.0f;
  out[(size_t)GO1RECOVERY_RECOVERY_TIME * K] = recovered ? (float)(t_s - p0) * c.dt : NAN;
  out[(size_t)GO1RECOVERY_HEIGHT_DROP * K] = zb - lowest;
  out[(size_t)GO1RECOVERY_YAW_RATE_DEV * K] = yaw_dev;
  out[(size_t)GO1RECOVERY_IAE_EXCESS * K] = (float)((double)c.dt * excess);
}

extern "C" __global__ void __launch_bounds__(RT) recovery_reduce_kernel(const RecoveryArgs A) {
  __shared__ double lds[NF][RT];
  values_table_row(A.b, A.c.num_traced, NV + 1, lds);
}

// ---- terrain traversal ----------------------------------------------------------------------------------------------------------
constexpr int NTM = GO1EVAL_NUM_TERRAIN, NTO = GO1EVAL_NUM_OUTCOME;

namespace {
// where the three samples under world (x, y) start: the truncated index, clamped in fp32 before the conversion (see the header).
// ok = false for a point that is not finite: its offset is 0 (in bounds, never used) and nothing of it is converted.
struct Cell { long at; bool ok; };
__device__ __forceinline__ long cell_index(float v, float border, float hscale, int samples) {
  const float q = (v + border) / hscale, last = (float)(samples - 2);
  return q > last ? (long)(samples - 2) : (q > 0.0f ? (long)q : 0L);
}
__device__ __forceinline__ Cell cell_under(const Go1TerrainConfig& c, bool field, float x, float y) {
  if (!(isfinite(x) && isfinite(y))) return {0L, false};
  if (!field) return {0L, true};                                 // the plane: no sample is read
  return {cell_index(x, c.hf_border, c.hf_hscale, c.hf_rows) * c.hf_cols + cell_index(y, c.hf_border, c.hf_hscale, c.hf_cols), true};
}

// outcome `which` of environment e, computed from its state: what Once reads in place of a stored value
struct TerrainOutcome {
  const uint8_t* status; const uint32_t* end_step; const float* max_dist; float dt; int which;
  __device__ float operator()(size_t e) const {
    const int st = status[e];
    switch (which) {
      case GO1TERRAIN_O_TRAVERSED: return st == GO1TERRAIN_S_RUNNING ? NAN : (st == GO1TERRAIN_S_TRAVERSED ? 1.0f : 0.0f);
      case GO1TERRAIN_O_FELL: return st == GO1TERRAIN_S_RUNNING ? NAN : (st == GO1TERRAIN_S_FELL ? 1.0f : 0.0f);
      case GO1TERRAIN_O_DISTANCE: return max_dist[e];
      default: return st == GO1TERRAIN_S_RUNNING ? NAN : (float)end_step[e] * dt;
    }
  }
};
}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) terrain_clear_kernel(const TerrainArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1TerrainBuffers& b = A.b;
  clear_rows(b, 0, NTM, N, e);
  b.status[e] = GO1TERRAIN_S_RUNNING; b.steps[e] = 0u; b.end_step[e] = 0u; b.max_dist[e] = 0.0f;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) terrain_accumulate_kernel(const TerrainArgs A) {
  const Go1TerrainConfig& c = A.c;
  const int N = c.num_envs;
  const int e = (int)(blockIdx.x * ACC_THREADS + threadIdx.x);
  if (e >= N) return;
  const Go1TerrainBuffers& b = A.b;
  if (b.status[e] != GO1TERRAIN_S_RUNNING) return;
  if (b.reset_buf[e]) {                                          // the episode ended: the buffers hold the next one's pose
    b.status[e] = b.time_out_buf[e] ? GO1TERRAIN_S_TIMED_OUT : GO1TERRAIN_S_FELL;
    b.end_step[e] = b.steps[e] + 1u;
    return;
  }
  const Row row = {N, e};
  const uint32_t steps = b.steps[e] + 1u;
  b.steps[e] = steps;
  const V3 base = {row(b.root_states, 0), row(b.root_states, 1), row(b.root_states, 2)};
  const float dx = base.x - row(b.env_origins, 0), dy = base.y - row(b.env_origins, 1);
  b.max_dist[e] = fmaxf(b.max_dist[e], sqrtf(dx * dx + dy * dy));
  if (isfinite(dx) && isfinite(dy) && (fabsf(dx) > c.tile_length / 2 || fabsf(dy) > c.tile_width / 2)) {
    b.status[e] = GO1TERRAIN_S_TRAVERSED; b.end_step[e] = steps;
    return;
  }
  if (b.episode_length_buf[e] <= c.warmup_steps) return;

  // the five points (base, four feet), then their fifteen samples: the only scattered loads, all issued before the first is used
  V3 pos[5];
  pos[0] = base;
  for (int f = 0; f < 4; f++) pos[1 + f] = {row(b.foot_positions, 3 * f), row(b.foot_positions, 3 * f + 1), row(b.foot_positions, 3 * f + 2)};
  const bool field = b.height_samples != nullptr;
  Cell cell[5];
  for (int p = 0; p < 5; p++) cell[p] = cell_under(c, field, pos[p].x, pos[p].y);
  int16_t s[5][3] = {};
  if (field) {
    for (int p = 0; p < 5; p++) {
      const int16_t* q = b.height_samples + cell[p].at;
      s[p][0] = q[0]; s[p][1] = q[c.hf_cols]; s[p][2] = q[1];
    }
  }
  float above[5];                                                // z minus the ground under the point
  for (int p = 0; p < 5; p++) {
    int16_t lowest = s[p][0] < s[p][1] ? s[p][0] : s[p][1];
    lowest = lowest < s[p][2] ? lowest : s[p][2];
    above[p] = pos[p].z - (cell[p].ok ? (field ? (float)lowest * c.hf_vscale : 0.0f) : NAN);
  }

  const float cmd_swing = row(b.commands, 9);
  double clearance = 0.0, swing = 0.0;                           // (fp64 carry over fp32 terms, one rounding: see the header)
  int swinging = 0;
  bool stumble = false;
  for (int f = 0; f < 4; f++) {
    const float desired = row(b.desired_contact_states, f), index = row(b.foot_indices, f), a = above[1 + f];
    clearance += (double)clearance_miss(cmd_swing, index, desired, a);
    if (desired <= 0.5f) { swing += (double)(a - (float)GO1EVAL_FOOT_RADIUS); swinging += 1; }
    const int body = 4 + 4 * f;
    const float fx = row(b.contact_forces, 3 * body), fy = row(b.contact_forces, 3 * body + 1), fz = row(b.contact_forces, 3 * body + 2);
    if (sqrtf(fx * fx + fy * fy) > (float)GO1EVAL_STUMBLE_RATIO * fabsf(fz)) stumble = true;
  }
  int collisions = 0;
  for (int body = 0; body < 17; body++) {
    if (!((c.penalised_body_mask >> body) & 1u)) continue;      // (the same branch in every lane)
    const float fx = row(b.contact_forces, 3 * body), fy = row(b.contact_forces, 3 * body + 1), fz = row(b.contact_forces, 3 * body + 2);
    collisions += sqrtf(fx * fx + fy * fy + fz * fz) > (float)GO1EVAL_COLLISION_FORCE ? 1 : 0;
  }
  fold(b, GO1TERRAIN_BASE_HEIGHT_TERRAIN, N, e, above[0]);
  fold(b, GO1TERRAIN_FEET_CLEARANCE_TERRAIN, N, e, (float)clearance);
  if (swinging > 0) fold(b, GO1TERRAIN_SWING_FOOT_HEIGHT, N, e, (float)(swing / (double)swinging));
  fold(b, GO1TERRAIN_STUMBLE, N, e, stumble ? 1.0f : 0.0f);
  fold(b, GO1TERRAIN_COLLISION, N, e, (float)collisions);
}

extern "C" __global__ void __launch_bounds__(RT) terrain_reduce_kernel(const TerrainArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = NTM + NTO + 1;
  const int N = A.c.num_envs;
  const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
  const Go1TerrainBuffers& b = A.b;
  double* out = b.results + ((size_t)g * rows + m) * NF;
  if (m < NTM) { reduce_metric_row(b, g, m, N, lds, out); return; }
  if (m < NTM + NTO) {
    const TerrainOutcome v = {b.status, b.end_step, b.max_dist, A.c.dt, m - NTM};
    reduce_metric_row(once(b.group, v), g, 0, N, lds, out);      // (row 0 of a table of one row: index e)
    return;
  }
  status_row(b.status, b.group, g, N, lds, out);                 // environments, status 0, 1, 2, 3
  if (threadIdx.x != 0) return;
  const double ended = out[GO1TERRAIN_G_TRAVERSED] + out[GO1TERRAIN_G_FELL] + out[GO1TERRAIN_G_TIMED_OUT];
  out[GO1TERRAIN_G_SUCCESS_RATE] = ended > 0.0 ? out[GO1TERRAIN_G_TRAVERSED] / ended : (double)NAN;
}

// ---- per-joint actuator usage ---------------------------------------------------------------------------------------------------
constexpr int NJ = GO1EVAL_NUM_JOINT, DOF = 12, TB = GO1JOINT_TAU_BINS, VB = GO1JOINT_VEL_BINS, CELLS = TB * VB;
static_assert(RT == 4 * CELLS, "joint_reduce_kernel: four slices of environments per histogram cell");

namespace {
// the histogram bin of x on the scale L: clamped as a float, then converted (see the header)
__device__ __forceinline__ int joint_bin(float x, float L, int bins) {
  const float b = floorf((x / L + 1.0f) * 4.0f), last = (float)(bins - 1);
  return (int)(b > last ? last : (b > 0.0f ? b : 0.0f));
}
}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) joint_clear_kernel(const JointArgs A) {
  const int N = A.c.num_envs;
  int j, e;
  if (!row_thread(N, DOF, &j, &e)) return;                      // (block k is joint k / blocks_per_joint)
  const Go1JointBuffers& b = A.b;
  clear_rows(b, j * NJ, NJ, N, e);
  for (int cell = 0; cell < CELLS; cell++) b.hist[(size_t)(j * CELLS + cell) * N + e] = 0u;
  b.prev_dof_vel[(size_t)j * N + e] = b.dof_vel[(size_t)j * N + e];
  if (j == 0) { b.steps[e] = 0u; b.resets[e] = 0u; }
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) joint_accumulate_kernel(const JointArgs A) {
  const Go1JointConfig& c = A.c;
  const int N = c.num_envs;
  int j, e;
  if (!row_thread(N, DOF, &j, &e)) return;                      // (block k is joint k / blocks_per_joint)
  const Go1JointBuffers& b = A.b;
  const size_t i = (size_t)j * N + e;
  const bool reset = b.reset_buf[e] != 0;
  if (j == 0) {
    b.steps[e] += 1u;
    if (reset) b.resets[e] += 1u;
  }
  const float qd = b.dof_vel[i];
  if (!reset && b.episode_length_buf[e] > c.warmup_steps) {
    const float tau = b.torques[i], q = b.dof_pos[i], prev = b.prev_dof_vel[i];
    const float tau_limit = c.torque_limit[j], vel_limit = c.vel_limit[j];            // (uniform per block)
    const float d = (prev - qd) / c.dt, p = tau * qd;
    const float below = q - c.pos_lower[j], above = q - c.pos_upper[j];
    float excess = (below < 0.0f ? -below : 0.0f) + (above > 0.0f ? above : 0.0f);
    if (q != q) excess = q;                                                            // (the selects would drop the NaN)
    const int row = j * NJ;
    fold(b, row + GO1JOINT_TORQUE_ABS, N, e, fabsf(tau));
    fold(b, row + GO1JOINT_TORQUE_SQ, N, e, tau * tau);
    fold(b, row + GO1JOINT_VEL_ABS, N, e, fabsf(qd));
    fold(b, row + GO1JOINT_VEL_SQ, N, e, qd * qd);
    fold(b, row + GO1JOINT_ACC_SQ, N, e, d * d);
    fold(b, row + GO1JOINT_POWER_POS, N, e, p > 0.0f ? p : 0.0f);
    fold(b, row + GO1JOINT_POWER_NEG, N, e, p < 0.0f ? -p : 0.0f);
    fold(b, row + GO1JOINT_POS_LIMIT_EXCESS, N, e, excess);
    fold(b, row + GO1JOINT_TORQUE_SATURATED, N, e, fabsf(tau) >= c.soft_torque_limit * tau_limit ? 1.0f : 0.0f);
    fold(b, row + GO1JOINT_VEL_SATURATED, N, e, fabsf(qd) >= c.soft_vel_limit * vel_limit ? 1.0f : 0.0f);
    if (isfinite(tau) && isfinite(qd)) {
      const int cell = joint_bin(tau, tau_limit, TB) * VB + joint_bin(qd, vel_limit, VB);   // in [0, CELLS): both bins are clamped
      b.hist[(size_t)(j * CELLS + cell) * N + e] += 1u;
    }
  }
  b.prev_dof_vel[i] = qd;
}

extern "C" __global__ void __launch_bounds__(RT) joint_reduce_kernel(const JointArgs A) {
  __shared__ double lds[NF][RT];
  __shared__ unsigned long long cells[RT];
  constexpr int rows = DOF * NJ + 1;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1JointBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m != rows - 1) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: a[0] envs, a[1] steps, a[2] resets
    group_sums<3>(b.group, g, N, lds, [&b](int e, double* a) { a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.resets[e]; });
    if (t != 0) return;
    out[GO1JOINT_G_ENVS] = lds[0][0]; out[GO1JOINT_G_STEPS] = lds[1][0]; out[GO1JOINT_G_RESETS] = lds[2][0];
    out[3] = 0.0; out[4] = 0.0; out[5] = 0.0;
    return;
  }
  // the histogram of (group, joint): thread t owns cell t % 64 and the environments t / 64, t / 64 + 4, ...
  const int k = (int)blockIdx.x - G * rows;
  const int g = k / DOF, j = k % DOF, cell = t % CELLS;
  const uint32_t* h = b.hist + (size_t)(j * CELLS + cell) * N;
  unsigned long long sum = 0ull;
  for (int e = t / CELLS; e < N; e += RT / CELLS) {
    if (b.group[e] == g) sum += (unsigned long long)h[e];
  }
  cells[t] = sum;
  __syncthreads();
  if (t < 2 * CELLS) cells[t] += cells[t + 2 * CELLS];
  __syncthreads();
  if (t < CELLS) b.hist_results[((size_t)g * DOF + j) * CELLS + t] = cells[t] + cells[t + CELLS];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch -------------------------------------------
namespace {
template <class C, class B> bool heights_without_points(const C* cfg, const B* buf) { return buf->measured_heights && cfg->num_height_points <= 0; }   // -4

// what every entry point of a family asks first: -1, -2 (and the response's -10 for a signal count outside the config's array)
int check(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->steps || !buf->episodes_terminated || !buf->episodes_timed_out) return -2;
  return 0;
}
int check(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev_contact || !buf->stride_steps || !buf->stance_steps || !buf->swing_peak) return -2;
  return 0;
}
int check(const Go1ResponseConfig* cfg, const Go1ResponseBuffers* buf) {
  if (!cfg || !buf || cfg->num_traced <= 0) return -1;
  if (!buf->values || !buf->status) return -2;
  if (cfg->num_signals < 1 || cfg->num_signals > GO1EVAL_MAX_SIGNALS) return -10;
  return 0;
}
int check(const Go1RecoveryConfig* cfg, const Go1RecoveryBuffers* buf) {
  if (!cfg || !buf || cfg->num_traced <= 0) return -1;
  if (!buf->values || !buf->status) return -2;
  return 0;
}
int check(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->status || !buf->steps || !buf->end_step || !buf->max_dist) return -2;
  return 0;
}
int check(const Go1JointConfig* cfg, const Go1JointBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev_dof_vel || !buf->steps || !buf->resets || !buf->hist) return -2;
  return 0;
}
}  // namespace

extern "C" int go1eval_clear(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(eval_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_accumulate(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->base_lin_vel || !buf->base_ang_vel || !buf->commands || !buf->root_states || !buf->torques || !buf->dof_vel || !buf->payloads ||
      !buf->reset_buf || !buf->time_out_buf || !buf->episode_length_buf) return -3;
  if (heights_without_points(cfg, buf)) return -4;
  return launch(eval_accumulate_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_reduce(const Go1EvalConfig* cfg, const Go1EvalBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf)) return -5;
  return launch(eval_reduce_kernel, table_grid(cfg->num_groups, NM + 1), RT, stream, cfg, buf);
}

extern "C" int go1eval_behaviour_clear(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(behaviour_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_behaviour_accumulate(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->commands || !buf->root_states || !buf->contact_forces || !buf->foot_positions || !buf->foot_velocities ||
      !buf->desired_contact_states || !buf->foot_indices || !buf->last_actions || !buf->last_last_actions || !buf->reset_buf ||
      !buf->episode_length_buf) return -3;
  if (heights_without_points(cfg, buf)) return -4;
  if (cfg->num_commands < 12 || !(cfg->dt > 0.0f)) return -6;
  return launch(behaviour_accumulate_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_behaviour_reduce(const Go1BehaviourConfig* cfg, const Go1BehaviourBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf)) return -5;
  return launch(behaviour_reduce_kernel, table_grid(cfg->num_groups, NB), RT, stream, cfg, buf);
}

extern "C" int go1eval_trace_record(const Go1TraceConfig* cfg, const Go1TraceBuffers* buf, int32_t row, void* stream) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (cfg->num_traced <= 0 || cfg->capacity <= 0 || !buf->trace) return -2;
  if (!buf->base_lin_vel || !buf->base_ang_vel || !buf->commands || !buf->root_states || !buf->contact_forces ||
      !buf->desired_contact_states || !buf->torques || !buf->dof_vel || !buf->dof_pos || !buf->reset_buf) return -3;
  if (heights_without_points(cfg, buf)) return -4;
  if (!buf->env_ids && cfg->num_traced != cfg->num_envs) return -8;
  if (row < 0 || row >= cfg->capacity) return -7;
  TraceArgs A; A.c = *cfg; A.b = *buf; A.row = row;
  return launch_args(trace_record_kernel, env_grid(cfg->num_traced), ACC_THREADS, stream, A);
}

extern "C" int go1eval_response(const Go1ResponseConfig* cfg, const Go1ResponseBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->trace) return -3;
  const int w = cfg->smooth, s0 = cfg->switch_row, rows = cfg->rows;
  if (!(1 <= w && w <= cfg->pre + 1 && cfg->pre <= s0 && s0 < rows && cfg->hold >= 1 && cfg->tail >= 1 && cfg->hold <= rows - s0 &&
        cfg->tail <= rows - s0 && cfg->dt > 0.0f && cfg->band > 0.0f)) return -9;
  for (int s = 0; s < cfg->num_signals; s++) {
    const Go1ResponseSignal& g = cfg->signal[s];
    if (g.y_channel < 0 || g.y_channel >= NT || g.r_channel >= NT) return -10;
  }
  return launch(response_kernel, env_grid(cfg->num_traced), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_response_reduce(const Go1ResponseConfig* cfg, const Go1ResponseBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf)) return -5;
  return launch(response_reduce_kernel, table_grid(cfg->num_groups, cfg->num_signals * NR + 1), RT, stream, cfg, buf);
}

extern "C" int go1eval_push(const Go1PushConfig* cfg, const Go1PushBuffers* buf, void* stream) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (cfg->num_pushed <= 0 || !buf->root_states || !buf->push) return -2;
  if (!buf->env_ids && cfg->num_pushed != cfg->num_envs) return -8;
  return launch(push_kernel, env_grid(cfg->num_pushed), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_recovery(const Go1RecoveryConfig* cfg, const Go1RecoveryBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->trace) return -3;
  const int w = cfg->smooth, p0 = cfg->push_row, rows = cfg->rows;
  if (!(1 <= cfg->pre && cfg->pre <= p0 && p0 < rows && 1 <= w && w <= cfg->pre + 1 && 1 <= cfg->hold && cfg->hold <= rows - p0 &&
        cfg->dt > 0.0f && cfg->band >= 0.0f)) return -11;
  return launch(recovery_kernel, env_grid(cfg->num_traced), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_recovery_reduce(const Go1RecoveryConfig* cfg, const Go1RecoveryBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf)) return -5;
  return launch(recovery_reduce_kernel, table_grid(cfg->num_groups, NV + 1), RT, stream, cfg, buf);
}

extern "C" int go1eval_terrain_clear(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(terrain_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_terrain_accumulate(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->root_states || !buf->commands || !buf->contact_forces || !buf->foot_positions || !buf->desired_contact_states ||
      !buf->foot_indices || !buf->env_origins || !buf->reset_buf || !buf->time_out_buf || !buf->episode_length_buf) return -3;
  if (buf->height_samples && (cfg->hf_rows < 2 || cfg->hf_cols < 2)) return -12;
  if (!(cfg->hf_hscale > 0.0f && cfg->tile_length > 0.0f && cfg->tile_width > 0.0f && cfg->dt > 0.0f)) return -12;
  return launch(terrain_accumulate_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_terrain_reduce(const Go1TerrainConfig* cfg, const Go1TerrainBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf)) return -5;
  if (!(cfg->dt > 0.0f)) return -12;
  return launch(terrain_reduce_kernel, table_grid(cfg->num_groups, NTM + NTO + 1), RT, stream, cfg, buf);
}

extern "C" int go1eval_joint_clear(const Go1JointConfig* cfg, const Go1JointBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->dof_vel) return -3;
  return launch(joint_clear_kernel, row_grid(DOF, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_joint_accumulate(const Go1JointConfig* cfg, const Go1JointBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->torques || !buf->dof_vel || !buf->dof_pos || !buf->reset_buf || !buf->episode_length_buf) return -3;
  if (!(positive(cfg->dt) && positive(cfg->soft_torque_limit) && positive(cfg->soft_vel_limit))) return -12;
  for (int j = 0; j < DOF; j++) {
    if (!(positive(cfg->torque_limit[j]) && positive(cfg->vel_limit[j]) && cfg->pos_lower[j] <= cfg->pos_upper[j])) return -12;
  }
  return launch(joint_accumulate_kernel, row_grid(DOF, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1eval_joint_reduce(const Go1JointConfig* cfg, const Go1JointBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->hist_results) return -5;
  return launch(joint_reduce_kernel, table_grid(cfg->num_groups, DOF * NJ + 1 + DOF), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1eval_version(void) { return "go1eval 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
