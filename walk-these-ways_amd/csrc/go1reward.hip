// go1reward.hip — the step reward of a policy rollout taken apart by term on the device (include/go1reward.h), gfx950.
//
// The terms are NOT written a third time: this file includes go1_maps.h and calls the step kernel's own load_reward_inputs,
// reward_partial, reward_raw_sign, hf_sample_min3 and quad_sum, and the library is compiled with libgo1sim.so's flags.
// reward_accumulate_kernel: four lanes per environment (lane = leg), a workgroup of 256 lanes holds 64 environments, so every partial
// sum is formed in the step kernel's order (per-leg partials, then the quad sum, then the scale).  The leg-0 lane of an environment is
// the one writer of its accumulator words, its last_* rows and its counts; every lane writes the snapshot rows of its own three joints
// and its own foot.  No atomics, no LDS.
// reward_reduce_kernel: one workgroup per (group, row of the result table), then one per group for the counts; go1_tables.h's
// fixed-order reduction.
//
// CfgRef / BufRef are references into the constant address space, so the configuration, the reward plan and the buffer table the
// device functions read live in one device block the handle owns (RewardConst).  Its `buf` is the simulator's table with
// last_actions / last_joint_pos_target pointed at the simulator's last_last_* (the roll moved them there) and the four histories the
// roll destroyed pointed at the family's snapshot; `sim` is the simulator's table as it is (the snapshot is copied from it).
#include "../../include/go1reward.h"
#include "go1_maps.h"
// The table side keeps the metric libraries' contract (a rounding after every multiply and every add: their -ffp-contract=off), so that
// the group table is tests/reward_ref.py's fixed-order reduction bit for bit; the library's flags are the step kernel's, which contract.
// The pragma is lexical: it covers go1_tables.h's functions wherever they are inlined, and nothing of go1_maps.h or of the kernels below.
#pragma clang fp contract(off)
#include "go1_tables.h"
#pragma clang fp contract(fast)

namespace {

GO1_TABLES_MATCH(GO1REWARD);
constexpr int XR = GO1REWARD_EXTRA_ROWS, EPB = GO1REWARD_ENVS_PER_BLOCK;
static_assert(EPB * 4 == ACC_THREADS, "reward_accumulate_kernel: a workgroup is 64 environments of four lanes");

struct RewardConst {         // one device allocation per handle; no kernel writes it
  Go1SimConfig cfg;
  RewardPlan plan;           // as go1sim.hip builds its own: terms indexed by id
  Go1SimBuffers buf;         // the table the step kernel's functions read here (see above)
  Go1SimBuffers sim;         // the simulator's own table
};

struct RewardArgs {
  const RewardConst* rc;
  Go1RewardConfig c;
  Go1RewardBuffers b;
  float gravity[3];
};

// the four histories of environment e this lane owns (the three joints of `leg`, its foot): simulator -> snapshot
__device__ __forceinline__ void snapshot_leg(BufRef S, const Go1RewardBuffers& b, int e, int N, int leg) {
#pragma unroll
  for (int jj = 0; jj < 3; jj++) {
    const int j = 3 * leg + jj;
    AT(b.snap_last_last_actions, j, e) = AT(S.last_last_actions, j, e);
    AT(b.snap_last_last_joint_pos_target, j, e) = AT(S.last_last_joint_pos_target, j, e);
    AT(b.snap_last_dof_vel, j, e) = AT(S.last_dof_vel, j, e);
  }
  AT(b.snap_last_contacts, leg, e) = AT(S.last_contacts, leg, e);
}

}  // namespace

// one thread per environment: the snapshot and, with clear, empty accumulators, counts and last_* rows
extern "C" __global__ void __launch_bounds__(ACC_THREADS) reward_snapshot_kernel(const RewardArgs A, const int clear) {
  const int N = A.c.num_envs, K = A.c.num_rewards;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const GO1_CONSTANT RewardConst* rc = (const GO1_CONSTANT RewardConst*)(uintptr_t)A.rc;
  const Go1RewardBuffers& b = A.b;
  for (int leg = 0; leg < 4; leg++) snapshot_leg(rc->sim, b, e, N, leg);
  if (!clear) return;
  clear_rows(b, 0, K + XR, N, e);
  for (int k = 0; k < K; k++) AT(b.last_raw, k, e) = NAN;
  for (int k = 0; k < K + XR; k++) AT(b.last_scaled, k, e) = NAN;
  b.last_valid[e] = 0;
  b.measured[e] = 0u; b.resets[e] = 0u; b.teleported[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) reward_accumulate_kernel(const RewardArgs A) {
  const GO1_CONSTANT RewardConst* rc = (const GO1_CONSTANT RewardConst*)(uintptr_t)A.rc;
  CfgRef cfg = rc->cfg;
  BufRef B = rc->buf;
  PlanRef plan = rc->plan;
  const Go1RewardBuffers& b = A.b;
  const int N = A.c.num_envs, K = A.c.num_rewards;
  const int lane = (int)threadIdx.x, leg = lane & 3;
  const int e = (int)blockIdx.x * EPB + (lane >> 2);
  if (e >= N) return;                                                       // (the four lanes of an environment leave together)
  const bool is0 = leg == 0;

  // ---- is this step measured?  The three tests are the same on the four lanes of the environment.
  FootCtx F;
  F.pos = v3(AT(B.foot_positions, 3 * leg, e), AT(B.foot_positions, 3 * leg + 1, e), AT(B.foot_positions, 3 * leg + 2, e));
  Derived d;
  d.base_pos = v3(AT(B.root_states, 0, e), AT(B.root_states, 1, e), AT(B.root_states, 2, e));
  const float tx = d.base_pos.x - F.pos.x, ty = d.base_pos.y - F.pos.y;
  const float limit = (float)GO1REWARD_TELEPORT_DISTANCE;
  const bool far = quad_sum(tx * tx + ty * ty > limit * limit ? 1.f : 0.f) > 0.f;
  const bool reset = B.reset_buf[e] != 0;
  const bool warm = B.episode_length_buf[e] <= A.c.warmup_steps;
  if (reset || far || warm) {
    if (is0) {
      if (reset) b.resets[e] += 1u;
      else if (far) b.teleported[e] += 1u;
      b.last_valid[e] = 0;
      for (int k = 0; k < K; k++) AT(b.last_raw, k, e) = NAN;
      for (int k = 0; k < K + XR; k++) AT(b.last_scaled, k, e) = NAN;
    }
    snapshot_leg(rc->sim, b, e, N, leg);
    return;
  }

  // ---- what post_physics() held in registers when it evaluated the rewards, from where it stored it
  d.qx = AT(B.root_states, 3, e); d.qy = AT(B.root_states, 4, e); d.qz = AT(B.root_states, 5, e); d.qw = AT(B.root_states, 6, e);
  d.blv = v3(AT(B.base_lin_vel, 0, e), AT(B.base_lin_vel, 1, e), AT(B.base_lin_vel, 2, e));
  d.bav = v3(AT(B.base_ang_vel, 0, e), AT(B.base_ang_vel, 1, e), AT(B.base_ang_vel, 2, e));
  d.pg = v3(AT(B.projected_gravity, 0, e), AT(B.projected_gravity, 1, e), AT(B.projected_gravity, 2, e));
  const V3 grav = v3(A.gravity[0], A.gravity[1], A.gravity[2]);
  d.gvec = (1.f / norm(grav)) * grav;
  F.foot_index = AT(B.foot_indices, leg, e);
  F.desired_contact = AT(B.desired_contact_states, leg, e);
  F.vel = v3(AT(B.foot_velocities, 3 * leg, e), AT(B.foot_velocities, 3 * leg + 1, e), AT(B.foot_velocities, 3 * leg + 2, e));
  {
    const int fb = 4 + 4 * leg;
    F.force = v3(AT(B.contact_forces, 3 * fb, e), AT(B.contact_forces, 3 * fb + 1, e), AT(B.contact_forces, 3 * fb + 2, e));
    F.fnorm = norm(F.force);
  }
  // the heights the terms read: post_physics()'s, the mean of the measured heights summed with its lane stride
  const bool measured = cfg.measure_heights && B.measured_heights;
  float mean_height = 0.f;
  if (measured) {
    const int np = cfg.num_height_x * cfg.num_height_y;
    float sum = 0.f;
#pragma unroll 1
    for (int p = leg; p < np; p += 4) sum += AT(B.measured_heights, p, e);
    mean_height = quad_sum(sum) / np;
  }
  F.hz = F.pos.z;
  d.base_hz = d.base_pos.z;
  if (cfg.reward_heights_above_terrain) {
    F.hz -= hf_sample_min3(cfg, B.height_samples, F.pos.x, F.pos.y);
    d.base_hz -= measured ? mean_height : hf_sample_min3(cfg, B.height_samples, d.base_pos.x, d.base_pos.y);
  }
  RewardIn rin;
  load_reward_inputs(cfg, B, e, N, leg, rin);

  // ---- the terms, in id order: go1_maps.h post_physics(), "compute_reward"
  float rew = 0.f, pos = 0.f, neg = 0.f;
#pragma unroll
  for (int id = 0; id < GO1_REW_COUNT; id++) {
    const int kx = plan.kx_by_id[id];
    if (kx >= 0) {
      // The step kernel forms r = q * scale, tests it (its failed-simulation guard may replace it by 0) and THEN adds it: a multiply and an
      // add, two roundings (read off its ISA: v_mul_f32, v_cndmask, v_add_f32).  Without the guard in between the compiler fuses the scale
      // into the running sums here (v_fmac_f32, one rounding), and sum / positive / negative / total are no longer the step kernel's bits.
#pragma clang fp contract(off)
      const float sc = plan.scale_by_id[id];
      const float raw = quad_sum(reward_partial(cfg, B, e, N, id, d, F, leg, rin));
      const float r = raw * sc;
      rew += r;
      if (reward_raw_sign(id) * sc >= 0) pos += r; else neg += r;
      if (is0) {
        AT(b.last_raw, kx, e) = raw;
        AT(b.last_scaled, kx, e) = r;
        fold(b, kx, N, e, r);
      }
    }
  }
  float total = rew;
  if (cfg.only_positive_rewards) total = fmaxf(rew, 0.f);
  else if (cfg.only_positive_rewards_ji22_style) total = pos * expf(neg / cfg.sigma_rew_neg);
  if (is0) {
    const float extra[XR] = {rew, pos, neg, total};
#pragma unroll
    for (int x = 0; x < XR; x++) {
      AT(b.last_scaled, K + x, e) = extra[x];
      fold(b, K + x, N, e, extra[x]);
    }
    b.last_valid[e] = 1;
    b.measured[e] += 1u;
  }
  snapshot_leg(rc->sim, b, e, N, leg);                                      // (after feet_slip's write of this lane's own last_contacts word)
}

extern "C" __global__ void __launch_bounds__(RT) reward_reduce_kernel(const RewardArgs A) {
  __shared__ double lds[NF][RT];
  const int N = A.c.num_envs, G = A.c.num_groups, rows = A.c.num_rewards + XR;
  const Go1RewardBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    reduce_metric_row(b, g, m, N, lds, b.results + ((size_t)g * rows + m) * NF);
    return;
  }
  const int g = (int)blockIdx.x - G * rows;
  group_sums<4>(b.group, g, N, lds, [&b](int e, double* a) {
    a[0] += 1.0; a[1] += (double)b.measured[e]; a[2] += (double)b.resets[e]; a[3] += (double)b.teleported[e];
  });
  if ((int)threadIdx.x != 0) return;
  double* out = b.group_results + (size_t)g * 4;
  out[GO1REWARD_G_ENVS] = lds[0][0]; out[GO1REWARD_G_MEASURED] = lds[1][0]; out[GO1REWARD_G_RESET] = lds[2][0];
  out[GO1REWARD_G_TELEPORTED] = lds[3][0];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
struct Go1Reward {
  Go1SimConfig sim_cfg;
  Go1SimBuffers sim_buf;
  RewardConst* dconst;
  Go1RewardConfig cfg;       // of the last go1reward_arm (num_envs 0: never armed)
  Go1RewardBuffers buf;
};

namespace {
bool rewards_ok(const Go1SimConfig* c) { return c->num_rewards >= 1 && c->num_rewards <= GO1_MAX_REWARDS; }

// -1, -2, -3 of a config and buffers against the handle
int check(const Go1Reward* h, const Go1RewardConfig* cfg, const Go1RewardBuffers* buf) {
  if (!h || !cfg || !buf || cfg->num_envs <= 0 || cfg->num_envs != h->sim_cfg.num_envs || cfg->num_rewards != h->sim_cfg.num_rewards) return -1;
  if (!has_accumulators(buf) || !buf->snap_last_last_actions || !buf->snap_last_last_joint_pos_target || !buf->snap_last_dof_vel ||
      !buf->snap_last_contacts || !buf->last_raw || !buf->last_scaled || !buf->last_valid || !buf->measured || !buf->resets || !buf->teleported)
    return -2;
  const Go1SimBuffers& s = h->sim_buf;
  if (!s.root_states || !s.base_lin_vel || !s.base_ang_vel || !s.projected_gravity || !s.commands || !s.torques || !s.dof_pos || !s.dof_vel ||
      !s.actions || !s.joint_pos_target || !s.contact_forces || !s.foot_positions || !s.foot_velocities || !s.prev_foot_velocities ||
      !s.foot_indices || !s.desired_contact_states || !s.last_last_actions || !s.last_last_joint_pos_target || !s.last_dof_vel ||
      !s.last_contacts || !s.reset_buf || !s.episode_length_buf)
    return -3;
  return 0;
}

RewardArgs args_of(const Go1Reward* h, const float* gravity) {
  RewardArgs A;
  A.rc = h->dconst; A.c = h->cfg; A.b = h->buf;
  for (int i = 0; i < 3; i++) A.gravity[i] = gravity ? gravity[i] : 0.f;
  return A;
}

// the device block: the configuration, the plan, and the buffer table with the histories redirected to `buf`'s snapshot (or, before the
// first arm, left as the simulator's)
int upload(Go1Reward* h, const Go1RewardBuffers* buf) {
  RewardConst c;
  c.cfg = h->sim_cfg; c.sim = h->sim_buf; c.buf = h->sim_buf;
  for (int id = 0; id < GO1_REW_COUNT; id++) { c.plan.kx_by_id[id] = -1; c.plan.scale_by_id[id] = 0.f; }
  for (int kx = 0; kx < h->sim_cfg.num_rewards; kx++) {
    const int id = h->sim_cfg.reward_ids[kx];
    if (id >= 0 && id < GO1_REW_COUNT) { c.plan.kx_by_id[id] = kx; c.plan.scale_by_id[id] = h->sim_cfg.reward_scales[kx]; }
  }
  c.buf.last_actions = h->sim_buf.last_last_actions;                        // the roll moved them there
  c.buf.last_joint_pos_target = h->sim_buf.last_last_joint_pos_target;
  if (buf) {
    c.buf.last_last_actions = buf->snap_last_last_actions;
    c.buf.last_last_joint_pos_target = buf->snap_last_last_joint_pos_target;
    c.buf.last_dof_vel = buf->snap_last_dof_vel;
    c.buf.last_contacts = buf->snap_last_contacts;
  }
  return hipMemcpy(h->dconst, &c, sizeof(RewardConst), hipMemcpyHostToDevice) == hipSuccess ? 0 : -13;
}
}  // namespace

// the device the calling thread has current is what it was when go1reward_create returns: the block is allocated on `device`, nothing else moves
// there.  (The host build under the SIMT emulator knows one device and no hipGetDevice.)
namespace {
int create_on(Go1Reward* h, int device) {
#if defined(__HIP__)
  int before = 0;
  if (hipGetDevice(&before) != hipSuccess || hipSetDevice(device) != hipSuccess) return -10;
#else
  if (hipSetDevice(device) != hipSuccess) return -10;
#endif
  int rc = 0;
  if (hipMalloc((void**)&h->dconst, sizeof(RewardConst)) != hipSuccess) { h->dconst = nullptr; rc = -12; }
  else if ((rc = upload(h, nullptr)) != 0) { (void)hipFree(h->dconst); h->dconst = nullptr; }
#if defined(__HIP__)
  if (hipSetDevice(before) != hipSuccess && rc == 0) { (void)hipFree(h->dconst); h->dconst = nullptr; rc = -10; }
#endif
  return rc;
}
}  // namespace

extern "C" int go1reward_create(const Go1SimConfig* sim_cfg, const Go1SimBuffers* sim_buf, int device, Go1Reward** out) {
  if (!sim_cfg || !sim_buf || !out || sim_cfg->num_envs <= 0 || !rewards_ok(sim_cfg)) return -1;
  Go1Reward* h = new Go1Reward();
  h->sim_cfg = *sim_cfg; h->sim_buf = *sim_buf; h->dconst = nullptr;
  h->cfg = Go1RewardConfig(); h->buf = Go1RewardBuffers();
  if (int rc = create_on(h, device)) { delete h; return rc; }
  *out = h;
  return 0;
}

extern "C" int go1reward_destroy(Go1Reward* h) {
  if (!h) return -1;
  (void)hipFree(h->dconst);
  delete h;
  return 0;
}

// (the upload is a blocking copy on the default stream, and happens only when the snapshot's buffers moved: the caller's stream is assumed to
// be the default one, or idle, at that moment; go1reward_host.Go1Reward keeps its snapshot tensors for its lifetime, so it uploads once)
extern "C" int go1reward_arm(Go1Reward* h, const Go1RewardConfig* cfg, const Go1RewardBuffers* buf, void* stream) {
  if (int rc = check(h, cfg, buf)) return rc;
  const Go1RewardBuffers& o = h->buf;
  const bool same = o.snap_last_last_actions == buf->snap_last_last_actions && o.snap_last_last_joint_pos_target == buf->snap_last_last_joint_pos_target &&
                    o.snap_last_dof_vel == buf->snap_last_dof_vel && o.snap_last_contacts == buf->snap_last_contacts;
  if (!same)
    if (int rc = upload(h, buf)) return rc;                                 // the handle keeps what it held: nothing was assigned yet
  h->cfg = *cfg; h->buf = *buf;
  hipLaunchKernelGGL(reward_snapshot_kernel, env_grid(cfg->num_envs), dim3(ACC_THREADS), 0, (hipStream_t)stream, args_of(h, nullptr), 1);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

extern "C" int go1reward_snapshot(Go1Reward* h, void* stream) {
  if (!h) return -1;
  if (int rc = check(h, &h->cfg, &h->buf)) return rc;
  hipLaunchKernelGGL(reward_snapshot_kernel, env_grid(h->cfg.num_envs), dim3(ACC_THREADS), 0, (hipStream_t)stream, args_of(h, nullptr), 0);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

extern "C" int go1reward_accumulate(Go1Reward* h, const float* gravity, void* stream) {
  if (!h || !gravity) return -1;
  if (int rc = check(h, &h->cfg, &h->buf)) return rc;
  const int n = h->cfg.num_envs;
  return launch_args(reward_accumulate_kernel, dim3((unsigned)((n + EPB - 1) / EPB)), ACC_THREADS, stream, args_of(h, gravity));
}

extern "C" int go1reward_reduce(Go1Reward* h, void* stream) {
  if (!h) return -1;
  const int rc = check(h, &h->cfg, &h->buf);
  if (rc != 0 && rc != -3) return rc;                                       // (the reduction reads no simulator buffer)
  if (!has_table(&h->cfg, &h->buf) || !h->buf.group_results) return -5;
  return launch_args(reward_reduce_kernel, table_grid(h->cfg.num_groups, h->cfg.num_rewards + XR + 1), RT, stream, args_of(h, nullptr));
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1reward_version(void) { return "go1reward 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
