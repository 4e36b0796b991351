/* go1reward.h — C-ABI of libgo1reward.so: the step reward of a policy rollout taken apart by term on the device (HIP, gfx950).
 *
 * The step kernel of libgo1sim.so evaluates up to 24 reward terms per environment and step (csrc/go1_maps.h reward_partial, ids
 * GO1_REW_* of go1sim.h), adds each to the running episode_sums and stores only the clipped total in rew_buf.  This library evaluates
 * the terms of the step just taken once more, AFTER the step, from the buffers the step left, with the step kernel's own device
 * functions (go1reward.hip includes csrc/go1_maps.h and is compiled with libgo1sim.so's flags: the same arithmetic, contraction
 * included), four lanes per environment (lane = leg), and folds them into per-environment accumulators.  The step path is untouched.
 *
 * With K = num_rewards active terms in the configuration's order (the rows of episode_sums), an environment has K + 4 rows:
 *   rows 0 .. K - 1   r_k = quad_sum(partial_k) * scale_k, the value the step added to episode_sums[k]
 *   row K     sum       sum of the r_k, added in id order as the step kernel adds them
 *   row K + 1 positive  sum of the r_k with reward_raw_sign(id) * scale >= 0   (the step kernel's `pos`)
 *   row K + 2 negative  sum of the others                                      (its `neg`)
 *   row K + 3 total     the sum after only_positive_rewards (max(sum, 0)) or the ji22 rule (positive * exp(negative / sigma_rew_neg)):
 *                       what the step stored in rew_buf; total - sum is what the clip forgave
 *
 * What a launch reads.  As stored by the step: base_lin_vel, base_ang_vel, projected_gravity (written before the step's callbacks, so a
 * push or a teleport does not disturb them), commands (post-callback), torques, dof_pos, dof_vel, actions, joint_pos_target,
 * contact_forces, foot_positions, foot_velocities, prev_foot_velocities, foot_indices, desired_contact_states, root_states (orientation
 * and position), measured_heights (summed with the step kernel's lane stride: p = leg, leg + 4, ..., then the quad sum, then / np) and
 * height_samples.  Rolled by the step and still there: the step's last_actions is the post-step last_last_actions, its
 * last_joint_pos_target the post-step last_last_joint_pos_target.  Lost in the roll: the step's last_last_actions,
 * last_last_joint_pos_target, last_dof_vel and last_contacts; each equals the post-step value of the step before, so the family keeps a
 * snapshot of these four buffers (snap_*), taken by go1reward_arm and again at the end of every go1reward_accumulate.  A reset of
 * environments from the host between two steps makes the snapshot stale: call go1reward_snapshot after it.
 *
 * Steps that are not measured, counted per environment: `resets` (reset_buf is set after the step: the state the reward saw is gone;
 * the failed-simulation guard forces a reset and is among these), then `teleported` (the base is more than 1 m horizontally from one of
 * its feet: the teleport callback moved root_states after the step read it), then warm-up steps (episode_length_buf <= warmup_steps,
 * not counted).  The snapshot is refreshed on such a step too, and last_valid is 0 and the last_* rows NaN.
 *
 * Return codes, in this precedence: -1 no handle / no config / num_envs <= 0 / num_rewards outside [1, GO1_MAX_REWARDS] / a size that
 * differs from the simulator's, -2 an output buffer missing (accumulators, snapshot, last_*, counts), -3 a simulator buffer missing,
 * -5 (reduce) no group table, -10 hipSetDevice, -12 allocation, -13 upload, -20 launch.
 */
#ifndef GO1REWARD_H
#define GO1REWARD_H

#include <stdint.h>

#include "go1sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO1REWARD_EXTRA_ROWS 4
#define GO1REWARD_NUM_FIELDS 6
#define GO1REWARD_REDUCE_THREADS 256
#define GO1REWARD_ENVS_PER_BLOCK 64
#define GO1REWARD_TELEPORT_DISTANCE 1.0

/* the rows after the K terms */
enum Go1RewardExtraRow { GO1REWARD_X_SUM = 0, GO1REWARD_X_POSITIVE = 1, GO1REWARD_X_NEGATIVE = 2, GO1REWARD_X_TOTAL = 3 };
/* columns of a metric row */
enum Go1RewardField { GO1REWARD_F_COUNT = 0, GO1REWARD_F_MEAN = 1, GO1REWARD_F_STD = 2, GO1REWARD_F_MIN = 3, GO1REWARD_F_MAX = 4, GO1REWARD_F_NONFINITE = 5 };
/* columns of group_results */
enum Go1RewardGroupField { GO1REWARD_G_ENVS = 0, GO1REWARD_G_MEASURED = 1, GO1REWARD_G_RESET = 2, GO1REWARD_G_TELEPORTED = 3 };

typedef struct Go1RewardConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* steps with episode_length_buf <= warmup_steps fold nothing */
  int32_t num_groups;          /* G of the result tables */
  int32_t num_rewards;         /* K: the simulator configuration's num_rewards */
} Go1RewardConfig;

typedef struct Go1RewardBuffers {
  /* accumulators, [K + 4][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* the snapshot: the post-step values of the step before */
  float* snap_last_last_actions;           /* [12][N] */
  float* snap_last_last_joint_pos_target;  /* [12][N] */
  float* snap_last_dof_vel;                /* [12][N] */
  uint8_t* snap_last_contacts;             /* [4][N] */
  /* the last accumulated step */
  float* last_raw;                         /* [K][N]: the unscaled quad sums */
  float* last_scaled;                      /* [K + 4][N] */
  uint8_t* last_valid;                     /* [N]: 1 where the last step was measured */
  /* counts */
  uint32_t* measured;                      /* [N] */
  uint32_t* resets;                        /* [N] */
  uint32_t* teleported;                    /* [N] */
  /* go1reward_reduce */
  const int32_t* group;                    /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                         /* [num_groups][K + 4][GO1REWARD_NUM_FIELDS] */
  double* group_results;                   /* [num_groups][4]: members, measured, reset, teleported env-steps */
} Go1RewardBuffers;

typedef struct Go1Reward Go1Reward;        /* opaque handle: owns one device allocation (the simulator's configuration, the reward plan,
                                              and the simulator's buffer table with four history pointers redirected to the snapshot) */

/* sim_cfg / sim_buf: the simulator's configuration and buffer table (copied; num_rewards in [1, GO1_MAX_REWARDS]) */
int go1reward_create(const Go1SimConfig* sim_cfg, const Go1SimBuffers* sim_buf, int device, Go1Reward** out);
int go1reward_destroy(Go1Reward* h);

/* start a measurement with this config and these buffers (kept by the handle): take the snapshot, empty the accumulators and the counts.
 * One launch, one thread per environment. */
int go1reward_arm(Go1Reward* h, const Go1RewardConfig* cfg, const Go1RewardBuffers* buf, void* stream);

/* take the snapshot again (after a reset of environments from the host between two steps).  One launch. */
int go1reward_snapshot(Go1Reward* h, void* stream);

/* after a simulator step: the terms of that step.  gravity: the three floats of the gravity vector in force during the step
 * (as go1sim_post_physics takes them; read on the host before the launch).  One launch, four lanes per environment. */
int go1reward_accumulate(Go1Reward* h, const float* gravity, void* stream);

/* results [G][K + 4][6] and group_results [G][4] from the accumulators and the counts.  One launch. */
int go1reward_reduce(Go1Reward* h, void* stream);

/* "go1reward <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1reward_version(void);

#ifdef __cplusplus
}
#endif

#endif
