/* go1state.h — C-ABI of libgo1state.so: save, restore and branch the simulator's state on the device (HIP, gfx950).
 *
 * The simulator's state is its caller-owned buffers (go1sim.h Go1SimBuffers) plus two counters in its handle (the step counter and
 * the head of the lag ring, go1sim_get_counters / go1sim_set_counters) and the slot of the observation-history ring
 * (go1sim_history_window_offset).  This library copies the buffers' part: a GATHER of chosen environments into a packed snapshot and
 * a SCATTER of snapshot rows into chosen environments, one launch each.  It is a library of its own, as the renderer and the metric
 * libraries are: libgo1sim.so's surface and kernels stay as they are, and no other binary or stamp depends on this one.  Nothing here
 * throws, nothing synchronises the stream; every entry point returns 0 or a negative code.  tests/state_ref.py restates the copy in
 * numpy from this text.
 *
 * What is copied.  Every member of Go1SimBuffers is in exactly one class:
 *   per environment   everything with an environment axis (the lists below): state, parameters, and the outputs of the last step, so
 *                     that after a restore the caller reads what it read at the capture
 *   global            curriculum_weights, curriculum_cdf, curriculum_success, episode_log, fault_counts, contact_drop_counts: copied by
 *                     go1state_capture_global / go1state_restore_global only
 *   static            curriculum_nbr_ptr, curriculum_nbr_idx (a function of the configuration), height_samples (the terrain),
 *                     contact_signature (a test record of the last step's substeps): never read, never written
 *
 * The packed snapshot of K environments has three per-environment sections and a global one.  `words` and `bytes` list their fields in
 * the order of their declaration in Go1SimBuffers, `rows` and `global` in the order given below; `K` is the snapshot's num_rows.
 *   words   uint32 [W][K], environment fastest: the fp32 / int32 / uint32 SoA arrays, row r of a field at section row off + r.
 *           root_states 13, dof_pos 12, dof_vel 12, contact_forces 51, foot_positions 12, foot_velocities 12, prev_foot_velocities 12,
 *           lag_buffer 12 (lag + 1), joint_pos_err_last 12, joint_pos_err_last_last 12, joint_vel_last 12, joint_vel_last_last 12,
 *           joint_pos_target 12, last_joint_pos_target 12, last_last_joint_pos_target 12, actions 12, last_actions 12,
 *           last_last_actions 12, last_dof_vel 12, torques 12, base_lin_vel 3, base_ang_vel 3, projected_gravity 3,
 *           commands command_rows, gait_indices 1, clock_inputs 4, desired_contact_states 4, foot_indices 4, episode_length_buf 1,
 *           rew_buf 1, episode_sums num_rewards + 1, command_sums num_rewards + 5, episode_sums_eval num_rewards + 1,
 *           friction_coeffs 1, restitutions 1, payloads 1, com_displacements 3, motor_strengths 12, motor_offsets 12, Kp_factors 12,
 *           Kd_factors 12, env_origins 3, env_command_bins 1, env_command_categories 1, fault_flags 1,
 *           measured_heights max(num_height_points, 1).
 *           The lag ring is stored in LOGICAL order: section row 12 i + j of the field is row j of the ring's slot
 *           (lag_head + i) % (lag + 1).  episode_sums_eval and measured_heights may be NULL in the buffers: their rows stay in the
 *           layout, a capture leaves them as they are (the host mirror hands in zeroed storage) and a restore skips them.
 *   bytes   uint8 [B][K], environment fastest: reset_buf 1, time_out_buf 1, last_contacts 4, resample_flags 1.  Copied byte by byte: a
 *           restore into some environments never touches the bytes of their neighbours.
 *   rows    uint32, three row-major blocks one after the other: obs_buf (K, num_obs), obs_history (K, R num_obs) with R =
 *           num_obs_history + 1, privileged_obs_buf (K, max(num_privileged_obs, 1)).  The history is stored in LOGICAL order: the R slots
 *           starting at slot (history_slot + 1) % R, i.e. oldest first, the spare (next-write) slot last.  A restore writes both copies of
 *           every slot (columns p and p + R num_obs of the simulator's row).
 *   global  uint32 [G]: curriculum_weights, curriculum_cdf (num_categories num_bins each), curriculum_success
 *           (curriculum_update_interval num_categories num_bins), episode_log num_rewards + 2, fault_counts GO1_FAULT_BITS,
 *           contact_drop_counts GO1_CC_COUNT (may be NULL: skipped).
 * Because both rings are stored in logical order a snapshot does not depend on the phase at which it was taken, and a restore
 * re-phases it to the lag_head / history_slot it is given: the handle's CURRENT ones.
 *
 * The layout is a function of the ten values of Go1StateConfig after num_envs.  A capture writes them, behind a magic word and the
 * layout's version, into the snapshot's header; a restore whose configuration gives another header is refused (-12) and writes nothing.
 *
 * Ids.  `ids` / `dst_ids` are DEVICE arrays of K int32 environment indices (NULL: the K = num_envs environments in order), `src_rows`
 * a DEVICE array of K int32 snapshot rows (NULL: row k for entry k).  Snapshot rows may repeat (fan-out); destinations must be
 * distinct, which the host checks where the ids come from the host (the library cannot without reading device memory: two entries with
 * one destination leave one of the two rows there, field by field).  On the device an id outside [0, num_envs) or a row outside
 * [0, num_rows) is never read or written through: the entry is skipped and counted once in the word `skipped` (a device uint32 the
 * caller zeroes; the only atomic in the library).
 *
 * Return codes (the numbering of go1eval.h): -1 no config, no buffers, num_envs <= 0 or K <= 0; -2 no snapshot, or a section's storage
 * or `skipped` missing; -3 a required simulator buffer is NULL; -8 no ids and K != num_envs; -12 a refused geometry: a layout value out
 * of range, lag_head outside [0, lag], history_slot outside [0, R), a restore into another layout, identity rows with K > num_rows;
 * -20 the launch failed.  The first that applies, in this order.
 */
#ifndef GO1STATE_H
#define GO1STATE_H
#include <stdint.h>

#include "go1sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GO1STATE_MAGIC 0x53314F47       /* "GO1S" */
#define GO1STATE_LAYOUT_VERSION 1
#define GO1STATE_HEADER_WORDS 12        /* magic, version, the ten layout values in the order of Go1StateConfig */
#define GO1STATE_MAX_BLOCKS 2048        /* the grid is capped here (eight workgroups of 256 for each of 256 CUs); tiles beyond are strided */

typedef struct Go1StateConfig {
  int32_t num_envs;                     /* N of the simulator's buffers; not part of the layout */
  int32_t num_obs, num_privileged_obs, num_obs_history, lag_timesteps, num_rewards;
  int32_t num_height_points;            /* num_height_x * num_height_y */
  int32_t command_rows;                 /* rows of `commands`: GO1_MAX_COMMANDS */
  int32_t num_categories, num_bins, curriculum_update_interval;
} Go1StateConfig;

typedef struct Go1StateLayout {
  int32_t header[GO1STATE_HEADER_WORDS];
  int32_t word_rows;                    /* W: 4-byte words per environment in the section `words` */
  int32_t byte_rows;                    /* B: bytes per environment in the section `bytes` */
  int32_t row_words;                    /* 4-byte words per environment in the section `rows` */
  int32_t global_words;                 /* G */
  int64_t bytes_per_env;                /* 4 (W + row_words) + B */
} Go1StateLayout;

typedef struct Go1StateSnapshot {
  int32_t header[GO1STATE_HEADER_WORDS]; /* written by go1state_capture / go1state_capture_global, compared by the restores */
  int32_t num_rows;                      /* K of the capture (written by go1state_capture) */
  uint32_t* words;                       /* device [W][num_rows] */
  uint8_t* bytes;                        /* device [B][num_rows] */
  uint32_t* rows;                        /* device [row_words * num_rows] */
  uint32_t* global;                      /* device [G]; only the _global entry points ask for it */
  uint32_t* skipped;                     /* device word: entries skipped for an id or a row out of range */
} Go1StateSnapshot;

/* the packed sizes of a configuration; -1 without cfg or out, -12 for a layout value out of range */
int go1state_layout(const Go1StateConfig* cfg, Go1StateLayout* out);

/* gather the K environments ids[0 .. K) (NULL: all, K = num_envs) into snap, whose storage holds K rows: one launch */
int go1state_capture(const Go1StateConfig* cfg, const Go1SimBuffers* buffers, const int32_t* ids, int32_t K, int32_t lag_head,
                     int32_t history_slot, Go1StateSnapshot* snap, void* stream);

/* scatter snapshot row src_rows[k] (NULL: k) into environment dst_ids[k] (NULL: k, K = num_envs), k in [0, K): one launch */
int go1state_restore(const Go1StateConfig* cfg, const Go1SimBuffers* buffers, const int32_t* dst_ids, const int32_t* src_rows, int32_t K,
                     int32_t lag_head, int32_t history_slot, const Go1StateSnapshot* snap, void* stream);

/* the arrays that are not per environment, to and from snap->global: one launch each */
int go1state_capture_global(const Go1StateConfig* cfg, const Go1SimBuffers* buffers, Go1StateSnapshot* snap, void* stream);
int go1state_restore_global(const Go1StateConfig* cfg, const Go1SimBuffers* buffers, const Go1StateSnapshot* snap, void* stream);

const char* go1state_version(void);

#ifdef __cplusplus
}
#endif
#endif
