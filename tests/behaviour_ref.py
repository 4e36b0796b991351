"""TEST INFRASTRUCTURE: fp64 numpy model of libgo1eval's behaviour kernels, written from the text of include/go1eval.h (the
seven per-step formulas, the stride rules, the accumulate order).  The group reduction is eval_ref.py's: the header gives both
tables one rule.  The GPU tests replay recorded steps through it; the CPU tests pin it to hand-computable cases."""
import numpy as np

import eval_ref as E

METRICS = ["contact_match", "body_height_err", "orientation_err", "feet_clearance", "raibert_heuristic", "feet_slip", "action_rate",
           "step_frequency_err", "duty_factor_err", "swing_height_err"]
M = len(METRICS)
PER_STEP, STRIDE = list(range(7)), [7, 8, 9]
FREQ, DUTY, SWING = 7, 8, 9
FEET_BODIES = (4, 8, 12, 16)
CONTACT_FORCE, FOOT_RADIUS = 1.0, 0.02
# the buffers go1eval_behaviour_accumulate reads (SoA, [k][N]); measured_heights may be absent (None)
INPUTS = ["commands", "root_states", "measured_heights", "contact_forces", "foot_positions", "foot_velocities", "desired_contact_states",
          "foot_indices", "last_actions", "last_last_actions", "reset_buf", "episode_length_buf"]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _rotate(q, v):
    """R(q) v, q = (x, y, z, w) rows, v = 3 rows"""
    u, w = q[:3], q[3]
    t = 2.0 * _cross(u, v)
    return v + w * t + _cross(u, t)


def _rotate_inverse(q, v):
    return _rotate(np.concatenate([-q[:3], q[3:4]]), v)


def contacts(snap):
    """(4, N) bool"""
    F = np.asarray(snap["contact_forces"], np.float64)
    return np.stack([F[3 * b + 2] > CONTACT_FORCE for b in FEET_BODIES])


def foot_heights(snap):
    return np.asarray(snap["foot_positions"], np.float64)[2::3]


def step_values(snap, num_commands, base_height_target):
    """(7, N) fp64: the per-step metrics of one step from the SoA buffers `snap`, every operation in fp64"""
    f = {k: (None if snap.get(k) is None else np.asarray(snap[k], np.float64)) for k in INPUTS[:10]}
    cmd, root = f["commands"], f["root_states"]
    N = root.shape[1]
    out = np.zeros((7, N))
    contact = contacts(snap)
    desired, index = f["desired_contact_states"], f["foot_indices"]
    out[0] = 0.25 * (contact == (desired > 0.5)).sum(axis=0)
    z = root[2]
    height = z if f["measured_heights"] is None else (z[None, :] - f["measured_heights"]).mean(axis=0)
    out[1] = height - (cmd[3] + np.float64(np.float32(base_height_target)))
    q = root[3:7]
    down = np.stack([np.zeros(N), np.zeros(N), -np.ones(N)])
    sr, cr, sp, cp = np.sin(-cmd[11] / 2), np.cos(-cmd[11] / 2), np.sin(-cmd[10] / 2), np.cos(-cmd[10] / 2)
    d = _rotate_inverse(q, down) - _rotate_inverse(np.stack([sr * cp, cr * sp, sr * sp, cr * cp]), down)
    out[2] = np.sqrt(d[0] ** 2 + d[1] ** 2)
    pos = f["foot_positions"].reshape(4, 3, N)
    vel = f["foot_velocities"].reshape(4, 3, N)
    width = cmd[12] if num_commands >= 13 else np.float64(np.float32(0.3))
    length = cmd[13] if num_commands >= 14 else np.float64(np.float32(0.45))
    yaw_norm = np.maximum(np.sqrt(q[2] ** 2 + q[3] ** 2), np.float64(np.float32(1e-9)))
    yaw = np.stack([np.zeros(N), np.zeros(N), -q[2] / yaw_norm, q[3] / yaw_norm])
    with np.errstate(divide="ignore", invalid="ignore"):
        half_period = 0.5 / cmd[4]
        for k in range(4):
            ph = 1.0 - np.abs(1.0 - 2.0 * np.clip(2.0 * index[k] - 1.0, 0.0, 1.0))
            out[3] += (cmd[9] * ph + np.float64(np.float32(FOOT_RADIUS)) - pos[k, 2]) ** 2 * (1.0 - desired[k])
            b = _rotate(yaw, pos[k] - root[0:3])
            xs = (1.0 if k < 2 else -1.0) * length / 2
            ys = (1.0 if k % 2 == 0 else -1.0) * width / 2
            ph = np.abs(1.0 - 2.0 * index[k]) - 0.5
            xo = ph * cmd[0] * half_period
            yo = ph * (cmd[2] * length / 2) * half_period * (1.0 if k < 2 else -1.0)
            out[4] += (xs + xo - b[0]) ** 2 + (ys + yo - b[1]) ** 2
            out[5] += np.where(contact[k], vel[k, 0] ** 2 + vel[k, 1] ** 2, 0.0)
    out[6] = ((f["last_actions"] - f["last_last_actions"]) ** 2).sum(axis=0)
    return out


class State(E.Accumulators):
    """the six accumulator arrays of eval_ref.Accumulators, shaped for the behaviour table, and the per-foot stride state"""

    def __init__(self, N):
        super().__init__(N)
        for k in ("count", "nonfinite"):
            setattr(self, k, np.zeros((M, N), np.int64))
        self.sum, self.sumsq = np.zeros((M, N)), np.zeros((M, N))
        self.min, self.max = np.full((M, N), np.inf), np.full((M, N), -np.inf)
        self.prev_contact = np.full((4, N), 2, np.int64)
        self.stride_steps = np.full((4, N), -1, np.int64)
        self.stance_steps = np.zeros((4, N), np.int64)
        self.swing_peak = np.full((4, N), -np.inf)
        # bookkeeping of the tests
        self.completed_strides = 0        # strides folded
        self.discarded_strides = 0        # strides under way (stride_steps >= 0) that a reset or the warm-up ended
        self.double_touchdowns = 0        # environment-steps in which two or more feet touched down
        self.excluded = 0                 # environment-steps rule 1 dropped


def accumulate(st, values, contact, foot_z, commands, reset_buf, episode_length_buf, warmup_steps, dt):
    """one go1eval_behaviour_accumulate launch.  values: (7, N) per-step metric values; contact (4, N) bool; foot_z (4, N);
    commands (>= 10, N)"""
    contact = np.asarray(contact, bool)
    foot_z, cmd = np.asarray(foot_z, np.float64), np.asarray(commands, np.float64)
    dropped = np.asarray(reset_buf).astype(bool) | (np.asarray(episode_length_buf).astype(np.int64) <= warmup_steps)       # rule 1
    st.excluded += int(dropped.sum())
    st.discarded_strides += int(((st.stride_steps >= 0) & dropped[None, :]).sum())
    st.prev_contact[:, dropped] = 2
    st.stride_steps[:, dropped] = -1
    live = ~dropped                                                                                                          # rule 2
    for m in PER_STEP:
        st._fold(m, live, np.asarray(values[m], np.float64))
    touched = np.zeros(st.N, np.int64)
    dt = np.float64(np.float32(dt))
    for f in range(4):
        touchdown = live & contact[f] & (st.prev_contact[f] == 0)
        touched += touchdown
        ended = touchdown & (st.stride_steps[f] >= 0)
        st.completed_strides += int(ended.sum())
        L = np.where(ended, st.stride_steps[f], 1).astype(np.float64)
        with np.errstate(all="ignore"):
            st._fold(FREQ, ended, 1.0 / (L * dt) - cmd[4])
            st._fold(DUTY, ended, st.stance_steps[f] / L - cmd[8])
            st._fold(SWING, ended, (st.swing_peak[f] - np.float64(np.float32(FOOT_RADIUS))) - cmd[9])
        st.stride_steps[f][touchdown] = 0
        st.stance_steps[f][touchdown] = 0
        st.swing_peak[f][touchdown] = -np.inf
        st.stride_steps[f] += live & (st.stride_steps[f] >= 0)
        st.stance_steps[f] += live & contact[f]
        st.swing_peak[f] = np.where(live, np.maximum(st.swing_peak[f], foot_z[f]), st.swing_peak[f])
        st.prev_contact[f] = np.where(live, contact[f].astype(np.int64), st.prev_contact[f])
    st.double_touchdowns += int((touched >= 2).sum())


def accumulate_snapshot(st, snap, warmup_steps, dt, num_commands, base_height_target, values=None):
    """`values`: per-step metric values computed elsewhere (the fp32 host definitions); default: this model's"""
    with np.errstate(all="ignore"):
        v = step_values(snap, num_commands, base_height_target) if values is None else values
    accumulate(st, v, contacts(snap), foot_heights(snap), snap["commands"], snap["reset_buf"], snap["episode_length_buf"], warmup_steps, dt)


def reduce(st, group, num_groups):
    """(G, M, 6) fp64 result table of go1eval_behaviour_reduce: eval_ref.reduce's metric rows (M happens to equal eval_ref.M)"""
    assert M == E.M
    return E.reduce(st, group, num_groups)[:, :M, :]
