"""numpy model of the reward family (include/go1reward.h): the 24 CoRLRewards terms restated from the reference's
go1_gym/envs/rewards/corl_rewards.py (its torch expressions and its torch_utils quaternion helpers, NOT csrc/go1_maps.h), evaluated in
the precision asked for (float64: the reference value; float32: what an fp32 evaluation beside the kernel gives), and the family's
bookkeeping: the snapshot of the four histories the step's roll destroys, the steps that are not measured, the K + 4 rows, the split
into positive and negative terms, the clip, and go1_tables.h's fixed-order group reduction.

A `view` is what the reference's reward functions see during compute_reward(): the SoA buffers ([k][N]) with the step's own
last_actions / last_last_actions / last_joint_pos_target / last_last_joint_pos_target / last_dof_vel / last_contacts.  `step_view`
builds it from the buffers a step left and the family's snapshot, the way the kernel does."""
import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

f32, f64 = np.float32, np.float64
TERMS = ["tracking_lin_vel", "tracking_ang_vel", "lin_vel_z", "ang_vel_xy", "orientation", "torques", "dof_acc", "action_rate", "collision",
         "dof_pos_limits", "jump", "tracking_contacts_shaped_force", "tracking_contacts_shaped_vel", "dof_pos", "dof_vel",
         "action_smoothness_1", "action_smoothness_2", "feet_slip", "feet_contact_vel", "feet_contact_forces", "feet_clearance_cmd_linear",
         "feet_impact_vel", "orientation_control", "raibert_heuristic"]               # ids 0 .. 23: enum GO1_REW_* of include/go1sim.h
NEGATIVE_RAW = ("jump", "tracking_contacts_shaped_force", "tracking_contacts_shaped_vel")     # terms whose raw value is <= 0
EXTRA = ["sum", "positive", "negative", "total"]
GROUP_FIELDS = ["envs", "measured", "reset", "teleported"]
SNAPSHOT = ["last_last_actions", "last_last_joint_pos_target", "last_dof_vel", "last_contacts"]
TELEPORT_DISTANCE = 1.0
FEET_BODIES = [4, 8, 12, 16]


# ---- isaacgym.torch_utils, as the reference calls them (vectors [3][N], quaternions x, y, z, w) ---------------------------------------------
def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def quat_rotate_inverse(q, v):
    w, qv = q[3], q[:3]
    a = v * (2.0 * w * w - 1.0)
    b = _cross(qv, v) * w * 2.0
    c = qv * (qv * v).sum(axis=0) * 2.0
    return a - b + c


def quat_apply(q, v):
    t = _cross(q[:3], v) * 2.0
    return v + q[3] * t + _cross(q[:3], t)


def quat_mul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def quat_from_angle_axis(angle, axis):
    half = angle / 2
    zero = np.zeros_like(angle)
    q = np.stack([np.sin(half) * axis[0] + zero, np.sin(half) * axis[1] + zero, np.sin(half) * axis[2] + zero, np.cos(half)])
    return q / np.sqrt((q * q).sum(axis=0))


def quat_apply_yaw(q, v):
    qy = q.copy()
    qy[:2] = 0
    qy = qy / np.sqrt((qy * qy).sum(axis=0))
    return quat_apply(qy, v)


def _norm3(rows):
    """[3 k][N] -> [k][N]: the norms of k stacked 3-vectors"""
    r = rows.reshape(-1, 3, rows.shape[-1])
    return np.sqrt((r * r).sum(axis=1))


# ---- the terms ----------------------------------------------------------------------------------------------------------------------------------
def terms(S, view, gravity, dtype=f64):
    """{name: (N,) raw value in `dtype`} of all 24 terms on the view (see the module text).  S: the simulator's Go1SimConfig; gravity:
    the gravity vector in force during the step (3,)"""
    c = lambda k: np.asarray(view[k]).astype(dtype)
    with np.errstate(all="ignore"):
        return _terms(S, c, np.asarray(gravity).astype(dtype), dtype, np.asarray(view["last_contacts"]) != 0)


def heights(S, c, dtype):
    """(base height, (4, N) foot heights) the terms read: world z as in the reference, or above the ground where the configuration
    says so (reward_heights_above_terrain, an extension of this project: over the mean of the measured heights; on the plane 0)"""
    base, feet = c("root_states")[2], c("foot_positions")[2::3]
    if S.reward_heights_above_terrain:
        assert S.terrain_type == 0 or S.measure_heights, "the model knows the plane and the measured heights"
        if S.measure_heights:
            np_ = int(S.num_height_x) * int(S.num_height_y)
            base = base - c("measured_heights")[:np_].sum(axis=0) / dtype(np_)
        assert S.terrain_type == 0, "foot heights above a height field are not modelled"
    return base, feet


def _terms(S, c, gravity, dtype, last_contacts):
    D = dtype
    cmd, blv, bav, pg = c("commands"), c("base_lin_vel"), c("base_ang_vel"), c("projected_gravity")
    q, qd, tq = c("dof_pos"), c("dof_vel"), c("torques")
    act, lact, llact = c("actions"), c("last_actions"), c("last_last_actions")
    jpt, ljpt, lljpt = c("joint_pos_target"), c("last_joint_pos_target"), c("last_last_joint_pos_target")
    cf = c("contact_forces")
    body_force = _norm3(cf)                                                           # (17, N)
    foot_force = body_force[FEET_BODIES]                                              # (4, N)
    fpos, fvel = c("foot_positions").reshape(4, 3, -1), c("foot_velocities").reshape(4, 3, -1)
    desired, findex = c("desired_contact_states"), c("foot_indices")
    base_h, foot_h = heights(S, c, D)
    rs = c("root_states")
    out = {}
    out["tracking_lin_vel"] = np.exp(-((cmd[:2] - blv[:2]) ** 2).sum(axis=0) / D(S.tracking_sigma))
    out["tracking_ang_vel"] = np.exp(-((cmd[2] - bav[2]) ** 2) / D(S.tracking_sigma_yaw))
    out["lin_vel_z"] = blv[2] ** 2
    out["ang_vel_xy"] = (bav[:2] ** 2).sum(axis=0)
    out["orientation"] = (pg[:2] ** 2).sum(axis=0)
    out["torques"] = (tq ** 2).sum(axis=0)
    out["dof_acc"] = (((c("last_dof_vel") - qd) / D(S.dt)) ** 2).sum(axis=0)
    out["action_rate"] = ((lact - act) ** 2).sum(axis=0)
    penalised = [b for b in range(17) if (int(S.penalised_body_mask) >> b) & 1]
    out["collision"] = (body_force[penalised] > D(0.1)).astype(D).sum(axis=0) if penalised else np.zeros(q.shape[1], D)
    lower = np.array([S.dof_pos_soft_lower[j] for j in range(12)], D)[:, None]
    upper = np.array([S.dof_pos_soft_upper[j] for j in range(12)], D)[:, None]
    out["dof_pos_limits"] = (-np.minimum(q - lower, 0) + np.maximum(q - upper, 0)).sum(axis=0)
    out["jump"] = -(base_h - (cmd[3] + D(S.base_height_target))) ** 2
    out["tracking_contacts_shaped_force"] = (-(1 - desired) * (1 - np.exp(-1 * foot_force ** 2 / D(S.gait_force_sigma)))).sum(axis=0) / 4
    foot_speed = np.sqrt((fvel ** 2).sum(axis=1))
    out["tracking_contacts_shaped_vel"] = (-(desired * (1 - np.exp(-1 * foot_speed ** 2 / D(S.gait_vel_sigma))))).sum(axis=0) / 4
    default = np.array([S.default_dof_pos[j] for j in range(12)], D)[:, None]
    out["dof_pos"] = ((q - default) ** 2).sum(axis=0)
    out["dof_vel"] = (qd ** 2).sum(axis=0)
    out["action_smoothness_1"] = (((jpt - ljpt) ** 2) * (lact != 0)).sum(axis=0)
    out["action_smoothness_2"] = (((jpt - 2 * ljpt + lljpt) ** 2) * (lact != 0) * (llact != 0)).sum(axis=0)
    contact = cf[[3 * b + 2 for b in FEET_BODIES]] > 1.0
    out["feet_slip"] = ((contact | last_contacts) * (fvel[:, 0] ** 2 + fvel[:, 1] ** 2)).sum(axis=0)
    out["feet_contact_vel"] = ((foot_h < D(0.03)) * (fvel ** 2).sum(axis=1)).sum(axis=0)
    out["feet_contact_forces"] = np.maximum(foot_force - D(S.max_contact_force), 0).sum(axis=0)
    phases = 1 - np.abs(1.0 - np.clip(findex * 2.0 - 1.0, 0.0, 1.0) * 2.0)
    out["feet_clearance_cmd_linear"] = (((cmd[9] * phases + D(0.02)) - foot_h) ** 2 * (1 - desired)).sum(axis=0)
    out["feet_impact_vel"] = ((foot_force > 1.0) * np.clip(c("prev_foot_velocities")[2::3], -100, 0) ** 2).sum(axis=0)
    n = q.shape[1]
    ones = np.ones(n, D)
    quat_roll = quat_from_angle_axis(-cmd[11], np.array([1, 0, 0], D))
    quat_pitch = quat_from_angle_axis(-cmd[10], np.array([0, 1, 0], D))
    gvec = (gravity / np.sqrt((gravity * gravity).sum()))[:, None] * ones
    desired_pg = quat_rotate_inverse(quat_mul(quat_roll, quat_pitch), gvec)
    out["orientation_control"] = ((pg[:2] - desired_pg[:2]) ** 2).sum(axis=0)
    conj = np.stack([-rs[3], -rs[4], -rs[5], rs[6]])
    width = cmd[12] if S.num_commands >= 13 else D(0.3) * ones
    length = cmd[13] if S.num_commands >= 14 else D(0.45) * ones
    ys_nom = np.stack([width / 2, -width / 2, width / 2, -width / 2])
    xs_nom = np.stack([length / 2, length / 2, -length / 2, -length / 2])
    ph = np.abs(1.0 - findex * 2.0) * 1.0 - 0.5
    y_vel = cmd[2] * length / 2
    ys_off = ph * y_vel * (0.5 / cmd[4])
    ys_off[2:4] *= -1
    xs_off = ph * cmd[0] * (0.5 / cmd[4])
    err = np.zeros(n, D)
    for i in range(4):
        body = quat_apply_yaw(conj, fpos[i] - rs[:3])
        err = err + np.abs((xs_nom[i] + xs_off[i]) - body[0]) ** 2 + np.abs((ys_nom[i] + ys_off[i]) - body[1]) ** 2
    out["raibert_heuristic"] = err
    assert list(out) == TERMS and all(v.dtype == D for v in out.values()), [(k, v.dtype) for k, v in out.items() if v.dtype != D]
    return out


def active(S):
    """[(term name, scale as np.float32)] in the configuration's order"""
    return [(TERMS[int(S.reward_ids[k])], f32(S.reward_scales[k])) for k in range(int(S.num_rewards))]


def rows(S, raw, dtype=f64):
    """(K + 4, N) in `dtype`: the K scaled terms in the configuration's order, then the four rows of combine()"""
    scaled = np.stack([raw[name].astype(dtype) * dtype(scale) for name, scale in active(S)])
    return np.concatenate([scaled, combine(S, scaled, dtype)])


def combine(S, scaled, dtype=f64):
    """(4, N) in `dtype` from the (K, N) scaled terms: sum, positive, negative (the terms are added in id order; a term counts as
    positive when the sign of its raw value times its scale is >= 0) and total (after only_positive_rewards or the ji22 rule)"""
    D = dtype
    act = active(S)
    scaled = np.asarray(scaled).astype(D)
    n = scaled.shape[1]
    total, pos, neg = np.zeros(n, D), np.zeros(n, D), np.zeros(n, D)
    for name in TERMS:                                                                # id order
        for (nm, scale), r in zip(act, scaled):
            if nm != name:
                continue
            total = total + r
            if (-1 if name in NEGATIVE_RAW else 1) * float(scale) >= 0:
                pos = pos + r
            else:
                neg = neg + r
    with np.errstate(all="ignore"):
        if S.only_positive_rewards:
            clipped = np.maximum(total, 0)
        elif S.only_positive_rewards_ji22_style:
            clipped = pos * np.exp(neg / D(S.sigma_rew_neg))
        else:
            clipped = total
    return np.stack([total, pos, neg, clipped])


# ---- the bookkeeping ------------------------------------------------------------------------------------------------------------------------------
def step_view(post, snap):
    """the view of the step that left the buffers `post`, given the snapshot `snap` taken before it (see the module text)"""
    view = dict(post)
    view["last_actions"] = post["last_last_actions"]                                  # rolled by the step, still there
    view["last_joint_pos_target"] = post["last_last_joint_pos_target"]
    for k in SNAPSHOT:                                                                # lost in the roll: the post-step values of the step before
        view[k] = snap[k]
    return view


def not_measured(post, warmup_steps=0):
    """(reset, teleported, warm-up) masks of a step, exclusive and in this precedence"""
    reset = np.asarray(post["reset_buf"]) != 0
    rs, fp = np.asarray(post["root_states"]), np.asarray(post["foot_positions"])
    with np.errstate(all="ignore"):
        d2 = (rs[0] - fp[0::3]) ** 2 + (rs[1] - fp[1::3]) ** 2                        # fp32, as stored
        far = (d2 > f32(TELEPORT_DISTANCE) * f32(TELEPORT_DISTANCE)).any(axis=0) & ~reset
    warm = (np.asarray(post["episode_length_buf"]) <= warmup_steps) & ~reset & ~far
    return reset, far, warm


class State:
    """the accumulators ([K + 4][N]), the snapshot, the last step's rows and the counts, after go1reward_arm on the buffers `post`"""

    def __init__(self, S, post, warmup_steps=0):
        N = self.N = np.asarray(post["reset_buf"]).shape[0]
        K = self.K = int(S.num_rewards)
        R = self.R = K + len(EXTRA)
        self.S, self.warmup_steps = S, warmup_steps
        self.count, self.nonfinite = np.zeros((R, N), np.uint32), np.zeros((R, N), np.uint32)
        self.sum, self.sumsq = np.zeros((R, N)), np.zeros((R, N))
        self.min, self.max = np.full((R, N), np.inf, f32), np.full((R, N), -np.inf, f32)
        self.last_raw, self.last_scaled = np.full((K, N), np.nan), np.full((R, N), np.nan)
        self.last_valid = np.zeros(N, np.uint8)
        self.measured, self.resets, self.teleported = (np.zeros(N, np.uint32) for _ in range(3))
        self.snapshot(post)

    def snapshot(self, post):
        self.snap = {k: np.array(post[k]) for k in SNAPSHOT}

    def fold(self, row, live, v):
        """fold the np.float32 vector v into `row` for the environments `live` (go1_tables.h fold)"""
        assert v.dtype == f32
        fin = np.isfinite(v)
        self.nonfinite[row] += (live & ~fin).astype(np.uint32)
        ok = live & fin
        self.count[row] += ok.astype(np.uint32)
        v64 = v.astype(f64)
        with np.errstate(all="ignore"):
            np.add(self.sum[row], v64, out=self.sum[row], where=ok)
            np.add(self.sumsq[row], v64 * v64, out=self.sumsq[row], where=ok)
            np.fmin(self.min[row], v, out=self.min[row], where=ok)
            np.fmax(self.max[row], v, out=self.max[row], where=ok)

    def accumulate(self, post, gravity, dtype=f64, values=None):
        """one go1reward_accumulate launch on the buffers `post` a step left.  The rows are the model's in `dtype`, rounded to fp32 for the
        fold, or `values` ((K + 4, N) np.float32, e.g. the kernel's own last_scaled) where the test is about the bookkeeping alone.
        Returns the (K + 4, N) rows in `dtype` (NaN where the step is not measured)."""
        reset, far, warm = not_measured(post, self.warmup_steps)
        live = ~(reset | far | warm)
        self.resets += reset.astype(np.uint32)
        self.teleported += far.astype(np.uint32)
        self.measured += live.astype(np.uint32)
        view = step_view(post, self.snap)
        raw = terms(self.S, view, gravity, dtype)
        table = rows(self.S, raw, dtype)
        folded = table.astype(f32) if values is None else np.asarray(values, f32)
        for r in range(self.R):
            self.fold(r, live, folded[r])
        self.last_raw = np.where(live, np.stack([raw[name] for name, _ in active(self.S)]), np.nan)
        self.last_scaled = np.where(live, table, np.nan)
        self.last_valid = live.astype(np.uint8)
        self.snapshot(post)                                                           # on every step, measured or not
        return self.last_scaled


def reduce(acc, counts, group, num_groups):
    """((G, K + 4, 6) result table, (G, 4) counts) of go1reward_reduce: go1_tables.h's fixed order.  acc: {"count", "sum", "sumsq", "min",
    "max", "nonfinite"} arrays ([K + 4][N]); counts: {"measured", "resets", "teleported"} ([N])"""
    group = np.asarray(group)
    R, N = acc["count"].shape
    out, gout = np.zeros((num_groups, R, len(E.FIELDS))), np.zeros((num_groups, len(GROUP_FIELDS)))
    counted = acc["count"] > 0
    lows = np.where(counted, acc["min"].astype(f64), np.inf)
    highs = np.where(counted, acc["max"].astype(f64), -np.inf)
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        n = _combine_rows(acc["count"].astype(f64), members, np.add, 0.0)
        nf = _combine_rows(acc["nonfinite"].astype(f64), members, np.add, 0.0)
        s, q = _combine_rows(acc["sum"], members, np.add, 0.0), _combine_rows(acc["sumsq"], members, np.add, 0.0)
        low, high = _combine_rows(lows, members, np.fmin, np.inf), _combine_rows(highs, members, np.fmax, -np.inf)
        with np.errstate(all="ignore"):
            mean = s / n
            var = q / n - mean * mean
            table = np.stack([n, mean, np.sqrt(np.fmax(var, 0.0)), low, high, nf], axis=1)
        table[~(n > 0), 1:5] = np.nan
        out[g] = table
        per_env = np.stack([np.ones(N), counts["measured"].astype(f64), counts["resets"].astype(f64), counts["teleported"].astype(f64)])
        gout[g] = _combine_rows(per_env, members, np.add, 0.0)
    return out, gout


# ---- TEST DATA: synthetic post-step buffers for the emulator test and the GPU test -----------------------------------------------------------
# the simulator buffers a go1reward_accumulate launch reads (SoA, [k][N]); the four of SNAPSHOT are read by the snapshot
BUFFERS = ["root_states", "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "torques", "dof_pos", "dof_vel", "actions",
           "joint_pos_target", "contact_forces", "foot_positions", "foot_velocities", "prev_foot_velocities", "foot_indices",
           "desired_contact_states", "measured_heights", "last_last_actions", "last_last_joint_pos_target", "last_dof_vel", "last_contacts",
           "reset_buf", "episode_length_buf"]
STANCE = np.array([[0.19, 0.14], [0.19, -0.14], [-0.19, 0.14], [-0.19, -0.14]], f32)          # FL, FR, RL, RR about the base


def synthetic_env(rng, S, events=True):
    """one environment's buffers after a step (a column each): a trotting-like state with every term awake.  With `events`, now and then
    a reset, a base teleported away from its feet, a young episode, a joint beyond its soft limit, a first step (last actions 0)"""
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, shape).astype(f32)
    p = {}
    rs = np.zeros(13, f32)
    rs[0:2], rs[2] = u(-3, 3, 2), u(0.22, 0.36)
    q = np.array([*rng.normal(0, 0.08, 2), *rng.normal(0, 1.0, 1), 1.0])
    rs[3:7] = (q / np.linalg.norm(q)).astype(f32)
    rs[7:13] = rng.normal(0, 0.4, 6).astype(f32)
    p["root_states"] = rs
    p["base_lin_vel"], p["base_ang_vel"] = rng.normal(0, 0.5, 3).astype(f32), rng.normal(0, 0.6, 3).astype(f32)
    g = np.array([*rng.normal(0, 0.1, 2), -1.0])
    p["projected_gravity"] = (g / np.linalg.norm(g)).astype(f32)
    cmd = np.zeros(15, f32)
    cmd[0:3], cmd[3], cmd[4] = u(-1, 1, 3), u(-0.1, 0.1), u(2.0, 4.0)
    cmd[5:8], cmd[8], cmd[9], cmd[10:12], cmd[12], cmd[13] = u(0, 1, 3), 0.5, u(0.03, 0.25), u(-0.3, 0.3, 2), u(0.25, 0.45), u(0.35, 0.45)
    p["commands"] = cmd
    default = np.array([S.default_dof_pos[j] for j in range(12)], f32)
    p["torques"], p["dof_pos"], p["dof_vel"] = rng.normal(0, 6, 12).astype(f32), default + rng.normal(0, 0.25, 12).astype(f32), rng.normal(0, 3, 12).astype(f32)
    p["actions"], p["last_last_actions"] = rng.normal(0, 1, 12).astype(f32), rng.normal(0, 1, 12).astype(f32)
    p["joint_pos_target"] = default + f32(0.25) * p["actions"]
    p["last_last_joint_pos_target"] = default + f32(0.25) * p["last_last_actions"]
    p["last_dof_vel"] = rng.normal(0, 3, 12).astype(f32)
    cf = np.zeros(51, f32)
    stance = rng.random(4) < 0.6
    for f in range(4):
        if stance[f]:
            cf[12 * (f + 1):12 * (f + 1) + 3] = [rng.normal(0, 8), rng.normal(0, 8), rng.uniform(0.5, 120)]
    if rng.random() < 0.2:
        cf[3 * int(rng.integers(0, 17)):][:3] = rng.normal(0, 2, 3)                   # a body that is no foot touches something
    p["contact_forces"] = cf
    feet = np.zeros((4, 3), f32)
    c, s = np.cos(2 * np.arctan2(rs[5], rs[6])), np.sin(2 * np.arctan2(rs[5], rs[6]))
    for f in range(4):
        x, y = STANCE[f] + rng.normal(0, 0.04, 2)
        feet[f] = [rs[0] + c * x - s * y, rs[1] + s * x + c * y, 0.02 if stance[f] else rng.uniform(0.02, 0.12)]
    p["foot_positions"] = feet.reshape(12)
    p["foot_velocities"] = (rng.normal(0, 0.8, (4, 3)) * np.where(stance, 0.05, 1.0)[:, None]).astype(f32).reshape(12)
    p["prev_foot_velocities"] = rng.normal(0, 0.8, 12).astype(f32)
    p["foot_indices"], p["desired_contact_states"] = u(0, 1, 4), u(0, 1, 4)
    p["measured_heights"] = np.zeros(max(int(S.num_height_x) * int(S.num_height_y), 1), f32)
    p["last_contacts"] = (rng.random(4) < 0.5).astype(np.uint8)
    p["reset_buf"], p["episode_length_buf"] = np.uint8(0), np.int32(rng.integers(5, 400))
    if events:
        kind = rng.random()
        if kind < 0.08:
            p["reset_buf"] = np.uint8(1)
        elif kind < 0.16:
            p["root_states"][0] += f32(4.0)                                           # teleported: 4 m from where its feet are
        elif kind < 0.24:
            p["episode_length_buf"] = np.int32(rng.integers(1, 4))
        elif kind < 0.32:
            p["dof_pos"][int(rng.integers(0, 12))] += f32(3.0)
        elif kind < 0.40:
            p["last_last_actions"][:] = 0
    return p


def synthetic_steps(rng, S, M, steps):
    """`steps` consecutive post-step buffer sets of M distinct environments, each {name: [k][M] array}"""
    out = []
    for _ in range(steps):
        cols = [synthetic_env(rng, S) for _ in range(M)]
        out.append({k: np.stack([c[k] for c in cols], axis=-1) for k in BUFFERS})
    return out


def place(post, index):
    """the buffer set with environment columns `index` (permuted, tiled)"""
    return {k: np.ascontiguousarray(v[..., index]) for k, v in post.items()}


def load(B, post):
    """write a buffer set into the tensors of a go1sim_host.SimBuffers"""
    import torch
    for k, v in post.items():
        B.tensors[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))


def read(B):
    """the buffer set a go1sim_host.SimBuffers holds, as numpy arrays"""
    return {k: B.tensors[k].detach().cpu().numpy().copy() for k in BUFFERS}
