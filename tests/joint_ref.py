"""TEST INFRASTRUCTURE: numpy model of libgo1eval's per-joint kernels, written from the text of include/go1eval.h (sixth kernel family:
the ten values per joint and step, the torque-speed histogram, the folding rules, the previous-velocity rule, the metric rows, the
group row and the histogram table).  Every value is formed in np.float32 in the header's operation order and summed in float64, so
accumulators, state and both result tables are compared with the kernels' bit for bit.  The group reduction is eval_ref.py's fixed
order (thread t combines environments t, t + 256, ... in ascending order, then the binary tree), vectorised over the rows."""
import types

import numpy as np

import eval_ref as E

METRICS = ["torque_abs", "torque_sq", "vel_abs", "vel_sq", "acc_sq", "power_pos", "power_neg", "pos_limit_excess", "torque_saturated",
           "vel_saturated"]
TORQUE_ABS, TORQUE_SQ, VEL_ABS, VEL_SQ, ACC_SQ, POWER_POS, POWER_NEG, POS_LIMIT_EXCESS, TORQUE_SATURATED, VEL_SATURATED = range(10)
M, DOF, TAU_BINS, VEL_BINS = len(METRICS), 12, 8, 8
CELLS = TAU_BINS * VEL_BINS
ROWS = DOF * M + 1
GROUP_FIELDS = ["envs", "steps", "resets"]
# the buffers go1eval_joint_accumulate reads (SoA, [k][N])
INPUTS = ["torques", "dof_vel", "dof_pos", "reset_buf", "episode_length_buf"]
STATE = ["prev_dof_vel", "steps", "resets", "hist"]
f32 = np.float32


def config(dt=0.02, soft_torque_limit=1.0, soft_vel_limit=1.0, torque_limit=(33.5,) * 12, vel_limit=(50.0, 28.0, 28.0) * 4,
           pos_lower=(-0.72, -0.78, -2.6) * 4, pos_upper=(0.72, 3.92, -1.0) * 4, warmup_steps=0):
    """what Go1JointConfig says"""
    return types.SimpleNamespace(dt=dt, soft_torque_limit=soft_torque_limit, soft_vel_limit=soft_vel_limit, torque_limit=list(torque_limit),
                                 vel_limit=list(vel_limit), pos_lower=list(pos_lower), pos_upper=list(pos_upper), warmup_steps=warmup_steps)


def bin_of(x, limit, bins=8):
    """the histogram bin of the finite np.float32 values x on the scale `limit`: clamped as a float, then converted"""
    with np.errstate(over="ignore"):
        b = np.floor((x / f32(limit) + f32(1.0)) * f32(4.0))
    assert b.dtype == f32
    b = np.where(b > f32(bins - 1), f32(bins - 1), np.where(b > f32(0.0), b, f32(0.0)))
    return b.astype(np.int64)


def step_values(cfg, j, tau, qd, q, prev):
    """(10, n) np.float32: the ten values of joint j for the np.float32 vectors tau, qd, q, prev"""
    assert all(a.dtype == f32 for a in (tau, qd, q, prev))
    zero, one = f32(0.0), f32(1.0)
    with np.errstate(all="ignore"):
        d = (prev - qd) / f32(cfg.dt)
        p = tau * qd
        lo, hi = q - f32(cfg.pos_lower[j]), q - f32(cfg.pos_upper[j])
        excess = np.where(lo < zero, -lo, zero) + np.where(hi > zero, hi, zero)
        excess = np.where(np.isnan(q), q, excess)
        values = [np.abs(tau), tau * tau, np.abs(qd), qd * qd, d * d, np.where(p > zero, p, zero), np.where(p < zero, -p, zero), excess,
                  np.where(np.abs(tau) >= f32(cfg.soft_torque_limit) * f32(cfg.torque_limit[j]), one, zero),
                  np.where(np.abs(qd) >= f32(cfg.soft_vel_limit) * f32(cfg.vel_limit[j]), one, zero)]
    assert all(v.dtype == f32 for v in values)
    return np.stack(values)


class State:
    """the accumulators and the state, in the kernel's own number formats"""

    def __init__(self, N, dof_vel):
        self.N = N
        R = DOF * M
        self.count, self.nonfinite = np.zeros((R, N), np.uint32), np.zeros((R, N), np.uint32)
        self.sum, self.sumsq = np.zeros((R, N)), np.zeros((R, N))
        self.min, self.max = np.full((R, N), np.inf, f32), np.full((R, N), -np.inf, f32)
        self.prev_dof_vel = np.array(dof_vel, f32)                       # go1eval_joint_clear
        self.steps, self.resets = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        self.hist = np.zeros((DOF, CELLS, N), np.uint32)

    def fold(self, row, live, v):
        """fold the np.float32 vector v into `row` for the environments `live`"""
        fin = np.isfinite(v)
        self.nonfinite[row] += (live & ~fin).astype(np.uint32)
        ok = live & fin
        self.count[row] += ok.astype(np.uint32)
        v64 = v.astype(np.float64)
        with np.errstate(all="ignore"):
            np.add(self.sum[row], v64, out=self.sum[row], where=ok)
            np.add(self.sumsq[row], v64 * v64, out=self.sumsq[row], where=ok)
            np.fmin(self.min[row], v, out=self.min[row], where=ok)
            np.fmax(self.max[row], v, out=self.max[row], where=ok)

    def arrays(self):
        return {k: getattr(self, k) for k in ["count", "sum", "sumsq", "min", "max", "nonfinite"] + STATE}


def accumulate(st, cfg, snap):
    """one go1eval_joint_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays)"""
    reset = snap["reset_buf"] != 0
    st.steps += 1                                                                        # 1
    st.resets += reset.astype(np.uint32)
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)                      # 2, 3
    env = np.arange(st.N)
    for j in range(DOF):
        tau, qd, q = snap["torques"][j], snap["dof_vel"][j], snap["dof_pos"][j]
        values = step_values(cfg, j, tau, qd, q, st.prev_dof_vel[j])                     # 4
        for m in range(M):
            st.fold(j * M + m, live, values[m])
        sample = live & np.isfinite(tau) & np.isfinite(qd)
        safe_tau, safe_qd = np.where(sample, tau, f32(0.0)), np.where(sample, qd, f32(0.0))
        cell = bin_of(safe_tau, cfg.torque_limit[j], TAU_BINS) * VEL_BINS + bin_of(safe_qd, cfg.vel_limit[j], VEL_BINS)
        st.hist[j, cell[sample], env[sample]] += 1
        st.prev_dof_vel[j] = qd                                                          # 5
    return st


def _combine_rows(per_env, members, op, init):
    """eval_ref._combine for every row of per_env (rows, N) at once: the same adds in the same order, elementwise"""
    T = E.REDUCE_THREADS
    partials = np.full((T, per_env.shape[0]), init, np.float64)
    for e in members:
        partials[e % T] = op(partials[e % T], per_env[:, e])
    s = T // 2
    while s > 0:
        partials[:s] = op(partials[:s], partials[s:2 * s])
        s //= 2
    return partials[0]


def reduce(st, group, num_groups):
    """((G, 12 * 10 + 1, 6) fp64 result table, (G, 12, 8, 8) uint64 histogram table) of go1eval_joint_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    hist = np.zeros((num_groups, DOF, TAU_BINS, VEL_BINS), np.uint64)
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        n = _combine_rows(st.count.astype(np.float64), members, np.add, 0.0)
        nf = _combine_rows(st.nonfinite.astype(np.float64), members, np.add, 0.0)
        S, Q = _combine_rows(st.sum, members, np.add, 0.0), _combine_rows(st.sumsq, members, np.add, 0.0)
        low, high = _combine_rows(lows, members, np.fmin, np.inf), _combine_rows(highs, members, np.fmax, -np.inf)
        some = n > 0
        with np.errstate(all="ignore"):
            mean = S / n
            var = Q / n - mean * mean
            rows = np.stack([n, mean, np.sqrt(np.fmax(var, 0.0)), low, high, nf], axis=1)
        rows[~some, 1:5] = np.nan
        out[g, :DOF * M] = rows
        per_env = np.stack([np.ones(st.N), st.steps.astype(np.float64), st.resets.astype(np.float64)])
        out[g, DOF * M, :3] = _combine_rows(per_env, members, np.add, 0.0)
        hist[g] = st.hist[:, :, members].astype(np.uint64).sum(axis=2).reshape(DOF, TAU_BINS, VEL_BINS)
    return out, hist


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP = 12, 2
KINDS = ["ordinary", "resets", "torque_edges", "speed_edges", "position_edges", "nonfinite", "never_moves"]


def script_config():
    """soft factors below 1 and joint-dependent limits, so that a limit, its soft share and the bin edges are all different numbers"""
    return config(dt=0.02, soft_torque_limit=0.9, soft_vel_limit=0.8, torque_limit=(33.5, 30.0, 35.5) * 4, warmup_steps=SCRIPT_WARMUP)


def edge_values(limit, soft):
    """np.float32 values on and around everything the header compares x with on the scale `limit`: +-limit, soft * limit and one ulp
    either side of each, every bin edge and one ulp either side, +-0, and +-1e30 (finite, far beyond an int's range once scaled)"""
    L, s = f32(limit), f32(soft) * f32(limit)
    out = []
    for v in [L, -L, s, -s] + [L * (f32(k) / f32(4.0) - f32(1.0)) for k in range(9)]:
        out += [v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))]
    return np.array(out + [0.0, -0.0, 1e30, -1e30], f32)


def scripted_steps(rng, N, steps=SCRIPT_STEPS):
    """`steps` snapshots of the input buffers for N environments, the velocities at the clear, and the kind of every environment:
    ordinary ones; ones that reset on the first step, mid-script and twice in a row (their episode_length_buf starts again, so the
    warm-up applies again); ones whose torque, speed or position of every joint walks through the edge values (each (step, joint)
    another one); ones that carry +-inf and NaN in each of the three inputs; and ones that never move.  Returns (config, snapshots,
    dof_vel at the clear, kind)."""
    cfg = script_config()
    kind = rng.integers(0, len(KINDS), N)
    kind[:len(KINDS)] = np.arange(len(KINDS))
    lower, upper = np.array(cfg.pos_lower, f32)[:, None], np.array(cfg.pos_upper, f32)[:, None]
    start = (8.0 * rng.standard_normal((DOF, N))).astype(f32)
    start[:, kind == 6] = 0.0
    still = rng.uniform(lower, upper, (DOF, N)).astype(f32)
    bad = np.array([np.inf, -np.inf, np.nan], f32)
    age = np.zeros(N, np.int32)
    snaps = []
    for t in range(steps):
        s = dict(torques=(14.0 * rng.standard_normal((DOF, N))).astype(f32), dof_vel=(11.0 * rng.standard_normal((DOF, N))).astype(f32),
                 dof_pos=rng.uniform(lower - 0.1, upper + 0.1, (DOF, N)).astype(f32))
        for j in range(DOF):
            k = t * DOF + j                                                # every (step, joint) another value
            edges = edge_values(cfg.torque_limit[j], cfg.soft_torque_limit)
            s["torques"][j, kind == 2] = edges[(k * 5) % len(edges)]
            edges = edge_values(cfg.vel_limit[j], cfg.soft_vel_limit)
            s["dof_vel"][j, kind == 3] = edges[(k * 5) % len(edges)]
            lo, hi = f32(cfg.pos_lower[j]), f32(cfg.pos_upper[j])
            spots = np.array([lo, hi, np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf)), lo - f32(0.25), hi + f32(0.5), np.nextafter(lo, f32(np.inf)),
                              np.nextafter(hi, f32(-np.inf))], f32)
            s["dof_pos"][j, kind == 4] = spots[k % len(spots)]
            which = ("torques", "dof_vel", "dof_pos")[k % 3]
            if (k // 3) % 2 == 0:                                          # half of the (step, joint) pairs carry one bad value
                s[which][j, kind == 5] = bad[(k // 6) % 3]
        s["dof_vel"][:, kind == 6] = 0.0
        s["dof_pos"][:, kind == 6] = still[:, kind == 6]
        reset = (kind == 1) & np.isin(t, (0, 5, 8, 9)) | (rng.random(N) < 0.03)
        s["dof_vel"][:, reset] = 0.0                                       # what the simulator leaves after a reset
        s["reset_buf"] = np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8)
        age = np.where(reset, 0, age + 1).astype(np.int32)
        s["episode_length_buf"] = age.copy()
        snaps.append(s)
    return cfg, snaps, start, kind


def run(cfg, snaps, N, dof_vel_at_clear):
    st = State(N, dof_vel_at_clear)
    for s in snaps:
        accumulate(st, cfg, s)
    return st
