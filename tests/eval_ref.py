"""TEST INFRASTRUCTURE: fp64 numpy model of libgo1eval's two kernels, written from the text of include/go1eval.h (the metric
formulas, the accumulate rules, the group reduction and its fixed combination order).  The GPU tests replay recorded steps
through it; the CPU tests pin it to hand-computable cases."""
import numpy as np

METRICS = ["lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques", "power_consumption", "CoT",
           "froude_number", "termination"]
M = len(METRICS)
TERMINATION = METRICS.index("termination")
FIELDS = ["count", "mean", "std", "min", "max", "nonfinite"]
GROUP_FIELDS = ["envs", "steps", "episodes_terminated", "episodes_timed_out", "fall_rate"]
REDUCE_THREADS = 256
GRAVITY, FROUDE_HEIGHT = 9.8, 0.30
# the buffers go1eval_accumulate reads (SoA, [k][N]); measured_heights may be absent (None)
INPUTS = ["base_lin_vel", "base_ang_vel", "commands", "root_states", "measured_heights", "torques", "dof_vel", "payloads", "reset_buf",
          "time_out_buf", "episode_length_buf"]


def metric_values(snap, default_body_mass=4.801):
    """(M, N) fp64: the ten metrics of one step from the SoA buffers `snap` (dict of arrays [k][N]), every operation in fp64.
    `termination` is 0 here; the accumulate rules decide what a reset step folds."""
    f = {k: (None if v is None else np.asarray(v, np.float64)) for k, v in snap.items() if k in
         ("base_lin_vel", "base_ang_vel", "commands", "root_states", "measured_heights", "torques", "dof_vel", "payloads")}
    vx, vy, wz = f["base_lin_vel"][0], f["base_lin_vel"][1], f["base_ang_vel"][2]
    N = vx.shape[0]
    out = np.zeros((M, N))
    out[0] = np.abs(vx - f["commands"][0])
    out[1] = np.abs(wz - f["commands"][2])
    out[2], out[3] = vx, wz
    z = f["root_states"][2]
    out[4] = z if f.get("measured_heights") is None else (z[None, :] - f["measured_heights"]).mean(axis=0)
    out[5] = np.abs(f["torques"]).max(axis=0)
    power = (f["torques"] * f["dof_vel"]).sum(axis=0)
    out[6] = power
    with np.errstate(divide="ignore", invalid="ignore"):
        out[7] = power / ((np.float64(np.float32(default_body_mass)) + f["payloads"]) * GRAVITY * np.sqrt(vx * vx + vy * vy))
    out[8] = vx * vx / (GRAVITY * FROUDE_HEIGHT)
    return out


class Accumulators:
    def __init__(self, N):
        self.N = N
        self.count = np.zeros((M, N), np.int64)
        self.nonfinite = np.zeros((M, N), np.int64)
        self.sum = np.zeros((M, N))
        self.sumsq = np.zeros((M, N))
        self.min = np.full((M, N), np.inf)
        self.max = np.full((M, N), -np.inf)
        self.steps = np.zeros(N, np.int64)
        self.episodes_terminated = np.zeros(N, np.int64)
        self.episodes_timed_out = np.zeros(N, np.int64)
        self.warmup_excluded = 0          # (bookkeeping of the tests: steps rule 3 dropped)

    def _fold(self, m, mask, v):
        fin = mask & np.isfinite(v)
        self.nonfinite[m] += mask & ~np.isfinite(v)
        self.count[m] += fin
        w = np.where(fin, v, 0.0)
        self.sum[m] += w
        self.sumsq[m] += w * w
        self.min[m] = np.where(fin, np.minimum(self.min[m], v), self.min[m])
        self.max[m] = np.where(fin, np.maximum(self.max[m], v), self.max[m])


def accumulate(acc, values, reset_buf, time_out_buf, episode_length_buf, warmup_steps):
    """one go1eval_accumulate launch: `values` (M, N) are the step's metric values (row `termination` is ignored)"""
    reset = np.asarray(reset_buf).astype(bool)
    tout = np.asarray(time_out_buf).astype(bool)
    elb = np.asarray(episode_length_buf).astype(np.int64)
    acc.steps += 1                                                        # rule 1
    acc.episodes_timed_out += reset & tout                                # rule 2
    acc.episodes_terminated += reset & ~tout
    acc._fold(TERMINATION, reset, np.ones(acc.N))
    warm = ~reset & (elb <= warmup_steps)                                 # rule 3
    acc.warmup_excluded += int(warm.sum())
    live = ~reset & ~warm                                                 # rule 4
    for m in range(M):
        acc._fold(m, live, np.zeros(acc.N) if m == TERMINATION else np.asarray(values[m], np.float64))


def accumulate_snapshot(acc, snap, warmup_steps, default_body_mass=4.801):
    accumulate(acc, metric_values(snap, default_body_mass), snap["reset_buf"], snap["time_out_buf"], snap["episode_length_buf"], warmup_steps)


def _tree(partials, op):
    """the binary tree over the threads: stride T/2, T/4, ... 1, thread t takes thread t + stride"""
    p = list(partials)
    s = len(p) // 2
    while s > 0:
        for t in range(s):
            p[t] = op(p[t], p[t + s])
        s //= 2
    return p[0]


def _combine(per_env, members, op, init):
    """thread t combines the group's environments t, t + T, ... in ascending order, then the tree"""
    partials = [init] * REDUCE_THREADS
    for e in members:
        partials[e % REDUCE_THREADS] = op(partials[e % REDUCE_THREADS], per_env[e])
    return _tree(partials, op)


def reduce(acc, group, num_groups):
    """(G, M + 1, 6) fp64 result table of go1eval_reduce"""
    group = np.asarray(group)
    add = lambda a, b: a + b
    out = np.zeros((num_groups, M + 1, len(FIELDS)))
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        for m in range(M):
            n = _combine(acc.count[m].astype(np.float64), members, add, 0.0)
            nf = _combine(acc.nonfinite[m].astype(np.float64), members, add, 0.0)
            if n > 0:
                S = _combine(acc.sum[m], members, add, 0.0)
                Q = _combine(acc.sumsq[m], members, add, 0.0)
                mean = S / n
                counted = [e for e in members if acc.count[m][e] > 0]
                out[g, m] = [n, mean, np.sqrt(max(Q / n - mean * mean, 0.0)), min(acc.min[m][e] for e in counted),
                             max(acc.max[m][e] for e in counted), nf]
            else:
                out[g, m] = [0.0, np.nan, np.nan, np.nan, np.nan, nf]
        envs = float(len(members))
        fallen = float(sum(1 for e in members if acc.episodes_terminated[e] > 0))
        out[g, M] = [envs, float(sum(acc.steps[e] for e in members)), float(sum(acc.episodes_terminated[e] for e in members)),
                     float(sum(acc.episodes_timed_out[e] for e in members)), fallen / envs if envs > 0 else np.nan, 0.0]
    return out
