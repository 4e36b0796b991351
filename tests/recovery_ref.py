"""TEST INFRASTRUCTURE: numpy model of libgo1eval's push and disturbance-recovery kernels, written from the text of
include/go1eval.h (fourth kernel family: the heading frame of the push, the status rules, the three signals, the eight values, the
group table).  The analysis and its reduction round exactly where the header says (fp32 operations, fp64 carries rounded once),
so the kernels' outputs are compared with them bit for bit.  The push is modelled in fp64: the kernel's fp32 result is compared
with it within a bound derived from its operation count (push_bound).  The group reduction is eval_ref.py's fixed order."""
import numpy as np

import eval_ref as E

C = 24
VX, VY, WZ, HEIGHT, CMD_VX, CMD_VY, CMD_WZ, RESET = 0, 1, 2, 3, 6, 7, 8, 11          # Go1TraceChannel
PUSH_ROWS = ["forward", "left", "up", "yaw_rate"]
VALUES = ["fell", "peak_vel_err", "peak_time", "recovered", "recovery_time", "height_drop", "yaw_rate_dev", "iae_excess"]
V = len(VALUES)
STATUS = ["ok", "baseline_reset", "not_held", "fell"]
GROUP_FIELDS = ["envs", "ok", "baseline_reset", "not_held", "fell"]
PUSHED_ROWS = [7, 8, 9, 12]                      # the rows of root_states a push writes
f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24                                 # half an ulp of 1 in fp32: the relative error of one rounding


def heading(quat):
    """(hx, hy) fp64 of quaternions (4, M) xyzw: R(q) (1, 0, 0) projected on the ground and normalised; (1, 0) below 1e-6"""
    x, y, z, w = (np.asarray(c, f64) for c in quat)
    fx = 1.0 - 2.0 * (y * y + z * z)             # R(q) (1, 0, 0), expanded
    fy = 2.0 * (x * y + w * z)
    n = np.sqrt(fx * fx + fy * fy)
    small = n < f64(f32(1e-6))
    safe = np.where(small, 1.0, n)
    return np.where(small, 1.0, fx / safe), np.where(small, 0.0, fy / safe)


def push(root_states, table, env_ids=None):
    """one go1eval_push launch in fp64.  root_states (13, N); table (K, 4) rows of PUSH_ROWS; env_ids (K,) or None.  Returns the
    new root_states (13, N) fp64 and `written` (N,) bool: the environments the kernel writes (a zero row and an id outside
    [0, N) write nothing)."""
    root = np.array(root_states, f64)
    N = root.shape[1]
    table = np.asarray(table, f64).reshape(-1, 4)
    ids = np.arange(N) if env_ids is None else np.asarray(env_ids, np.int64)
    assert ids.size == table.shape[0] and (env_ids is not None or table.shape[0] == N)
    written = np.zeros(N, bool)
    for k, e in enumerate(ids):
        if not table[k].any() or e < 0 or e >= N:
            continue
        hx, hy = heading(root[3:7, e:e + 1])
        forward, left, up, dyaw = table[k]
        root[7, e] += forward * hx[0] - left * hy[0]
        root[8, e] += forward * hy[0] + left * hx[0]
        root[9, e] += up
        root[12, e] += dyaw
        written[e] = True
    return root, written


def push_bound(table_row, new_value):
    """the largest distance of the kernel's fp32 element from the fp64 model: the heading and the rotated push are at most a
    dozen fp32 roundings of terms bounded by the push's norm (16 leaves room for the normalisation of a non-unit quaternion's
    forward axis), and the final add rounds the new value once"""
    return 16.0 * EPS * np.linalg.norm(np.asarray(table_row, f64)) + EPS * np.abs(new_value)


def window_ok(rows, push_row, pre, smooth, hold, band, dt):
    """the conditions go1eval_recovery checks before it launches"""
    return bool(1 <= pre <= push_row < rows and 1 <= smooth <= pre + 1 and 1 <= hold <= rows - push_row and dt > 0 and band >= 0)


def _mean(x, lo, hi):
    """the mean of rows [lo, hi) of x (rows, K) fp32: fp64 carry in ascending order, divided in fp64, rounded to fp32 once"""
    acc = np.zeros(x.shape[1], f64)
    for u in range(lo, hi):
        acc += x[u].astype(f64)
    return (acc / f64(hi - lo)).astype(f32)


def recovery(trace, push_row, pre, smooth, band, hold, dt):
    """one go1eval_recovery launch.  trace: (rows, 24, K) fp32.  Returns values (8, K) fp32 and status (K,) int32."""
    trace = np.asarray(trace, f32)
    end, _, K = trace.shape
    p0, w, first = push_row, smooth, push_row - pre
    assert window_ok(end, p0, pre, w, hold, band, dt)
    dt, band = f32(dt), f32(band)
    with np.errstate(all="ignore"):
        spoiled = (trace[first:p0, RESET] != 0).any(axis=0)                                          # rule 1
        fell = (trace[p0:end, RESET] != 0).any(axis=0)
        moved = np.zeros(K, bool)
        for ch in (CMD_VX, CMD_VY, CMD_WZ):
            moved |= (trace[first:end, ch] != trace[first, ch]).any(axis=0)
        status = np.where(spoiled, 1, np.where(fell, 3, np.where(moved, 2, 0))).astype(np.int32)
        dx, dy = trace[:, VX] - trace[:, CMD_VX], trace[:, VY] - trace[:, CMD_VY]                    # rule 2
        e = np.sqrt(dx * dx + dy * dy)
        z = trace[:, HEIGHT]
        y = trace[:, WZ] - trace[:, CMD_WZ]
        assert e.dtype == f32 and y.dtype == f32
        eb, zb, yb = (_mean(x, first, p0) for x in (e, z, y))
        t_peak, t_s = np.full(K, p0), np.full(K, p0)                                                 # rule 3
        peak, lowest, yaw_dev = np.full(K, -np.inf, f32), np.full(K, np.inf, f32), np.zeros(K, f32)
        excess = np.zeros(K, f64)
        for t in range(p0, end):
            es = _mean(e, t - w + 1, t + 1)
            higher = es > peak
            peak, t_peak = np.where(higher, es, peak), np.where(higher, t, t_peak)
            t_s = np.where(es - eb > band, t + 1, t_s)
            lowest = np.fmin(lowest, _mean(z, t - w + 1, t + 1))
            yaw_dev = np.fmax(yaw_dev, np.abs(_mean(y, t - w + 1, t + 1) - yb))
            excess += (e[t] - eb).astype(f64)
        recovered = t_s <= end - hold
        values = np.zeros((V, K), f32)
        values[1] = peak - eb
        values[2] = (t_peak - p0 + 1).astype(f32) * dt
        values[3] = recovered
        values[4] = np.where(recovered, (t_s - p0).astype(f32) * dt, f32(np.nan))
        values[5] = zb - lowest
        values[6] = yaw_dev
        values[7] = (f64(dt) * excess).astype(f32)
        values[:, status != 0] = np.nan
        values[0, status == 3] = 1.0
    return values, status


def recovery_reduce(values, status, group, num_groups):
    """(G, 8 + 1, 6) fp64 result table of go1eval_recovery_reduce: per row the metric row of eval_ref.reduce over accumulators
    that folded the one value, and the group's own row (environments, status 0, 1, 2, 3, then 0)"""
    values, status, group = np.asarray(values, f32), np.asarray(status), np.asarray(group)
    flat = values.astype(f64)
    add = lambda a, b: a + b
    out = np.zeros((num_groups, V + 1, len(E.FIELDS)))
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        for m in range(V):
            v = flat[m]
            fin = np.isfinite(v)
            n = E._combine(fin.astype(f64), members, add, 0.0)
            nf = E._combine((~fin).astype(f64), members, add, 0.0)
            if n > 0:
                total = E._combine(np.where(fin, v, 0.0), members, add, 0.0)
                squares = E._combine(np.where(fin, v * v, 0.0), members, add, 0.0)
                mean = total / n
                counted = [e for e in members if fin[e]]
                out[g, m] = [n, mean, np.sqrt(max(squares / n - mean * mean, 0.0)), min(v[e] for e in counted), max(v[e] for e in counted), nf]
            else:
                out[g, m] = [0.0, np.nan, np.nan, np.nan, np.nan, nf]
        out[g, V] = [float(len(members))] + [float(sum(1 for e in members if status[e] == k)) for k in (0, 1, 2, 3)] + [0.0]
    return out


def synthetic_traces(rng, K, rows, p0, pre):
    """TEST DATA.  (rows, 24, K) traces that mix, at random: a robot that is not disturbed, bumps of the velocity error that decay
    fast or slowly or not at all, a bump that comes back inside the hold rows, height dips and yaw kicks, resets before the
    window / inside the baseline / after the push (with the reset's own command draw on that row), commands that move, and the
    all-NaN trace of an id outside the simulator.  Returns the traces and the kind of each."""
    t = (rng.standard_normal((rows, C, K)) * 0.01).astype(f32)
    t[:, RESET] = 0.0
    kind = rng.integers(0, 10, K)
    i = np.arange(rows - p0)
    for k in range(K):
        cmd = (rng.choice([0.5, 1.0, 1.5]), rng.choice([0.0, 0.25]), rng.choice([0.0, -0.5]))
        for c, r in enumerate(cmd):
            t[:, 6 + c, k] = r
            t[:, c, k] += r + rng.uniform(-0.02, 0.02)                                   # a steady tracking offset: the baseline
        t[:, HEIGHT, k] += 0.3
        height, tau = rng.uniform(0.6, 1.5), rng.uniform(2.0, 6.0)
        if kind[k] in (1, 4, 5, 6, 7, 8):
            bump = height * np.exp(-i / tau)
            t[p0:, VY, k] += bump * rng.choice([-1.0, 1.0])
            t[p0:, HEIGHT, k] -= 0.2 * bump
            t[p0:, WZ, k] += 0.5 * bump
        if kind[k] == 2:
            t[p0:, VX, k] -= height                                                      # never comes back
        if kind[k] == 3:
            t[p0:, VY, k] += height * np.exp(-i / tau)
            t[rows - int(rng.integers(1, 5)), VY, k] += 1.0                              # leaves the band again in the last four rows
        if kind[k] == 4 and p0 - pre >= 1:
            t[p0 - pre - 1, RESET, k] = 1.0                                              # before the window: ignored
        if kind[k] == 5:
            t[int(rng.integers(p0 - pre, p0)), RESET, k] = 1.0                           # the baseline is spoiled
        if kind[k] == 6:
            r = int(rng.integers(p0, rows))
            t[r, RESET, k] = 1.0                                                         # fell: that row carries a new command draw
            t[r, 6:9, k] = rng.standard_normal(3).astype(f32)
        if kind[k] == 7:
            t[int(rng.integers(p0 - pre + 1, rows)):, 6 + int(rng.integers(0, 3)), k] += 0.25      # the command moves
        if kind[k] == 9:
            t[:, :, k] = np.nan                                                          # an id outside the simulator
    return t, kind
