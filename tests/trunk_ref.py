"""TEST INFRASTRUCTURE: numpy model of libgo1trunk's kernels, written from the text of include/go1trunk.h (the seventeen rows, the
previous-velocity rule, the support polygon's edge distances, the drift segments, the tilt histogram, the folding rules, the metric
rows, the group row and the histogram table).  Every value is formed in np.float32 in the header's operation order and summed in
float64, so accumulators, state, histogram and both result tables are compared with the kernels' bit for bit.  The metric-row
reduction is joint_ref.py's (eval_ref.py's fixed order, vectorised over the rows); the histogram's own order is restated here."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

METRICS = ["roll_sin", "pitch_sin", "tilt", "tilt_exceeded", "roll_rate", "pitch_rate", "vertical_vel", "accel_horizontal", "accel_vertical",
           "ang_accel", "support_feet", "support_margin", "margin_negative", "support_line_dist", "lateral_drift", "heading_drift", "progress_err"]
(ROLL_SIN, PITCH_SIN, TILT, TILT_EXCEEDED, ROLL_RATE, PITCH_RATE, VERTICAL_VEL, ACCEL_HORIZONTAL, ACCEL_VERTICAL, ANG_ACCEL, SUPPORT_FEET,
 SUPPORT_MARGIN, MARGIN_NEGATIVE, SUPPORT_LINE_DIST, LATERAL_DRIFT, HEADING_DRIFT, PROGRESS_ERR) = range(17)
M, BINS = len(METRICS), 16
ROWS = M + 1
GROUP_FIELDS = ["envs", "steps", "resets", "segments_dropped"]
# the buffers go1trunk_accumulate reads (SoA, [k][N])
INPUTS = ["root_states", "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "contact_forces", "foot_positions", "reset_buf",
          "episode_length_buf"]
STATE = ["prev_valid", "prev_lin_vel", "prev_ang_vel", "seg_valid", "seg_steps", "seg_anchor", "seg_command", "segments_dropped", "steps", "resets",
         "tilt_hist"]
CYCLIC = [0, 2, 3, 1]          # FL, RL, RR, FR: counter-clockwise seen from above
f32 = np.float32


def config(dt=0.02, tilt_limit=0.25, segment_steps=50, warmup_steps=0):
    """what Go1TrunkConfig says"""
    return types.SimpleNamespace(dt=dt, tilt_limit=tilt_limit, segment_steps=segment_steps, warmup_steps=warmup_steps)


def tilt_bin(tilt):
    """the histogram bin of the finite np.float32 values tilt: clamped as a float, then converted"""
    with np.errstate(over="ignore"):
        b = np.floor(tilt * f32(32.0))
    assert b.dtype == f32
    b = np.where(b > f32(BINS - 1), f32(BINS - 1), np.where(b > f32(0.0), b, f32(0.0)))
    return b.astype(np.int64)


def edge_distance(ax, ay, bx, by, px, py):
    """d(A, B) of the header for np.float32 values"""
    with np.errstate(all="ignore"):
        ex, ey = bx - ax, by - ay
        d = (ex * (py - ay) - ey * (px - ax)) / np.sqrt(ex * ex + ey * ey)
    assert d.dtype == f32
    return d


def support(fz, x, y, px, py):
    """(n_c, margin, line distance) of one environment: fz, x, y the four feet's np.float32 values in the simulator's order.  margin is
    None unless n_c >= 3, the line distance None unless n_c == 2"""
    feet = [f for f in CYCLIC if fz[f] > f32(1.0)]
    if len(feet) < 2:
        return len(feet), None, None
    if len(feet) == 2:
        a, b = feet
        return 2, None, np.abs(edge_distance(x[a], y[a], x[b], y[b], px, py))
    pairs = list(zip(feet, feet[1:] + feet[:1]))                             # consecutive, wrapping round
    m = None
    for a, b in pairs:
        d = edge_distance(x[a], y[a], x[b], y[b], px, py)
        if m is None or d < m or np.isnan(d):
            m = d
    return len(feet), m, None


def heading(qx, qy, qz, qw, px, py):
    """(hx, hy, heading_ok) for np.float32 vectors"""
    with np.errstate(all="ignore"):
        h0x = f32(1.0) - f32(2.0) * (qy * qy + qz * qz)
        h0y = f32(2.0) * (qx * qy + qw * qz)
        n = np.sqrt(h0x * h0x + h0y * h0y)
        hx, hy = h0x / n, h0y / n
    assert hx.dtype == f32 and hy.dtype == f32
    return hx, hy, np.isfinite(n) & (n > 0) & np.isfinite(px) & np.isfinite(py)


class State:
    """the accumulators and the state after go1trunk_clear, in the kernel's own number formats"""

    def __init__(self, N):
        self.N = N
        self.count, self.nonfinite = np.zeros((M, N), np.uint32), np.zeros((M, N), np.uint32)
        self.sum, self.sumsq = np.zeros((M, N)), np.zeros((M, N))
        self.min, self.max = np.full((M, N), np.inf, f32), np.full((M, N), -np.inf, f32)
        self.prev_valid, self.seg_valid = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        self.prev_lin_vel, self.prev_ang_vel = np.zeros((3, N), f32), np.zeros((3, N), f32)
        self.seg_steps = np.zeros(N, np.int32)
        self.seg_anchor, self.seg_command = np.zeros((4, N), f32), np.zeros((2, N), f32)
        self.segments_dropped, self.steps, self.resets = (np.zeros(N, np.uint32) for _ in range(3))
        self.tilt_hist = np.zeros((BINS, N), np.uint32)

    def fold(self, row, live, v):
        """fold the np.float32 vector v into `row` for the environments `live`"""
        assert v.dtype == f32
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
    """one go1trunk_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays).  Returns what the step formed, for
    the tests that look at single steps: {"live", "accel_valid", "ax", "ay", "az", "closed", "n_c"}"""
    N = st.N
    zero, one = f32(0.0), f32(1.0)
    dt = f32(cfg.dt)
    reset = snap["reset_buf"] != 0
    st.steps += 1                                                                        # 1
    st.resets += reset.astype(np.uint32)
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)                      # 2, 3
    rs = snap["root_states"]
    px, py, v, w = rs[0], rs[1], rs[7:10], rs[10:13]
    gx, gy = snap["projected_gravity"][0], snap["projected_gravity"][1]
    bwx, bwy, bvz = snap["base_ang_vel"][0], snap["base_ang_vel"][1], snap["base_lin_vel"][2]
    with np.errstate(all="ignore"):
        tilt = np.sqrt(gx * gx + gy * gy)
        st.fold(ROLL_SIN, live, gy)                                                      # 4: the rows in the enum's order
        st.fold(PITCH_SIN, live, gx)
        st.fold(TILT, live, tilt)
        st.fold(TILT_EXCEEDED, live, np.where(tilt > f32(cfg.tilt_limit), one, zero))
        st.fold(ROLL_RATE, live, bwx)
        st.fold(PITCH_RATE, live, bwy)
        st.fold(VERTICAL_VEL, live, bvz)
        a = (v - st.prev_lin_vel) / dt
        u = (w - st.prev_ang_vel) / dt
        assert a.dtype == f32 and u.dtype == f32
        seen = live & (st.prev_valid != 0)
        st.fold(ACCEL_HORIZONTAL, seen, np.sqrt(a[0] * a[0] + a[1] * a[1]))
        st.fold(ACCEL_VERTICAL, seen, a[2])
        st.fold(ANG_ACCEL, seen, np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]))
    fz = np.stack([snap["contact_forces"][12 * (f + 1) + 2] for f in range(4)])
    fx_, fy_ = snap["foot_positions"][0::3], snap["foot_positions"][1::3]
    n_c, margin, line = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32)
    has_margin, has_line = np.zeros(N, bool), np.zeros(N, bool)
    for e in range(N):
        k, m, d = support(fz[:, e], fx_[:, e], fy_[:, e], px[e], py[e])
        n_c[e] = k
        if m is not None:
            margin[e], has_margin[e] = m, True
        if d is not None:
            line[e], has_line[e] = d, True
    st.fold(SUPPORT_FEET, live, n_c)
    st.fold(SUPPORT_MARGIN, live & has_margin, margin)
    st.fold(MARGIN_NEGATIVE, live & has_margin, np.where(margin < zero, one, zero))
    st.fold(SUPPORT_LINE_DIST, live & has_line, line)
    sample = live & np.isfinite(tilt)                                                    # the histogram
    b = tilt_bin(np.where(sample, tilt, zero))
    env = np.arange(N)
    st.tilt_hist[b[sample], env[sample]] += 1
    st.prev_lin_vel[:, live], st.prev_ang_vel[:, live] = v[:, live], w[:, live]          # the velocities of the last folded step
    st.prev_valid = live.astype(np.uint8)
    # the segment, on the state as the step found it
    hx, hy, ok = heading(rs[3], rs[4], rs[5], rs[6], px, py)
    cx, cy, cw = snap["commands"][0], snap["commands"][1], snap["commands"][2]
    was_open = st.seg_valid != 0
    opens = live & ~was_open & ok
    drops = live & was_open & (~(cw == 0) | ~ok)
    goes_on = live & was_open & ~drops
    with np.errstate(all="ignore"):
        sx, sy = st.seg_command[0] + cx * dt, st.seg_command[1] + cy * dt
        steps = st.seg_steps + 1
        closes = goes_on & (steps == cfg.segment_steps)
        x0, y0, hx0, hy0 = st.seg_anchor
        dx, dy = px - x0, py - y0
        along, lateral = dx * hx0 + dy * hy0, dy * hx0 - dx * hy0
        st.fold(LATERAL_DRIFT, closes, lateral - sy)
        st.fold(HEADING_DRIFT, closes, hx0 * hy - hy0 * hx)
        st.fold(PROGRESS_ERR, closes, along - sx)
    st.segments_dropped += drops.astype(np.uint32)
    further = goes_on & ~closes
    st.seg_command[0], st.seg_command[1] = np.where(further, sx, st.seg_command[0]), np.where(further, sy, st.seg_command[1])
    st.seg_steps = np.where(further, steps, st.seg_steps).astype(np.int32)
    anchor = opens | closes
    for k, value in enumerate((px, py, hx, hy)):
        st.seg_anchor[k] = np.where(anchor, value, st.seg_anchor[k])
    st.seg_command[:, anchor] = zero
    st.seg_steps[anchor] = 0
    st.seg_valid = np.where(live, np.where(drops, 0, np.where(opens, 1, st.seg_valid)), 0).astype(np.uint8)
    assert st.seg_command.dtype == f32 and st.seg_anchor.dtype == f32
    return dict(live=live, accel_valid=seen, ax=a[0], ay=a[1], az=a[2], closed=closes, n_c=n_c)


def reduce(st, group, num_groups):
    """((G, 17 + 1, 6) fp64 result table, (G, 16) fp64 histogram table) of go1trunk_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    hist = np.zeros((num_groups, BINS))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    slices = E.REDUCE_THREADS // BINS
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
        out[g, :M] = rows
        per_env = np.stack([np.ones(st.N), st.steps.astype(np.float64), st.resets.astype(np.float64), st.segments_dropped.astype(np.float64)])
        out[g, M, :4] = _combine_rows(per_env, members, np.add, 0.0)
        # the histogram: slice k adds the members e = k, k + 16, ... in ascending order; then slice k takes k + 8, + 4, + 2, + 1
        partial = np.zeros((slices, BINS))
        for e in members:
            partial[e % slices] += st.tilt_hist[:, e].astype(np.float64)
        k = slices // 2
        while k > 0:
            partial[:k] += partial[k:2 * k]
            k //= 2
        hist[g] = partial[0]
    return out, hist


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_SEGMENT = 14, 2, 3
KINDS = ["walks", "resets", "turns", "threshold", "nonfinite", "stands", "vertical"]
# on the ground (1) or in the air (0) per script step; foot f starts the pattern at step f, so the number of supporting feet varies
PATTERN = [1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1]
STANCE = np.array([[0.19, 0.14], [0.19, -0.14], [-0.19, 0.14], [-0.19, -0.14]], f32)          # FL, FR, RL, RR about the base


def script_config():
    return config(dt=0.02, tilt_limit=0.25, segment_steps=SCRIPT_SEGMENT, warmup_steps=SCRIPT_WARMUP)


def scripted_steps(rng, N, steps=SCRIPT_STEPS):
    """`steps` snapshots of the input buffers for N environments and the kind of every environment: ones that walk with a zero yaw
    command (segments of three steps close one after the other); ones that reset on the first step, mid-script and twice in a row
    (episode_length_buf starts again, so the warm-up applies again); ones whose yaw command is not zero on some steps and a NaN on
    another (segments drop and begin again); ones whose feet carry one ulp either side of the contact threshold; ones that carry +-inf
    and NaN in each input and whose feet coincide; ones that stand on a square stance throughout; ones whose body x axis is vertical on
    some steps (no heading) and whose tilt lies on the histogram's edges and beyond its last bin.  Returns (config, snapshots, kind)."""
    cfg = script_config()
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    bad = np.array([np.inf, -np.inf, np.nan], f32)
    one = f32(1.0)
    edge = np.array([one, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), 0.0, -0.0, -5.0, 30.0], f32)
    tilts = np.array([0.0, 0.03125, 0.031249998, 0.46875, 0.46874997, 0.9, 3.0, 0.25, 0.25000003], f32)
    age = np.zeros(N, np.int32)
    pos = (2.0 * rng.standard_normal((2, N))).astype(f32)
    snaps = []
    for t in range(steps):
        s = dict(root_states=rng.standard_normal((13, N)).astype(f32), base_lin_vel=(0.3 * rng.standard_normal((3, N))).astype(f32),
                 base_ang_vel=(0.5 * rng.standard_normal((3, N))).astype(f32), projected_gravity=(0.12 * rng.standard_normal((3, N))).astype(f32),
                 commands=rng.standard_normal((15, N)).astype(f32), contact_forces=(3.0 * rng.standard_normal((51, N))).astype(f32),
                 foot_positions=rng.standard_normal((12, N)).astype(f32))
        pos = pos + (0.02 * rng.standard_normal((2, N))).astype(f32)
        s["root_states"][0:2] = pos
        q = rng.standard_normal((4, N))
        s["root_states"][3:7] = (q / np.linalg.norm(q, axis=0)).astype(f32)
        s["commands"][2] = 0.0
        for f in range(4):
            z = 12 * (f + 1) + 2
            down = PATTERN[(t + f) % len(PATTERN)] == 1
            s["contact_forces"][z] = rng.uniform(20.0, 90.0, N).astype(f32) if down else rng.uniform(-0.5, 0.9, N).astype(f32)
            s["foot_positions"][3 * f:3 * f + 2] = pos + STANCE[f][:, None] + (0.03 * rng.standard_normal((2, N))).astype(f32)
            k = t * 4 + f
            s["contact_forces"][z, kind == 3] = edge[(k * 3) % len(edge)]
            s["contact_forces"][z, kind == 5] = f32(30.0) + f32(k % 5)
            s["foot_positions"][3 * f:3 * f + 2, kind == 5] = (pos + STANCE[f][:, None])[:, kind == 5]
        turns = kind == 2
        s["commands"][2, turns] = f32((0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, np.nan, 0.0, -0.0, 0.0)[t % 14])
        odd = kind == 4
        which = INPUTS[t % 7]
        rows = dict(root_states=(0, 4, 8, 11, 1, 6, 9)[(t // 7) % 7], base_lin_vel=2, base_ang_vel=t % 2, projected_gravity=t % 2, commands=t % 3,
                    contact_forces=12 * (t % 4 + 1) + 2, foot_positions=3 * (t % 4) + t % 2)
        if t % 3 != 2:
            s[which][rows[which], odd] = bad[(t // 3) % 3]
        else:                                                                # two feet in one place: a zero-length edge
            s["foot_positions"][0:2, odd] = s["foot_positions"][6:8, odd]
            s["contact_forces"][12 * 1 + 2, odd] = s["contact_forces"][12 * 3 + 2, odd] = s["contact_forces"][12 * 4 + 2, odd] = f32(40.0)
        up = kind == 6
        s["projected_gravity"][0, up] = tilts[t % len(tilts)]
        s["projected_gravity"][1, up] = 0.0
        if t in (5, 6, 11):
            s["root_states"][3:7, up] = np.array([0.5, 0.5, 0.5, -0.5], f32)[:, None]
        reset = (kind == 1) & np.isin(t, (0, 5, 8, 9)) | (rng.random(N) < 0.03)
        s["reset_buf"] = np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8)
        age = np.where(reset, 0, age + 1).astype(np.int32)
        s["episode_length_buf"] = age.copy()
        snaps.append(s)
    return cfg, snaps, kind


def run(cfg, snaps, N):
    st = State(N)
    for s in snaps:
        accumulate(st, cfg, s)
    return st
