"""TEST INFRASTRUCTURE: numpy model of libgo1place's kernels, written from the text of include/go1place.h (the Raibert quantities, the
fourteen rows per foot, the touchdown, stride and liftoff rules, the footprint map, the folding rule, the metric rows, the group row
and the map table).  Every value is formed in np.float32 in the header's operation order and summed in float64, so accumulators, state,
map and both result tables are compared with the kernels' bit for bit.  The metric-row reduction is joint_ref.py's (eval_ref.py's
fixed order, vectorised over the rows); the map's own order (the foot profile's, sixteen cells at a time) is restated here."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

METRICS = ["stance_err_x", "stance_err_y", "swing_err_x", "swing_err_y", "touchdown_x", "touchdown_y", "touchdown_err_x", "touchdown_err_y",
           "track_width_err", "stride_length", "stride_length_err", "liftoff_x", "liftoff_y", "stance_sweep"]
(STANCE_ERR_X, STANCE_ERR_Y, SWING_ERR_X, SWING_ERR_Y, TOUCHDOWN_X, TOUCHDOWN_Y, TOUCHDOWN_ERR_X, TOUCHDOWN_ERR_Y, TRACK_WIDTH_ERR, STRIDE_LENGTH,
 STRIDE_LENGTH_ERR, LIFTOFF_X, LIFTOFF_Y, STANCE_SWEEP) = range(14)
M, FEET, SIDE, CELLS, BINS = len(METRICS), 4, 8, 64, 16
ROWS = FEET * M + 1
GROUP_FIELDS = ["envs", "steps", "resets", "touchdowns", "strides", "map_outside"]
# the buffers go1place_accumulate reads (SoA, [k][N])
INPUTS = ["commands", "root_states", "foot_positions", "contact_forces", "foot_indices", "reset_buf", "episode_length_buf"]
STATE = ["prev_contact", "stance_open", "stride_open", "td_x", "last_x", "last_y", "td_world_x", "td_world_y", "touchdowns", "liftoffs", "strides",
         "map_outside", "map", "steps", "resets"]
AIR, GROUND, UNKNOWN = 0, 1, 2
f32 = np.float32


def config(warmup_steps=0, num_commands=15, map_cell=0.03):
    """what Go1PlaceConfig says"""
    return types.SimpleNamespace(warmup_steps=warmup_steps, num_commands=num_commands, map_cell=map_cell)


def yaw_rotate(z, w, vx, vy, vz):
    """(bx, by): the x and y of R v = v + w t + u x t with u = (0, 0, z), t = 2 (u x v), every product formed"""
    zero, two = f32(0.0), f32(2.0)
    cx, cy, cz = zero * vz - z * vy, z * vx - zero * vz, zero * vy - zero * vx
    tx, ty, tz = two * cx, two * cy, two * cz
    dx, dy = zero * tz - z * ty, z * tx - zero * tz
    return vx + w * tx + dx, vy + w * ty + dy


def step_values(cfg, snap):
    """the quantities of one step from the SoA buffers `snap`: {"bx", "by", "by_p", "ex", "ey", "px", "py", "xs", "ys", "xo", "yo", "fz":
    (4, N) np.float32, "c": (4, N) bool, "width", "length", "commanded_stride": (N,) np.float32}"""
    cmd, root, pos = snap["commands"], snap["root_states"], snap["foot_positions"]
    assert cmd.dtype == root.dtype == pos.dtype == snap["contact_forces"].dtype == snap["foot_indices"].dtype == f32
    N = root.shape[1]
    one, two, half = f32(1.0), f32(2.0), f32(0.5)
    width = cmd[12] if cfg.num_commands >= 13 else np.full(N, 0.3, f32)
    length = cmd[13] if cfg.num_commands >= 14 else np.full(N, 0.45, f32)
    out = {k: np.zeros((FEET, N), f32) for k in ("bx", "by", "by_p", "ex", "ey", "px", "py", "xs", "ys", "xo", "yo", "fz")}
    with np.errstate(all="ignore"):
        qz, qw = root[5], root[6]
        yn = np.fmax(np.sqrt(qz * qz + qw * qw), f32(1e-9))
        yz, yw = -qz / yn, qw / yn
        half_period, cmd_vy = half / cmd[4], cmd[2] * length / two
        rel = [yaw_rotate(yz, yw, pos[3 * f] - root[0], pos[3 * f + 1] - root[1], pos[3 * f + 2] - root[2]) for f in range(FEET)]
        for f in range(FEET):
            bx, by = rel[f]
            xs, ys = f32(1.0 if f < 2 else -1.0) * length / two, f32(1.0 if f % 2 == 0 else -1.0) * width / two
            ph = np.abs(one - snap["foot_indices"][f] * two) * one - half
            xo = ph * cmd[0] * half_period
            yo = ph * cmd_vy * half_period
            if f >= 2:
                yo = -yo
            values = dict(bx=bx, by=by, by_p=rel[f ^ 1][1], ex=bx - (xs + xo), ey=by - (ys + yo), px=bx - xs, py=by - ys, xs=xs, ys=ys, xo=xo, yo=yo,
                          fz=snap["contact_forces"][12 * (f + 1) + 2])
            for k, v in values.items():
                assert v.dtype == f32, k
                out[k][f] = v
        out["c"] = out["fz"] > f32(1.0)
        out["commanded_stride"] = np.sqrt(cmd[0] * cmd[0] + cmd[1] * cmd[1]) / cmd[4]
    out["width"], out["length"] = width, length
    assert out["commanded_stride"].dtype == f32
    return out


def map_coord(p, cell):
    """floorf((p + 4.0f * cell) / cell) of the np.float32 values p, as np.float32"""
    cell = f32(cell)
    with np.errstate(all="ignore"):
        u = np.floor((p + f32(4.0) * cell) / cell)
    assert u.dtype == f32
    return u


class State:
    """the accumulators and the state after go1place_clear, in the kernel's own number formats"""

    def __init__(self, N):
        self.N = N
        R = FEET * M
        self.count, self.nonfinite = np.zeros((R, N), np.uint32), np.zeros((R, N), np.uint32)
        self.sum, self.sumsq = np.zeros((R, N)), np.zeros((R, N))
        self.min, self.max = np.full((R, N), np.inf, f32), np.full((R, N), -np.inf, f32)
        self.prev_contact = np.full((FEET, N), UNKNOWN, np.uint8)
        self.stance_open, self.stride_open = np.zeros((FEET, N), np.uint8), np.zeros((FEET, N), np.uint8)
        self.td_x, self.last_x, self.last_y, self.td_world_x, self.td_world_y = (np.zeros((FEET, N), f32) for _ in range(5))
        self.touchdowns, self.liftoffs, self.strides, self.map_outside = (np.zeros((FEET, N), np.uint32) for _ in range(4))
        self.map = np.zeros((FEET, CELLS, N), np.uint32)
        self.steps, self.resets = np.zeros(N, np.uint32), np.zeros(N, np.uint32)

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
    """one go1place_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays).  Returns what the step did, for the
    tests that look at single steps: {"live": (N,), "contact", "touchdown", "stride", "liftoff" (a folded one), "unseen_liftoff",
    "outside": (4, N) bool, "values": step_values}"""
    N = st.N
    env = np.arange(N)
    reset = snap["reset_buf"] != 0
    st.steps += 1                                                                        # 1
    st.resets += reset.astype(np.uint32)
    live = ~reset & (snap["episode_length_buf"] > cfg.warmup_steps)                      # 2
    st.prev_contact[:, ~live] = UNKNOWN
    st.stance_open[:, ~live] = 0
    st.stride_open[:, ~live] = 0
    v = step_values(cfg, snap)                                                           # 3
    pos = snap["foot_positions"]
    did = {k: np.zeros((FEET, N), bool) for k in ("touchdown", "stride", "liftoff", "unseen_liftoff", "outside")}
    side = f32(SIDE)
    for f in range(FEET):
        r = f * M
        c, ex, ey, px, py = v["c"][f], v["ex"][f], v["ey"][f], v["px"][f], v["py"][f]
        st.fold(r + STANCE_ERR_X, live & c, ex)
        st.fold(r + STANCE_ERR_Y, live & c, ey)
        st.fold(r + SWING_ERR_X, live & ~c, ex)
        st.fold(r + SWING_ERR_Y, live & ~c, ey)
        prev = st.prev_contact[f].copy()
        td = live & c & (prev == AIR)                                                    # 4
        st.fold(r + TOUCHDOWN_X, td, px)
        st.fold(r + TOUCHDOWN_Y, td, py)
        st.fold(r + TOUCHDOWN_ERR_X, td, ex)
        st.fold(r + TOUCHDOWN_ERR_Y, td, ey)
        with np.errstate(all="ignore"):
            st.fold(r + TRACK_WIDTH_ERR, td, np.abs(v["by"][f] - v["by_p"][f]) - v["width"])
            mu, mv = map_coord(px, cfg.map_cell), map_coord(py, cfg.map_cell)
            inside = (mu >= f32(0.0)) & (mu < side) & (mv >= f32(0.0)) & (mv < side)
        hit = td & inside
        cell = (SIDE * np.where(hit, mv, f32(0.0)).astype(np.int64) + np.where(hit, mu, f32(0.0)).astype(np.int64))
        st.map[f, cell[hit], env[hit]] += 1
        st.map_outside[f] += (td & ~inside).astype(np.uint32)
        closes = td & (st.stride_open[f] != 0)
        with np.errstate(all="ignore"):
            dx, dy = pos[3 * f] - st.td_world_x[f], pos[3 * f + 1] - st.td_world_y[f]
            stride = np.sqrt(dx * dx + dy * dy)
            st.fold(r + STRIDE_LENGTH, closes, stride)
            st.fold(r + STRIDE_LENGTH_ERR, closes, stride - v["commanded_stride"])
        st.strides[f] += closes.astype(np.uint32)
        st.td_x[f] = np.where(td, px, st.td_x[f])
        st.td_world_x[f] = np.where(td, pos[3 * f], st.td_world_x[f])
        st.td_world_y[f] = np.where(td, pos[3 * f + 1], st.td_world_y[f])
        st.stance_open[f] = np.where(td, 1, st.stance_open[f]).astype(np.uint8)
        st.stride_open[f] = np.where(td, 1, st.stride_open[f]).astype(np.uint8)
        st.touchdowns[f] += td.astype(np.uint32)
        lift = live & ~c & (prev == GROUND)                                              # 5
        seen = lift & (st.stance_open[f] != 0)
        st.fold(r + LIFTOFF_X, seen, st.last_x[f])
        st.fold(r + LIFTOFF_Y, seen, st.last_y[f])
        with np.errstate(all="ignore"):
            st.fold(r + STANCE_SWEEP, seen, st.td_x[f] - st.last_x[f])
        st.liftoffs[f] += seen.astype(np.uint32)
        st.stance_open[f] = np.where(lift, 0, st.stance_open[f]).astype(np.uint8)
        st.last_x[f] = np.where(live & c, px, st.last_x[f])                              # 6
        st.last_y[f] = np.where(live & c, py, st.last_y[f])
        st.prev_contact[f] = np.where(live, np.where(c, GROUND, AIR), UNKNOWN).astype(np.uint8)      # 7
        did["touchdown"][f], did["stride"][f], did["liftoff"][f], did["unseen_liftoff"][f], did["outside"][f] = td, closes, seen, lift & ~seen, td & ~inside
    for k in ("td_x", "last_x", "last_y", "td_world_x", "td_world_y"):
        assert getattr(st, k).dtype == f32, k
    did.update(live=live, contact=v["c"], values=v)
    return did


def reduce(st, group, num_groups):
    """((G, 4 * 14 + 1, 6) fp64 result table, (G, 4, 64) fp64 map table) of go1place_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    cells = np.zeros((num_groups, FEET, CELLS))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    slices = E.REDUCE_THREADS // BINS
    words = st.map.astype(np.float64)
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
        out[g, :FEET * M] = rows
        # the last three: an environment's four words, feet 0 .. 3 in this order, each as a double (exact: they are integers)
        per_foot = [sum(getattr(st, k)[f].astype(np.float64) for f in range(FEET)) for k in ("touchdowns", "strides", "map_outside")]
        per_env = np.stack([np.ones(st.N), st.steps.astype(np.float64), st.resets.astype(np.float64)] + per_foot)
        out[g, FEET * M, :6] = _combine_rows(per_env, members, np.add, 0.0)
        # a cell: slice k adds the members e = k, k + 16, ... in ascending order; then slice k takes k + 8, + 4, + 2, + 1
        partial = np.zeros((slices, FEET, CELLS))
        for e in members:
            partial[e % slices] += words[:, :, e]
        k = slices // 2
        while k > 0:
            partial[:k] += partial[k:2 * k]
            k //= 2
        cells[g] = partial[0]
    return out, cells


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_MAP_CELL = 40, 2, 0.03
KINDS = ["walks", "resets", "chatters", "stands", "threshold", "nonfinite", "outside"]
TROT_PERIOD, CHATTER_PERIOD, DT = 10, 12, 0.02


def script_config():
    return config(warmup_steps=SCRIPT_WARMUP, num_commands=15, map_cell=SCRIPT_MAP_CELL)


def _on_ground(kind, t, f):
    """whether foot f of an environment of `kind` is on the ground at script step t (the threshold kind has forces of its own)"""
    if kind == 2:                       # a touchdown at phase 0, a bounce (in the air at 1, down again at 2), a liftoff at 6
        return (t + 3 * f) % CHATTER_PERIOD in (0, 2, 3, 4, 5)
    if kind == 3:
        return True
    return (t + (TROT_PERIOD // 2) * (f in (1, 2))) % TROT_PERIOD < TROT_PERIOD // 2      # a trot of ten steps: FL + RR, then FR + RL


def scripted_steps(rng, N, steps=SCRIPT_STEPS):
    """`steps` snapshots of the input buffers for N environments and the kind of every environment: robots that walk a clean trot along
    their own heading, the feet within the map of their nominal points; ones that trot and reset on the first step, mid-script and twice
    in a row (episode_length_buf starts again, so the warm-up applies again); ones whose feet bounce two steps after a touchdown; ones
    that stand throughout; ones whose feet carry one ulp either side of the contact threshold; ones that trot with +-inf and NaN in the
    forces and the positions and with cmd[4] = 0; ones whose feet land outside the map.  Returns (config, snapshots, kind)."""
    cfg = script_config()
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    bad = np.array([np.inf, -np.inf, np.nan], f32)
    one = f32(1.0)
    edge = np.array([one, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), 0.0, -0.0, -5.0, 30.0], f32)
    age = np.zeros(N, np.int32)
    vx, vy, yaw_rate = rng.uniform(0.3, 1.0, N), rng.uniform(-0.2, 0.2, N), rng.uniform(-0.5, 0.5, N)
    freq, width, length = rng.uniform(2.0, 4.0, N), rng.uniform(0.10, 0.45, N), rng.uniform(0.35, 0.45, N)
    heading, where = rng.uniform(-np.pi, np.pi, N), rng.uniform(-3.0, 3.0, (2, N))
    x_sign, y_sign = np.array([1.0, 1.0, -1.0, -1.0]), np.array([1.0, -1.0, 1.0, -1.0])
    snaps = []
    for t in range(steps):
        s = dict(commands=rng.uniform(-1.0, 1.0, (15, N)).astype(f32), root_states=(0.1 * rng.standard_normal((13, N))).astype(f32),
                 foot_positions=np.zeros((12, N), f32), contact_forces=(3.0 * rng.standard_normal((51, N))).astype(f32),
                 foot_indices=rng.random((4, N)).astype(f32))
        for k, column in ((0, vx), (1, vy), (2, yaw_rate), (4, freq), (12, width), (13, length)):
            s["commands"][k] = column.astype(f32)
        heading = heading + yaw_rate * DT
        where = where + DT * np.stack([vx * np.cos(heading) - vy * np.sin(heading), vx * np.sin(heading) + vy * np.cos(heading)])
        s["root_states"][0:2] = where.astype(f32)
        s["root_states"][2] = (0.3 + 0.01 * rng.standard_normal(N)).astype(f32)
        s["root_states"][5], s["root_states"][6] = np.sin(heading / 2).astype(f32), np.cos(heading / 2).astype(f32)
        for f in range(4):
            z = 12 * (f + 1) + 2
            down = np.array([_on_ground(int(k), t, f) for k in kind])
            s["contact_forces"][z] = np.where(down, rng.uniform(20.0, 90.0, N), rng.uniform(-0.5, 0.9, N)).astype(f32)
            s["contact_forces"][z, kind == 4] = edge[((t * 4 + f) * 3) % len(edge)]
            # the foot in the body frame: its nominal point and a scatter within the map (+-0.12 m); far outside it for the last kind
            spread = np.where(kind == 6, 0.5, 0.1)
            local = np.stack([x_sign[f] * length / 2 + spread * rng.uniform(-1.0, 1.0, N), y_sign[f] * width / 2 + spread * rng.uniform(-1.0, 1.0, N)])
            s["foot_positions"][3 * f] = (where[0] + np.cos(heading) * local[0] - np.sin(heading) * local[1]).astype(f32)
            s["foot_positions"][3 * f + 1] = (where[1] + np.sin(heading) * local[0] + np.cos(heading) * local[1]).astype(f32)
            s["foot_positions"][3 * f + 2] = np.where(down, 0.02, 0.08).astype(f32)
        odd = kind == 5
        if t % 3 == 0:
            s["contact_forces"][12 * ((t // 3) % 4 + 1) + 2, odd] = bad[(t // 3) % 3]
        if t % 3 == 1:
            s["foot_positions"][(t // 3) % 12, odd] = bad[(t // 3) % 3]
        if t % 5 == 2:
            s["commands"][4, odd] = 0.0
        reset = (kind == 1) & np.isin(t, (0, 17, 18, 29)) | (kind == 1) & (rng.random(N) < 0.02)
        s["reset_buf"] = np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8)
        age = np.where(reset, 0, age + 1).astype(np.int32)
        s["episode_length_buf"] = age.copy()
        snaps.append(s)
    return cfg, snaps, kind


def run(cfg, snaps, N):
    """(the state after the snapshots, what every step did)"""
    st, did = State(N), []
    for s in snaps:
        did.append(accumulate(st, cfg, s))
    return st, did
