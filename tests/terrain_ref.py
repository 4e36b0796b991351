"""TEST INFRASTRUCTURE: numpy model of libgo1eval's terrain-traversal kernels, written from the text of include/go1eval.h (fifth
kernel family: the height sample, the five per-step metrics, the status rules, the outcome rows and the group row).  It rounds
exactly where the header says (fp32 operations as np.float32, fp64 carries as Python floats, rounded once), so accumulators,
state and result table are compared with the kernels' bit for bit.  The group reduction is eval_ref.py's fixed order."""
import types

import numpy as np

import eval_ref as E

METRICS = ["base_height_terrain", "feet_clearance_terrain", "swing_foot_height", "stumble", "collision"]
BASE_HEIGHT, CLEARANCE, SWING, STUMBLE, COLLISION = range(5)
M = len(METRICS)
OUTCOMES = ["traversed", "fell", "distance", "end_time"]
STATUS = ["running", "traversed", "fell", "timed_out"]
RUNNING, TRAVERSED, FELL, TIMED_OUT = range(4)
GROUP_FIELDS = ["envs", "running", "traversed", "fell", "timed_out", "success_rate"]
ROWS = M + len(OUTCOMES) + 1
FEET_BODIES = (4, 8, 12, 16)
# the buffers go1eval_terrain_accumulate reads (SoA, [k][N]; height_samples is [hf_rows][hf_cols] int16 and may be absent)
INPUTS = ["root_states", "commands", "contact_forces", "foot_positions", "desired_contact_states", "foot_indices", "env_origins",
          "height_samples", "reset_buf", "time_out_buf", "episode_length_buf"]
STATE = ["status", "steps", "end_step", "max_dist"]
f32 = np.float32
FOOT_RADIUS, STUMBLE_RATIO, COLLISION_FORCE = f32(0.02), f32(5.0), f32(0.1)
NAN32 = f32(np.nan)


def geometry(hf_hscale=0.25, hf_vscale=0.005, hf_border=0.5, tile_length=1.0, tile_width=0.75, dt=0.02, warmup_steps=0,
             penalised_body_mask=0, height_samples=None):
    """what Go1TerrainConfig and the height field say about the ground"""
    return types.SimpleNamespace(hf_hscale=hf_hscale, hf_vscale=hf_vscale, hf_border=hf_border, tile_length=tile_length, tile_width=tile_width,
                                 dt=dt, warmup_steps=warmup_steps, penalised_body_mask=penalised_body_mask, height_samples=height_samples)


def _index(v, border, hscale, samples):
    q = (v + f32(border)) / f32(hscale)
    last = f32(samples - 2)
    if q > last:
        return samples - 2
    return int(q) if q > 0 else 0                   # (truncation; the clamp comes first, in fp32)


def height(geo, x, y):
    """h(x, y) as an np.float32"""
    x, y = f32(x), f32(y)
    if not (np.isfinite(x) and np.isfinite(y)):
        return NAN32
    hs = geo.height_samples
    if hs is None:
        return f32(0.0)
    with np.errstate(over="ignore"):
        px, py = _index(x, geo.hf_border, geo.hf_hscale, hs.shape[0]), _index(y, geo.hf_border, geo.hf_hscale, hs.shape[1])
    lowest = min(int(hs[px, py]), int(hs[px + 1, py]), int(hs[px, py + 1]))
    return f32(lowest) * f32(geo.hf_vscale)


def step_values(geo, snap, e):
    """[base_height_terrain, feet_clearance_terrain, swing_foot_height or None, stumble, collision] of environment e: np.float32"""
    root, cmd, F = snap["root_states"], snap["commands"], snap["contact_forces"]
    pos, desired, index = snap["foot_positions"], snap["desired_contact_states"], snap["foot_indices"]
    with np.errstate(all="ignore"):
        base = root[2, e] - height(geo, root[0, e], root[1, e])
        clearance, swing, swinging, stumble = 0.0, 0.0, 0, False
        for f in range(4):
            a = pos[3 * f + 2, e] - height(geo, pos[3 * f, e], pos[3 * f + 1, e])
            d, i = desired[f, e], index[f, e]
            ph = f32(1) - np.abs(f32(1) - np.fmin(np.fmax(i * f32(2) - f32(1), f32(0)), f32(1)) * f32(2))
            miss = cmd[9, e] * ph + FOOT_RADIUS - a
            clearance += float(miss * miss * (f32(1) - d))
            if d <= f32(0.5):
                swing += float(a - FOOT_RADIUS)
                swinging += 1
            fx, fy, fz = (F[3 * FEET_BODIES[f] + k, e] for k in range(3))
            if np.sqrt(fx * fx + fy * fy) > STUMBLE_RATIO * np.abs(fz):
                stumble = True
        collisions = 0
        for b in range(17):
            if (geo.penalised_body_mask >> b) & 1:
                fx, fy, fz = (F[3 * b + k, e] for k in range(3))
                collisions += bool(np.sqrt(fx * fx + fy * fy + fz * fz) > COLLISION_FORCE)
        values = [base, f32(clearance), f32(swing / swinging) if swinging else None, f32(1.0 if stumble else 0.0), f32(collisions)]
    assert all(v is None or type(v) is f32 for v in values)
    return values


class State:
    """the accumulators and the per-environment state, in the kernel's own number formats"""

    def __init__(self, N):
        self.N = N
        self.count, self.nonfinite = np.zeros((M, N), np.uint32), np.zeros((M, N), np.uint32)
        self.sum, self.sumsq = np.zeros((M, N)), np.zeros((M, N))
        self.min, self.max = np.full((M, N), np.inf, f32), np.full((M, N), -np.inf, f32)
        self.status, self.steps, self.end_step = np.zeros(N, np.uint8), np.zeros(N, np.uint32), np.zeros(N, np.uint32)
        self.max_dist = np.zeros(N, f32)

    def fold(self, m, e, v):
        if not np.isfinite(v):
            self.nonfinite[m, e] += 1
            return
        self.count[m, e] += 1
        self.sum[m, e] += float(v)
        self.sumsq[m, e] += float(v) * float(v)
        self.min[m, e] = min(self.min[m, e], v)
        self.max[m, e] = max(self.max[m, e], v)

    def arrays(self):
        return {k: getattr(self, k) for k in ["count", "sum", "sumsq", "min", "max", "nonfinite"] + STATE}


def accumulate(st, geo, snap):
    """one go1eval_terrain_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays)"""
    root, origin = snap["root_states"], snap["env_origins"]
    assert root.dtype == f32 and origin.dtype == f32
    half_length, half_width = f32(geo.tile_length) / f32(2), f32(geo.tile_width) / f32(2)
    for e in range(st.N):
        if st.status[e] != RUNNING:                                                      # 1
            continue
        if snap["reset_buf"][e] != 0:                                                    # 2
            st.status[e] = TIMED_OUT if snap["time_out_buf"][e] != 0 else FELL
            st.end_step[e] = st.steps[e] + 1
            continue
        st.steps[e] += 1                                                                 # 3
        with np.errstate(all="ignore"):
            dx, dy = root[0, e] - origin[0, e], root[1, e] - origin[1, e]
            st.max_dist[e] = np.fmax(st.max_dist[e], np.sqrt(dx * dx + dy * dy))
            left = np.isfinite(dx) and np.isfinite(dy) and (np.abs(dx) > half_length or np.abs(dy) > half_width)
        if left:
            st.status[e], st.end_step[e] = TRAVERSED, st.steps[e]
            continue
        if snap["episode_length_buf"][e] <= geo.warmup_steps:                            # 4
            continue
        for m, v in enumerate(step_values(geo, snap, e)):                                # 5
            if v is not None:
                st.fold(m, e, v)


def outcome_values(st, dt):
    """(4, N) np.float32: the one value per environment of the outcome rows"""
    running = st.status == RUNNING
    out = np.zeros((len(OUTCOMES), st.N), f32)
    out[0] = np.where(running, NAN32, (st.status == TRAVERSED).astype(f32))
    out[1] = np.where(running, NAN32, (st.status == FELL).astype(f32))
    out[2] = st.max_dist
    out[3] = np.where(running, NAN32, st.end_step.astype(f32) * f32(dt))
    return out


def _metric_row(n_per_env, nf_per_env, sum_per_env, sumsq_per_env, min_per_env, max_per_env, members):
    add = lambda a, b: a + b
    n = E._combine(n_per_env.astype(np.float64), members, add, 0.0)
    nf = E._combine(nf_per_env.astype(np.float64), members, add, 0.0)
    if not n > 0:
        return [0.0, np.nan, np.nan, np.nan, np.nan, nf]
    mean = E._combine(sum_per_env, members, add, 0.0) / n
    var = E._combine(sumsq_per_env, members, add, 0.0) / n - mean * mean
    counted = [e for e in members if n_per_env[e] > 0]
    return [n, mean, np.sqrt(max(var, 0.0)), min(float(min_per_env[e]) for e in counted), max(float(max_per_env[e]) for e in counted), nf]


def reduce(st, group, num_groups, dt):
    """(G, 5 + 4 + 1, 6) fp64 result table of go1eval_terrain_reduce"""
    group = np.asarray(group)
    once = outcome_values(st, dt)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    for g in range(num_groups):
        members = [int(e) for e in np.nonzero(group == g)[0]]
        for m in range(M):
            out[g, m] = _metric_row(st.count[m], st.nonfinite[m], st.sum[m], st.sumsq[m], st.min[m], st.max[m], members)
        for o in range(len(OUTCOMES)):
            v = once[o].astype(np.float64)
            fin = np.isfinite(v)
            out[g, M + o] = _metric_row(fin, ~fin, np.where(fin, v, 0.0), np.where(fin, v * v, 0.0), v, v, members)
        counts = [float(sum(1 for e in members if st.status[e] == k)) for k in range(4)]
        ended = counts[1] + counts[2] + counts[3]
        out[g, M + len(OUTCOMES)] = [float(len(members))] + counts + [counts[1] / ended if ended > 0 else np.nan]
    return out


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_MASK = 12, 2, 0b0_0110_0110_0110_0111            # bits 0, 1, 2, 5, 6, 9, 10, 13, 14: the trunk and hips and thighs of the legs, no foot
KINDS = ["stays", "traverses", "falls", "times_out", "reset_on_first_step", "odd_coordinates"]


def scripted_field(rng):
    """a 7 x 9 field whose neighbouring samples all differ"""
    return rng.permutation(63).reshape(7, 9).astype(np.int16) * np.int16(3) - np.int16(60)


def scripted_steps(rng, N, steps=SCRIPT_STEPS):
    """`steps` snapshots of the input buffers for N environments on a 7 x 9 field (0.25 m samples, 0.5 m border: world x in
    [-0.5, 1.25), y in [-0.5, 1.75)) with tiles of 1.0 x 0.75 m, and the kind of every environment: one that stays on its tile,
    one that leaves it at some step and is then fed resets and garbage (which must change nothing), one that falls, one that times
    out, one whose very first step is a reset, and one with odd coordinates (NaN and infinite positions, points far outside the
    field, a base exactly on the tile's edge).  Returns (geometry, snapshots, kind)."""
    geo = geometry(warmup_steps=SCRIPT_WARMUP, penalised_body_mask=SCRIPT_MASK, height_samples=scripted_field(rng))
    kind = rng.integers(0, len(KINDS), N)
    kind[:len(KINDS)] = np.arange(len(KINDS))
    when = rng.integers(1, steps - 1, N)                      # the step (0-based) at which kinds 1, 2, 3 end
    origin = np.zeros((3, N), f32)
    origin[0], origin[1] = rng.uniform(0.0, 0.75, N), rng.uniform(0.0, 1.0, N)
    origin[0, kind == 5], origin[1, kind == 5] = 0.25, 0.5    # (dyadic: the edge is hit exactly)
    snaps = []
    for t in range(steps):
        s = dict(root_states=rng.standard_normal((13, N)), commands=rng.uniform(0.0, 0.2, (15, N)), contact_forces=rng.standard_normal((51, N)) * 0.2,
                 foot_positions=np.zeros((12, N)), desired_contact_states=rng.random((4, N)), foot_indices=rng.random((4, N)))
        s = {k: v.astype(f32) for k, v in s.items()}
        s["root_states"][0] = origin[0] + rng.uniform(-0.45, 0.45, N).astype(f32)
        s["root_states"][1] = origin[1] + rng.uniform(-0.35, 0.35, N).astype(f32)
        s["root_states"][2] = rng.uniform(0.2, 0.4, N)
        gone = (kind == 1) & (t >= when)
        s["root_states"][0, gone & (np.arange(N) % 2 == 0)] += 1.0            # leaves along x ...
        s["root_states"][1, gone & (np.arange(N) % 2 == 1)] -= 0.8            # ... or along y
        for f in range(4):
            s["foot_positions"][3 * f] = s["root_states"][0] + rng.uniform(-0.3, 0.3, N).astype(f32)
            s["foot_positions"][3 * f + 1] = s["root_states"][1] + rng.uniform(-0.3, 0.3, N).astype(f32)
            s["foot_positions"][3 * f + 2] = rng.uniform(-0.3, 0.3, N)
        s["contact_forces"][2::3] = np.abs(s["contact_forces"][2::3]) * rng.choice([0.0, 0.05, 1.0], (17, N)).astype(f32)
        quiet = rng.random(N) < 0.5                                           # no sideways force on any foot: no stumble on this step
        for b in FEET_BODIES:
            s["contact_forces"][3 * b:3 * b + 2, quiet] = 0.0
        s["desired_contact_states"][:, rng.random(N) < 0.2] = 0.75            # a step with no swing foot
        odd = kind == 5
        if t == 3:
            s["root_states"][0, odd] = np.nan
        if t == 4:
            s["foot_positions"][3, odd], s["foot_positions"][7, odd] = np.inf, -np.inf
        if t == 5:
            s["foot_positions"][0, odd], s["foot_positions"][4, odd] = -40.0, 3.0e38         # beyond the field on both sides
            s["foot_positions"][6, odd], s["foot_positions"][10, odd] = 1.0e30, -1.0e30
        if t == 6:
            s["root_states"][0, odd] = 0.75                                   # dx = 0.5 = tile_length / 2 exactly: still on the tile
            s["root_states"][1, odd] = 0.125                                  # dy = -0.375 = -tile_width / 2 exactly
        if t == 7:
            s["root_states"][2, odd] = np.inf
        s["reset_buf"] = np.zeros(N, np.uint8)
        s["time_out_buf"] = (rng.random(N) < 0.3).astype(np.uint8)            # time_out_buf alone means nothing
        ends = np.isin(kind, (2, 3)) & (t == when) | (kind == 4) & (t == 0)
        s["reset_buf"][ends] = rng.integers(1, 3, N).astype(np.uint8)[ends]
        s["time_out_buf"][ends] = kind[ends] == 3
        after = (np.isin(kind, (1, 2, 3)) & (t > when)) | ((kind == 4) & (t > 0))
        s["reset_buf"][after] = (rng.random(N) < 0.5).astype(np.uint8)[after]
        s["episode_length_buf"] = np.full(N, t + 1, np.int32)
        s["env_origins"] = origin
        snaps.append(s)
    return geo, snaps, kind


def run(geo, snaps, N):
    st = State(N)
    for s in snaps:
        accumulate(st, geo, s)
    return st
