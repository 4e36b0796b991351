"""TEST INFRASTRUCTURE: numpy model of libgo1obs's kernels, written from the text of include/go1obs.h (the channels and where the
simulator keeps them, the warm-up by age, the folding rule, the fp32 bin of a value and its two tails, the clip count, the step-to-step
change with a reset step and the first measured step folding none, the clear and the break, the `value` and `delta` rows, the group row,
the bins and the tails).  Every value is formed in np.float32 in the header's operation order and summed in float64, so accumulators,
state and the three result tables are compared with the kernels' bit for bit.  The metric-row reduction is joint_ref.py's (eval_ref.py's
fixed order, vectorised over the rows); the per-bin order is sens_ref.py's (the foot profile's)."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows
from sens_ref import _bin_sums

MAX_CHANNELS, BINS = 160, 16
TAILS = ["below", "above", "at_clip"]
GROUP_FIELDS = ["envs", "launches", "measured", "resets"]
INPUTS = ["obs_buf", "privileged_obs_buf", "reset_buf"]
STATE = ["prev", "age", "hist", "below", "above", "at_clip", "launches", "resets"]
f32 = np.float32


def config(spans, num_obs, num_privileged_obs=0, privileged=False, warmup_steps=0, clip=100.0):
    """what Go1ObsConfig says for [(lo, hi)] per channel: lo and scale = 16 / (hi - lo), all in fp32"""
    C = num_obs + (num_privileged_obs if privileged else 0)
    assert len(spans) == C
    lo = np.array([s[0] for s in spans], f32)
    hi = np.array([s[1] for s in spans], f32)
    scale = f32(BINS) / (hi - lo)
    assert scale.dtype == f32
    return types.SimpleNamespace(num_obs=num_obs, num_privileged_obs=num_privileged_obs, privileged=bool(privileged), C=C, warmup_steps=warmup_steps,
                                 clip=f32(clip), lo=lo, scale=scale, spans=[(float(f32(a)), float(f32(b))) for a, b in spans])


def values(cfg, snap):
    """(C, N) np.float32: value(c, e) of the header from the environment-major buffers"""
    obs = snap["obs_buf"]
    assert obs.dtype == f32 and obs.shape[1] == cfg.num_obs
    rows = [obs.T]
    if cfg.privileged:
        priv = snap["privileged_obs_buf"]
        assert priv.dtype == f32 and priv.shape[1] == cfg.num_privileged_obs
        rows.append(priv.T)
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


class State:
    """the accumulators and the state after go1obs_clear, in the kernel's own number formats"""

    def __init__(self, N, cfg):
        C = cfg.C
        self.N, self.C = N, C
        self.count, self.nonfinite = np.zeros((2 * C, N), np.uint32), np.zeros((2 * C, N), np.uint32)
        self.sum, self.sumsq = np.zeros((2 * C, N)), np.zeros((2 * C, N))
        self.min, self.max = np.full((2 * C, N), np.inf, f32), np.full((2 * C, N), -np.inf, f32)
        self.prev, self.age = np.zeros((C, N), f32), np.zeros((C, N), np.uint32)
        self.hist = np.zeros((C, BINS, N), np.uint32)
        self.below, self.above, self.at_clip = (np.zeros((C, N), np.uint32) for _ in range(3))
        self.launches, self.resets = np.zeros(N, np.uint32), np.zeros(N, np.uint32)

    def fold(self, rows, live, v):
        """fold the np.float32 array v (C, N) into the rows `rows` (a slice) where `live`"""
        assert v.dtype == f32
        fin = np.isfinite(v)
        self.nonfinite[rows] += (live & ~fin).astype(np.uint32)
        ok = live & fin
        self.count[rows] += ok.astype(np.uint32)
        v64 = v.astype(np.float64)
        with np.errstate(all="ignore"):
            np.add(self.sum[rows], v64, out=self.sum[rows], where=ok)
            np.add(self.sumsq[rows], v64 * v64, out=self.sumsq[rows], where=ok)
            np.fmin(self.min[rows], v, out=self.min[rows], where=ok)
            np.fmax(self.max[rows], v, out=self.max[rows], where=ok)


def clear(N, cfg):
    """go1obs_clear"""
    return State(N, cfg)


def break_(st, cfg, ids=None):
    """go1obs_break: age = min(age, warmup_steps) and resets += 1 of the named environments (None: all; ids outside [0, N) are left alone)"""
    ids = np.arange(st.N) if ids is None else np.asarray(ids, np.int64)
    ids = ids[(ids >= 0) & (ids < st.N)]
    st.age[:, ids] = np.minimum(st.age[:, ids], np.uint32(max(cfg.warmup_steps, 0)))
    st.resets[ids] += 1


def accumulate(st, cfg, snap):
    """one go1obs_accumulate launch on the buffers `snap` (obs_buf (N, num_obs), privileged_obs_buf (N, num_privileged_obs) np.float32,
    reset_buf (N,) uint8).  Returns what the step did: {"measured": (C, N), "bin": (C, N) (-3 not measured, -2 no bin, -1 below, 16
    above), "delta": (C, N) bool: a change was folded}"""
    C, N = st.C, st.N
    v = values(cfg, snap)
    reset = snap["reset_buf"] != 0
    st.launches += 1                                                                     # 0
    st.age += 1                                                                          # 1
    a = st.age.astype(np.int64)
    measured = a > cfg.warmup_steps
    st.fold(slice(0, C), measured, v)                                                    # 2
    fin = np.isfinite(v)
    with np.errstate(all="ignore"):
        t = (v - cfg.lo[:, None]) * cfg.scale[:, None]                                   # 3
    assert t.dtype == f32
    below, inside = fin & (t < 0), fin & (t >= 0) & (t < BINS)
    above = fin & ~below & ~inside
    st.below += (measured & below).astype(np.uint32)
    st.above += (measured & above).astype(np.uint32)
    which = np.where(inside, t, 0).astype(np.int64)
    c_, e_ = np.nonzero(measured & inside)
    st.hist[c_, which[c_, e_], e_] += 1
    with np.errstate(all="ignore"):
        st.at_clip += (measured & (np.abs(v) >= cfg.clip)).astype(np.uint32)             # 4
        change = np.abs(v - st.prev)
    st.resets += (measured[0] & reset).astype(np.uint32)                                 # 5
    folds = measured & ~reset[None, :] & (a - 1 > cfg.warmup_steps)
    st.fold(slice(C, 2 * C), folds, change)
    st.prev = v.copy()                                                                   # 6 (and step 1's)
    return dict(measured=measured, delta=folds, bin=np.where(~measured, -3, np.where(~fin, -2, np.where(below, -1, np.where(above, BINS, which)))))


def reduce(st, group, num_groups):
    """((G, 2 C + 1, 6) result table, (G, C, 16) bins, (G, C, 3) tails) of go1obs_reduce, fp64"""
    C = st.C
    group = np.asarray(group)
    out = np.zeros((num_groups, 2 * C + 1, len(E.FIELDS)))
    hist = np.zeros((num_groups, C, BINS))
    tails = np.zeros((num_groups, C, len(TAILS)))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    words = st.hist.astype(np.float64)
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
        out[g, :2 * C] = rows
        measured = st.count[0].astype(np.float64) + st.nonfinite[0].astype(np.float64)
        out[g, 2 * C, :4] = _combine_rows(np.stack([np.ones(st.N), st.launches.astype(np.float64), measured, st.resets.astype(np.float64)]), members, np.add, 0.0)
        hist[g] = _bin_sums(words, members)
        for c in range(C):
            tails[g, c] = _combine_rows(np.stack([getattr(st, k)[c].astype(np.float64) for k in TAILS]), members, np.add, 0.0)
    return out, hist, tails


def run(cfg, snaps, N, breaks=None):
    """(the state after a clear and a launch on each of `snaps`, what every launch did); breaks = {launch index: ids or None}: a
    go1obs_break of those environments in front of that launch"""
    st, did = clear(N, cfg), []
    for k, s in enumerate(snaps):
        if breaks and k in breaks:
            break_(st, cfg, breaks[k])
        did.append(accumulate(st, cfg, s))
    return st, did


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_CLIP, SCRIPT_BREAK = 12, 2, 3.0, 7
SCRIPT_BREAK_IDS = [0, 3, 5]                   # (those below N) are named by the go1obs_break in front of launch SCRIPT_BREAK
KINDS = ["steady", "resets", "constant", "nonfinite", "outside", "edges", "random"]


def script_spans(C):
    """channel c's sixteen bins: spans of several widths and offsets, every bound exact in fp32"""
    return [(-2.0 + 0.25 * (c % 5), 2.0 + 0.5 * (c % 3)) for c in range(C)]


def scripted_steps(rng, N, num_obs, num_privileged_obs=0, privileged=False, steps=SCRIPT_STEPS):
    """(config, `steps` snapshots of the buffers after a step, {SCRIPT_BREAK: ids}, the kind of every environment).  The kinds: "steady"
    never resets; "resets" resets on launches 4 and 9; "constant" holds one value per channel throughout; "nonfinite" carries a NaN in
    its even channels on launch 5, +inf on launch 6 and -inf on launch 8; "outside" sits below lo in its even and above hi in its odd
    channels, beyond the clip; "edges" walks through exactly lo, exactly hi, exactly +clip, exactly -clip and -0.0; "random" resets with
    probability 0.2.  Observations are normal with a scale of 1.2, clipped to +-SCRIPT_CLIP as the simulator clips them (so +-clip
    itself occurs)."""
    C = num_obs + (num_privileged_obs if privileged else 0)
    cfg = config(script_spans(C), num_obs, num_privileged_obs, privileged, warmup_steps=SCRIPT_WARMUP, clip=SCRIPT_CLIP)
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    steady, resets, constant, odd, outside, edges, random_ = (kind == k for k in range(len(KINDS)))
    width = num_obs + num_privileged_obs
    held = rng.uniform(-1.0, 1.0, (N, width)).astype(f32)
    walk = [None, None, None, "lo", "hi", "clip", "-clip", "-0", "lo", None, "hi", None]
    lo_all = np.concatenate([cfg.lo, np.zeros(width - C, f32)])
    hi_all = np.concatenate([np.array([s[1] for s in script_spans(C)], f32), np.ones(width - C, f32)])
    even = (np.arange(width) % 2 == 0)[None, :]
    snaps = []
    for t in range(steps):
        x = np.clip((1.2 * rng.standard_normal((N, width))).astype(f32), -f32(SCRIPT_CLIP), f32(SCRIPT_CLIP))
        x[constant] = held[constant]
        x[outside] = np.where(even, f32(-50.0), f32(50.0)).astype(f32)
        if t == 5:
            x[odd] = np.where(even, f32(np.nan), x[odd])
        if t == 6:
            x[odd] = np.where(even, f32(np.inf), x[odd])
        if t == 8:
            x[odd] = np.where(even, f32(-np.inf), x[odd])
        what = walk[t % len(walk)]
        if what is not None:
            x[edges] = dict(lo=lo_all, hi=hi_all, clip=np.full(width, SCRIPT_CLIP, f32), **{"-clip": np.full(width, -SCRIPT_CLIP, f32), "-0": np.full(width, -0.0, f32)})[what]
        reset = resets & ((t == 4) | (t == 9)) | random_ & (rng.random(N) < 0.2)
        snaps.append(dict(obs_buf=np.ascontiguousarray(x[:, :num_obs]), privileged_obs_buf=np.ascontiguousarray(x[:, num_obs:]),
                          reset_buf=np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8)))
    return cfg, snaps, {SCRIPT_BREAK: [e for e in SCRIPT_BREAK_IDS if e < N]}, kind
