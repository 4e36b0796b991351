"""TEST INFRASTRUCTURE: numpy model of libgo1episode's kernels, written from the text of include/go1episode.h (the eleven rows, the
state of the open episode, the close on a reset step with its terminal reward, the unseen and the cut episodes, the first sight with
the return taken from episode_sums, the step inside an episode, the tracking errors behind the warm-up, the two length histograms, the
folding rule, the metric rows, the two group rows and the histogram table with the open episodes by age).  Every value is formed in
np.float32 in the header's operation order and summed in float64, so accumulators, state, histograms and both result tables are compared
with the kernels' bit for bit.  The metric-row reduction is joint_ref.py's (eval_ref.py's fixed order, vectorised over the rows); the
histograms' own order (the foot profile's) is restated here."""
import types

import numpy as np

import eval_ref as E
from joint_ref import _combine_rows

METRICS = ["step_reward", "length", "fell", "length_fell", "return", "reward_rate", "lin_vel_err", "yaw_vel_err", "discounted_return", "displacement",
           "path_length"]
STEP_REWARD, LENGTH, FELL, LENGTH_FELL, RETURN, REWARD_RATE, LIN_VEL_ERR, YAW_VEL_ERR, DISCOUNTED_RETURN, DISPLACEMENT, PATH_LENGTH = range(11)
M, BINS, HISTS = len(METRICS), 16, 3
ROWS = M + 2
GROUP_FIELDS = ["envs", "steps", "closed", "fell", "timed_out", "open", "cut", "unseen", "open_steps"]
# the buffers go1episode_accumulate reads (SoA, [k][N])
INPUTS = ["rew_buf", "reset_buf", "time_out_buf", "episode_length_buf", "root_states", "base_lin_vel", "base_ang_vel", "commands", "episode_sums"]
STATE = ["age", "whole", "ret", "disc_ret", "disc_w", "first_pos", "prev_pos", "path", "lin_err", "yaw_err", "track_steps", "steps", "closed", "fell",
         "timed_out", "cut", "unseen", "fall_hist", "timeout_hist"]
f32 = np.float32


def config(warmup_steps=0, gamma=0.99, bin_steps=63, return_row=3):
    """what Go1EpisodeConfig says"""
    return types.SimpleNamespace(warmup_steps=warmup_steps, gamma=gamma, bin_steps=bin_steps, return_row=return_row)


class State:
    """the accumulators and the state after go1episode_clear, in the kernel's own number formats"""

    def __init__(self, N):
        self.N = N
        self.count, self.nonfinite = np.zeros((M, N), np.uint32), np.zeros((M, N), np.uint32)
        self.sum, self.sumsq = np.zeros((M, N)), np.zeros((M, N))
        self.min, self.max = np.full((M, N), np.inf, f32), np.full((M, N), -np.inf, f32)
        self.age, self.whole = np.full(N, -1, np.int32), np.zeros(N, np.uint8)
        self.ret, self.disc_ret, self.disc_w = np.zeros(N, f32), np.zeros(N, f32), np.ones(N, f32)
        self.first_pos, self.prev_pos = np.zeros((2, N), f32), np.zeros((2, N), f32)
        self.path, self.lin_err, self.yaw_err, self.track_steps = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, np.int32)
        self.steps, self.closed, self.fell, self.timed_out, self.cut, self.unseen = (np.zeros(N, np.uint32) for _ in range(6))
        self.fall_hist, self.timeout_hist = np.zeros((BINS, N), np.uint32), np.zeros((BINS, N), np.uint32)

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


def clear(N):
    """go1episode_clear"""
    return State(N)


def length_bin(age, bin_steps):
    """min(age / bin_steps, 15) of the ages >= 0: the bin of an episode of age + 1 steps"""
    return np.minimum(np.asarray(age, np.int64) // int(bin_steps), BINS - 1)


def accumulate(st, cfg, snap):
    """one go1episode_accumulate launch on the SoA buffers `snap` (np.float32 / uint8 / int32 arrays).  Returns what the step did, per
    environment, for the tests that look at single steps: {"closed", "length" (0 where none closed), "timed", "unseen", "cut", "first",
    "whole_close", "tracked", "clamped"}"""
    N = st.N
    zero, one = f32(0.0), f32(1.0)
    env = np.arange(N)
    gamma = f32(cfg.gamma)
    r = snap["rew_buf"]
    assert r.dtype == f32
    reset = snap["reset_buf"] != 0
    timed = snap["time_out_buf"] != 0
    elb = snap["episode_length_buf"]
    x, y = snap["root_states"][0], snap["root_states"][1]
    st.steps += 1                                                                        # 1
    st.fold(STEP_REWARD, np.ones(N, bool), r)
    age = st.age.astype(np.int64)
    known = age >= 0
    close = reset & known                                                                # 2 (a)
    with np.errstate(all="ignore"):
        L = (age + 1).astype(f32)
        ret = st.ret + r
        disc = st.disc_ret + st.disc_w * r
        rate = ret / L
        steps = st.track_steps.astype(f32)
        lin_mean, yaw_mean = st.lin_err / steps, st.yaw_err / steps
        dx, dy = st.prev_pos[0] - st.first_pos[0], st.prev_pos[1] - st.first_pos[1]
        far = np.sqrt(dx * dx + dy * dy)
    assert ret.dtype == disc.dtype == rate.dtype == lin_mean.dtype == far.dtype == f32
    fall = close & ~timed
    st.fold(LENGTH, close, L)
    st.fold(FELL, close, np.where(timed, zero, one))
    st.fold(LENGTH_FELL, fall, L)
    st.fold(RETURN, close, ret)
    st.fold(REWARD_RATE, close, rate)
    tracked = close & (st.track_steps > 0)
    st.fold(LIN_VEL_ERR, tracked, lin_mean)
    st.fold(YAW_VEL_ERR, tracked, yaw_mean)
    whole_close = close & (st.whole != 0)
    st.fold(DISCOUNTED_RETURN, whole_close, disc)
    st.fold(DISPLACEMENT, whole_close, far)
    st.fold(PATH_LENGTH, whole_close, st.path)
    bins = length_bin(np.where(close, age, 0), cfg.bin_steps)
    st.timeout_hist[bins[close & timed], env[close & timed]] += 1
    st.fall_hist[bins[fall], env[fall]] += 1
    st.closed += close.astype(np.uint32)
    st.timed_out += (close & timed).astype(np.uint32)
    st.fell += fall.astype(np.uint32)
    unseen = reset & ~known                                                              # 2 (b)
    st.unseen += unseen.astype(np.uint32)
    running = ~reset
    cut = running & known & (elb.astype(np.int64) != age + 1)                            # 3
    st.cut += cut.astype(np.uint32)
    first = running & (~known | cut)                                                     # 4
    inside = running & ~first                                                            # 5
    with np.errstate(all="ignore"):
        ret_in = st.ret + r
        disc_in = st.disc_ret + st.disc_w * r
        w_in = st.disc_w * gamma
        sx, sy = x - st.prev_pos[0], y - st.prev_pos[1]
        path_in = st.path + np.sqrt(sx * sx + sy * sy)
        ex, ey = snap["base_lin_vel"][0] - snap["commands"][0], snap["base_lin_vel"][1] - snap["commands"][1]
        lin_term = np.sqrt(ex * ex + ey * ey)
        yaw_term = np.abs(snap["base_ang_vel"][2] - snap["commands"][2])
    assert disc_in.dtype == w_in.dtype == path_in.dtype == lin_term.dtype == yaw_term.dtype == f32
    total = snap["episode_sums"][cfg.return_row]
    st.age = np.where(reset, 0, elb).astype(np.int32)                                    # 2 (c), 4, 5
    st.whole = np.where(reset, 1, np.where(first, elb == 1, st.whole)).astype(np.uint8)
    st.ret = np.where(reset, zero, np.where(first, total, ret_in)).astype(f32)
    st.disc_ret = np.where(reset, zero, np.where(first, r, disc_in)).astype(f32)
    st.disc_w = np.where(reset, one, np.where(first, gamma, w_in)).astype(f32)
    fresh = reset | first
    st.first_pos = np.where(fresh, np.stack([x, y]), st.first_pos).astype(f32)
    st.prev_pos = np.stack([x, y]).astype(f32)
    st.path = np.where(fresh, zero, path_in).astype(f32)
    live = running & (elb > cfg.warmup_steps)                                            # 6
    lin0, yaw0, n0 = np.where(fresh, zero, st.lin_err), np.where(fresh, zero, st.yaw_err), np.where(fresh, 0, st.track_steps)
    with np.errstate(all="ignore"):
        st.lin_err = np.where(live, lin0 + lin_term, lin0).astype(f32)
        st.yaw_err = np.where(live, yaw0 + yaw_term, yaw0).astype(f32)
    st.track_steps = np.where(live, n0 + 1, n0).astype(np.int32)
    return dict(closed=close, length=np.where(close, age + 1, 0), timed=close & timed, unseen=unseen, cut=cut, first=first, whole_close=whole_close,
                tracked=tracked, clamped=close & (age // int(cfg.bin_steps) > BINS - 1))


def open_words(st, bin_steps):
    """(16, N): 1 in the bin of every open episode's age"""
    words = np.zeros((BINS, st.N))
    known = st.age >= 0
    words[length_bin(st.age[known], bin_steps), np.arange(st.N)[known]] = 1.0
    return words


def reduce(st, cfg, group, num_groups):
    """((G, 11 + 2, 6) fp64 result table, (G, 3, 16) fp64 histogram table) of go1episode_reduce"""
    group = np.asarray(group)
    out = np.zeros((num_groups, ROWS, len(E.FIELDS)))
    hist = np.zeros((num_groups, HISTS, BINS))
    counted = st.count > 0
    lows = np.where(counted, st.min.astype(np.float64), np.inf)
    highs = np.where(counted, st.max.astype(np.float64), -np.inf)
    slices = E.REDUCE_THREADS // BINS
    words = np.stack([st.fall_hist.astype(np.float64), st.timeout_hist.astype(np.float64), open_words(st, cfg.bin_steps)])      # (3, 16, N)
    known = st.age >= 0
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
        first = np.stack([np.ones(st.N)] + [getattr(st, k).astype(np.float64) for k in ("steps", "closed", "fell", "timed_out")] + [known.astype(np.float64)])
        out[g, M] = _combine_rows(first, members, np.add, 0.0)
        second = np.stack([st.cut.astype(np.float64), st.unseen.astype(np.float64), np.where(known, st.age, 0).astype(np.float64)])
        out[g, M + 1, :3] = _combine_rows(second, members, np.add, 0.0)
        # a histogram: slice k adds the members e = k, k + 16, ... in ascending order; then slice k takes k + 8, + 4, + 2, + 1
        partial = np.zeros((slices, HISTS, BINS))
        for e in members:
            partial[e % slices] += words[:, :, e]
        k = slices // 2
        while k > 0:
            partial[:k] += partial[k:2 * k]
            k //= 2
        hist[g] = partial[0]
    return out, hist


def groups_of(table):
    """the (G, 9) array Go1Episodes.read() calls "groups" from a (G, 13, 6) result table"""
    return np.concatenate([table[:, M, :], table[:, M + 1, :3]], axis=1)


# ---- TEST DATA: the scripted buffers of the emulator test and of the GPU test -----------------------------------------------------------
SCRIPT_STEPS, SCRIPT_WARMUP, SCRIPT_GAMMA, SCRIPT_RETURN_ROW, SCRIPT_COMMANDS = 40, 4, 0.9, 3, 15
KINDS = ["long", "first_reset", "short", "cut", "nonfinite", "random", "fresh"]
SHORT_PERIOD = 3                       # the short kind resets every third step: no step of its episodes gets past the warm-up of 4


def script_config(bin_steps=2):
    return config(warmup_steps=SCRIPT_WARMUP, gamma=SCRIPT_GAMMA, bin_steps=bin_steps, return_row=SCRIPT_RETURN_ROW)


def scripted_steps(rng, N, steps=SCRIPT_STEPS, bin_steps=2):
    """`steps` snapshots of the input buffers for N environments and the kind of every environment.  episode_length_buf is kept
    consistent with the reset flags (0 on a reset step, one more on every other step), except where the script cuts an episode on
    purpose.  The kinds: "long" began before the first launch (a first sight at an age of 5 to 60, the return taken from episode_sums)
    and runs until it times out on step 36 (longer than 16 * bin_steps steps for bin_steps <= 2: the clamp); "first_reset" resets on
    the very first launch (unseen), then falls or times out at random; "short" resets every third step, so its warm-up of 4 steps is
    longer than its episodes (track_steps == 0: no tracking error folded); "cut" has its episode_length_buf set back to 1 on step 10 (a
    reset from outside: the new episode is whole) and pushed on by 7 on step 25 (not whole), and falls on step 33; "nonfinite" gets NaN
    and infinite rewards and a NaN velocity and falls at random; "random" resets with probability 0.1, half of them time-outs; "fresh"
    is first seen at episode_length_buf == 1 (whole) and falls on step 20.  time_out_buf carries noise on the steps without a reset:
    nothing reads it there.  Returns (config, snapshots, kind)."""
    cfg = script_config(bin_steps)
    kind = rng.integers(0, len(KINDS), N)
    kind[:min(N, len(KINDS))] = np.arange(len(KINDS))[:N]
    long_, first_reset, short, cutk, odd, random_, fresh = (kind == k for k in range(len(KINDS)))
    bad = np.array([np.inf, -np.inf, np.nan], f32)
    age = np.where(long_, rng.integers(4, 60, N), np.where(fresh, 0, rng.integers(0, 9, N))).astype(np.int32)
    total = np.where(age > 0, rng.standard_normal(N) * 3.0, 0.0).astype(f32)              # the open episode's rewards before the first launch
    pos = rng.uniform(-5.0, 5.0, (2, N)).astype(f32)
    snaps = []
    for t in range(steps):
        reset = first_reset & (t == 0) | long_ & (t == 36) | short & (t % SHORT_PERIOD == 1) | cutk & (t == 33) | fresh & (t == 20) | \
                (odd | random_ | first_reset) & (t > 0) & (rng.random(N) < 0.1)
        timed = np.where(reset, rng.random(N) < 0.5, rng.random(N) < 0.2)
        timed = np.where(long_, True, np.where(fresh | cutk, False, timed))
        r = (0.02 * rng.standard_normal(N) + 0.01).astype(f32)
        if t % 5 == 2:
            r[odd] = bad[(t // 5) % 3]
        age = np.where(reset, 0, age + 1).astype(np.int32)
        if t == 10:
            age[cutk] = 1
        if t == 25:
            age[cutk] += 7
        with np.errstate(all="ignore"):
            total = np.where(reset, f32(0.0), total + r).astype(f32)                       # the step kernel clears it on a reset
        pos = np.where(reset, rng.uniform(-5.0, 5.0, (2, N)), pos + 0.02 * rng.standard_normal((2, N))).astype(f32)
        s = dict(rew_buf=r, reset_buf=np.where(reset, rng.integers(1, 3, N), 0).astype(np.uint8), time_out_buf=timed.astype(np.uint8),
                 episode_length_buf=age.copy(), root_states=rng.standard_normal((13, N)).astype(f32),
                 base_lin_vel=rng.standard_normal((3, N)).astype(f32), base_ang_vel=rng.standard_normal((3, N)).astype(f32),
                 commands=rng.standard_normal((SCRIPT_COMMANDS, N)).astype(f32), episode_sums=rng.standard_normal((SCRIPT_RETURN_ROW + 1, N)).astype(f32))
        s["root_states"][:2] = pos
        s["episode_sums"][SCRIPT_RETURN_ROW] = total
        if t == 13:
            s["base_lin_vel"][0, odd] = np.nan
        snaps.append(s)
    return cfg, snaps, kind


def run(cfg, snaps, N):
    """(the state after the snapshots, what every step did)"""
    st, did = clear(N), []
    for s in snaps:
        did.append(accumulate(st, cfg, s))
    return st, did
