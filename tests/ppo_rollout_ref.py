"""float64 models of the rollout half of libgo1ppo.so (go1ppo_act, go1ppo_store_step, go1ppo_gae, go1ppo_normalize and the observation
ring go1ppo_ring_snapshot / _step / _gather), the recipes that build their test inputs, the comparators, and the tables of cases the CPU
and the GPU tests share.

The models are plain numpy on the CPU, written from the statements of go1_gym_learn/ppo_cse/ppo.py (PPO.act, process_env_step,
gaussian_log_prob) and rollout_storage.py (compute_returns, _global_mean_std).  They read the bits the kernels read: the bf16 head outputs
widened exactly, gamma, lam and 1e-8 as the fp32 numbers the kernels receive, widened.

Every model returns a value and a per-element bound.  u = 2^-24 is the unit round-off of fp32 (2^-53 of fp64); the bounds count the
roundings of the kernel's expression with every multiply-add rounded twice, so they hold whether or not the compiler contracts it (a
contracted one rounds once), and they take fp32 divide and sqrt as correctly rounded.  None is taken from what the kernels give.

  act        mu, sigma, values: bit for bit.  actions a = fl(m + fl(s n)): |got - (m + s n)| <= u |s n| + u (|m| + |s n|) (1 + u)
             <= 2^-23 (|m| + |s n|).  logp is evaluated from the actions the kernel WROTE (the reference takes the log-probability of
             the sampled actions): q_j = (a_j - m_j)^2 / (2 s_j^2), L_j = log s_j, C = A log(2 pi) / 2, logp = -sum q - (sum L + C).
             fp32: a - m and the divide round once each and enter squared, the square rounds once (5 u on q_j, from 3 roundings), logf is
             within 2 ulp (4 u on L_j), each running sum makes A additions (A u), the fp32 constant and its product with A round once
             each (2 u on C), and two closing operations (2 u): at most (A + 7) u of sum q + sum |L| + C, bounded by
             (A + 8) 2^-23 (sum q + sum |L| + C), a factor 2 above the count.
  store_step rewards_out == rewards (as numbers) where no time-out applies; else |got - (r + g v)| <= 2^-23 (|r| + |g v|) as for the
             actions; dones byte for byte; env_bins_out == float32(env_bins) bit for bit (round to nearest even above 2^24).
  gae        adv_t = r_t + al g v_{t+1} - v_t + al g lam adv_{t+1}, al = 1 - done_t.  fp32: the product with v_{t+1} rounds once, the
             two additions of delta once each on partial sums below |r| + al g |v_next| + |v| (3 u of it in all); fl(g lam) and its
             product with adv_{t+1} round once each (2 u al g lam |adv_{t+1}|, and the incoming error grows by (1 + 2 u)); the last
             addition rounds once on at most mag_t (1 + 3 u) + the incoming error.  With
                 mag_t = |r| + al g |v_next| + |v| + al g lam |adv_{t+1}|,   err_t = al g lam err_{t+1} (1 + 4 u) + 6 u mag_t
             |adv_fp32 - adv_t| <= err_t.  returns = fl(adv + v): err_t + 2 u (|adv| + |v|); advantages = fl(ret - v), formed as the
             reference forms them: the returns' bound + 2 u (|ret| + |v|).
             stats: float64 sums of the kernel's OWN fp32 advantages (the square of an fp32 number is exact in double), exact
             (math.fsum); the kernel makes T additions per thread, 6 in the butterfly, 3 over the waves, one per workgroup and the
             closing `+=`: |got - ref| <= n_add 2^-53 (sum |term| + |start|), n_add = T + 12 + workgroups.
  normalize  out = (adv - mean) / (sd + 1e-8) from the given stats, the variance by the kernel's formula clamped at 0.  fp32: mean
             rounds to fp32 (u |mean| / (sd + eps) on the result), sd rounds and the addition of eps rounds (2 u relative), the
             subtraction and the divide once each (2 u relative): 2^-22 |out| + 2^-23 |mean| / (sd + eps).
  ring       an integer model on the bf16 bit patterns: round to nearest even as (b + 0x7FFF + ((b >> 16) & 1)) >> 16 on the fp32 bits
             b; rows [window oldest first | 1.0 | bf16(priv) | 0 ...]; compared bit for bit, a NaN input only as "is a NaN"."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24                                  # fp32 unit round-off
U64 = 2.0 ** -53
GAMMA, LAM = float(np.float32(0.99)), float(np.float32(0.95))      # as the kernels receive them
EPS = float(np.float32(1e-8))
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
F32, F64 = np.float32, np.float64

ActCase = namedtuple("ActCase", "name rows A head_ld shared")                 # shared: value is column A of the buffer that holds mean
StoreCase = namedtuple("StoreCase", "name n time_outs env_bins share")         # share: of the elements that timed out
GaeCase = namedtuple("GaeCase", "name T N dones scale gamma lam")
NormCase = namedtuple("NormCase", "name n kind mu sd")
RingCase = namedtuple("RingCase", "name N T H no npv Kp")

ACT_CASES = [ActCase(f"rows{r}-A{A}-ld{ld}" + ("-shared" if sh else ""), r, A, ld, sh) for r, A, ld, sh in (
    (1, 12, 64, False), (63, 5, 5, False), (64, 12, 12, False), (65, 1, 1, False), (257, 12, 64, True), (257, 32, 36, True),
    (65, 32, 32, False), (257, 5, 36, False), (64, 1, 64, True), (257, 12, 36, False))]

STORE_CASES = [StoreCase(f"n{n}-{'to' if to else 'noto'}-{'bins' if b else 'nobins'}" + (f"-share{sh:g}" if to else ""), n, to, b, sh)
               for n, to, b, sh in ((1, True, True, 1.0), (255, True, False, 0.05), (256, False, True, 0.0), (257, False, False, 0.0),
                                    (1000, True, True, 0.05), (257, True, True, 0.0), (1000, True, False, 1.0))]
SPECIAL_BINS = (16777217, 2147483647, -1, 0, 16777216)

GAE_DONES = ("none", "random", "all", "last", "first")
GAE_CASES = [GaeCase(f"T{T}-N{N}-{p}" + ("-x100" if sc != 1.0 else "") + ("-g1" if g == 1.0 else ""), T, N, p, sc, g, g if g == 1.0 else LAM)
             for T, N, p, sc, g in ((1, 1, "none", 1.0, GAMMA), (1, 1, "all", 1.0, GAMMA), (1, 64, "random", 1.0, GAMMA), (2, 63, "last", 1.0, GAMMA),
                                    (2, 63, "first", 1.0, GAMMA), (7, 65, "random", 1.0, GAMMA), (7, 65, "all", 1.0, GAMMA),
                                    (7, 256, "none", 1.0, GAMMA), (7, 256, "first", 1.0, GAMMA), (24, 257, "random", 1.0, GAMMA),
                                    (24, 257, "random", 100.0, GAMMA), (24, 257, "last", 1.0, GAMMA), (3, 1000, "random", 1.0, 1.0),
                                    (3, 1000, "none", 1.0, GAMMA), (24, 1025, "random", 1.0, GAMMA), (24, 1025, "all", 1.0, 1.0))]
TICKET_N = (1, 257, 1000, 64, 1025)             # go1ppo_gae launches of the ticket-counter test (1, 2, 4, 1 and 5 workgroups), T = 3

NORM_CASES = [NormCase("n2", 2, "plain", 0.0, 1.0), NormCase("n255", 255, "plain", 3.0, 0.5), NormCase("n257", 257, "plain", -10.0, 2.0),
              NormCase("n1000", 1000, "plain", 100.0, 1.0), NormCase("n1000-two-ranks", 1000, "two-ranks", 0.5, 1.0),
              NormCase("n257-constant", 257, "constant", 1.5, 0.0), NormCase("n255-negative-variance", 255, "negative-variance", 1.5, 1e-5)]


def ring_min_kp(H, no, npv):
    return (H * no + 1 + npv + 1) // 2 * 2


RING_PAD = 300                                  # extra bf16 columns of a padded case: 150 dwords, more than two wavefront passes
RING_CASES = [RingCase(f"N{N}-T{T}-H{H}-no{no}-npv{npv}" + ("-padded" if pad else ""), N, T, H, no, npv, ring_min_kp(H, no, npv) + pad)
              for N, T, H, no, npv, pad in ((1, 1, 1, 2, 0, 0), (3, 3, 2, 70, 2, 0), (4, 1, 5, 130, 1, 0), (5, 3, 6, 70, 65, 0),
                                            (37, 3, 7, 2, 2, RING_PAD), (37, 1, 12, 70, 0, 0), (5, 3, 13, 130, 2, 0), (3, 1, 6, 2, 1, RING_PAD),
                                            (4, 3, 7, 70, 1, 0), (1, 3, 13, 70, 65, RING_PAD), (37, 3, 1, 130, 65, 0), (5, 1, 12, 2, 0, RING_PAD),
                                            (3, 3, 5, 70, 2, 0))]
RING_PATTERN_CASE = RingCase("rounding-patterns", 5, 3, 2, 70, 2, ring_min_kp(2, 70, 2))
RING_WRAPPER_CASE = RingCase("wrappers", 37, 3, 7, 70, 2, (7 * 70 + 1 + 2 + 7) // 8 * 8)       # RolloutStorage pads the rows to 8 columns


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def _rng(name):
    return np.random.default_rng(_seed(name))


# ------------------------------------------------------------------------------------------------------------------ comparing
def ratio(err, bound):
    """largest err / bound; inf where an error is outside a zero bound or is a NaN"""
    err, bound = np.asarray(err, F64).ravel(), np.asarray(bound, F64).ravel()
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= bound, np.where(bound > 0, err / bound, 0.0), np.inf)
    return float(r.max())


def passes(checks):
    return all(ratio(e, b) <= 1.0 for e, b in checks.values())


def bit_diff(a, b):
    """1.0 where the bit patterns differ (to be held against a zero bound)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    v = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    d = (a.view(v) != b.view(v)).astype(F64)
    return d, np.zeros_like(d)


# ------------------------------------------------------------------------------------------------------------------ bf16
def f32_bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def bf16_bits(x, truncate=False):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even in integer arithmetic; a NaN becomes a quiet NaN of its sign"""
    b = f32_bits(x).astype(np.uint64)
    r = (b >> 16) if truncate else ((b + 0x7FFF + ((b >> 16) & 1)) >> 16)
    if not truncate:
        r = np.where((b & 0x7FFFFFFF) > 0x7F800000, (b >> 16) | 0x40, r)
    return r.astype(np.uint16)


def bf16_widen(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_is_nan(bits):
    return (np.asarray(bits, np.uint16) & 0x7FFF) > 0x7F80


def rounding_patterns():
    """fp32 bit patterns (uint32) at which a bf16 conversion can go wrong: around the ties, into infinity, NaNs; no subnormals"""
    p = []
    for sign in (0, 0x80000000):
        for e in (1, 100, 126, 127, 128, 200, 254):
            for m7 in (0x12, 0x13, 0x7E, 0x7F):                    # even and odd upper halves; 0x7F carries into the exponent
                for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
                    p.append(sign | (e << 23) | (m7 << 16) | low)
    p += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0xFF7F8000, 0x00800000, 0x80800000,
          0x7FC00000, 0x7F800001, 0xFFFFFFFF]
    return np.array(p, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------------------------ act
def act_inputs(c):
    """mean (|m| up to 8) and value as bf16 bit patterns inside their [rows][head_ld] buffers, std in [0.05, 2] (log std of both signs
    where A > 1), noise with exact zeros and with |std noise| = 1e-3 (a - m cancels against |m| up to 8)"""
    g = _rng(c.name)
    rows, A, ld = c.rows, c.A, c.head_ld
    assert ld >= A and (not c.shared or ld > A)
    mean = bf16_bits(g.uniform(-8.0, 8.0, (rows, A)).astype(F32))
    mean[0, 0] = bf16_bits(np.array([8.0], F32))[0]
    value = bf16_bits(g.standard_normal(rows).astype(F32))
    std = g.uniform(0.05, 2.0, A).astype(F32)
    std[0] = 0.05
    if A > 1:
        std[-1] = 2.0
    noise = g.standard_normal((rows, A)).astype(F32)
    k = g.random((rows, A))
    small = (k >= 0.05) & (k < 0.25)
    noise[small] = (np.sign(noise) * (1e-3 / std.astype(F64)))[small].astype(F32)
    noise[k < 0.05] = 0.0
    if rows * A > 1:
        noise[0, 0] = 0.0
        noise[-1, -1] = F32(1e-3 / float(std[-1]))
    junk = bf16_bits(np.array([-3.0], F32))[0]                     # columns nobody may read as data hold -3
    head = np.full((rows, ld), junk, np.uint16)
    head[:, :A] = mean
    value_head = None
    if c.shared:
        head[:, A] = value
    else:
        value_head = np.full((rows, ld), junk, np.uint16)
        value_head[:, 0] = value
    return dict(case=c, mean=mean, value=value, std=std, noise=noise, head=head, value_head=value_head)


def act_model(d):
    m, s, n = bf16_widen(d["mean"]).astype(F64), d["std"].astype(F64), d["noise"].astype(F64)
    sn = s * n                                                      # exact: 24 x 24 bits
    return dict(mu=bf16_widen(d["mean"]), sigma=np.ascontiguousarray(np.broadcast_to(d["std"], d["mean"].shape)), values=bf16_widen(d["value"]),
                actions=m + sn, actions_bound=2.0 ** -23 * (np.abs(m) + np.abs(sn)))


def act_logp(d, actions):
    """log-probability of the given (fp32) actions in float64, and its bound"""
    A = d["case"].A
    m, s = bf16_widen(d["mean"]).astype(F64), d["std"].astype(F64)
    q = 0.5 * ((actions.astype(F64) - m) / s) ** 2
    L = np.log(s)
    C = A * HALF_LOG_2PI
    return -q.sum(-1) - (L.sum() + C), (A + 8) * 2.0 ** -23 * (q.sum(-1) + np.abs(L).sum() + C)


def act_compare(d, got):
    """got: actions, mu, sigma [rows, A], values, logp [rows] as fp32 arrays -> {name: (err, bound)}"""
    m = act_model(d)
    logp, logp_bound = act_logp(d, got["actions"])
    return dict(mu=bit_diff(got["mu"], m["mu"]), sigma=bit_diff(got["sigma"], m["sigma"]), values=bit_diff(got["values"], m["values"]),
                actions=(np.abs(got["actions"].astype(F64) - m["actions"]), m["actions_bound"]),
                logp=(np.abs(got["logp"].astype(F64) - logp), logp_bound))


def act_fp32(d, variant=None):
    """the kernel's statements in fp32 numpy, a rounding after every operation; `variant`: a deliberately wrong one"""
    A = d["case"].A
    m, sg, n = bf16_widen(d["mean"]), d["std"], d["noise"]
    a = (m + sg * n).astype(F32)
    lp, logs = np.zeros(m.shape[0], F32), F32(0.0)
    for j in range(A):
        z = ((a[:, j] - m[:, j]) / sg[j]).astype(F32)
        lp = (lp + (F32(-0.5) * z) * z).astype(F32)
        L = np.log(sg[j]).astype(F32)
        logs = F32(logs + (F32(2.0) * L if variant == "log_sigma_squared" else L))
    const = F32(0.0) if variant == "no_constant" else F32(F32(A) * F32(0.9189385332046727))
    return dict(actions=a, mu=m.copy(), sigma=np.ascontiguousarray(np.broadcast_to(sg, m.shape)), values=bf16_widen(d["value"]),
                logp=(lp - F32(logs + const)).astype(F32))


# ------------------------------------------------------------------------------------------------------------------ store_step
def store_inputs(c):
    g = _rng(c.name)
    n = c.n
    d = dict(case=c, rewards=g.standard_normal(n).astype(F32), values=(2.0 * g.standard_normal(n)).astype(F32),
             dones=g.integers(0, 256, n).astype(np.uint8), gamma=GAMMA, time_outs=None, env_bins=None)
    d["rewards"][0] = -0.0                                          # -0 + 0 is +0: compared as a number
    if c.time_outs:
        to = (g.random(n) < c.share).astype(np.uint8)
        if 0.0 < c.share < 1.0:
            to[n // 2], to[n // 3] = 1, 0                           # both kinds present whatever the draw
        d["time_outs"] = to
    if c.env_bins:
        bins = g.integers(0, 4000, n).astype(np.int32)
        big = g.random(n) < 0.2
        bins[big] = g.integers(1 << 24, (1 << 31) - 1, n)[big].astype(np.int32)
        k = min(n, len(SPECIAL_BINS))
        bins[:k] = SPECIAL_BINS[:k]
        d["env_bins"] = bins
    return d


def store_compare(d, got, canary=7.0):
    """got: rewards_out, env_bins_out (fp32), dones_out (uint8)"""
    r, v = d["rewards"].astype(F64), d["values"].astype(F64)
    to = d["time_outs"].astype(bool) if d["time_outs"] is not None else np.zeros(r.shape, bool)
    ref = np.where(to, r + d["gamma"] * v, r)
    bound = np.where(to, 2.0 ** -23 * (np.abs(r) + np.abs(d["gamma"] * v)), 0.0)
    bins = d["env_bins"].astype(F32) if d["env_bins"] is not None else np.full(r.shape, canary, F32)
    return dict(rewards=(np.abs(got["rewards_out"].astype(F64) - ref), bound), dones=bit_diff(got["dones_out"], d["dones"]),
                env_bins=bit_diff(got["env_bins_out"], bins))


def store_fp32(d, variant=None, canary=7.0):
    r, v, g = d["rewards"], d["values"], F32(d["gamma"])
    if variant == "bootstrap_all":
        flag = np.ones(r.shape, F32)
    else:
        flag = d["time_outs"].astype(bool).astype(F32) if d["time_outs"] is not None else None
    out = r.copy() if flag is None else (r + g * (v * flag)).astype(F32)
    bins = d["env_bins"].astype(F32) if d["env_bins"] is not None else np.full(r.shape, canary, F32)
    return dict(rewards_out=out, dones_out=d["dones"].copy(), env_bins_out=bins)


# ------------------------------------------------------------------------------------------------------------------ gae
def gae_inputs(c, name=None):
    g = _rng(name or c.name)
    T, N = c.T, c.N
    dones = np.zeros((T, N), np.uint8)
    if c.dones == "random":
        dones = (g.random((T, N)) < 0.1).astype(np.uint8)
        dones.flat[g.integers(0, T * N)] = 1
    elif c.dones == "all":
        dones[:] = 1
    elif c.dones == "last":
        dones[T - 1] = 1
    elif c.dones == "first":
        dones[0] = 1
    rnd = lambda *s: (c.scale * g.standard_normal(s)).astype(F32)
    return dict(case=c, rewards=rnd(T, N), values=rnd(T, N), last_values=rnd(N), dones=dones, gamma=c.gamma, lam=c.lam)


def gae_model(d):
    """float64 scan with the running error bound beside it: returns, advantages (= returns - values, un-normalised) and their bounds"""
    r, v, last = d["rewards"].astype(F64), d["values"].astype(F64), d["last_values"].astype(F64)
    g, gl = d["gamma"], d["gamma"] * d["lam"]
    T, N = r.shape
    adv, err, nv = np.zeros(N), np.zeros(N), last
    ret, ret_b, advs, adv_b = (np.zeros((T, N)) for _ in range(4))
    for t in range(T - 1, -1, -1):
        al = 1.0 - d["dones"][t].astype(F64)
        mag = np.abs(r[t]) + al * g * np.abs(nv) + np.abs(v[t]) + al * gl * np.abs(adv)
        err = al * gl * err * (1.0 + 4.0 * U) + 6.0 * U * mag
        adv = r[t] + al * g * nv - v[t] + al * gl * adv
        ret[t] = adv + v[t]
        ret_b[t] = err + 2.0 * U * (np.abs(adv) + np.abs(v[t]))
        advs[t] = ret[t] - v[t]
        adv_b[t] = ret_b[t] + 2.0 * U * (np.abs(ret[t]) + np.abs(v[t]))
        nv = v[t]
    return dict(returns=ret, returns_bound=ret_b, advantages=advs, advantages_bound=adv_b)


def gae_compare(d, got):
    m = gae_model(d)
    return dict(returns=(np.abs(got["returns"].astype(F64) - m["returns"]), m["returns_bound"]),
                advantages=(np.abs(got["advantages"].astype(F64) - m["advantages"]), m["advantages_bound"]))


def gae_fp32(d, variant=None):
    r, v = d["rewards"], d["values"]
    g, lam = F32(d["gamma"]), F32(1.0 if variant == "no_lambda" else d["lam"])
    T, N = r.shape
    adv, nv = np.zeros(N, F32), d["last_values"]
    ret, advs = np.zeros((T, N), F32), np.zeros((T, N), F32)
    one = np.ones(N, F32)
    for t in range(T - 1, -1, -1):
        al = (F32(1.0) - d["dones"][t].astype(F32)).astype(F32)
        boot = v[t] if variant == "bootstrap_same_step" else nv
        delta = ((r[t] + ((one if variant == "no_mask_value" else al) * g) * boot).astype(F32) - v[t]).astype(F32)
        adv = (delta + ((((one if variant == "no_mask_advantage" else al) * g) * lam).astype(F32) * adv).astype(F32)).astype(F32)
        ret[t] = (adv + v[t]).astype(F32)
        advs[t] = (ret[t] - v[t]).astype(F32)
        nv = v[t]
    return dict(returns=ret, advantages=advs)


def gae_workgroups(N):
    return (N + 255) // 256


def gae_stat_terms(adv):
    """exact float64 sums (and sums of magnitudes) of the fp32 advantages and of their squares"""
    a = adv.astype(F64).ravel()
    sq = a * a                                                      # exact: 24 x 24 bits
    return np.array([math.fsum(a), math.fsum(sq)]), np.array([math.fsum(np.abs(a)), math.fsum(sq)])


def gae_stats_start(d):
    """what the destination holds before the launch: a quarter of sum |term| with alternating signs (sizes from the model)"""
    _, mags = gae_stat_terms(gae_model(d)["advantages"].astype(F32))
    return np.array([0.25, -0.25]) * mags


def gae_stats_check(adv, start, got, T, N):
    """(err, bound) of the two sums after `start += sum` over the fp32 advantages `adv` of one launch"""
    sums, mags = gae_stat_terms(adv)
    n_add = T + 12 + gae_workgroups(N)
    return np.abs(np.asarray(got, F64) - (start + sums)), n_add * U64 * (mags + np.abs(start))


# ------------------------------------------------------------------------------------------------------------------ normalize
def norm_inputs(c):
    g = _rng(c.name)
    n = c.n
    if c.kind == "constant":
        adv = np.full(n, c.mu, F32)
    elif c.kind == "negative-variance":
        adv = (c.mu + c.sd * g.integers(-4, 5, n)).astype(F32)     # a true variance near 1e-10 on a mean of 1.5
    else:
        adv = (c.mu + c.sd * g.standard_normal(n)).astype(F32)
    a = adv.astype(F64)
    ranks = 2.0 if c.kind == "two-ranks" else 1.0
    stats = np.array([ranks * math.fsum(a), ranks * math.fsum(a * a), ranks * n])
    if c.kind == "negative-variance":
        stats[1] *= 1.0 - 1e-9                                      # the sum of squares a little below count * mean^2
    return dict(case=c, adv=adv, stats=stats)


def norm_moments(stats):
    cnt = stats[2]
    mean = stats[0] / cnt
    var = (stats[1] - cnt * mean * mean) / (cnt - 1.0)
    return mean, var


def norm_model(d):
    mean, var = norm_moments(d["stats"])
    s = math.sqrt(max(var, 0.0)) + EPS
    out = (d["adv"].astype(F64) - mean) / s
    return out, 2.0 ** -22 * np.abs(out) + 2.0 ** -23 * abs(mean) / s


def norm_compare(d, got):
    out, bound = norm_model(d)
    checks = dict(advantages=(np.abs(got.astype(F64) - out), bound))
    if d["case"].kind == "constant":
        checks["exact_zero"] = (np.abs(got.astype(F64)), np.zeros(got.shape))
    return checks


def norm_fp32(d, variant=None):
    cnt = d["stats"][2]
    mean, var = norm_moments(d["stats"])
    if variant == "biased":
        var = var * (cnt - 1.0) / cnt
    var = max(var, 0.0)
    if variant == "eps_inside_sqrt":
        den = F32(math.sqrt(var + EPS))
    else:
        den = F32(F32(math.sqrt(var)) + F32(1e-8))
    return ((d["adv"] - F32(mean)).astype(F32) / den).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ ring
def ring_inputs(c, patterns=False):
    """the observation stream of a rollout, [T + H - 1][N][no] fp32 (entry t is the newest of step t - H + 1), the privileged
    observations [T][N][npv], and the environments' history windows of step 0 inside rows of ld_hist > H * no elements"""
    g = _rng(c.name)
    N, T, H, no, npv = c.N, c.T, c.H, c.no, c.npv
    assert c.Kp % 2 == 0 and c.Kp >= H * no + 1 + npv and no % 2 == 0
    stream = (3.0 * g.standard_normal((T + H - 1, N, no))).astype(F32)
    priv = g.standard_normal((T, N, npv)).astype(F32)
    if patterns:
        p = rounding_patterns()
        stream = np.resize(p, stream.size).reshape(stream.shape).view(F32).copy()
        priv = np.resize(p[::-1], priv.size).reshape(priv.shape).view(F32).copy()
    ld_hist = H * no + 6
    hist = np.full((N, ld_hist), -5.0, F32)
    hist[:, :H * no] = stream[:H].transpose(1, 0, 2).reshape(N, H * no)
    return dict(case=c, stream=stream, priv=priv, hist=hist, ld_hist=ld_hist)


def ring_rows(window, priv, Kp, variant=None):
    """augmented rows [window oldest first | 1.0 | bf16(priv) | 0 ...] as bf16 bit patterns; window: uint16 [rows][H][no] (oldest
    first), priv: fp32 [rows][npv]"""
    rows, H, no = window.shape
    npv = priv.shape[1]
    X = np.zeros((rows, Kp), np.uint16)
    X[:, :H * no] = (window[:, ::-1] if variant == "newest_first" else window).reshape(rows, H * no)
    X[:, H * no] = 0x3F80
    X[:, H * no + 1:H * no + 1 + npv] = bf16_bits(priv, truncate=variant == "truncate")
    if variant == "bias_swapped":
        X[:, [H * no, H * no + 1]] = X[:, [H * no + 1, H * no]]
    return X


def ring_model(d, variant=None):
    """ring: the stream in bf16, uint16 [T + H - 1][N][no]; X[s]: the inference rows of step s, [N][Kp]; gather(idx): mini-batch rows"""
    c = d["case"]
    ring = bf16_bits(d["stream"], truncate=variant == "truncate")
    window = lambda s, n: ring[s:s + c.H, n]                        # [H][..][no]
    X = [ring_rows(np.stack([window(s, n) for n in range(c.N)]), d["priv"][s], c.Kp, variant) for s in range(c.T)]

    def gather(idx):
        s, n = np.asarray(idx) // c.N, np.asarray(idx) % c.N
        return ring_rows(np.stack([window(a, b) for a, b in zip(s, n)]), d["priv"][s, n], c.Kp, variant)
    return dict(ring=ring, X=X, gather=gather)


def ring_gather_idx(c):
    """descending, with duplicates, entries of the last step included, not a multiple of 4 long where that is possible: all in range"""
    idx = list(range(c.T * c.N - 1, -1, -1))
    idx = idx[:1] + idx[:1] + idx + [c.T * c.N // 2] * 2
    return np.array(sorted(idx, reverse=True), np.int64)


def bf16_compare(got, want, nan_in):
    """bit for bit outside `nan_in` (where the fp32 input was a NaN), "is a NaN" inside"""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    assert got.shape == want.shape == nan_in.shape, (got.shape, want.shape, nan_in.shape)
    bad = np.where(nan_in, ~bf16_is_nan(got), got != want).astype(F64)
    return bad, np.zeros_like(bad)


def ring_nan_masks(d):
    """where the model's ring / rows come from a NaN input: (ring mask, rows mask of a step, rows mask of an index set)"""
    c = d["case"]
    r_nan, p_nan = np.isnan(d["stream"]), np.isnan(d["priv"])

    def rows(win, pv):
        m = np.zeros((win.shape[0], c.Kp), bool)
        m[:, :c.H * c.no] = win.reshape(win.shape[0], -1)
        m[:, c.H * c.no + 1:c.H * c.no + 1 + c.npv] = pv
        return m
    step = lambda s: rows(np.stack([r_nan[s:s + c.H, n] for n in range(c.N)]), p_nan[s])

    def gather(idx):
        s, n = np.asarray(idx) // c.N, np.asarray(idx) % c.N
        return rows(np.stack([r_nan[a:a + c.H, b] for a, b in zip(s, n)]), p_nan[s, n])
    return r_nan, step, gather


def ring_compare(d, got):
    """got: ring [T + H - 1][N][no], X (list over the steps of [N][Kp]), gathered [rows][Kp] for ring_gather_idx as bf16 bit patterns;
    obs_store [T][N][no], priv_store [T][N][npv] fp32"""
    c = d["case"]
    m = ring_model(d)
    r_nan, step_nan, gather_nan = ring_nan_masks(d)
    idx = ring_gather_idx(c)
    checks = dict(ring=bf16_compare(got["ring"], m["ring"], r_nan), gathered=bf16_compare(got["gathered"], m["gather"](idx), gather_nan(idx)))
    for s in range(c.T):
        checks[f"X{s}"] = bf16_compare(got["X"][s], m["X"][s], step_nan(s))
    if "obs_store" in got:
        checks["obs_store"] = bit_diff(got["obs_store"], d["stream"][c.H - 1:])
        checks["priv_store"] = bit_diff(got["priv_store"], d["priv"])
    return checks
