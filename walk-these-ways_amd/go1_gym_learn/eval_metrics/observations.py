"""The distribution of what the policy is fed: which input channels leave the range they had under the training preset, which sit at
the observation clip, how much each jitters from step to step, and whether a logged run feeds the policy what the simulator did.

`run_observation_sweep` arms the device-side tables (include/go1obs.h, libgo1obs.so) beside the scalar table over a command grid and
reads them once at the end: per cell and per column of obs_buf (and of privileged_obs_buf) the moments, sixteen bins and two tails over
the channel's range, the steps at the clip and the moments of the step-to-step change.  What is made of them here: the names and kinds
of the columns (`channel_names`, `channel_kinds`: post_observations of csrc/go1_maps.h, switch by switch), the default ranges, the
JSON-able `profile` of a cell or of all cells pooled, the same profile from a (T, C) array such as a robot log's observations
(`profile_from_array`), and `shift` between two profiles: mean shift, standard-deviation ratio, Jensen-Shannon divergence over the
eighteen cells of a histogram, the share of samples in cells the baseline never visited, clip shares and the jitter ratio.

Every fixed span of KIND_SPANS is a placeholder with nothing measured behind it: measure once and hand `ranges_from(result)` to the
next run.  The observation of a reset step is the respawned robot's and is measured; the policy sees the history of observations, of
which this is the newest row; values outside a range go to the tails; `delta` includes the injected noise.
"""
import json
import math

import numpy as np

from . import sweep
from .sweep import clean, number

BINS, CELLS = 16, 18                  # the bins of a channel; below + the bins + above
LEGS = ["FL", "FR", "RL", "RR"]
JOINTS = [f"{leg}_{part}" for leg in LEGS for part in ("hip", "thigh", "calf")]
COMMANDS = ["vx", "vy", "yaw", "body_height", "frequency", "phase", "offset", "bound", "duration", "footswing_height", "pitch", "roll",
            "stance_width", "stance_length", "aux_reward"]                    # behaviour.COMMAND_INDEX's names, and the fifteenth column
# command -> (its limits in cfg.commands, its scale in cfg.obs_scales): commands_scale of the simulator's configuration
COMMAND_LIMITS = dict(vx=("limit_vel_x", "lin_vel"), vy=("limit_vel_y", "lin_vel"), yaw=("limit_vel_yaw", "ang_vel"),
                      body_height=("limit_body_height", "body_height_cmd"), frequency=("limit_gait_frequency", "gait_freq_cmd"),
                      phase=("limit_gait_phase", "gait_phase_cmd"), offset=("limit_gait_offset", "gait_phase_cmd"),
                      bound=("limit_gait_bound", "gait_phase_cmd"), duration=("limit_gait_duration", "gait_phase_cmd"),
                      footswing_height=("limit_footswing_height", "footswing_height_cmd"), pitch=("limit_body_pitch", "body_pitch_cmd"),
                      roll=("limit_body_roll", "body_roll_cmd"), stance_width=("limit_stance_width", "stance_width_cmd"),
                      stance_length=("limit_stance_length", "stance_length_cmd"), aux_reward=("limit_aux_reward_coef", "aux_reward_cmd"))
# kind -> (lo, hi) in physical units and the cfg.obs_scales entry that turns them into observation units (None: none).  PLACEHOLDERS:
# nothing is measured behind any of these spans
KIND_SPANS = dict(lin_vel=((-2.0, 2.0), "lin_vel"), ang_vel=((-4.0, 4.0), "ang_vel"), dof_pos=((-1.5, 1.5), "dof_pos"), dof_vel=((-30.0, 30.0), "dof_vel"),
                  timing=((0.0, 1.0), None), yaw=((-math.pi, math.pi), None), height=((-1.0, 1.0), "height_measurements"), command=((-1.0, 1.0), None),
                  privileged=((-1.0, 1.0), None))
MIN_WIDTH = 1e-3                      # a configured command range narrower than this says nothing about where the bins should lie
TOP = 10                              # the channels listed per cell under the table
SHIFT_KEYS = ["mean_shift", "std_ratio", "js", "novel", "clip_share_a", "clip_share_b", "jitter_ratio"]


# ---- the channels ----------------------------------------------------------------------------------------------------------------------
def _columns(cfg, privileged):
    """[(name, kind)]: post_observations' running column, switch by switch, then the privileged columns"""
    env, out = cfg.env, []
    axes = "xyz"
    if env.observe_only_lin_vel:
        out += [(f"lin_vel_{a}", "lin_vel") for a in axes]
    if env.observe_only_ang_vel:
        out += [(f"ang_vel_{a}", "ang_vel") for a in axes]
    if env.observe_vel:
        out += [(f"lin_vel_{a}", "lin_vel") for a in axes] + [(f"ang_vel_{a}", "ang_vel") for a in axes]
    out += [(f"gravity_{a}", "gravity") for a in axes]
    if env.observe_command:
        n = int(cfg.commands.num_commands)
        out += [(f"cmd_{COMMANDS[k]}" if k < len(COMMANDS) else f"cmd_{k}", "command") for k in range(n)]
    out += [(f"dof_pos_{j}", "dof_pos") for j in JOINTS] + [(f"dof_vel_{j}", "dof_vel") for j in JOINTS] + [(f"action_{j}", "action") for j in JOINTS]
    if env.observe_two_prev_actions:
        out += [(f"last_action_{j}", "last_action") for j in JOINTS]
    if env.observe_timing_parameter:
        out.append(("timing", "timing"))
    if env.observe_clock_inputs:
        out += [(f"clock_{leg}", "clock") for leg in LEGS]
    if env.observe_yaw:
        out.append(("yaw", "yaw"))
    if env.observe_contact_states:
        out += [(f"contact_{leg}", "contact") for leg in LEGS]
    if getattr(env, "observe_heights", False) and cfg.terrain.measure_heights:
        points = len(cfg.terrain.measured_points_x) * len(cfg.terrain.measured_points_y)
        out += [(f"height_{k}", "height") for k in range(points)]
    if privileged:
        out += [(f"priv_{k}", "privileged") for k in range(int(env.num_privileged_obs))]
    return out


def channel_names(cfg, privileged=False):
    """one name per column of obs_buf for the configuration `cfg` (lin_vel_x, gravity_z, cmd_vx, dof_pos_FL_hip, action_RR_calf, clock_FL,
    ...), with `privileged` followed by priv_0 ... for the columns of privileged_obs_buf"""
    return [name for name, _ in _columns(cfg, privileged)]


def channel_kinds(cfg, privileged=False):
    """the kind of every channel of channel_names(): lin_vel, ang_vel, gravity, command, dof_pos, dof_vel, action, last_action, timing,
    clock, yaw, contact, height or privileged"""
    return [kind for _, kind in _columns(cfg, privileged)]


def kind_of(name):
    """the kind of a channel by its name"""
    for prefix, kind in (("lin_vel_", "lin_vel"), ("ang_vel_", "ang_vel"), ("gravity_", "gravity"), ("cmd_", "command"), ("dof_pos_", "dof_pos"),
                         ("dof_vel_", "dof_vel"), ("last_action_", "last_action"), ("action_", "action"), ("clock_", "clock"), ("contact_", "contact"),
                         ("height_", "height"), ("priv_", "privileged")):
        if name.startswith(prefix):
            return kind
    return name if name in ("timing", "yaw") else "other"


def default_ranges(cfg, privileged=True):
    """{channel name: (lo, hi)} in observation units, one rule per kind: gravity and clock +-1, contact [0, 1], actions +- clip_actions,
    commands the configuration's limits times commands_scale where it has them (and they have a width), everything else the fixed spans
    of KIND_SPANS times the configuration's observation scale.  Every fixed span is a PLACEHOLDER with nothing measured behind it."""
    out = {}
    clip_actions = float(cfg.normalization.clip_actions)
    for name, kind in _columns(cfg, privileged):
        if kind in ("gravity", "clock"):
            span = (-1.0, 1.0)
        elif kind == "contact":
            span = (0.0, 1.0)
        elif kind in ("action", "last_action"):
            span = (-clip_actions, clip_actions)
        else:
            span, scale = None, 1.0
            if kind == "command" and name[4:] in COMMAND_LIMITS:
                limits, unit = COMMAND_LIMITS[name[4:]]
                scale = float(getattr(cfg.obs_scales, unit, 1.0))
                lo, hi = sorted(float(x) for x in getattr(cfg.commands, limits, (0.0, 0.0)))
                if math.isfinite(lo) and math.isfinite(hi) and (hi - lo) * scale >= MIN_WIDTH:
                    span = (lo * scale, hi * scale)
                    scale = 1.0
            if span is None:
                (lo, hi), unit = KIND_SPANS[kind]
                scale = scale if kind == "command" else (float(getattr(cfg.obs_scales, unit)) if unit else 1.0)
                span = (lo * scale, hi * scale)
        out[name] = span
    return out


def channel_spans(cfg, names, kinds, ranges=None):
    """[(lo, hi)] for the channels `names` of `kinds`: default_ranges(cfg), replaced by the entries of `ranges` = {channel name or kind:
    (lo, hi)} (a name wins over its kind); ValueError for a key that is neither a channel nor a kind of the configuration (a privileged
    channel's entry is passed over when the privileged columns are left out: an earlier read's ranges fit either way)"""
    ranges = dict(ranges or {})
    defaults = default_ranges(cfg, privileged=True)
    unknown = [key for key in ranges if key not in defaults and key not in kinds and key != "privileged"]
    if unknown:
        raise ValueError(f"observations: {unknown[0]!r} is neither a channel nor a kind of this configuration")
    return [tuple(float(x) for x in ranges.get(name, ranges.get(kind, defaults[name]))) for name, kind in zip(names, kinds)]


def ranges_from(result, margin=0.1):
    """{channel name: (lo, hi)} from an earlier read or sweep result: every channel's minimum and maximum over all groups, widened by
    `margin` of their distance on both sides (a constant channel: by MIN_WIDTH); a channel that measured nothing is left out"""
    value = np.asarray(result["value"], np.float64)
    out = {}
    for c, name in enumerate(result["channels"]):
        seen = value[:, c, 0] > 0
        if seen.any():
            lo, hi = float(value[seen, c, 3].min()), float(value[seen, c, 4].max())
            pad = max(margin * (hi - lo), MIN_WIDTH)
            out[name] = (lo - pad, hi + pad)
    return out


# ---- profiles ----------------------------------------------------------------------------------------------------------------------------
def _pooled(rows):
    """(count, mean, std, min, max, nonfinite) per channel of the metric rows (G, C, 6) pooled over G, recombined in fp64"""
    rows = np.asarray(rows, np.float64)
    n = rows[:, :, 0]
    some = n > 0
    mean, std = np.where(some, rows[:, :, 1], 0.0), np.where(some, rows[:, :, 2], 0.0)
    total, S, Q = n.sum(axis=0), (n * mean).sum(axis=0), (n * (std * std + mean * mean)).sum(axis=0)
    with np.errstate(all="ignore"):
        m = np.where(total > 0, S / total, np.nan)
        s = np.where(total > 0, np.sqrt(np.fmax(Q / total - m * m, 0.0)), np.nan)
        low = np.where(total > 0, np.where(some, rows[:, :, 3], np.inf).min(axis=0), np.nan)
        high = np.where(total > 0, np.where(some, rows[:, :, 4], -np.inf).max(axis=0), np.nan)
    return total, m, s, low, high, rows[:, :, 5].sum(axis=0)


def profile(result, group=None):
    """The JSON-able profile of group `group` of a read or a sweep result, or of all groups pooled on the host (None): per channel the
    count, mean, std, min, max and nonfinite of the value, the sixteen bins, below, above and at_clip, and count, mean, std and max of the
    step-to-step change; counts, means and standard deviations recombined in fp64, histograms added."""
    pick = slice(None) if group is None else slice(group, group + 1)
    n, mean, std, low, high, bad = _pooled(np.asarray(result["value"])[pick])
    dn, dmean, dstd, _, dhigh, _ = _pooled(np.asarray(result["delta"])[pick])
    hist = np.asarray(result["hist"], np.float64)[pick].sum(axis=0)
    tails = np.asarray(result["tails"], np.float64)[pick].sum(axis=0)
    groups = np.asarray(result["obs_groups"] if "obs_groups" in result else result["groups"], np.float64)[pick].sum(axis=0)
    return clean(dict(channels=list(result["channels"]), kinds=list(result["kinds"]), edges=np.asarray(result["edges"], np.float64).tolist(),
                      clip=float(result["clip"]), count=n.tolist(), mean=mean.tolist(), std=std.tolist(), min=low.tolist(), max=high.tolist(),
                      nonfinite=bad.tolist(), hist=hist.tolist(), below=tails[:, 0].tolist(), above=tails[:, 1].tolist(), at_clip=tails[:, 2].tolist(),
                      delta_count=dn.tolist(), delta_mean=dmean.tolist(), delta_std=dstd.tolist(), delta_max=dhigh.tolist(),
                      env_steps=float(groups[2]), resets=float(groups[3])))


def profile_from_array(obs, channels, edges, clip, resets=None):
    """The same dictionary as profile() from a (T, C) array of observations in time order, for example the observations of a robot log:
    the rows binned as the kernel bins them (fp32: (v - lo) * (16 / (hi - lo))), moments in fp64; resets: (T,) bool, row t is the first
    of a new episode (no change is taken from row t - 1 to it).  Vectorised numpy on an array the caller has already loaded."""
    v = np.asarray(obs, np.float32)
    edges = np.asarray(edges, np.float64)
    if v.ndim != 2 or v.shape[1] != len(channels) or edges.shape != (len(channels), BINS + 1):
        raise ValueError(f"profile_from_array: {v.shape} observations and {edges.shape} edges for {len(channels)} channels")
    T = v.shape[0]
    reset = np.zeros(T, bool) if resets is None else np.asarray(resets).astype(bool).reshape(T)
    lo, hi = edges[:, 0].astype(np.float32), edges[:, BINS].astype(np.float32)
    scale = np.float32(BINS) / (hi - lo)
    fin = np.isfinite(v)
    with np.errstate(all="ignore"):
        t = (v - lo) * scale
        below, inside = fin & (t < 0), fin & (t >= 0) & (t < BINS)
        above = fin & ~below & ~inside
        at_clip = np.abs(v) >= np.float32(clip)
        which = np.where(inside, t, 0).astype(np.int64)
        hist = np.stack([np.bincount(which[inside[:, c], c], minlength=BINS)[:BINS] for c in range(v.shape[1])]) if v.shape[1] else np.zeros((0, BINS))
        d = np.abs(v[1:] - v[:-1])[~reset[1:]]

    def moments(x):
        ok = np.isfinite(x)
        x64, n = np.where(ok, x, 0).astype(np.float64), ok.sum(axis=0).astype(np.float64)
        with np.errstate(all="ignore"):
            m = np.where(n > 0, x64.sum(axis=0) / n, np.nan)
            s = np.where(n > 0, np.sqrt(np.fmax((x64 * x64).sum(axis=0) / n - m * m, 0.0)), np.nan)
            low = np.where(n > 0, np.where(ok, x, np.inf).min(axis=0, initial=np.inf), np.nan)
            high = np.where(n > 0, np.where(ok, x, -np.inf).max(axis=0, initial=-np.inf), np.nan)
        return n, m, s, low.astype(np.float64), high.astype(np.float64), (~ok).sum(axis=0).astype(np.float64)
    n, mean, std, low, high, bad = moments(v)
    dn, dmean, dstd, _, dhigh, _ = moments(d)
    return clean(dict(channels=list(channels), kinds=[kind_of(name) for name in channels], edges=edges.tolist(), clip=float(clip), count=n.tolist(),
                      mean=mean.tolist(), std=std.tolist(), min=low.tolist(), max=high.tolist(), nonfinite=bad.tolist(), hist=hist.astype(np.float64).tolist(),
                      below=below.sum(axis=0).astype(np.float64).tolist(), above=above.sum(axis=0).astype(np.float64).tolist(),
                      at_clip=at_clip.sum(axis=0).astype(np.float64).tolist(), delta_count=dn.tolist(), delta_mean=dmean.tolist(), delta_std=dstd.tolist(),
                      delta_max=dhigh.tolist(), env_steps=float(T), resets=float(reset.sum())))


def _column(p, key):
    """a profile's per-channel list as an fp64 array, None (a JSON null) as NaN"""
    return np.array([np.nan if x is None else x for x in p[key]], np.float64)


def cells18(p):
    """(C, 18): below, the sixteen bins, above"""
    return np.concatenate([_column(p, "below")[:, None], np.asarray(p["hist"], np.float64).reshape(len(p["channels"]), BINS), _column(p, "above")[:, None]], axis=1)


def shift(a, b):
    """How profile `b` differs from the baseline profile `a`, per channel; ValueError unless channels and edges are equal.
    {"channels", "mean_shift": (mean_b - mean_a) / s_a with s_a = max(std_a, (hi - lo) / 1024), "std_ratio": std_b / s_a, "js": the
    Jensen-Shannon divergence in bits over the eighteen cells (below, the bins, above; 0 log 0 = 0; NaN if either is empty), "novel": the
    share of b's samples in cells where a has none, "clip_share_a", "clip_share_b": at_clip / (count + nonfinite), "jitter_ratio":
    mean delta_b / max(mean delta_a, (hi - lo) / 1024)}: lists, NaN where nothing was measured"""
    if list(a["channels"]) != list(b["channels"]):
        raise ValueError("shift: the two profiles have other channels")
    ea, eb = np.array(a["edges"], np.float64), np.array(b["edges"], np.float64)
    if ea.shape != eb.shape or not np.array_equal(ea, eb):
        raise ValueError("shift: the two profiles have other bin edges; measure the second with the first one's ranges")
    floor = (ea[:, BINS] - ea[:, 0]) / 1024.0
    ha, hb = cells18(a), cells18(b)
    na, nb = ha.sum(axis=1), hb.sum(axis=1)
    with np.errstate(all="ignore"):
        s_a = np.fmax(_column(a, "std"), floor)
        pa, pb = ha / na[:, None], hb / nb[:, None]
        mid = 0.5 * (pa + pb)
        kl = lambda p: np.where(p > 0, p * np.log2(p / mid), 0.0).sum(axis=1)
        js = np.where((na > 0) & (nb > 0), 0.5 * kl(pa) + 0.5 * kl(pb), np.nan)
        novel = np.where((na > 0) & (nb > 0), np.where(ha == 0, hb, 0.0).sum(axis=1) / nb, np.nan)
        share = lambda p: _column(p, "at_clip") / (_column(p, "count") + _column(p, "nonfinite"))
        out = dict(channels=list(a["channels"]), mean_shift=(_column(b, "mean") - _column(a, "mean")) / s_a, std_ratio=_column(b, "std") / s_a, js=js,
                   novel=novel, clip_share_a=share(a), clip_share_b=share(b), jitter_ratio=_column(b, "delta_mean") / np.fmax(_column(a, "delta_mean"), floor))
    return {k: (v if k == "channels" else np.asarray(v, np.float64).tolist()) for k, v in out.items()}


def rank_channels(shift_, key="js"):
    """[(channel, value)] of a shift(), the largest first: js, novel and the clip shares by their value, mean_shift by its magnitude, the
    two ratios by the magnitude of their logarithm; a channel without a value (NaN) comes last, equal values keep the channels' order"""
    if key not in SHIFT_KEYS:
        raise ValueError(f"rank_channels: {key!r} is no key of a shift: one of {SHIFT_KEYS}")

    def size(x):
        if x is None or math.isnan(x):
            return math.nan
        if key.endswith("_ratio"):
            return abs(math.log(x)) if x > 0 else math.inf
        return abs(x)
    rows = [(name, float("nan") if x is None else float(x)) for name, x in zip(shift_["channels"], shift_[key])]
    return sorted(rows, key=lambda row: (math.isnan(size(row[1])), -size(row[1]) if not math.isnan(size(row[1])) else 0.0))


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------------
def load_baseline(against):
    """the JSON `against` names (a path), or `against` itself if it is a dictionary already"""
    if isinstance(against, dict):
        return against
    with open(against) as f:
        return json.load(f)


def baselines(baseline, cells):
    """[the profile every cell is compared with]: the baseline's own profile of that cell when its cell list equals `cells` (an earlier
    run's JSON over the same grid), otherwise its pooled profile (its top level: another grid, or a profile_from_array) for every cell"""
    if baseline is None:
        return None
    if "profiles" in baseline and baseline.get("cells") == sweep.cells_to_json(cells):
        return list(baseline["profiles"])
    return [baseline] * len(cells)


def run_observation_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, against=None, no_privileged=False,
                          ranges=None):
    """One observation table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the
    scalar table armed beside it with the same groups and warm-up.  against: an earlier run's JSON (a path or the dictionary) or a
    profile_from_array's; its edges become this run's ranges, so that the two can be compared.  no_privileged: leave the privileged
    columns out.  ranges: {channel or kind: (lo, hi)}, replacing the defaults (and the baseline's).
    Returns {"preset", "cells", "channels", "kinds", "edges": (C, 17), "clip", "value", "delta": (cells, C, 6), "hist": (cells, C, 16),
    "tails": (cells, C, 3), "obs_groups": (cells, 4), "privileged", "baseline": the loaded JSON or None, "metrics": the scalar table
    {name: (cells, 6)}, "groups": (cells, 5), ...}."""
    baseline = load_baseline(against) if against is not None else None
    start_ranges = {}
    if baseline is not None:
        start_ranges.update({name: (edge[0], edge[-1]) for name, edge in zip(baseline["channels"], baseline["edges"])})
    start_ranges.update(ranges or {})
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    start = dict(ranges=start_ranges or None, privileged=not no_privileged)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_observation_sweep", "observation", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain,
                                                           start_kwargs=start)
    return dict(preset=preset, cells=cells, channels=res["channels"], kinds=res["kinds"], edges=res["edges"], clip=res["clip"], value=res["value"],
                delta=res["delta"], hist=res["hist"], tails=res["tails"], obs_groups=res["groups"], privileged=not no_privileged, baseline=baseline,
                metrics=scalar, groups=groups, num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def cell_shifts(result):
    """[shift(the baseline of cell g, the profile of cell g)] or None without a baseline"""
    base = baselines(result.get("baseline"), result["cells"])
    if base is None:
        return None
    return [shift(base[g], profile(result, g)) for g in range(len(result["cells"]))]


def out_of_range(p):
    """(C,) the share of a profile's finite samples in the two tails, NaN where there is none"""
    total = cells18(p).sum(axis=1)
    with np.errstate(all="ignore"):
        return np.where(total > 0, (_column(p, "below") + _column(p, "above")) / total, np.nan)


def observation_to_json(result):
    """the JSON form of a run_observation_sweep result: the profile of all cells pooled at the top level (so the file is a baseline for
    --against whatever the other run's grid), "profiles": the profile of every cell, and with a baseline "shift": per cell, and
    "ranking": per cell the channels by js (NaN and infinities as null)"""
    out = profile(result)
    out.update({k: result[k] for k in ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "privileged")})
    shifts = cell_shifts(result)
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), group_fields=["envs", "launches", "measured", "resets"],
               obs_groups=np.asarray(result["obs_groups"]).tolist(), profiles=[profile(result, g) for g in range(len(result["cells"]))],
               shift=clean(shifts) if shifts is not None else None,
               ranking=[[[name, clean(x)] for name, x in rank_channels(s)[:TOP]] for s in shifts] if shifts is not None else None)
    return out


def observation_markdown_table(result):
    """one row per cell and channel kind: its channels, the samples, the share of them inside the bins, below, above and at the clip,
    the mean step-to-step change, and with a baseline the largest and the mean js and the largest share of novel samples of the kind's
    channels; below the table per cell the ten highest-ranked channels: by js with a baseline, by the share outside the range without"""
    shifts = cell_shifts(result)
    head = ["vx", "yaw", "gait", "kind", "channels", "samples", "in range", "below", "above", "at clip", "mean delta"]
    head += ["js max [bit]", "js mean [bit]", "novel max"] if shifts is not None else []
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    listing = []
    kinds = list(dict.fromkeys(result["kinds"]))
    for g, (vx, yaw, gait) in enumerate(result["cells"]):
        cell = [f"{vx:g}", f"{yaw:g}", "/".join(f"{x:g}" for x in gait)]
        p = profile(result, g)
        eighteen, at_clip, dmean, dn = cells18(p), _column(p, "at_clip"), _column(p, "delta_mean"), _column(p, "delta_count")
        for kind in kinds:
            pick = np.array([k == kind for k in result["kinds"]])
            total = eighteen[pick].sum()
            samples = _column(p, "count")[pick].sum() + _column(p, "nonfinite")[pick].sum()
            share = lambda x: number(x / total if total > 0 else math.nan, ".3g")
            weight = dn[pick].sum()
            row = cell + [kind, str(int(pick.sum())), f"{samples:.0f}", share(eighteen[pick, 1:BINS + 1].sum()), share(eighteen[pick, 0].sum()),
                          share(eighteen[pick, BINS + 1].sum()), number(at_clip[pick].sum() / samples if samples > 0 else math.nan, ".3g"),
                          number(np.nansum(dmean[pick] * dn[pick]) / weight if weight > 0 else math.nan, ".3g")]
            if shifts is not None:
                js, novel = np.array(shifts[g]["js"], np.float64)[pick], np.array(shifts[g]["novel"], np.float64)[pick]
                some = np.isfinite(js)
                row += [number(js[some].max() if some.any() else math.nan, ".3g"), number(js[some].mean() if some.any() else math.nan, ".3g"),
                        number(np.nanmax(novel) if np.isfinite(novel).any() else math.nan, ".3g")]
            lines.append("| " + " | ".join(row) + " |")
        if shifts is not None:
            top, by = rank_channels(shifts[g])[:TOP], "by js"
        else:
            outside = out_of_range(p)
            order = sorted(range(len(outside)), key=lambda c: (math.isnan(outside[c]), -outside[c] if not math.isnan(outside[c]) else 0.0))[:TOP]
            top, by = [(p["channels"][c], float(outside[c])) for c in order], "by the share outside the range"
        listing.append(f"- vx {cell[0]}, yaw {cell[1]}, gait {cell[2]}: {by}: " + ", ".join(f"{name} ({number(x, '.3g')})" for name, x in top))
    note = "The default ranges are placeholders by kind; a reset step's observation is the respawned robot's and is measured; delta includes the injected noise."
    return "\n".join(lines + ["", note] + listing)


def plot_observations(result, path):
    """The observation figure as a PNG: per cell a heat map of channels x 18 cells (below, the sixteen bins, above) with logarithmic
    counts; with a baseline a bar per channel beside it: the Jensen-Shannon divergence from the baseline in bits."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    from matplotlib.colors import LogNorm
    cells, shifts = result["cells"], cell_shifts(result)
    columns, C = (2 if shifts is not None else 1), len(result["channels"])
    height = max(2.6, 0.085 * C)
    figure, axes = plt.subplots(len(cells), columns, figsize=(4.6 * columns, height * len(cells)), constrained_layout=True, squeeze=False,
                                gridspec_kw=dict(width_ratios=[3, 1][:columns]))
    for g, (vx, yaw, gait) in enumerate(cells):
        counts = cells18(profile(result, g))
        ax = axes[g][0]
        image = ax.imshow(np.where(counts > 0, counts, np.nan), aspect="auto", interpolation="nearest", cmap="viridis",
                          norm=LogNorm(vmin=1.0, vmax=max(float(counts.max()), 10.0)), extent=[-1.5, BINS + 0.5, C - 0.5, -0.5])
        ax.axvline(-0.5, color="w", linewidth=0.6)
        ax.axvline(BINS - 0.5, color="w", linewidth=0.6)
        ax.set_yticks(range(C))
        ax.set_yticklabels(result["channels"], fontsize=3.5)
        ax.set_xticks([-1, 0, BINS - 1, BINS])
        ax.set_xticklabels(["below", "lo", "hi", "above"], fontsize=6)
        ax.set_ylabel(f"vx {vx:g}, yaw {yaw:g}", fontsize=7)
        figure.colorbar(image, ax=ax).ax.tick_params(labelsize=6)
        if shifts is not None:
            bars = axes[g][1]
            bars.barh(range(C), np.nan_to_num(np.array(shifts[g]["js"], np.float64)), color="tab:red")
            bars.set_ylim(C - 0.5, -0.5)
            bars.set_xlim(0.0, 1.0)
            bars.set_yticks([])
            bars.set_xlabel("js from the baseline [bit]", fontsize=6)
            bars.tick_params(labelsize=6)
    figure.suptitle(f"{result['preset']}: samples per channel and cell of its range (log)", fontsize=8)
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
