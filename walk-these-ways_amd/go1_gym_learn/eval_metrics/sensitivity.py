"""Robustness against the randomised dynamics: at which friction a policy starts to fall, what a payload costs in tracking accuracy,
whether weak motors or a shifted centre of mass matter more.

`run_sensitivity_sweep` arms the device-side tables (include/go1sens.h, libgo1sens.so) beside the scalar table over a command grid and
reads them once at the end: per cell and per dynamics parameter sixteen bins of its value, each with the steps spent there, the falls
and time-outs charged to the value that was in force, and the sums of the reward, the two tracking errors and the power.  What is made
of them here: the hazard (falls per 1000 steps) with its Wilson interval, the means per bin, the effect of a parameter (the spread of a
curve over the bins with enough exposure) and the ranking of the parameters by it.

The curves are marginal: inside one bin of a parameter the others vary freely; only the one pair map shows an interaction.
`min_exposure` (200 steps) is a placeholder with nothing measured behind it.
"""
import math

import numpy as np

from . import sweep
from .sweep import clean, number

PARAMETERS = ["friction", "restitution", "payload", "com_x", "com_y", "com_z", "motor_strength", "Kp_factor", "Kd_factor"]
QUANTITIES = ["steps", "measured", "falls", "timeouts", "reward_sum", "lin_err_sum", "yaw_err_sum", "power_sum"]
COUNTS = ["unbinned", "redraws", "bad"]
PAIR_QUANTITIES = ["steps", "falls", "measured", "lin_err_sum"]
BINS, QUARTER = 16, 4
MIN_EXPOSURE = 200                    # steps a bin needs before it enters an effect: a placeholder, nothing is measured behind it


def hazard(falls, steps, per=1000):
    """falls per `per` steps of exposure, elementwise; NaN without exposure"""
    falls, steps = np.asarray(falls, np.float64), np.asarray(steps, np.float64)
    with np.errstate(all="ignore"):
        return np.where(steps > 0, falls / steps * per, np.nan)


def wilson(falls, steps, z=1.96):
    """(lower, upper): the Wilson score interval of the share falls / steps, elementwise; NaN without exposure"""
    falls, steps = np.asarray(falls, np.float64), np.asarray(steps, np.float64)
    with np.errstate(all="ignore"):
        share = falls / steps
        centre = (share + z * z / (2.0 * steps)) / (1.0 + z * z / steps)
        half = z * np.sqrt(share * (1.0 - share) / steps + z * z / (4.0 * steps * steps)) / (1.0 + z * z / steps)
        return np.where(steps > 0, centre - half, np.nan), np.where(steps > 0, centre + half, np.nan)


def effect(curve, steps, min_exposure=MIN_EXPOSURE):
    """the largest minus the smallest value of `curve` (16,) over the bins with at least `min_exposure` steps and a finite value; NaN
    with fewer than two such bins"""
    curve, steps = np.asarray(curve, np.float64), np.asarray(steps, np.float64)
    kept = curve[(steps >= min_exposure) & np.isfinite(curve)]
    return float(kept.max() - kept.min()) if kept.size >= 2 else float("nan")


def bin_means(result, g, p):
    """the curves of cell g and parameter index p: {"steps", "hazard", "hazard_low", "hazard_high" (the Wilson band, per 1000 steps),
    "reward", "lin_vel_err", "yaw_vel_err", "power"}: (16,) each, the means NaN where nothing was measured"""
    c = {q: np.asarray(result["curves"][q][g][p], np.float64) for q in QUANTITIES}
    low, high = wilson(c["falls"], c["steps"])
    with np.errstate(all="ignore"):
        per_measured = lambda q: np.where(c["measured"] > 0, c[q] / c["measured"], np.nan)
        return dict(steps=c["steps"], hazard=hazard(c["falls"], c["steps"]), hazard_low=low * 1000.0, hazard_high=high * 1000.0,
                    reward=np.where(c["steps"] > 0, c["reward_sum"] / c["steps"], np.nan), lin_vel_err=per_measured("lin_err_sum"),
                    yaw_vel_err=per_measured("yaw_err_sum"), power=per_measured("power_sum"))


def quarters(result, g, p):
    """the lowest and the highest quarter of the bins (four each) of cell g and parameter index p, pooled: {"hazard", "lin_vel_err",
    "power"}: (low, high) each"""
    c = {q: np.asarray(result["curves"][q][g][p], np.float64) for q in QUANTITIES}
    out = {}
    for name, top, bottom, per in (("hazard", "falls", "steps", 1000.0), ("lin_vel_err", "lin_err_sum", "measured", 1.0), ("power", "power_sum", "measured", 1.0)):
        pooled = []
        for part in (slice(0, QUARTER), slice(BINS - QUARTER, BINS)):
            n = c[bottom][part].sum()
            pooled.append(float(c[top][part].sum() / n * per) if n > 0 else float("nan"))
        out[name] = tuple(pooled)
    return out


def reported(result):
    """the indices of the parameters a result reports: the active ones, and of them those the sweep was asked for"""
    wanted = result.get("parameters") or PARAMETERS
    return [p for p, name in enumerate(PARAMETERS) if result["active"][p] and name in wanted]


def parameter_summary(result, g, p):
    """what the table and the JSON say about cell g and parameter index p"""
    m = bin_means(result, g, p)
    q = quarters(result, g, p)
    value = np.asarray(result["value"][PARAMETERS[p]][g], np.float64)
    counts = np.asarray(result["counts"][g][p], np.float64)
    least = result["min_exposure"]
    return dict(parameter=PARAMETERS[p], lo=float(result["edges"][p][0]), hi=float(result["edges"][p][-1]), realised_min=float(value[3]),
                realised_max=float(value[4]), exposure=float(m["steps"].sum()), hazard_low=q["hazard"][0], hazard_high=q["hazard"][1],
                lin_vel_err_low=q["lin_vel_err"][0], lin_vel_err_high=q["lin_vel_err"][1], power_low=q["power"][0], power_high=q["power"][1],
                effect_hazard=effect(m["hazard"], m["steps"], least), effect_lin_vel_err=effect(m["lin_vel_err"], m["steps"], least),
                unbinned=float(counts[0]), redraws=float(counts[1]), bad=float(counts[2]))


def rank_parameters(result, g, by="effect_hazard"):
    """[(name, effect)] of cell g's reported parameters, the largest effect first; a parameter without an effect (NaN) comes last, and
    equal effects keep the order of PARAMETERS"""
    rows = [(PARAMETERS[p], parameter_summary(result, g, p)[by]) for p in reported(result)]
    return sorted(rows, key=lambda row: (math.isnan(row[1]), -row[1] if not math.isnan(row[1]) else 0.0))


def run_sensitivity_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, parameters=None, pair=None,
                          min_exposure=None):
    """One sensitivity table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the
    scalar table armed beside it with the same groups and warm-up.  parameters: the names to report (None: every parameter the preset
    randomises); a name whose randomize_* switch is off is measured over the configuration's range all the same.  pair: two of the
    names for the 8 x 8 map.  min_exposure: the steps a bin needs before it enters an effect (None: MIN_EXPOSURE, a placeholder).
    Returns {"preset", "cells", "parameters", "active": (9,), "edges": (9, 17), "ranges", "value": {name: (cells, 6)}, "curves":
    {quantity: (cells, 9, 16)}, "counts": (cells, 9, 3), "sens_groups": (cells, 2), "pair", "pair_map": (cells, 4, 8, 8) or None,
    "min_exposure", "metrics": the scalar table {name: (cells, 6)}, "groups": (cells, 5), ...}."""
    names = list(parameters) if parameters else None
    for name in list(names or []) + list(pair or []):
        if name not in PARAMETERS:
            raise ValueError(f"run_sensitivity_sweep: {name!r} is no parameter: one of {PARAMETERS}")
    min_exposure = MIN_EXPOSURE if min_exposure is None else int(min_exposure)
    if min_exposure < 1:
        raise ValueError("run_sensitivity_sweep: min_exposure has to be at least 1")
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    start = dict(ranges={name: None for name in list(names or []) + list(pair or [])} or None, pair=tuple(pair) if pair else None)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_sensitivity_sweep", "sensitivity", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain,
                                                           start_kwargs=start)
    return dict(preset=preset, cells=cells, parameters=names or [n for n, on in zip(PARAMETERS, res["active"]) if on], active=res["active"], edges=res["edges"],
                ranges=res["ranges"], value=res["value"], curves=res["curves"], counts=res["counts"], sens_groups=res["groups"], pair=res["pair"],
                pair_map=res["pair_map"], min_exposure=min_exposure, metrics=scalar, groups=groups, num_envs=num_envs, steps=steps,
                warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def sensitivity_markdown_table(result):
    """one row per cell and reported parameter: its range, the realised min / max, the exposure in steps, the hazard (falls per 1000
    steps) in the lowest and the highest quarter of the bins, the mean lin_vel_err and the mean power in both quarters, the effect on the
    hazard and on lin_vel_err, the re-draws and the unbinned steps; below them per cell the ranking of the parameters by their effect"""
    head = ["vx", "yaw", "gait", "parameter", "range", "realised min / max", "exposure", "hazard low / high [1/1000 steps]", "lin vel err low / high",
            "power low / high [W]", "effect on hazard", "effect on lin vel err", "re-draws", "unbinned"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    ranking = []
    for g, (vx, yaw, gait) in enumerate(result["cells"]):
        cell = [f"{vx:g}", f"{yaw:g}", "/".join(f"{x:g}" for x in gait)]
        for p in reported(result):
            s = parameter_summary(result, g, p)
            row = cell + [s["parameter"], f"{s['lo']:g} .. {s['hi']:g}", f"{number(s['realised_min'], '.3g')} / {number(s['realised_max'], '.3g')}",
                          f"{s['exposure']:.0f}", f"{number(s['hazard_low'], '.3g')} / {number(s['hazard_high'], '.3g')}",
                          f"{number(s['lin_vel_err_low'], '.3g')} / {number(s['lin_vel_err_high'], '.3g')}",
                          f"{number(s['power_low'], '.3g')} / {number(s['power_high'], '.3g')}", number(s["effect_hazard"], ".3g"),
                          number(s["effect_lin_vel_err"], ".3g"), f"{s['redraws']:.0f}", f"{s['unbinned']:.0f}"]
            lines.append("| " + " | ".join(row) + " |")
        by_hazard = ", ".join(f"{name} ({number(x, '.3g')})" for name, x in rank_parameters(result, g))
        by_error = ", ".join(f"{name} ({number(x, '.3g')})" for name, x in rank_parameters(result, g, "effect_lin_vel_err"))
        ranking.append(f"- vx {cell[0]}, yaw {cell[1]}, gait {cell[2]}: by effect on the hazard: {by_hazard}; on lin vel err: {by_error}")
    note = f"Effects are taken over the bins with at least {result['min_exposure']} steps (a placeholder); the curves are marginal."
    return "\n".join(lines + ["", note] + ranking)


def sensitivity_to_json(result):
    """the JSON form of a run_sensitivity_sweep result (NaN and infinities as null)"""
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "min_exposure")
    out = {k: result[k] for k in keep}
    shown = reported(result)
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), parameters=list(PARAMETERS), reported=[PARAMETERS[p] for p in shown],
               active=[bool(x) for x in result["active"]], quantities=list(QUANTITIES), count_fields=list(COUNTS), pair_quantities=list(PAIR_QUANTITIES),
               edges=clean(np.asarray(result["edges"]).tolist()), ranges={k: list(v) for k, v in result["ranges"].items()},
               value={m: clean(np.asarray(t).tolist()) for m, t in result["value"].items()},
               curves={q: np.asarray(t).tolist() for q, t in result["curves"].items()}, counts=np.asarray(result["counts"]).tolist(),
               sens_groups=np.asarray(result["sens_groups"]).tolist(), pair=list(result["pair"]) if result["pair"] else None,
               pair_map=np.asarray(result["pair_map"]).tolist() if result["pair_map"] is not None else None,
               summary=[[clean(parameter_summary(result, g, p)) for p in shown] for g in range(len(result["cells"]))],
               ranking=[[[name, clean(x)] for name, x in rank_parameters(result, g)] for g in range(len(result["cells"]))])
    return out


def plot_sensitivity(result, path):
    """The sensitivity figure as a PNG: one panel per cell (row) and reported parameter (column): the hazard per 1000 steps with its
    Wilson band over the parameter's value, the mean lin_vel_err on a second axis, and the exposure as bars behind them; with a pair one
    more column holds the 8 x 8 hazard map."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    shown, cells = reported(result), result["cells"]
    columns = max(1, len(shown) + (1 if result["pair_map"] is not None else 0))
    figure, axes = plt.subplots(len(cells), columns, figsize=(3.2 * columns, 2.6 * len(cells)), constrained_layout=True, squeeze=False)
    for g, (vx, yaw, gait) in enumerate(cells):
        for k, p in enumerate(shown):
            ax = axes[g][k]
            edges = np.asarray(result["edges"][p], np.float64)
            centres, width = 0.5 * (edges[:-1] + edges[1:]), edges[1] - edges[0]
            m = bin_means(result, g, p)
            bars = ax.twinx()
            bars.bar(centres, m["steps"], width=0.9 * width, color="0.85", zorder=0)
            bars.set_yticks([])
            ax.set_zorder(bars.get_zorder() + 1)
            ax.patch.set_visible(False)
            ax.fill_between(centres, m["hazard_low"], m["hazard_high"], color="tab:red", alpha=0.25, linewidth=0)
            ax.plot(centres, m["hazard"], color="tab:red", marker=".", linewidth=1.0)
            ax.set_xlabel(PARAMETERS[p], fontsize=7)
            ax.tick_params(labelsize=6)
            if k == 0:
                ax.set_ylabel(f"vx {vx:g}, yaw {yaw:g}\nfalls / 1000 steps", fontsize=7)
            error = ax.twinx()
            error.plot(centres, m["lin_vel_err"], color="tab:blue", marker=".", linewidth=1.0)
            error.tick_params(labelsize=6, colors="tab:blue")
        if result["pair_map"] is not None:
            ax = axes[g][len(shown)]
            steps, falls = np.asarray(result["pair_map"][g][0], np.float64), np.asarray(result["pair_map"][g][1], np.float64)
            a, b = (PARAMETERS.index(name) for name in result["pair"])
            extent = [result["edges"][b][0], result["edges"][b][-1], result["edges"][a][0], result["edges"][a][-1]]
            image = ax.imshow(hazard(falls, steps), origin="lower", aspect="auto", extent=extent, cmap="magma")
            ax.set_xlabel(result["pair"][1], fontsize=7)
            ax.set_ylabel(result["pair"][0], fontsize=7)
            ax.tick_params(labelsize=6)
            figure.colorbar(image, ax=ax).ax.tick_params(labelsize=6)
        for k in range(len(shown) + (1 if result["pair_map"] is not None else 0), columns):
            axes[g][k].set_axis_off()
    figure.suptitle(f"{result['preset']}: hazard (red, Wilson band), lin vel err (blue), exposure (bars) over the dynamics parameters", fontsize=8)
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
