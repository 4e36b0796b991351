"""Inter-leg coordination: which legs move together, at which phase of FL's stride the other three feet touch down against where the
gait command puts them, which of the named gaits that is, and how the time divides among flight, a diagonal pair, a lateral pair, three
and four feet.

`run_gait_sweep` arms the device-side tables (include/go1gait.h, libgo1gait.so) beside the scalar table over a command grid whose `gait`
axis is what the sweep is for, and reads them once at the end.  The device folds no trigonometric function: the circular mean and the
mean resultant length of a leg's touchdown phase are taken here from its sixteen-bin histogram (the bin centres k / 16 are the angles,
so their resolution is 1/16 cycle), and `classify` names the nearest of `sweep.GAITS`.
"""
import numpy as np

from . import sweep
from .sweep import clean, number

LEGS = ["FR", "RL", "RR"]                                                    # the feet placed within FL's stride
GAIT_METRICS = ["sync_FL_FR", "sync_FL_RL", "sync_FL_RR", "sync_FR_RL", "sync_FR_RR", "sync_RL_RR"] + \
               [f"{kind}_{leg}" for kind in ("phase_err", "phase_abs_err", "touchdowns") for leg in LEGS]
BINS = 16
# support patterns by mask = sum of c_f << f (FL 1, FR 2, RL 4, RR 8)
SUPPORT_SHARES = {"flight": [0], "single": [1, 2, 4, 8], "diagonal": [9, 6], "lateral": [5, 10], "fore_hind": [3, 12], "three": [7, 11, 13, 14],
                  "four": [15]}
# phase_abs_err beyond this mean: the errors pile up near +-0.5, where the wrap makes the mean of phase_err meaningless
WRAP_PILE_UP = 0.25


def commanded_phases(gait):
    """the commanded touchdown phases (FR, RL, RR) within FL's stride of a (phase, offset, bound) triple: frac(clock_FL - clock_f) with the
    simulator's clocks FL = g + phase + offset + bound, FR = g + offset, RL = g + bound, RR = g + phase (include/go1gait.h: a foot whose clock
    is ahead touches down earlier).  For the named gaits every value is 0 or 0.5, where the sign of the difference does not matter."""
    p, o, b = (float(x) for x in gait)
    return tuple(x % 1.0 for x in (p + b, p + o, o + b))


def circular_distance(a, b):
    """the distance of two phases on the circle of circumference 1: in [0, 0.5]"""
    return abs((a - b + 0.5) % 1.0 - 0.5)


def circular_stats(hist):
    """(circular mean in [0, 1), mean resultant length in [0, 1]) of a (16,) touchdown-phase histogram, the bin centres k / 16 as the
    angles; (NaN, NaN) of an empty one.  A resultant length near 1 says the touchdowns fall in one bin, near 0 that they are spread round
    the stride."""
    h = np.asarray(hist, np.float64)
    n = h.sum()
    if not n > 0:
        return float("nan"), float("nan")
    angle = 2.0 * np.pi * np.arange(BINS) / BINS
    c, s = float((h * np.cos(angle)).sum()), float((h * np.sin(angle)).sum())
    length = float(np.hypot(c, s) / n)
    if length < 1e-12:                                                       # spread evenly: no direction
        return float("nan"), 0.0
    return float((np.arctan2(s, c) / (2.0 * np.pi)) % 1.0), length


def classify(phases):
    """(name, distance): the gait of sweep.GAITS whose commanded touchdown phases of (FR, RL, RR) relative to FL lie nearest to `phases`
    by the summed circular distance, and that distance (cycles, at most 1.5).  ("none", NaN) when a leg has no phase: it never touched down
    in a closed stride of FL."""
    phases = [float(x) for x in phases]
    if len(phases) != 3 or not all(np.isfinite(phases)):
        return "none", float("nan")
    best = min(sweep.GAITS, key=lambda name: (sum(circular_distance(a, b) for a, b in zip(phases, commanded_phases(sweep.GAITS[name]))), name))
    return best, float(sum(circular_distance(a, b) for a, b in zip(phases, commanded_phases(sweep.GAITS[best]))))


def gait_name(gait):
    """the name of a (phase, offset, bound) triple in sweep.GAITS, or the triple itself"""
    for name, triple in sweep.GAITS.items():
        if tuple(float(x) for x in triple) == tuple(float(x) for x in gait):
            return name
    return "(" + ", ".join(f"{float(x):g}" for x in gait) + ")"


def run_gait_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, min_stride_steps=1, max_stride_steps=100):
    """One gait table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the scalar
    table armed beside it with the same groups and warm-up.  Returns {"preset", "cells", "gait": {name: (cells, 6)}, "gait_groups":
    (cells, 5) array of envs, steps, resets, strides, strides_dropped, "support_hist": (cells, 16), "phase_hist": (cells, 3, 16),
    "phase_centres": (16,), "support_patterns", "metrics": the scalar table {name: (cells, 6)}, "groups": (cells, 5), "min_stride_steps",
    "max_stride_steps", ...}."""
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_gait_sweep", "gait", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain,
                                                           dict(min_stride_steps=min_stride_steps, max_stride_steps=max_stride_steps))
    return dict(preset=preset, cells=cells, gait=res["metrics"], gait_groups=res["groups"], support_hist=res["support_hist"], phase_hist=res["phase_hist"],
                phase_centres=res["phase_centres"], support_patterns=res["support_patterns"], metrics=scalar, groups=groups,
                min_stride_steps=int(min_stride_steps), max_stride_steps=int(max_stride_steps), num_envs=num_envs, steps=steps, warmup_steps=warmup_steps,
                seed=seed, dt=float(base.dt))


def cell_summary(result, g):
    """what the table, the JSON and the figure say about cell g: {"commanded_gait", "commanded": (3,), "realised": (3,) circular means of
    the histograms, "resultant": (3,), "err": (3,) the figure shown, "err_std": (3,), "err_from_histogram": (3,) bools, "class",
    "class_distance", "sync": {"diagonal", "lateral", "fore_hind"}, "support": {share name: share of the folded steps}, "touchdowns":
    (3,) mean per stride, "strides", "strides_dropped"}.  err is the device's phase_err mean (exact to a policy step in the stride's
    length) unless the leg's phase_abs_err mean is beyond WRAP_PILE_UP: then the errors sit near +-0.5, their signed mean is meaningless,
    and the figure is the histogram's: realised minus commanded, wrapped to [-0.5, 0.5), to 1/16 cycle."""
    t = result["gait"]
    cell = result["cells"][g]
    commanded = commanded_phases(cell[2])
    stats = [circular_stats(result["phase_hist"][g][k]) for k in range(3)]
    realised = [s[0] for s in stats]
    err, err_std, from_hist = [], [], []
    for k, leg in enumerate(LEGS):
        row, spread = np.asarray(t[f"phase_err_{leg}"][g], np.float64), np.asarray(t[f"phase_abs_err_{leg}"][g], np.float64)
        piled = bool(spread[0] > 0 and spread[1] > WRAP_PILE_UP)
        from_hist.append(piled)
        err.append(float((realised[k] - commanded[k] + 0.5) % 1.0 - 0.5) if piled else float(row[1]))
        err_std.append(float("nan") if piled else float(row[2]))
    name, distance = classify(realised)
    mean = lambda *rows: float(np.mean([t[r][g][1] for r in rows]))
    hist = np.asarray(result["support_hist"][g], np.float64)
    total = hist.sum()
    support = {k: float(hist[masks].sum() / total) if total > 0 else float("nan") for k, masks in SUPPORT_SHARES.items()}
    return dict(commanded_gait=gait_name(cell[2]), commanded=list(commanded), realised=realised, resultant=[s[1] for s in stats], err=err, err_std=err_std,
                err_from_histogram=from_hist, **{"class": name}, class_distance=distance,
                sync=dict(diagonal=mean("sync_FL_RR", "sync_FR_RL"), lateral=mean("sync_FL_RL", "sync_FR_RR"), fore_hind=mean("sync_FL_FR", "sync_RL_RR")),
                support=support, touchdowns=[float(t[f"touchdowns_{leg}"][g][1]) for leg in LEGS], strides=float(result["gait_groups"][g][3]),
                strides_dropped=float(result["gait_groups"][g][4]))


def gait_markdown_table(result):
    """one row per cell: the commanded gait and the realised class (with its distance), per leg the touchdown phase within FL's stride
    commanded / realised / error (the device's mean +- std, or ~ the histogram's where the errors wrap), the resultant lengths, the
    diagonal, lateral and fore-hind synchrony, the shares of the support patterns, the touchdowns per stride, and the strides closed
    and dropped"""
    head = ["vx", "yaw", "commanded", "realised", "distance"] + [f"{leg} cmd / real / err" for leg in LEGS] + \
           ["resultant FR / RL / RR", "sync diagonal", "sync lateral", "sync fore-hind"] + list(SUPPORT_SHARES) + ["touchdowns FR / RL / RR", "strides", "dropped"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, cell in enumerate(result["cells"]):
        s = cell_summary(result, g)
        row = [f"{cell[0]:g}", f"{cell[1]:g}", s["commanded_gait"], s["class"], number(s["class_distance"], ".3f")]
        for k in range(3):
            shown = ("~" + number(s["err"][k], "+.3f")) if s["err_from_histogram"][k] else (number(s["err"][k], "+.3f") + " ± " + number(s["err_std"][k], ".3f"))
            row.append(f"{s['commanded'][k]:.3f} / {number(s['realised'][k], '.3f')} / {shown}")
        row.append(" / ".join(number(x, ".2f") for x in s["resultant"]))
        row += [number(s["sync"][k], ".3f") for k in ("diagonal", "lateral", "fore_hind")]
        row += [number(s["support"][k], ".3f") for k in SUPPORT_SHARES]
        row += [" / ".join(number(x, ".2f") for x in s["touchdowns"]), f"{s['strides']:.0f}", f"{s['strides_dropped']:.0f}"]
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def gait_to_json(result):
    """the JSON form of a run_gait_sweep result (NaN and infinities as null)"""
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "min_stride_steps", "max_stride_steps")
    out = {k: result[k] for k in keep}
    out.update(cells=sweep.cells_to_json(result["cells"], gait_name=[gait_name(c[2]) for c in result["cells"]]),
               fields=list(sweep.FIELDS), group_fields=["envs", "steps", "resets", "strides", "strides_dropped"],
               gait={m: clean(np.asarray(t).tolist()) for m, t in result["gait"].items()}, gait_groups=np.asarray(result["gait_groups"]).tolist(),
               support_hist=np.asarray(result["support_hist"]).tolist(), phase_hist=np.asarray(result["phase_hist"]).tolist(),
               phase_centres=np.asarray(result["phase_centres"]).tolist(), support_patterns=list(result["support_patterns"]), legs=list(LEGS),
               summary=[clean(cell_summary(result, g)) for g in range(len(result["cells"]))])
    return out


def plot_gait(result, path):
    """The coordination figure as a PNG: per cell a polar panel (one turn = one stride of FL, FL's touchdown at the top) with the three
    touchdown-phase histograms as rings of bars and the commanded phases as radial lines, and beside it the shares of the sixteen
    support patterns as bars."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    cells = result["cells"]
    colours = ["tab:blue", "tab:orange", "tab:green"]
    figure = plt.figure(figsize=(9, 3.6 * len(cells)), constrained_layout=True)
    angle = 2.0 * np.pi * np.asarray(result["phase_centres"], np.float64)
    for g, cell in enumerate(cells):
        s = cell_summary(result, g)
        polar = figure.add_subplot(len(cells), 2, 2 * g + 1, projection="polar")
        polar.set_theta_zero_location("N")
        polar.set_theta_direction(-1)
        for k, leg in enumerate(LEGS):
            h = np.asarray(result["phase_hist"][g][k], np.float64)
            share = h / h.sum() if h.sum() > 0 else h
            polar.bar(angle, 0.9 * share, width=2.0 * np.pi / BINS, bottom=1.0 + k, color=colours[k], alpha=0.8, label=leg)
            polar.plot([2.0 * np.pi * s["commanded"][k]] * 2, [1.0 + k, 1.9 + k], color="black", linewidth=2.0)
        polar.set_yticks([])
        polar.set_ylim(0.0, 4.0)
        polar.set_xticks(2.0 * np.pi * np.arange(8) / 8)
        polar.set_xticklabels([f"{k / 8:g}" for k in range(8)])
        polar.set_title(f"vx {cell[0]:g} m/s, {s['commanded_gait']} -> {s['class']}", fontsize=9)
        if g == 0:
            polar.legend(loc="lower left", bbox_to_anchor=(-0.25, -0.1), fontsize=7, title="touchdown phase in FL's stride; black: commanded", title_fontsize=6)
        bars = figure.add_subplot(len(cells), 2, 2 * g + 2)
        hist = np.asarray(result["support_hist"][g], np.float64)
        bars.bar(np.arange(BINS), hist / hist.sum() if hist.sum() > 0 else hist, color="tab:gray", edgecolor="black", linewidth=0.3)
        bars.set_xticks(np.arange(BINS))
        bars.set_xticklabels(result["support_patterns"], rotation=90, fontsize=6)
        bars.set(ylabel="share of steps", ylim=(0.0, 1.0), title="feet on the ground")
        bars.grid(True, axis="y", linewidth=0.3)
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
