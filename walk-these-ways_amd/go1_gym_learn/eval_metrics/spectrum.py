"""Spectra: where in frequency a policy's actions, torques, joint speeds and trunk rates carry their energy: whether it chatters, how
much sits above what the actuators can follow, and whether the motion is locked to the commanded step frequency.

`run_spectrum_sweep` arms the device-side tables (include/go1spectrum.h, libgo1spectrum.so) beside the scalar table over the velocity
grid and reads them once at the end.  The device keeps, per group and signal, the mean power spectral density over the closed segments
and five band figures per segment; the table, the JSON and the figure average the four legs' joints of one type on the host and read
the dominant frequency, the shares and `gait_locked` off the mean density.
"""
import numpy as np

from . import sweep
from .behaviour import COMMAND_INDEX
from .sweep import clean, number

SPECTRUM_ROWS = ["power", "peak_freq", "peak_share", "high_share", "centroid"]
QUANTITIES = ["action", "torque", "dof_vel"]                                  # signals 0..11, 12..23, 24..35; joint j of leg j // 3
QUANTITY_LABELS = {"action": "action", "torque": "torque", "dof_vel": "joint speed"}
JOINT_TYPES = ["hip", "thigh", "calf"]                                        # joint j is JOINT_TYPES[j % 3]
TRUNK_SIGNALS = ["roll_rate", "pitch_rate", "yaw_rate", "vertical_vel"]       # signals 36..39
NUM_SIGNALS = 40


def row_signals():
    """[(quantity, part, [signal indices])]: per quantity and joint type the four legs' signals, then the four trunk signals"""
    rows = [(q, part, [12 * i + 3 * leg + p for leg in range(4)]) for i, q in enumerate(QUANTITIES) for p, part in enumerate(JOINT_TYPES)]
    return rows + [("trunk", name, [36 + i]) for i, name in enumerate(TRUNK_SIGNALS)]


def harmonic_bins(freq, f_cmd):
    """the bins k >= 1 within one bin of a harmonic h * f_cmd <= fs / 2 (freq[-1]) of the commanded step frequency, ascending; none
    for a frequency that is not positive"""
    freq = np.asarray(freq, np.float64)
    F, width = len(freq), float(freq[1] - freq[0])
    bins = set()
    if np.isfinite(f_cmd) and f_cmd > 0:
        h = 1
        while h * f_cmd <= freq[-1] * (1.0 + 1e-9):
            k = int(round(h * f_cmd / width))
            bins.update(j for j in (k - 1, k, k + 1) if 1 <= j <= F - 1)
            h += 1
    return sorted(bins)


def gait_locked(psd, freq, f_cmd):
    """the share of sum over k >= 1 of the density `psd` (F,) that lies within one bin of the harmonics of f_cmd; NaN without power"""
    psd = np.asarray(psd, np.float64)
    total = psd[1:].sum()
    if not (np.isfinite(total) and total > 0):
        return float("nan")
    return float(psd[harmonic_bins(freq, f_cmd)].sum() / total)


def density_figures(psd, freq, high_bin, f_cmd):
    """what a table row reads off a mean density (F,): {"peak_freq", "peak_share", "high_share", "centroid", "gait_locked"}; NaN without
    power.  The same definitions as the device's per-segment rows, applied to the mean density in fp64."""
    psd, freq = np.asarray(psd, np.float64), np.asarray(freq, np.float64)
    total = psd[1:].sum()
    if not (np.isfinite(total) and total > 0):
        return dict(peak_freq=float("nan"), peak_share=float("nan"), high_share=float("nan"), centroid=float("nan"), gait_locked=float("nan"))
    kp = 1 + int(np.argmax(psd[1:]))
    return dict(peak_freq=float(freq[kp]), peak_share=float(psd[kp] / total), high_share=float(psd[high_bin:].sum() / total),
                centroid=float((freq[1:] * psd[1:]).sum() / total), gait_locked=gait_locked(psd, freq, f_cmd))


def run_spectrum_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, segment_steps=100, high_freq=10.0,
                       taper="hann"):
    """One spectral table for one preset over the velocity grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the
    scalar table armed beside it with the same groups and warm-up.  Returns {"preset", "cells", "step_freq": the commanded step
    frequency of every cell (Hz), "spectrum": {row: (cells, 40, 6)}, "spectrum_groups": (cells, 5) array of envs, steps, resets, segments,
    segments_dropped, "psd": (cells, 40, F) mean density, "psd_segments": (cells, 40), "freq": (F,), "signals", "high_bin", "metrics": the
    scalar table {name: (cells, 6)}, "groups": (cells, 5), "segment_steps", "high_freq", "taper", ...}."""
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_spectrum_sweep", "spectrum", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain,
                                                           dict(segment_steps=segment_steps, high_freq=high_freq, taper=taper))
    step_freq = [float(x) for x in sweep.command_table(cells, base.commands.shape[1], "cpu")[:, COMMAND_INDEX["frequency"]]]
    return dict(preset=preset, cells=cells, step_freq=step_freq, spectrum=res["metrics"], spectrum_groups=res["groups"], psd=res["psd"],
                psd_segments=res["psd_segments"], freq=res["freq"], signals=res["signals"], high_bin=int(res["high_bin"]), metrics=scalar, groups=groups,
                segment_steps=int(segment_steps), high_freq=float(high_freq), taper=taper, num_envs=num_envs, steps=steps, warmup_steps=warmup_steps,
                seed=seed, dt=float(base.dt))


def cell_summary(result, g):
    """the table rows of cell g: [{"quantity", "part", "rms": sqrt of the mean power of the row's signals, "mean_psd": (F,) the mean of
    their mean densities, "peak_freq", "peak_share", "high_share", "centroid", "gait_locked": read off mean_psd}, ...] in row_signals()'s
    order.  A signal without a folded segment leaves its row's figures NaN."""
    out = []
    freq = np.asarray(result["freq"], np.float64)
    for quantity, part, signals in row_signals():
        power = np.array([result["spectrum"]["power"][g][s][1] for s in signals], np.float64)
        psd = np.asarray(result["psd"], np.float64)[g, signals].mean(axis=0)
        row = dict(quantity=quantity, part=part, rms=float(np.sqrt(power.mean())), mean_psd=psd.tolist())
        row.update(density_figures(psd, freq, result["high_bin"], result["step_freq"][g]))
        out.append(row)
    return out


def spectrum_markdown_table(result):
    """per cell one row per quantity and joint type (the four legs averaged) and four trunk rows: the rms, the dominant frequency of the
    mean density, its share, the share at and above high_freq, the centroid, and the share locked to the commanded step frequency's
    harmonics"""
    head = ["vx", "yaw", "step Hz", "quantity", "part", "rms", "peak Hz", "peak share", f"share >= {result['high_freq']:g} Hz", "centroid Hz", "gait_locked",
            "segments", "dropped"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, cell in enumerate(result["cells"]):
        for row in cell_summary(result, g):
            lines.append("| " + " | ".join([f"{cell[0]:g}", f"{cell[1]:g}", f"{result['step_freq'][g]:g}", QUANTITY_LABELS.get(row["quantity"], row["quantity"]),
                                            row["part"], number(row["rms"], ".4g"), number(row["peak_freq"], ".2f"), number(row["peak_share"], ".3f"),
                                            number(row["high_share"], ".3f"), number(row["centroid"], ".2f"), number(row["gait_locked"], ".3f"),
                                            f"{result['spectrum_groups'][g][3]:.0f}", f"{result['spectrum_groups'][g][4]:.0f}"]) + " |")
    return "\n".join(lines)


def spectrum_to_json(result):
    """the JSON form of a run_spectrum_sweep result (NaN and infinities as null)"""
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "segment_steps", "high_freq", "high_bin", "taper")
    out = {k: result[k] for k in keep}
    out.update(cells=sweep.cells_to_json(result["cells"], step_freq=result["step_freq"]), fields=list(sweep.FIELDS), group_fields=["envs", "steps", "resets", "segments", "segments_dropped"],
               signals=list(result["signals"]), freq=np.asarray(result["freq"], np.float64).tolist(),
               spectrum={m: clean(np.asarray(t).tolist()) for m, t in result["spectrum"].items()},
               spectrum_groups=np.asarray(result["spectrum_groups"]).tolist(), psd=clean(np.asarray(result["psd"]).tolist()),
               psd_segments=np.asarray(result["psd_segments"]).tolist(),
               summary=[clean(cell_summary(result, g)) for g in range(len(result["cells"]))])
    return out


def plot_spectrum(result, path):
    """The spectra as a PNG: one panel per cell and quantity (action, torque, joint speed, trunk), the mean density over frequency on a
    logarithmic axis, one line per joint type (or trunk signal), the harmonics of the commanded step frequency as dotted lines and
    high_freq as a dashed one."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    cells = result["cells"]
    freq = np.asarray(result["freq"], np.float64)
    columns = QUANTITIES + ["trunk"]
    figure, axes = plt.subplots(len(cells), len(columns), figsize=(3.6 * len(columns), 2.8 * len(cells)), squeeze=False, constrained_layout=True)
    for g, cell in enumerate(cells):
        rows = cell_summary(result, g)
        for c, quantity in enumerate(columns):
            ax = axes[g][c]
            drawn = False
            for row in rows:
                if row["quantity"] != quantity:
                    continue
                psd = np.asarray(row["mean_psd"], np.float64)[1:]
                ax.plot(freq[1:], np.where(psd > 0, psd, np.nan), label=row["part"], linewidth=1.0)
                drawn = drawn or bool((psd > 0).any())
            f_cmd, h = result["step_freq"][g], 1
            while f_cmd > 0 and h * f_cmd <= freq[-1]:
                ax.axvline(h * f_cmd, color="gray", linestyle=":", linewidth=0.6)
                h += 1
            ax.axvline(result["high_freq"], color="black", linestyle="--", linewidth=0.8)
            if drawn:                                                       # (a panel without power, a trunk at rest, has no logarithmic axis)
                ax.set_yscale("log")
            ax.set_title(f"vx {cell[0]:g} m/s: {QUANTITY_LABELS.get(quantity, quantity)}", fontsize=8)
            ax.set_xlabel("Hz", fontsize=7)
            ax.tick_params(labelsize=6)
            ax.grid(True, linewidth=0.3)
            if g == 0:
                ax.legend(fontsize=6)
            if c == 0:
                ax.set_ylabel("units² / Hz", fontsize=7)
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
