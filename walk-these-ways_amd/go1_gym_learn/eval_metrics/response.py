"""Command step responses: how fast does a policy reach a command that changes at run time, does it overshoot, does it settle,
does it fall in the attempt?

`run_response_sweep` holds one command value for every environment, switches environment i to `to_values[i % cells]`, and
records the trace of libgo1eval (include/go1eval.h, third kernel family) around the switch: one more launch per step, no host
read in the step loop.  The analysis (rise time, overshoot, settling time, steady-state error, integrated error per
environment, reduced per cell) runs on the device as well; the host reads one small table.  `plot_trace` draws what the
reference's scripts/play.py shows after its 250 host reads, for any traced environment.
"""
import numpy as np
import torch

from . import behaviour, sweep

# name -> (y_channel, r_channel or None[, fixed_target, fixed_scale]); channel numbers of include/go1eval.h `enum Go1TraceChannel`
RESPONSE_SIGNALS = {"lin_vel_x": (0, 6), "lin_vel_y": (1, 7), "ang_vel_yaw": (2, 8), "base_height": (3, 9),
                    "contact_match": (4, None, 1.0, 1.0)}
# the signal a command drives; a switch of any other command (step frequency, gait, ...) shows in contact_match only
DRIVEN_SIGNAL = dict(vx="lin_vel_x", vy="lin_vel_y", yaw="ang_vel_yaw", body_height="base_height")
COMMAND_OF_SIGNAL = {signal: command for command, signal in DRIVEN_SIGNAL.items()}        # a driven signal's name also names its command
BASE_CELL = (1.0, 0.0, sweep.GAITS["trotting"])          # what every other command holds: behaviour.behaviour_command_table's trot at 1 m/s


def switch_commands(command, values, num_commands, device):
    """(len(values), num_commands) commands: `command` (a name of behaviour.COMMAND_INDEX, or "gait" with names of sweep.GAITS) at
    each of `values`, every other command as sweep.command_table holds it for BASE_CELL"""
    if command == "gait":
        return sweep.command_table([(BASE_CELL[0], BASE_CELL[1], sweep.GAITS[v]) for v in values], num_commands, device)
    command = COMMAND_OF_SIGNAL.get(command, command)
    if command not in behaviour.COMMAND_INDEX:
        raise KeyError(f"switch_commands: unknown command {command!r}; \"gait\" or one of {sorted(behaviour.COMMAND_INDEX)}")
    return behaviour.behaviour_command_table([{command: float(v)} for v in values], num_commands, device, BASE_CELL)


def default_signals(command):
    command = COMMAND_OF_SIGNAL.get(command, command)
    return ([DRIVEN_SIGNAL[command]] if command in DRIVEN_SIGNAL else []) + ["contact_match"]


def stride_rows(commands, dt):
    """rows of one stride at the lowest commanded step frequency (command 4): 17 at 3 Hz and dt = 0.02 s"""
    return int(round(1.0 / (float(commands[:, 4].min()) * dt)))


def run_response_sweep(policy, preset, command, from_value, to_values, signals=None, num_envs=4096, settle_steps=100, pre=25, window=150,
                       smooth=None, band=0.1, hold=10, tail=25, seed=1, terrain=None, trace_envs=None):
    """One response table for one preset: every environment holds `command` = from_value for settle_steps + pre steps, then
    environment i holds to_values[i % cells] for `window` steps; the trace covers the last pre + window steps and is analysed
    with switch_row = pre.  smooth=None: one stride (stride_rows).  Returns {"preset", "command", "from_value", "cells":
    to_values, "signals": [names], "response": {signal: {metric: (cells, 6)}}, "groups": (cells, 4) array of envs, ok, reset,
    not held, "values", "status", ...}; with trace_envs also "trace": read_trace() restricted to those environments."""
    to_values = list(to_values)
    names = list(signals) if signals is not None else default_signals(command)
    env, _ = sweep.build_eval_env(preset, num_envs, seed, terrain)
    if hasattr(policy, "eval"):
        policy.eval()
    base = env.env
    env.reset()
    group = torch.arange(base.num_envs, device=base.device) % len(to_values)
    num_commands = base.commands.shape[1]
    before = switch_commands(command, [from_value], num_commands, base.device).repeat(base.num_envs, 1)
    after = switch_commands(command, to_values, num_commands, base.device)[group]
    w = stride_rows(torch.cat([before[:1], after[:len(to_values)]]), base.dt) if smooth is None else int(smooth)
    if not 1 <= w <= pre + 1:
        raise ValueError(f"run_response_sweep: the filter of {w} rows needs pre >= {w - 1}")
    base.commands[:] = before
    obs = env.get_observations()
    obs = sweep.rollout(env, policy, obs, settle_steps, before)
    base.start_trace(capacity=pre + window)
    obs = sweep.rollout(env, policy, obs, pre, before)
    sweep.rollout(env, policy, obs, window, after)
    base.stop_trace()
    if not sweep.commands_held(env, after):
        raise RuntimeError("run_response_sweep: an environment left its cell's commands during the rollout")
    res = base.trace_response({n: RESPONSE_SIGNALS[n] for n in names}, switch_row=pre, pre=pre, smooth=w, band=band, hold=hold, tail=tail,
                              groups=group.to(torch.int32))
    out = dict(preset=preset, command=command, from_value=from_value, cells=to_values, signals=names, response={n: res[n] for n in names},
               groups=res["groups"], values=res["values"], status=res["status"], num_envs=num_envs, settle_steps=settle_steps, pre=pre,
               window=window, smooth=w, band=band, hold=hold, tail=tail, dt=float(base.dt), seed=seed)
    if trace_envs is not None:
        out["trace"] = select_envs(base.read_trace(), trace_envs)
    return out


def select_envs(trace, envs):
    """the columns of a read_trace() result that belong to the environments `envs`"""
    ids = list(trace["env_ids"])
    cols = [ids.index(int(e)) for e in envs]
    out = {k: (v[:, cols] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in trace.items()}
    out["env_ids"] = np.asarray([int(e) for e in envs], np.int32)
    return out


def response_markdown_table(result, signal=None):
    """one row per cell for one signal (default: the first): ok / fell / not held, the reached and settled fractions of the
    environments with status 0, then mean +- std of rise time, settling time, overshoot and steady-state error"""
    signal = signal or result["signals"][0]
    r = result["response"][signal]
    head = [result["command"], "signal", "ok / fell / not held", "reached", "settled", "rise time [s]", "settling time [s]", "overshoot",
            "steady-state err"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, value in enumerate(result["cells"]):
        ok, fell, moved = (int(x) for x in result["groups"][g, 1:4])
        row = [f"{result['from_value']} → {value}", signal, f"{ok} / {fell} / {moved}"]
        row += [f"{r[m][g, 1]:.3f}" if r[m][g, 0] > 0 else "–" for m in ("reached", "settled")]
        row += [sweep.mean_std(r[m][g]) for m in ("rise_time", "settling_time", "overshoot", "steady_state_err")]
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def response_to_json(result):
    """the JSON form of a run_response_sweep result (without the per-environment values and the trace)"""
    keep = ("preset", "command", "from_value", "cells", "signals", "num_envs", "settle_steps", "pre", "window", "smooth", "band", "hold",
            "tail", "dt", "seed")
    out = {k: result[k] for k in keep}
    out.update(fields=list(sweep.FIELDS), group_fields=["envs", "ok", "reset", "not_held"],
               response={s: {m: t.tolist() for m, t in metrics.items()} for s, metrics in result["response"].items()},
               groups=result["groups"].tolist(), status_counts=[int((result["status"] == k).sum()) for k in (0, 1, 2)])
    return out


def plot_trace(trace, env, path, dt=0.02):
    """The figure of the reference's scripts/play.py for the traced environment `env` of a read_trace() result, as a PNG:
    measured and desired forward velocity over time, and the twelve joint positions."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    col = list(trace["env_ids"]).index(int(env))
    rows = int(trace["rows"])
    seconds = dt * np.arange(1, rows + 1)                       # row t is the state t + 1 policy steps after arming
    figure, (velocity, joints) = plt.subplots(nrows=2, sharex=True, figsize=(10, 6), constrained_layout=True)
    velocity.plot(seconds, trace["cmd_lin_vel_x"][:rows, col], "k:", label="commanded")
    velocity.plot(seconds, trace["lin_vel_x"][:rows, col], "C0", label="measured")
    velocity.set(ylabel="forward velocity [m/s]", title=f"environment {int(env)}")
    velocity.legend(loc="best")
    for j in range(12):
        joints.plot(seconds, trace[f"dof_pos_{j}"][:rows, col], linewidth=0.9, label=f"joint {j}")
    joints.set(xlabel="time since the trace was armed [s]", ylabel="joint position [rad]")
    joints.legend(ncol=6, fontsize="x-small", loc="upper center")
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
