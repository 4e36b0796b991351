"""Evaluate a trained policy over a grid of commands under the reference's domain-randomisation presets
(go1_gym_learn/eval_metrics): for every preset one rollout of `--envs` environments, the ten scalar metrics accumulated on
the device (include/go1eval.h), one table per preset.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --presets static_medium rand_large --vx 0.5 1.0 1.5 --out RUN_DIR

The checkpoint directory holds `ac_weights_last.pt` (the Runner's state dict) or the exported TorchScript pair
`adaptation_module_latest.jit` + `body_latest.jit`.  Writes `<out>/eval/<preset>.json` and prints a Markdown table per preset.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --behaviour --axis frequency 2 3 4 --axis footswing_height 0.05 0.15

With `--behaviour` the sweep runs over the product of the `--axis NAME V1 V2 ...` command values instead (names:
go1_gym_learn.eval_metrics.behaviour.COMMAND_INDEX), both tables are accumulated on the device, `<out>/eval/<preset>_behaviour.json`
is written and the commanded-versus-realised table is printed.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --response --switch vx 0.5 1.0 1.5 --trace-envs 0 1

With `--response` every environment holds the command `--switch NAME FROM TO [TO ...]` at FROM and is switched to one of the TO
values (NAME: a name of COMMAND_INDEX, or `gait` with gait names); the trace around the switch is recorded and analysed on the
device (go1_gym_learn.eval_metrics.response), `<out>/eval/<preset>_response.json` is written and the step-response table is
printed and appended to `<out>/eval/<preset>_response.md`.  `--trace-envs I [I ...]` also writes those environments' traces to
`<out>/eval/<preset>_trace.npz` and the velocity / joint-position figure of each to `<preset>_trace_env<I>.png`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --push --magnitude 0 0.5 1.0 --direction 0 90 180 270

With `--push` every environment trots at 1 m/s and is pushed once with one cell of the `--magnitude M ...` (m/s) x `--direction D ...`
(degrees in the robot's heading frame: 0 a shove from behind, 90 a push to the left) grid; the trace around the push is recorded
and analysed on the device (go1_gym_learn.eval_metrics.recovery), `<out>/eval/<preset>_push.json` is written and the recovery table
is printed and appended to `<out>/eval/<preset>_push.md`.  `--paired` copies the settled state of the first envs // cells environments
to all of them first (LeggedRobot.save_state / load_state), so that every cell pushes the same robots at the same instant; with a magnitude-0 cell
the table gains the paired excess of the peak velocity error over that control.  `--trace-envs I [I ...]` also writes `<preset>_push_trace.npz` and the
figure of each to `<preset>_push_trace_env<I>.png`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --terrain --rows 4 --cols 5 --vx 1.0 --window 500

With a bare `--terrain` every environment is placed on one tile of a curriculum grid of `--rows` difficulties x `--cols` terrain
types (`--mesh trimesh | heightfield`, `--proportions P ...` for the mix of types), commanded `--vx` m/s forward, and measured for `--window` steps on the device
(go1_gym_learn.eval_metrics.terrain): did it leave its tile, fall or time out, how often did it stumble, how high did its feet
swing above the ground.  `<out>/eval/<preset>_terrain.json` is written and the grid (rows = difficulty, columns = terrain type) is
printed and appended to `<out>/eval/<preset>_terrain.md`.  (`--terrain MESH` with a value keeps its meaning for the other sweeps:
the mesh type of their terrain.)

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --joints --vx 0.5 1.0 1.5

With `--joints` the velocity grid is swept with the per-joint table armed beside the scalar one (go1_gym_learn.eval_metrics.joints):
torque, speed, acceleration, driving and braking power, soft-limit excess and the shares of steps at the torque clip and at the
URDF's speed limit for each of the twelve joints, and a torque-speed histogram per joint.  `<out>/eval/<preset>_joints.json` and the
torque-speed envelope `<preset>_envelope.png` are written and the per-joint table is printed and appended to `<preset>_joints.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --feet --vx 0.5 1.0 1.5

With `--feet` the velocity grid is swept with the foot-loading table armed beside the scalar one (go1_gym_learn.eval_metrics.feet,
include/go1feet.h): duty factor, vertical force, friction use, touchdown speed, impulse and slip per stance for each of the four feet,
and the ground-reaction-force profile over the gait phase.  `<out>/eval/<preset>_feet.json` and the profile figure `<preset>_grf.png`
are written and the per-foot table is printed and appended to `<preset>_feet.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --trunk --vx 0.5 1.0 1.5 --segment-steps 50 --tilt-limit 0.25

With `--trunk` the velocity grid is swept with the trunk table armed beside the scalar one (go1_gym_learn.eval_metrics.trunk,
include/go1trunk.h): roll, pitch and tilt, their rates, the trunk's accelerations, the number of supporting feet, the base's margin inside
the support polygon, and the lateral drift, heading drift and progress error per straight segment of `--segment-steps` steps;
`--tilt-limit` is the sine beyond which a step counts as tilted too far.  `<out>/eval/<preset>_trunk.json` and the tilt histogram
`<preset>_tilt.png` are written and the table is printed and appended to `<preset>_trunk.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --coordination --vx 1.0 --gaits trotting pacing bounding pronking

With `--coordination` the grid (its `--gaits` axis is what this sweep is for) is swept with the gait table armed beside the scalar one
(go1_gym_learn.eval_metrics.gait, include/go1gait.h): the synchrony of the pairs of feet, the touchdown phases of FR, RL and RR within
FL's stride against the commanded ones, the realised gait's class, and the shares of flight, single, pair, three- and four-foot support.
`--min-stride-steps` debounces FL's touchdowns (default 1: none), `--max-stride-steps` drops longer strides (default 100).
`<out>/eval/<preset>_gait.json` and the polar figure `<preset>_gait.png` are written and the table is printed and appended to
`<preset>_gait.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --spectrum --vx 0.5 1.0 1.5

With `--spectrum` the velocity grid is swept with the spectral table armed beside the scalar one (go1_gym_learn.eval_metrics.spectrum,
include/go1spectrum.h): the power spectral density of the actions, torques, joint speeds and trunk rates over segments of
`--segment-steps` steps (even, 8 to 128, default 100), and per quantity and joint type the rms, the dominant frequency and its share,
the share at and above `--high-freq` (default 10 Hz, a placeholder), the centroid and the share locked to the harmonics of the
commanded step frequency; `--taper` is hann (default) or boxcar.  `<out>/eval/<preset>_spectrum.json` and the figure
`<preset>_spectrum.png` are written and the table is printed and appended to `<preset>_spectrum.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --rewards --vx 0.5 1.0 1.5

With `--rewards` the velocity grid is swept with the reward table armed beside the scalar one (go1_gym_learn.eval_metrics.rewards,
include/go1reward.h): the mean scaled reward per step of every active term and its share, their sum, its positive and negative part,
the total after the clip and what the clip forgave, per cell.  `<out>/eval/<preset>_rewards.json` and the stacked-bar figure
`<preset>_rewards.png` are written and the table is printed and appended to `<preset>_rewards.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --placement --axis stance_width 0.1 0.3 0.45

With `--placement` the product of the `--axis NAME V1 V2 ...` command values (as with `--behaviour`: stance_width, stance_length, vx,
frequency, ...) is swept with the placement table armed beside the scalar one (go1_gym_learn.eval_metrics.placement,
include/go1place.h): per foot where it touches down against its nominal stance point and against the Raibert heuristic's target, the
mean error in stance and in swing, the stance sweep, the stride length against |v| / f, the track width against the commanded one, and
an 8 x 8 footprint map of `--map-cell` metres per cell (default 0.03, a placeholder).  `<out>/eval/<preset>_placement.json` and the
footprint figure `<preset>_footprints.png` are written and the table is printed and appended to `<preset>_placement.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --episodes --steps 1500 --vx 0.5 1.0 1.5

With `--episodes` the velocity grid is swept with the episode table armed beside the scalar one, both before the reset that starts the
rollout (go1_gym_learn.eval_metrics.episodes, include/go1episode.h): per cell the episodes closed, still open and cut, the share that
fell, return, length, time to a fall, reward per step, the return discounted with `--gamma` (default 0.99), displacement, path length, the
two tracking errors over an episode, and the Kaplan-Meier survival estimate over sixteen length bins of `--bin-steps` steps (default 0:
ceil(steps / 16)), the episodes still open at the end counted as censored.  `--steps 1500` lets every environment finish an episode of
the 20 s configuration.  `<out>/eval/<preset>_episodes.json` and the survival figure `<preset>_survival.png` are written and the table
is printed and appended to `<preset>_episodes.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --sensitivity --presets rand_large --pair friction motor_strength

With `--sensitivity` the velocity grid is swept with the sensitivity table armed beside the scalar one
(go1_gym_learn.eval_metrics.sensitivity, include/go1sens.h): per cell and per dynamics parameter the preset randomises (friction,
restitution, payload, com_x, com_y, com_z, motor_strength; Kp_factor and Kd_factor when asked for) sixteen bins of its value with the
exposure, the falls charged to the value that was in force, the tracking errors and the power.  `--parameters NAME ...` chooses the
parameters reported, `--pair A B` adds the 8 x 8 hazard map over two of them, `--min-exposure K` (default 200, a placeholder) is the
number of steps a bin needs before it enters an effect.  `<out>/eval/<preset>_sensitivity.json` and the figure
`<preset>_sensitivity.png` are written and the table, with the ranking of the parameters below it, is printed and appended to
`<preset>_sensitivity.md`.

    python tools/eval_sweep.py --checkpoint RUN_DIR/checkpoints --out RUN_DIR --observations --presets rand_large --against RUN_DIR/eval/static_medium_observations.json

With `--observations` the velocity grid is swept with the observation table armed beside the scalar one
(go1_gym_learn.eval_metrics.observations, include/go1obs.h): per cell and per column of obs_buf (and of privileged_obs_buf unless
`--no-privileged`) the moments, sixteen bins and two tails over the channel's range (placeholders by kind unless `--against` gives
them), the steps at the observation clip and the step-to-step change.  `--against FILE.json` takes an earlier run's
`<preset>_observations.json` or a profile written from `observations.profile_from_array` (a robot log's observations): its bin edges
become this run's, and every cell is compared with the file's profile of the same cell when the two cell lists are equal, with the
file's pooled profile otherwise (mean shift, std ratio, Jensen-Shannon divergence, novel share, clip shares, jitter ratio).
`<out>/eval/<preset>_observations.json` (itself a profile: the pooled one at its top level, one per cell under "profiles") and the
figure `<preset>_observations.png` are written and the table, with the ten highest-ranked channels per cell below it, is printed and
appended to `<preset>_observations.md`.
Run on the GPU box."""
import argparse
import functools
import json
import os
import sys
from typing import Callable, NamedTuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "walk-these-ways_amd")
for p in (os.path.join(PKG, "shims"), PKG, REPO):
    sys.path.insert(0, p)
import torch  # noqa: E402


class ScriptedPolicy:
    """the exported TorchScript pair behind the ActorCritic's inference surface"""

    def __init__(self, adaptation_module, body):
        self.adaptation_module, self.body = adaptation_module, body

    def _latent(self, observation_history):
        return self.adaptation_module(observation_history)

    def _actor(self, observation_history, latent):
        return self.body(torch.cat((observation_history, latent), dim=-1))

    def act_inference(self, obs, policy_info={}):
        h = obs["obs_history"]
        return self._actor(h, self._latent(h))


def load_policy(checkpoint_dir, device):
    """ac_weights_last.pt if present (its shapes give the ActorCritic's sizes), else the TorchScript pair"""
    weights = os.path.join(checkpoint_dir, "ac_weights_last.pt")
    if os.path.exists(weights):
        from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
        sd = torch.load(weights, map_location=device)
        first, last = sd["adaptation_module.0.weight"], [k for k in sd if k.startswith("adaptation_module.") and k.endswith(".weight")][-1]
        num_obs_history, num_priv = first.shape[1], sd[last].shape[0]
        num_actions = sd["std"].shape[0]
        policy = ActorCritic(0, num_priv, num_obs_history, num_actions).to(device)
        policy.load_state_dict(sd)
        return policy.eval()
    adapt, body = (os.path.join(checkpoint_dir, n) for n in ("adaptation_module_latest.jit", "body_latest.jit"))
    if os.path.exists(adapt) and os.path.exists(body):
        return ScriptedPolicy(torch.jit.load(adapt, map_location=device), torch.jit.load(body, map_location=device))
    raise FileNotFoundError(f"{checkpoint_dir}: neither ac_weights_last.pt nor adaptation_module_latest.jit + body_latest.jit")


def to_json(result):
    from go1_gym_learn.eval_metrics import sweep
    return dict(preset=result["preset"], num_envs=result["num_envs"], steps=result["steps"], warmup_steps=result["warmup_steps"],
                seed=result["seed"], cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS),
                metrics={k: v.tolist() for k, v in result["metrics"].items()},
                group_fields=["envs", "steps", "episodes_terminated", "episodes_timed_out", "fall_rate"], groups=result["groups"].tolist())


class Mode(NamedTuple):
    """a sweep that arms one family's table beside the scalar one: where its functions are, what it writes and what it takes"""
    flag: str                      # the option that chooses it
    module: str                    # of go1_gym_learn.eval_metrics, and in it the names of
    sweep: str                     # the sweep: (policy, preset, grid, num_envs=, steps=, warmup_steps=, seed=, terrain=, **options) -> result
    to_json: str                   # result -> what <preset><suffix>.json holds
    table: str                     # result -> the Markdown table printed and appended to <preset><suffix>.md
    figure: str                    # (result, path) -> the figure <preset><figure_suffix>
    suffix: str
    figure_suffix: str
    headline: str                  # the end of the table's headline, formatted with a = the arguments and grid
    options: dict = {}             # the mode's own options: name in the arguments -> default
    check: Callable = lambda a: None                  # the arguments with the defaults in -> what is wrong with the options, if anything
    figure_input: Callable = lambda res: (res, {})    # result -> what the figure function takes before the path, and its keywords
    axes: bool = False             # swept over the --axis product instead of the velocity grid

    @property
    def dest(self):
        return self.flag[2:]


def _joint_envelope(res):
    return res["hist"], dict(torque_limit=res["torque_limit"][0], vel_limit=res["vel_limit"][:3], soft_torque_limit=res["soft_torque_limit"],
                             soft_vel_limit=res["soft_vel_limit"])


def _check_sensitivity(a):
    from go1_gym_learn.eval_metrics.sensitivity import PARAMETERS
    unknown = [name for name in (a.parameters or []) + (a.pair or []) if name not in PARAMETERS]
    if unknown:
        return f"--parameters and --pair take names of {PARAMETERS}, not {unknown[0]}"
    if a.pair and a.pair[0] == a.pair[1]:
        return "--pair takes two different parameters"
    return a.min_exposure < 1 and "--min-exposure has to be at least 1"


MODES = (
    Mode("--joints", "joints", "run_joint_sweep", "joint_to_json", "joint_markdown_table", "plot_envelope", "_joints", "_envelope.png",
         "vx {a.vx}, per-joint actuator usage", figure_input=_joint_envelope),
    Mode("--feet", "feet", "run_foot_sweep", "foot_to_json", "foot_markdown_table", "plot_grf", "_feet", "_grf.png", "vx {a.vx}, foot loading"),
    Mode("--trunk", "trunk", "run_trunk_sweep", "trunk_to_json", "trunk_markdown_table", "plot_tilt", "_trunk", "_tilt.png", "vx {a.vx}, trunk motion",
         options=dict(segment_steps=50, tilt_limit=0.25),
         check=lambda a: (a.segment_steps < 1 or not 0.0 <= a.tilt_limit < float("inf")) and
         "--segment-steps has to be at least 1 and --tilt-limit a finite sine that is not negative"),
    Mode("--rewards", "rewards", "run_reward_sweep", "reward_to_json", "reward_table", "plot_reward_shares", "_rewards", "_rewards.png",
         "vx {a.vx}, reward by term (mean per step, share)"),
    Mode("--coordination", "gait", "run_gait_sweep", "gait_to_json", "gait_markdown_table", "plot_gait", "_gait", "_gait.png",
         "vx {a.vx}, gaits {a.gaits}, inter-leg coordination", options=dict(min_stride_steps=1, max_stride_steps=100),
         check=lambda a: (a.min_stride_steps < 1 or a.max_stride_steps < a.min_stride_steps) and
         "--min-stride-steps has to be at least 1 and --max-stride-steps no smaller than it"),
    Mode("--spectrum", "spectrum", "run_spectrum_sweep", "spectrum_to_json", "spectrum_markdown_table", "plot_spectrum", "_spectrum", "_spectrum.png",
         "vx {a.vx}, spectra over {a.segment_steps}-step segments ({a.taper})", options=dict(segment_steps=100, high_freq=10.0, taper="hann"),
         check=lambda a: ((a.segment_steps % 2 or not 8 <= a.segment_steps <= 128) and "--segment-steps has to be even and in [8, 128] with --spectrum") or
         (not 0.0 < a.high_freq < float("inf") and "--high-freq has to be a positive frequency")),
    Mode("--placement", "placement", "run_placement_sweep", "placement_to_json", "placement_table", "plot_footprints", "_placement", "_footprints.png",
         "axes {grid}, foot placement", options=dict(map_cell=0.03), axes=True,
         check=lambda a: not 0.0 < a.map_cell < float("inf") and "--map-cell has to be a positive length"),
    Mode("--episodes", "episodes", "run_episode_sweep", "episode_to_json", "episode_markdown_table", "plot_survival", "_episodes", "_survival.png",
         "vx {a.vx}, whole episodes (gamma {a.gamma})", options=dict(gamma=0.99, bin_steps=0),
         check=lambda a: (not 0.0 < a.gamma <= 1.0 or a.bin_steps < 0) and "--gamma has to lie in (0, 1] and --bin-steps must not be negative (0: steps / 16)"),
    Mode("--sensitivity", "sensitivity", "run_sensitivity_sweep", "sensitivity_to_json", "sensitivity_markdown_table", "plot_sensitivity", "_sensitivity",
         "_sensitivity.png", "vx {a.vx}, robustness against the randomised dynamics", options=dict(parameters=None, pair=None, min_exposure=200),
         check=_check_sensitivity),
    Mode("--observations", "observations", "run_observation_sweep", "observation_to_json", "observation_markdown_table", "plot_observations", "_observations",
         "_observations.png", "vx {a.vx}, the distribution of the policy's observations", options=dict(against=None, no_privileged=False),
         check=lambda a: a.against is not None and not os.path.isfile(a.against) and f"--against {a.against}: no such file"),
)
MODE = {mode.dest: mode for mode in MODES}


def parse_args(argv=None):
    from go1_gym_learn.eval_metrics import sweep
    from go1_gym_learn.eval_metrics.domain_randomization import DR_SETTINGS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--presets", nargs="+", default=["static_medium", "rand_large"], choices=sorted(DR_SETTINGS))
    ap.add_argument("--vx", nargs="+", type=float, default=None, help="default: 0.5 1.0 1.5; with a bare --terrain one value, default 1.0")
    ap.add_argument("--yaw", nargs="+", type=float, default=[0.0])
    ap.add_argument("--gaits", nargs="+", default=["trotting"], choices=sorted(sweep.GAITS))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup-steps", type=int, default=25)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--terrain", nargs="?", default=None, const="tiles", choices=["plane", "heightfield", "trimesh", "tiles"],
                    help="with a value: the mesh type of the sweep's terrain; bare: the terrain-traversal sweep over a tile grid")
    ap.add_argument("--rows", type=int, default=None, help="with a bare --terrain: difficulties (tile rows) of the grid, default 4")
    ap.add_argument("--cols", type=int, default=None, help="with a bare --terrain: terrain types (tile columns) of the grid, default 5")
    ap.add_argument("--window", type=int, default=None, help="with a bare --terrain: measured steps, default 500")
    ap.add_argument("--mesh", default=None, choices=["heightfield", "trimesh"], help="with a bare --terrain: the mesh type, default trimesh")
    ap.add_argument("--proportions", nargs="+", type=float, default=None,
                    help="with a bare --terrain: terrain_proportions of the grid (default: slopes, rough slopes, stairs down, stairs up, obstacles)")
    ap.add_argument("--behaviour", action="store_true", help="measure gait and behaviour tracking over the --axis product instead of the velocity grid")
    ap.add_argument("--axis", nargs="+", action="append", metavar=("NAME", "VALUE"), help="a behaviour command and its values; repeatable")
    ap.add_argument("--response", action="store_true", help="measure the step response to the --switch of one command instead of the velocity grid")
    ap.add_argument("--switch", nargs="+", metavar=("NAME", "VALUE"), help="the switched command, its value before and its values after")
    ap.add_argument("--trace-envs", nargs="+", type=int, default=None, help="with --response or --push: environments whose trace and figure are written")
    ap.add_argument("--push", action="store_true", help="measure the recovery from one push per environment over the --magnitude x --direction grid")
    ap.add_argument("--magnitude", nargs="+", type=float, default=None, help="with --push: velocity steps in m/s; 0 is the control cell")
    ap.add_argument("--paired", action="store_true",
                    help="with --push: the first envs // cells environments' state after settling is copied to all, so every cell pushes the same robots at the same instant")
    ap.add_argument("--direction", nargs="+", type=float, default=None,
                    help="with --push: directions in degrees in the robot's heading frame (0 a shove from behind, 90 a push to the left)")
    ap.add_argument("--joints", action="store_true", help="measure per-joint actuator usage over the velocity grid, beside the scalar table")
    ap.add_argument("--feet", action="store_true", help="measure per-foot ground reaction forces over the velocity grid, beside the scalar table")
    ap.add_argument("--trunk", action="store_true", help="measure trunk motion, support margin and path drift over the velocity grid, beside the scalar table")
    ap.add_argument("--segment-steps", type=int, default=None, help="with --trunk: policy steps of a drift segment, default 50; with --spectrum: of a transformed segment, default 100")
    ap.add_argument("--tilt-limit", type=float, default=None, help="with --trunk: the sine of the tilt beyond which a step is counted, default 0.25")
    ap.add_argument("--coordination", action="store_true", help="measure inter-leg coordination and the realised gait over the grid, beside the scalar table")
    ap.add_argument("--min-stride-steps", type=int, default=None, help="with --coordination: a touchdown of FL sooner after the last is chatter, default 1")
    ap.add_argument("--max-stride-steps", type=int, default=None, help="with --coordination: a stride that outgrows it is dropped, default 100")
    ap.add_argument("--spectrum", action="store_true", help="measure action, torque, joint-speed and trunk-rate spectra over the velocity grid, beside the scalar table")
    ap.add_argument("--high-freq", type=float, default=None, help="with --spectrum: high_share counts the bins from this frequency on, default 10 Hz")
    ap.add_argument("--taper", default=None, choices=["hann", "boxcar"], help="with --spectrum: the taper of a segment, default hann")
    ap.add_argument("--rewards", action="store_true", help="break the step reward down by term over the velocity grid, beside the scalar table")
    ap.add_argument("--placement", action="store_true", help="measure foot placement and stride geometry over the --axis product, beside the scalar table")
    ap.add_argument("--map-cell", type=float, default=None, help="with --placement: the side of a cell of the footprint map in metres, default 0.03")
    ap.add_argument("--episodes", action="store_true", help="measure whole episodes (return, length, survival) over the velocity grid, beside the scalar table")
    ap.add_argument("--gamma", type=float, default=None, help="with --episodes: the discount of the discounted return, in (0, 1], default 0.99")
    ap.add_argument("--bin-steps", type=int, default=None, help="with --episodes: the width of a length bin in steps, default 0: ceil(steps / 16)")
    ap.add_argument("--sensitivity", action="store_true", help="measure exposure, falls and tracking per bin of the randomised dynamics parameters, beside the scalar table")
    ap.add_argument("--parameters", nargs="+", default=None, metavar="NAME", help="with --sensitivity: the parameters reported, default: those the preset randomises")
    ap.add_argument("--pair", nargs=2, default=None, metavar=("A", "B"), help="with --sensitivity: two parameters for the 8 x 8 hazard map")
    ap.add_argument("--min-exposure", type=int, default=None, help="with --sensitivity: steps a bin needs before it enters an effect, default 200 (a placeholder)")
    ap.add_argument("--observations", action="store_true", help="measure the distribution of every observation column over the velocity grid, beside the scalar table")
    ap.add_argument("--against", default=None, metavar="FILE.json", help="with --observations: an earlier run's JSON or a profile_from_array's to compare with; its edges become the ranges")
    ap.add_argument("--no-privileged", action="store_const", const=True, default=None, help="with --observations: leave the privileged columns out")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    a.tiles = a.terrain == "tiles"
    if not a.tiles and any(v is not None for v in (a.rows, a.cols, a.window, a.mesh, a.proportions)):
        ap.error("--rows, --cols, --window, --mesh and --proportions need a bare --terrain")
    # one mode per run: every pair of modes excludes each other, except that --response is accepted with --behaviour (the response runs)
    flags = [("--terrain (bare)", "tiles"), ("--response", "response"), ("--behaviour", "behaviour"), ("--push", "push")] + [(m.flag, m.dest) for m in MODES]
    chosen = [flag for flag, dest in flags if getattr(a, dest)]
    if len(chosen) > 1 and chosen != ["--response", "--behaviour"]:
        ap.error(f"{chosen[0]} excludes {chosen[1]}")
    if a.tiles:
        if a.vx is not None and len(a.vx) != 1:
            ap.error("a bare --terrain takes one --vx")
        a.terrain = None
        a.rows, a.cols, a.window = (d if v is None else v for v, d in ((a.rows, 4), (a.cols, 5), (a.window, 500)))
        a.mesh = a.mesh or "trimesh"
        a.vx = a.vx or [1.0]
        if a.rows < 1 or a.cols < 1 or a.window < 1:
            ap.error("--rows, --cols and --window have to be at least 1")
    a.vx = a.vx or [0.5, 1.0, 1.5]
    # a mode's own option needs that mode (--segment-steps: either of the two that have one); the chosen mode's options get its defaults
    owners = {}
    for mode in MODES:
        for option in mode.options:
            owners.setdefault(option, []).append(mode)
    for option, modes in owners.items():
        if getattr(a, option) is not None and not any(getattr(a, m.dest) for m in modes):
            ap.error(f"--{option.replace('_', '-')} needs " + " or ".join(m.flag for m in modes))
    for mode in MODES:
        if getattr(a, mode.dest):
            for option, default in mode.options.items():
                if getattr(a, option) is None:
                    setattr(a, option, default)
            problem = mode.check(a)
            if problem:
                ap.error(problem)
    if a.switch and not a.response:
        ap.error("--switch needs --response")
    if a.trace_envs and not (a.response or a.push):
        ap.error("--trace-envs needs --response or --push")
    if (a.magnitude or a.direction) and not a.push:
        ap.error("--magnitude and --direction need --push")
    if a.paired and not a.push:
        ap.error("--paired needs --push")
    if a.push and not (a.magnitude and a.direction):
        ap.error("--push needs --magnitude M [M ...] and --direction D [D ...]")
    if a.push and any(m < 0 for m in a.magnitude):
        ap.error("--magnitude: a push has no negative magnitude; turn its direction by 180 degrees")
    if a.response and (not a.switch or len(a.switch) < 3):
        ap.error("--response needs --switch NAME FROM TO [TO ...]")
    return a


def response_switch(a):
    """(command, from value, [to values]) of the --switch option: gait names for `gait`, numbers otherwise"""
    name, first, *rest = a.switch
    if name == "gait":
        return name, first, rest
    return name, float(first), [float(v) for v in rest]


def run_response(a, policy):
    import numpy as np
    from go1_gym_learn.eval_metrics import response
    command, from_value, to_values = response_switch(a)
    for preset in a.presets:
        res = response.run_response_sweep(policy, preset, command, from_value, to_values, num_envs=a.envs, seed=a.seed, terrain=a.terrain,
                                          trace_envs=a.trace_envs)
        stem = os.path.join(a.out, "eval", preset)
        with open(stem + "_response.json", "w") as f:
            json.dump(response.response_to_json(res), f, indent=1)
        text = f"### {preset}: {a.envs} environments, {command} {from_value} -> {to_values}, step response\n\n"
        text += "\n\n".join(response.response_markdown_table(res, s) for s in res["signals"]) + "\n"
        print(text)
        with open(stem + "_response.md", "a") as f:
            f.write(text + "\n")
        if a.trace_envs:
            np.savez(stem + "_trace.npz", **res["trace"])
            for e in a.trace_envs:
                response.plot_trace(res["trace"], e, f"{stem}_trace_env{e}.png", dt=res["dt"])


def run_push(a, policy):
    import numpy as np
    from go1_gym_learn.eval_metrics import recovery, response
    for preset in a.presets:
        res = recovery.run_push_sweep(policy, preset, a.magnitude, a.direction, num_envs=a.envs, seed=a.seed, terrain=a.terrain,
                                      trace_envs=a.trace_envs, **(dict(paired=True) if a.paired else {}))
        stem = os.path.join(a.out, "eval", preset)
        with open(stem + "_push.json", "w") as f:
            json.dump(recovery.recovery_to_json(res), f, indent=1)
        text = f"### {preset}: {a.envs} environments, pushes of {a.magnitude} m/s towards {a.direction} degrees, recovery\n\n"
        text += recovery.recovery_markdown_table(res) + "\n"
        print(text)
        with open(stem + "_push.md", "a") as f:
            f.write(text + "\n")
        if a.trace_envs:
            np.savez(stem + "_push_trace.npz", **res["trace"])
            for e in a.trace_envs:
                response.plot_trace(res["trace"], e, f"{stem}_push_trace_env{e}.png", dt=res["dt"])


def run_terrain(a, policy):
    from go1_gym_learn.eval_metrics import terrain
    for preset in a.presets:
        res = terrain.run_terrain_sweep(policy, preset, vx=a.vx[0], num_envs=a.envs, window=a.window, warmup=a.warmup_steps, seed=a.seed,
                                        num_rows=a.rows, num_cols=a.cols, mesh_type=a.mesh, terrain_proportions=a.proportions)
        stem = os.path.join(a.out, "eval", preset)
        with open(stem + "_terrain.json", "w") as f:
            json.dump(terrain.terrain_to_json(res), f, indent=1)
        text = f"### {preset}: {a.envs} environments on {a.rows} x {a.cols} {a.mesh} tiles, {a.vx[0]} m/s forward, {a.window} steps, terrain traversal\n\n"
        text += "success rate / stumble rate / mean swing foot height [m] / fall rate\n\n" + terrain.terrain_markdown_grid(res) + "\n"
        print(text)
        with open(stem + "_terrain.md", "a") as f:
            f.write(text + "\n")


def run_mode(mode, a, policy, grid):
    """the sweep of one row of MODES for every preset: <preset><suffix>.json, the headline and the table printed and appended to
    <preset><suffix>.md, and the figure.  The module's functions are looked up by name when they are called."""
    import importlib
    module = importlib.import_module("go1_gym_learn.eval_metrics." + mode.module)
    for preset in a.presets:
        res = getattr(module, mode.sweep)(policy, preset, grid, num_envs=a.envs, steps=a.steps, warmup_steps=a.warmup_steps, seed=a.seed, terrain=a.terrain,
                                          **{option: getattr(a, option) for option in mode.options})
        stem = os.path.join(a.out, "eval", preset)
        with open(stem + mode.suffix + ".json", "w") as f:
            json.dump(getattr(module, mode.to_json)(res), f, indent=1)
        text = f"### {preset}: {a.envs} environments, {a.steps} steps, " + mode.headline.format(a=a, grid=grid) + "\n\n" + getattr(module, mode.table)(res) + "\n"
        print(text)
        with open(stem + mode.suffix + ".md", "a") as f:
            f.write(text + "\n")
        subject, keywords = mode.figure_input(res)
        getattr(module, mode.figure)(subject, stem + mode.figure_suffix, **keywords)


run_joints = functools.partial(run_mode, MODE["joints"])                     # run_X(a, policy, grid): each mode under a name of its own
run_feet = functools.partial(run_mode, MODE["feet"])
run_trunk = functools.partial(run_mode, MODE["trunk"])
run_rewards = functools.partial(run_mode, MODE["rewards"])
run_gait = functools.partial(run_mode, MODE["coordination"])
run_spectrum = functools.partial(run_mode, MODE["spectrum"])
run_placement = functools.partial(run_mode, MODE["placement"])              # (its grid is the --axis product)
run_episodes = functools.partial(run_mode, MODE["episodes"])
run_sensitivity = functools.partial(run_mode, MODE["sensitivity"])
run_observations = functools.partial(run_mode, MODE["observations"])


def behaviour_axes(a):
    """{command name: [values]} of the --axis options, in the order given"""
    from go1_gym_learn.eval_metrics.behaviour import COMMAND_INDEX
    if not a.axis:
        raise SystemExit(("--placement" if a.placement else "--behaviour") + " needs at least one --axis NAME V1 V2 ...")
    axes = {}
    for name, *values in a.axis:
        if name not in COMMAND_INDEX or not values:
            raise SystemExit(f"--axis {name}: a name of {sorted(COMMAND_INDEX)} followed by at least one value")
        axes[name] = [float(v) for v in values]
    return axes


def main(argv=None):
    from go1_gym_learn.eval_metrics import sweep
    a = parse_args(argv)
    assert torch.cuda.is_available(), "eval_sweep needs a GPU"
    policy = load_policy(a.checkpoint, "cuda:0")
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    os.makedirs(os.path.join(a.out, "eval"), exist_ok=True)
    if a.response:
        return run_response(a, policy)
    if a.push:
        return run_push(a, policy)
    if a.tiles:
        return run_terrain(a, policy)
    for mode in MODES:
        if getattr(a, mode.dest):
            return run_mode(mode, a, policy, behaviour_axes(a) if mode.axes else grid)
    if a.behaviour:
        from go1_gym_learn.eval_metrics import behaviour
        axes = behaviour_axes(a)
        for preset in a.presets:
            res = behaviour.run_behaviour_sweep(policy, preset, axes, num_envs=a.envs, steps=a.steps, warmup_steps=a.warmup_steps, seed=a.seed,
                                                terrain=a.terrain)
            with open(os.path.join(a.out, "eval", preset + "_behaviour.json"), "w") as f:
                json.dump(behaviour.behaviour_to_json(res), f, indent=1)
            print(f"### {preset}: {a.envs} environments, {a.steps} steps, behaviour\n")
            print(behaviour.behaviour_markdown_table(res) + "\n")
        return
    for preset in a.presets:
        res = sweep.run_sweep(policy, preset, grid, num_envs=a.envs, steps=a.steps, warmup_steps=a.warmup_steps, seed=a.seed, terrain=a.terrain)
        with open(os.path.join(a.out, "eval", preset + ".json"), "w") as f:
            json.dump(to_json(res), f, indent=1)
        print(f"### {preset}: {a.envs} environments, {a.steps} steps\n")
        print(sweep.markdown_table(res) + "\n")


if __name__ == "__main__":
    main()
