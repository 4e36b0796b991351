"""`DR_SETTINGS` and `base_set`: the reference's evaluation presets (go1_gym_learn/eval_metrics/domain_randomization.py),
writing the same `Cfg` fields with the same values.

Called without an argument they write the module-level `Cfg` of go1_gym/envs/base/legged_robot_config.py, as the reference's
do; they also accept a configuration built by `make_cfg()` (`rand_large(cfg)`), which is what `sweep.run_sweep` and the tests
use so that no setting leaks from one run into the next.

What reaches the device (go1sim_host.build_sim_config): every `randomize_*` switch and range below, `push_robots`,
`teleport_robots`, `use_terminal_body_height` / `terminal_body_height`, `resampling_time`, `episode_length_s` and the terrain
sizes.  `domain_rand.restitution` is not a field of the reference's `Cfg` class either: the presets create it, nothing in the
reference or here reads it (accepted and unused).
"""
from go1_gym.envs.base.legged_robot_config import Cfg


# what every evaluation run has in common: no periodic command resampling (an episode reset still draws new commands: sweep.py
# writes the grid's before every step), no time-outs to speak of, termination when the body reaches height 0, robots teleported
# back at the terrain's edge
_BASE = dict(
    terrain=dict(teleport_robots=True, border_size=50, num_rows=10, num_cols=10),
    commands=dict(resampling_time=1e9),
    env=dict(episode_length_s=500),
    rewards=dict(terminal_body_height=0.0, use_terminal_body_height=True),
)

# preset -> the five ranges of cfg.domain_rand that tell the presets apart
_RANGE_FIELDS = ("friction_range", "restitution_range", "added_mass_range", "com_displacement_range", "motor_strength_range")
_RANGES = dict(
    rand_regular=([0.05, 4.5], [0, 1.0], [-1., 3.], [-0.1, 0.1], [0.9, 1.1]),
    rand_large=([0.04, 6.0], [0, 1.0], [-1.5, 4.], [-0.13, 0.13], [0.88, 1.12]),
    # motor strength [0.9, -0.99]: an upper bound below the lower one, most likely a typo for 0.91 in the reference; kept, as
    # the reference's other quirks are — the simulator draws lo + (hi - lo) * u, i.e. strengths down to -0.99
    static_low=([0.05, 0.06], [0, 0.01], [-1., -0.99], [-0.1, -0.09], [0.9, -0.99]),
    static_medium=([1.0, 1.01], [0.5, 0.51], [0.0, 0.01], [0.0, 0.01], [1.0, 1.01]),
    static_high=([4.49, 4.5], [0.99, 1.0], [2.99, 3.], [0.09, 0.1], [1.09, 1.1]),
    only_base_mass=([1.0, 1.01], [0.5, 0.51], [-1, 3], [0.0, 0.01], [1.0, 1.01]),
)
# the same in every preset: which randomisations are on (the five above), which are off, and the ranges of those that are off
_COMMON = dict(
    randomize_friction=True, randomize_restitution=True, randomize_base_mass=True, randomize_com_displacement=True,
    randomize_motor_strength=True, restitution=0.5,
    randomize_Kp_factor=False, Kp_factor_range=[0.8, 1.3], randomize_Kd_factor=False, Kd_factor_range=[0.5, 1.5],
    push_robots=False, push_interval_s=15, max_push_vel_xy=1.,
)


def _write(section, values):
    for field, value in values.items():
        setattr(section, field, list(value) if isinstance(value, list) else value)


def base_set(cfg=None):
    cfg = Cfg if cfg is None else cfg
    for section, values in _BASE.items():
        _write(getattr(cfg, section), values)


def _apply(name, cfg):
    dr = (Cfg if cfg is None else cfg).domain_rand
    _write(dr, _COMMON)
    _write(dr, dict(zip(_RANGE_FIELDS, _RANGES[name])))


def _preset(name):
    def preset(cfg=None):
        _apply(name, cfg)
    preset.__name__ = preset.__qualname__ = name
    return preset


DR_SETTINGS = {name: _preset(name) for name in _RANGES}
# the reference's module-level names: rand_regular(), rand_large(), static_low(), static_medium(), static_high(), only_base_mass()
globals().update(DR_SETTINGS)
