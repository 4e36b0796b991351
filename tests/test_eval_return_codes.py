"""The validation codes of libgo1eval (include/go1eval.h), pinned: for every entry point but go1eval_version, each negative code
it can return short of -20, and which code wins where two conditions fail at once.  The expected codes are read off the order of
the tests in walk-these-ways_amd/csrc/go1eval.hip.  Every case fails validation, so nothing is launched: dlopen needs no GPU."""
import ctypes

import pytest

import go1eval_host as G

FAKE = 0x1000           # a pointer that is not NULL; validation never follows it
NAN, INF = float("nan"), float("inf")
ACC = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


class Call:
    """one call of an entry point: a valid config and every pointer bound, before the case spoils it"""

    def __init__(self, config, buffers, base):
        self.c, self.b, self.row, self.no_cfg, self.no_buf = config(), buffers(), 0, False, False
        for n, _ in buffers._fields_:
            setattr(self.b, n, FAKE)
        base(self.c)


def cfg(**fields):
    def spoil(a):
        for n, v in fields.items():
            setattr(a.c, n, v)
    return spoil


def null(*names):
    def spoil(a):
        for n in names:
            setattr(a.b, n, None)
    return spoil


def element(array, j, value):
    return lambda a: getattr(a.c, array).__setitem__(j, value)


def signal(s, **fields):
    return lambda a: [setattr(a.c.signal[s], n, v) for n, v in fields.items()]


def no_cfg(a):
    a.no_cfg = True


def no_buf(a):
    a.no_buf = True


def row(r):
    return lambda a: setattr(a, "row", r)


def each(names, code):
    return [(f"{n} = NULL", code, [null(n)]) for n in names]


def nobody(count="num_envs"):
    return [("cfg = NULL", -1, [no_cfg]), ("buf = NULL", -1, [no_buf]), ("both NULL", -1, [no_cfg, no_buf]), (f"{count} = 0", -1, [cfg(**{count: 0})]),
            (f"{count} < 0", -1, [cfg(**{count: -3})])]


def groups(extra=()):
    return [("num_groups = 0", -5, [cfg(num_groups=0)]), ("num_groups < 0", -5, [cfg(num_groups=-1)])] + each(["group", "results", *extra], -5)


# ---- the six families: a valid config each
def eval_base(c):
    c.num_envs, c.num_height_points, c.warmup_steps, c.num_groups, c.default_body_mass = 70, 17, 2, 3, 4.801


def behaviour_base(c):
    c.num_envs, c.num_commands, c.num_height_points, c.warmup_steps, c.num_groups, c.dt, c.base_height_target = 70, 15, 17, 2, 3, 0.02, 0.3


def trace_base(c):
    c.num_envs, c.num_traced, c.capacity, c.num_height_points, c.base_height_target = 70, 9, 30, 17, 0.3


def response_base(c):
    c.num_traced, c.rows, c.switch_row, c.pre, c.smooth, c.hold, c.tail, c.band, c.dt = 9, 20, 8, 4, 3, 5, 4, 0.05, 0.02
    c.num_signals, c.num_groups = 2, 3
    c.signal[0].y_channel, c.signal[0].r_channel = 0, 6
    c.signal[1].y_channel, c.signal[1].r_channel, c.signal[1].fixed_target, c.signal[1].fixed_scale = 3, -1, 0.3, 0.1


def push_base(c):
    c.num_envs, c.num_pushed = 70, 9


def recovery_base(c):
    c.num_traced, c.rows, c.push_row, c.pre, c.smooth, c.hold, c.band, c.dt, c.num_groups = 9, 20, 8, 4, 3, 5, 0.1, 0.02, 3


def terrain_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.hf_rows, c.hf_cols, c.penalised_body_mask = 70, 2, 3, 40, 50, 0x6
    c.dt, c.hf_hscale, c.hf_vscale, c.hf_border, c.tile_length, c.tile_width = 0.02, 0.1, 0.005, 5.0, 5.0, 5.0


def joint_base(c):
    c.num_envs, c.warmup_steps, c.num_groups, c.dt, c.soft_torque_limit, c.soft_vel_limit = 70, 2, 3, 0.02, 0.9, 0.9
    for j in range(12):
        c.torque_limit[j], c.vel_limit[j], c.pos_lower[j], c.pos_upper[j] = 23.7, 30.1, -1.0, 1.0


EVAL = (G.Go1EvalConfig, G.Go1EvalBuffers, eval_base)
BEHAVIOUR = (G.Go1BehaviourConfig, G.Go1BehaviourBuffers, behaviour_base)
TRACE = (G.Go1TraceConfig, G.Go1TraceBuffers, trace_base)
RESPONSE = (G.Go1ResponseConfig, G.Go1ResponseBuffers, response_base)
PUSH = (G.Go1PushConfig, G.Go1PushBuffers, push_base)
RECOVERY = (G.Go1RecoveryConfig, G.Go1RecoveryBuffers, recovery_base)
TERRAIN = (G.Go1TerrainConfig, G.Go1TerrainBuffers, terrain_base)
JOINT = (G.Go1JointConfig, G.Go1JointBuffers, joint_base)

EVAL_ACC = ACC + ["steps", "episodes_terminated", "episodes_timed_out"]
EVAL_IN = ["base_lin_vel", "base_ang_vel", "commands", "root_states", "torques", "dof_vel", "payloads", "reset_buf", "time_out_buf", "episode_length_buf"]
BEHAVIOUR_ACC = ACC + ["prev_contact", "stride_steps", "stance_steps", "swing_peak"]
BEHAVIOUR_IN = ["commands", "root_states", "contact_forces", "foot_positions", "foot_velocities", "desired_contact_states", "foot_indices",
                "last_actions", "last_last_actions", "reset_buf", "episode_length_buf"]
TRACE_IN = ["base_lin_vel", "base_ang_vel", "commands", "root_states", "contact_forces", "desired_contact_states", "torques", "dof_vel", "dof_pos",
            "reset_buf"]
TERRAIN_ACC = ACC + ["status", "steps", "end_step", "max_dist"]
TERRAIN_IN = ["root_states", "commands", "contact_forces", "foot_positions", "desired_contact_states", "foot_indices", "env_origins", "reset_buf",
              "time_out_buf", "episode_length_buf"]
JOINT_ACC = ACC + ["prev_dof_vel", "steps", "resets", "hist"]
JOINT_IN = ["torques", "dof_vel", "dof_pos", "reset_buf", "episode_length_buf"]

NO_HEIGHT_POINTS = [("heights bound, num_height_points = 0", -4, [cfg(num_height_points=0)]),
                    ("heights bound, num_height_points < 0", -4, [cfg(num_height_points=-1)])]
RESPONSE_CHECK = nobody("num_traced") + each(["values", "status"], -2) + [
    ("num_signals = 0", -10, [cfg(num_signals=0)]), ("num_signals = 9", -10, [cfg(num_signals=9)]),
    ("num_traced = 0 and no values", -1, [cfg(num_traced=0), null("values")]),
    ("no status and num_signals = 0", -2, [null("status"), cfg(num_signals=0)])]
RECOVERY_CHECK = nobody("num_traced") + each(["values", "status"], -2) + [("num_traced = 0 and no values", -1, [cfg(num_traced=0), null("values")])]

# {entry point: (family, [(what is wrong, expected code, [spoilers])])}
CASES = {
    "go1eval_clear": (EVAL, nobody() + each(EVAL_ACC, -2) + [("num_envs = 0 and no count", -1, [cfg(num_envs=0), null("count")])]),
    "go1eval_accumulate": (EVAL, nobody() + each(EVAL_ACC, -2) + each(EVAL_IN, -3) + NO_HEIGHT_POINTS + [
        ("num_envs = 0 and no sum", -1, [cfg(num_envs=0), null("sum")]),
        ("no count and no commands", -2, [null("count", "commands")]),
        ("no steps, no inputs, no height points", -2, [null("steps", *EVAL_IN), cfg(num_height_points=0)]),
        ("no commands and no height points", -3, [null("commands"), cfg(num_height_points=0)])]),
    "go1eval_reduce": (EVAL, nobody() + each(EVAL_ACC, -2) + groups() + [
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)]),
        ("no max and num_groups = 0", -2, [null("max"), cfg(num_groups=0)]),
        ("no episodes_timed_out and no results", -2, [null("episodes_timed_out", "results")])]),

    "go1eval_behaviour_clear": (BEHAVIOUR, nobody() + each(BEHAVIOUR_ACC, -2) + [("num_envs = 0 and no swing_peak", -1, [cfg(num_envs=0), null("swing_peak")])]),
    "go1eval_behaviour_accumulate": (BEHAVIOUR, nobody() + each(BEHAVIOUR_ACC, -2) + each(BEHAVIOUR_IN, -3) + NO_HEIGHT_POINTS + [
        ("num_commands = 11", -6, [cfg(num_commands=11)]), ("dt = 0", -6, [cfg(dt=0.0)]), ("dt < 0", -6, [cfg(dt=-0.02)]), ("dt = NaN", -6, [cfg(dt=NAN)]),
        ("num_envs = 0 and no min", -1, [cfg(num_envs=0), null("min")]),
        ("no stride_steps and no foot_indices", -2, [null("stride_steps", "foot_indices")]),
        ("no last_actions and no height points", -3, [null("last_actions"), cfg(num_height_points=0)]),
        ("no height points and dt = 0", -4, [cfg(num_height_points=0, dt=0.0)]),
        ("no reset_buf and num_commands = 3", -3, [null("reset_buf"), cfg(num_commands=3)])]),
    "go1eval_behaviour_reduce": (BEHAVIOUR, nobody() + each(BEHAVIOUR_ACC, -2) + groups() + [
        ("num_envs < 0 and no group", -1, [cfg(num_envs=-1), null("group")]),
        ("no prev_contact and num_groups = 0", -2, [null("prev_contact"), cfg(num_groups=0)])]),

    "go1eval_trace_record": (TRACE, nobody() + each(["trace"], -2) + each(TRACE_IN, -3) + NO_HEIGHT_POINTS + [
        ("num_traced = 0", -2, [cfg(num_traced=0)]), ("capacity = 0", -2, [cfg(capacity=0)]),
        ("no env_ids, num_traced != num_envs", -8, [null("env_ids")]),
        ("row < 0", -7, [row(-1)]), ("row = capacity", -7, [row(30)]),
        ("num_envs = 0 and capacity = 0", -1, [cfg(num_envs=0, capacity=0)]),
        ("no trace and no dof_pos", -2, [null("trace", "dof_pos")]),
        ("no torques and no height points", -3, [null("torques"), cfg(num_height_points=0)]),
        ("no height points and no env_ids", -4, [cfg(num_height_points=0), null("env_ids")]),
        ("no env_ids and row = capacity", -8, [null("env_ids"), row(30)]),
        ("capacity = 0 and row = 0", -2, [cfg(capacity=0), row(0)])]),
    "go1eval_response": (RESPONSE, RESPONSE_CHECK + each(["trace"], -3) + [
        ("smooth = 0", -9, [cfg(smooth=0)]), ("smooth > pre + 1", -9, [cfg(smooth=6)]), ("pre > switch_row", -9, [cfg(pre=9, smooth=1)]),
        ("switch_row = rows", -9, [cfg(switch_row=20)]), ("hold = 0", -9, [cfg(hold=0)]), ("tail = 0", -9, [cfg(tail=0)]),
        ("hold > rows - switch_row", -9, [cfg(hold=13)]), ("tail > rows - switch_row", -9, [cfg(tail=13)]),
        ("dt = 0", -9, [cfg(dt=0.0)]), ("dt = NaN", -9, [cfg(dt=NAN)]), ("band = 0", -9, [cfg(band=0.0)]),
        ("y_channel < 0", -10, [signal(0, y_channel=-1)]), ("y_channel = 24", -10, [signal(1, y_channel=24)]),
        ("r_channel = 24", -10, [signal(0, r_channel=24)]),
        ("num_signals = 0 and no trace", -10, [cfg(num_signals=0), null("trace")]),
        ("no trace and smooth = 0", -3, [null("trace"), cfg(smooth=0)]),
        ("hold = 0 and y_channel = 24", -9, [cfg(hold=0), signal(0, y_channel=24)])]),
    "go1eval_response_reduce": (RESPONSE, RESPONSE_CHECK + groups() + [
        ("num_signals = 9 and num_groups = 0", -10, [cfg(num_signals=9, num_groups=0)]),
        ("no values and no results", -2, [null("values", "results")])]),

    "go1eval_push": (PUSH, nobody() + each(["root_states", "push"], -2) + [
        ("num_pushed = 0", -2, [cfg(num_pushed=0)]), ("no env_ids, num_pushed != num_envs", -8, [null("env_ids")]),
        ("num_envs = 0 and num_pushed = 0", -1, [cfg(num_envs=0, num_pushed=0)]),
        ("no push and no env_ids", -2, [null("push", "env_ids")])]),
    "go1eval_recovery": (RECOVERY, RECOVERY_CHECK + each(["trace"], -3) + [
        ("pre = 0", -11, [cfg(pre=0, smooth=1)]), ("pre > push_row", -11, [cfg(pre=9)]), ("push_row = rows", -11, [cfg(push_row=20)]),
        ("smooth = 0", -11, [cfg(smooth=0)]), ("smooth > pre + 1", -11, [cfg(smooth=6)]), ("hold = 0", -11, [cfg(hold=0)]),
        ("hold > rows - push_row", -11, [cfg(hold=13)]), ("dt = 0", -11, [cfg(dt=0.0)]), ("dt = NaN", -11, [cfg(dt=NAN)]),
        ("band < 0", -11, [cfg(band=-0.1)]), ("band = NaN", -11, [cfg(band=NAN)]),
        ("no status and no trace", -2, [null("status", "trace")]),
        ("no trace and hold = 0", -3, [null("trace"), cfg(hold=0)])]),
    "go1eval_recovery_reduce": (RECOVERY, RECOVERY_CHECK + groups() + [
        ("no values and num_groups = 0", -2, [null("values"), cfg(num_groups=0)]),
        ("num_traced = 0 and no group", -1, [cfg(num_traced=0), null("group")])]),

    "go1eval_terrain_clear": (TERRAIN, nobody() + each(TERRAIN_ACC, -2) + [("num_envs = 0 and no status", -1, [cfg(num_envs=0), null("status")])]),
    "go1eval_terrain_accumulate": (TERRAIN, nobody() + each(TERRAIN_ACC, -2) + each(TERRAIN_IN, -3) + [
        ("field bound, hf_rows = 1", -12, [cfg(hf_rows=1)]), ("field bound, hf_cols = 1", -12, [cfg(hf_cols=1)]),
        ("hf_hscale = 0", -12, [cfg(hf_hscale=0.0)]), ("no field, hf_hscale = 0", -12, [null("height_samples"), cfg(hf_rows=0, hf_cols=0, hf_hscale=0.0)]),
        ("tile_length = 0", -12, [cfg(tile_length=0.0)]), ("tile_width < 0", -12, [cfg(tile_width=-5.0)]), ("dt = 0", -12, [cfg(dt=0.0)]),
        ("dt = NaN", -12, [cfg(dt=NAN)]),
        ("num_envs = 0 and no max_dist", -1, [cfg(num_envs=0), null("max_dist")]),
        ("no end_step and no env_origins", -2, [null("end_step", "env_origins")]),
        ("no env_origins and hf_rows = 1", -3, [null("env_origins"), cfg(hf_rows=1)]),
        ("no time_out_buf and dt = 0", -3, [null("time_out_buf"), cfg(dt=0.0)])]),
    "go1eval_terrain_reduce": (TERRAIN, nobody() + each(TERRAIN_ACC, -2) + groups() + [
        ("dt = 0", -12, [cfg(dt=0.0)]), ("dt = NaN", -12, [cfg(dt=NAN)]),
        ("num_groups = 0 and dt = 0", -5, [cfg(num_groups=0, dt=0.0)]),
        ("no results and dt = 0", -5, [null("results"), cfg(dt=0.0)]),
        ("no steps and num_groups = 0", -2, [null("steps"), cfg(num_groups=0)])]),

    "go1eval_joint_clear": (JOINT, nobody() + each(JOINT_ACC, -2) + each(["dof_vel"], -3) + [
        ("num_envs = 0 and no dof_vel", -1, [cfg(num_envs=0), null("dof_vel")]),
        ("no hist and no dof_vel", -2, [null("hist", "dof_vel")])]),
    "go1eval_joint_accumulate": (JOINT, nobody() + each(JOINT_ACC, -2) + each(JOINT_IN, -3) + [
        ("dt = 0", -12, [cfg(dt=0.0)]), ("dt = inf", -12, [cfg(dt=INF)]), ("dt = NaN", -12, [cfg(dt=NAN)]),
        ("soft_torque_limit = 0", -12, [cfg(soft_torque_limit=0.0)]), ("soft_vel_limit < 0", -12, [cfg(soft_vel_limit=-1.0)]),
        ("torque_limit[0] = 0", -12, [element("torque_limit", 0, 0.0)]), ("torque_limit[11] = NaN", -12, [element("torque_limit", 11, NAN)]),
        ("vel_limit[5] = inf", -12, [element("vel_limit", 5, INF)]), ("vel_limit[11] = 0", -12, [element("vel_limit", 11, 0.0)]),
        ("pos_lower[7] > pos_upper[7]", -12, [element("pos_lower", 7, 1.5)]), ("pos_upper[11] = NaN", -12, [element("pos_upper", 11, NAN)]),
        ("no resets and no torques", -2, [null("resets", "torques")]),
        ("no dof_pos and dt = 0", -3, [null("dof_pos"), cfg(dt=0.0)]),
        ("no episode_length_buf and vel_limit[3] = 0", -3, [null("episode_length_buf"), element("vel_limit", 3, 0.0)])]),
    "go1eval_joint_reduce": (JOINT, nobody() + each(JOINT_ACC, -2) + groups(["hist_results"]) + [
        ("no prev_dof_vel and no hist_results", -2, [null("prev_dof_vel", "hist_results")]),
        ("num_envs = 0 and num_groups = 0", -1, [cfg(num_envs=0, num_groups=0)])]),
}


def test_every_entry_point_is_covered():
    assert sorted(CASES) == sorted(s for s in G.EXPORTED_SYMBOLS if s != "go1eval_version") and len(CASES) == 18
    for symbol, (_, cases) in CASES.items():
        assert len({label for label, _, _ in cases}) == len(cases), symbol
        assert sum(len(spoilers) > 1 for _, _, spoilers in cases) >= 1, symbol          # two conditions at once: precedence


@pytest.mark.parametrize("symbol", sorted(CASES))
def test_validation_codes_and_their_precedence(symbol):
    lib = G.load_library()
    fn = getattr(lib, symbol)
    family, cases = CASES[symbol]
    for label, code, spoilers in cases:
        a = Call(*family)
        for spoil in spoilers:
            spoil(a)
        args = [None if a.no_cfg else ctypes.byref(a.c), None if a.no_buf else ctypes.byref(a.b)]
        if symbol == "go1eval_trace_record":
            args.append(a.row)
        assert fn(*args, None) == code, (symbol, label)
