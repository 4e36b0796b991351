"""`METRICS_FNS`: the reference's fourteen evaluation metrics (go1_gym_learn/eval_metrics/metrics.py), each
`fn(env, actor_critic, obs)` on the environment's `[N, k]` views, returning a CPU value per environment.

The ten scalar ones (`SCALAR_METRICS`) are the host-side definition of what libgo1eval's accumulate kernel evaluates per
environment in fp32 (include/go1eval.h, same order as `enum Go1EvalMetric`); tests/golden/eval_metrics.npz pins them bit for
bit to the reference's results.  A sweep does not call them per step — `sweep.run_sweep` arms the device-side metrics
instead — they serve scripts written against the reference and the tests that compare the kernel with them.
"""
import torch

GRAVITY = 9.8            # m/s^2
FROUDE_HEIGHT = 0.30     # m, leg length of the Froude number


def lin_vel_rmsd(env, actor_critic, obs):
    """per-step root of the squared forward-velocity error, i.e. |v_x - commanded v_x|"""
    err = env.base_lin_vel[:, 0] - env.commands[:, 0]
    return (err ** 2).cpu() ** 0.5


def ang_vel_rmsd(env, actor_critic, obs):
    """|yaw rate - commanded yaw rate|"""
    err = env.base_ang_vel[:, 2] - env.commands[:, 2]
    return (err ** 2).cpu() ** 0.5


def lin_vel_x(env, actor_critic, obs):
    return env.base_lin_vel[:, 0].cpu()


def ang_vel_yaw(env, actor_critic, obs):
    return env.base_ang_vel[:, 2].cpu()


def base_height(env, actor_critic, obs):
    """base z above the mean of the measured terrain heights (env.measured_heights is the scalar 0 without a height scan)"""
    clearance = env.root_states[:, 2].unsqueeze(1) - env.measured_heights
    return clearance.mean(dim=1).cpu()


def max_torques(env, actor_critic, obs):
    return env.torques.abs().max(dim=1).values.cpu()


def power_consumption(env, actor_critic, obs):
    """mechanical power: sum over the joints of torque x joint velocity"""
    return (env.torques * env.dof_vel).sum(dim=1).cpu()


def CoT(env, actor_critic, obs):
    """cost of transport P / (m g v); infinite (or NaN) for a robot whose planar speed is zero"""
    power = power_consumption(env, actor_critic, obs)
    mass = (env.default_body_mass + env.payloads).cpu()
    speed = env.base_lin_vel[:, 0:2].norm(dim=1).cpu()
    return power / (mass * GRAVITY * speed)


def froude_number(env, actor_critic, obs):
    """v_x^2 / (g h)"""
    return lin_vel_x(env, actor_critic, obs) ** 2 / (GRAVITY * FROUDE_HEIGHT)


def adaptation_loss(env, actor_critic, obs):
    """mean squared distance between the adaptation module's latent and the privileged encoder's (None for a policy without one)"""
    if not hasattr(actor_critic, "adaptation_module"):
        return None
    estimate = actor_critic.adaptation_module(obs["obs_history"]).detach().cpu()
    target = actor_critic.env_factor_encoder(obs["privileged_obs"]).detach().cpu()
    return ((estimate - target) ** 2).mean(dim=1)


def auxiliary_rewards(env, actor_critic, obs):
    """{reward name: scaled reward}.  The reference returns from inside its loop, after the FIRST reward term; kept (SURVEY.md
    App. D: the reference's quirks are reproduced, not repaired), so the dict holds one entry — or the call returns None for an
    environment without reward terms.  LeggedRobot has `reward_functions` while its reward family is armed and has accumulated a step
    (`start_reward_metrics`, include/go1reward.h): the callables return the LAST step's raw terms, NaN where that step was not measured."""
    if not hasattr(env, "reward_functions"):
        # LeggedRobot here evaluates the reward terms inside the step kernel: there are no per-term callables to run
        raise NotImplementedError("auxiliary_rewards: this environment has no `reward_functions` (the rewards are computed by the step kernel)")
    for name, fn in zip(env.reward_names, env.reward_functions):
        return {name: (fn() * env.reward_scales[name]).detach().cpu()}


def termination(env, actor_critic, obs):
    return env.reset_buf.detach().cpu()


def privileged_obs(env, actor_critic, obs):
    return obs["privileged_obs"].cpu().numpy()


def latents(env, actor_critic, obs):
    return actor_critic.env_factor_encoder(obs["privileged_obs"]).cpu().numpy()


# the order of include/go1eval.h `enum Go1EvalMetric`
SCALAR_METRICS = ["lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques", "power_consumption",
                  "CoT", "froude_number", "termination"]

METRICS_FNS = {fn.__name__: fn for fn in (
    lin_vel_rmsd, ang_vel_rmsd, lin_vel_x, ang_vel_yaw, base_height, max_torques, power_consumption, CoT, froude_number,
    adaptation_loss, auxiliary_rewards, termination, privileged_obs, latents)}
