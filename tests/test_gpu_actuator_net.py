"""The actuator network as a run-time input on the MI355X (include/go1sim.h go1sim_set_actuator_net, Cfg.control.actuator_net_file):
the run-time table carrying the built-in weights reproduces the built-in run bit for bit on every product instance, a different
network is evaluated as torch does in float64 on both torque paths, it changes the trajectory without faults, train and evaluation
environments share it, and a training run's logged parameters rebuild an environment that uses it.  The oracle keeps the built-in
network, so parity with a loaded one rests on these torque-level and bit-identity checks."""
import os
import pickle

import numpy as np
import pytest
import torch

import go1sim_host as H
from test_actuator_net import builtin_table, model_of, perturbed_table, random_table, save_scripted, snapshot, torch_reference_torques
from util import make_sim, randomize_dr

pytestmark = pytest.mark.gpu


def _sim(N, terrain="plane", seed=11):
    cfg, S, meta, Bc = make_sim("train", N, seed=seed)
    randomize_dr(Bc, seed)
    if terrain != "plane":
        from test_gpu_parity import rough_field
        hs, hscale, vscale = rough_field()
        H.bind_height_field(S, Bc, hs, hscale, vscale, 0.0, slope_threshold=0.75 if terrain == "walls" else None)
        assert (S.hf_wall_units > 0) == (terrain == "walls")
        Bc.env_origins[0].uniform_(4.0, 19.0, generator=torch.Generator().manual_seed(1))
        Bc.env_origins[1].uniform_(4.0, 19.0, generator=torch.Generator().manual_seed(2))
        ix, iy = (Bc.env_origins[0] / hscale).long(), (Bc.env_origins[1] / hscale).long()
        Bc.env_origins[2] = torch.from_numpy(hs.astype(np.float32))[ix, iy] * vscale + 0.05
    return S, Bc


def _gpu(S, Bc, table=None):
    Bg = Bc.clone_to("cuda:0")                   # no contact-signature buffer: the product instances (go1_step_kernel / _hf / _walls)
    sim = H.Go1Sim(S, Bg, 0)
    if table is not None:
        sim.set_actuator_net(table)
    sim.reset_idx()
    return Bg, sim


def _fatal(Bg):
    counts = Bg.fault_counts.cpu().numpy().astype(np.int64)
    return int(sum(counts[b] for b in range(len(counts)) if (H.FAULT_FATAL_MASK >> b) & 1))


def test_fresh_handle_carries_the_builtin_table():
    S, Bc = _sim(64)
    Bg, sim = _gpu(S, Bc)
    np.testing.assert_array_equal(sim.actuator_net(), builtin_table())


OUTPUTS = ("root_states", "dof_pos", "dof_vel", "obs_buf", "privileged_obs_buf", "obs_history", "rew_buf", "reset_buf", "time_out_buf",
           "contact_forces", "torques", "episode_length_buf", "fault_flags", "fault_counts")


@pytest.mark.parametrize("terrain", ["plane", "hf", "walls"])
def test_builtin_weights_from_a_file_are_bit_identical_to_the_builtin_table(tmp_path, terrain):
    N, steps = 4096, 200
    table = H.load_actuator_net(save_scripted(model_of(builtin_table()), tmp_path / "builtin.pt"))
    S, Bc = _sim(N, terrain)
    runs = []
    for tab in (None, table):
        Bg, sim = _gpu(S, Bc, tab)
        g = torch.Generator(device="cuda:0").manual_seed(5)
        for _ in range(steps):
            sim.step(0.5 * torch.randn(N, 12, device="cuda:0", generator=g))
        torch.cuda.synchronize()
        runs.append({k: Bg.tensors[k].cpu().clone() for k in OUTPUTS})
        assert _fatal(Bg) == 0
        del sim
    for k in OUTPUTS:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert int(runs[0]["reset_buf"].sum()) >= 0 and float(runs[0]["torques"].abs().max()) > 1.0


@pytest.mark.parametrize("N", [256, 200])         # 256: full workgroups (matrix-core path); 200: a partial last one (actuator_net3)
@pytest.mark.parametrize("net", ["random", "perturbed"])
def test_torques_of_a_loaded_network_match_torch(tmp_path, N, net):
    """go1sim_compute_torques with a loaded network against the float64 torch evaluation of the scripted module (the pattern of
    test_gpu_parity.py::test_torque_model_matches_oracle, whose oracle only knows the built-in network)"""
    table = random_table(5) if net == "random" else perturbed_table(6)
    path = save_scripted(model_of(table), tmp_path / f"{net}.pt")
    S, Bc = _sim(N)
    Bg, sim = _gpu(S, Bc, H.load_actuator_net(path))
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for _ in range(9):
        Bg.dof_pos.copy_(torch.tensor(list(S.default_dof_pos)).unsqueeze(1) + torch.empty(12, N).uniform_(-0.8, 0.8, generator=g))
        Bg.dof_vel.copy_(torch.empty(12, N).uniform_(-10, 10, generator=g))
        a = torch.empty(12, N).uniform_(-4, 4, generator=g)
        before = snapshot(Bg, S)
        sim.compute_torques(a.cuda().contiguous())
        torch.cuda.synchronize()
        want = torch_reference_torques(path, before, snapshot(Bg, S))
        got = Bg.torques.cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-5)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"torque parity {net} N={N} ({'matrix-core' if N % 64 == 0 else 'with a partial workgroup'}): max |dtau| = {worst:.2e} N m")


def test_loaded_network_changes_the_trajectory_without_faults(tmp_path):
    N = 4096
    table = H.load_actuator_net(save_scripted(model_of(perturbed_table(7)), tmp_path / "perturbed.pt"))
    S, Bc = _sim(N)
    out = []
    for tab in (None, table):
        Bg, sim = _gpu(S, Bc, tab)
        g = torch.Generator(device="cuda:0").manual_seed(9)
        for t in range(1000):
            sim.step(0.5 * torch.randn(N, 12, device="cuda:0", generator=g))
            if t == 49:
                out.append(Bg.dof_pos.cpu().clone())
        torch.cuda.synchronize()
        assert _fatal(Bg) == 0, Bg.fault_counts.cpu().tolist()
        assert torch.isfinite(Bg.root_states).all() and torch.isfinite(Bg.dof_pos).all()
        del sim
    assert float((out[0] - out[1]).abs().max()) > 1e-2


def test_train_and_eval_environments_share_the_loaded_table(tmp_path):
    N, NT = 256, 128
    path = save_scripted(model_of(perturbed_table(8)), tmp_path / "perturbed.pt")
    table = H.load_actuator_net(path)
    S, Bc = _sim(N)
    Bg, sim = _gpu(S, Bc, table)
    sim.set_eval_config(H.make_eval_sim_config(S, S), NT)
    sim.set_config(S)                                            # (re-installs both blocks: the table stays)
    np.testing.assert_array_equal(sim.actuator_net(), table)
    g = torch.Generator().manual_seed(1)
    Bg.dof_pos.copy_(torch.tensor(list(S.default_dof_pos)).unsqueeze(1) + torch.empty(12, N).uniform_(-0.8, 0.8, generator=g))
    Bg.dof_vel.copy_(torch.empty(12, N).uniform_(-10, 10, generator=g))
    before = snapshot(Bg, S)
    sim.compute_torques(torch.empty(12, N).uniform_(-4, 4, generator=g).cuda().contiguous())
    torch.cuda.synchronize()
    want = torch_reference_torques(path, before, snapshot(Bg, S))
    got = Bg.torques.cpu().numpy()
    np.testing.assert_allclose(got[:, :NT], want[:, :NT], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got[:, NT:], want[:, NT:], rtol=1e-5, atol=2e-5)


def test_training_run_logs_the_file_and_play_rebuilds_it(tmp_path):
    """two Runner.learn iterations (bf16 policy) with actuator_net_file set; the parameters logged as scripts/train.py logs them
    (logger.log_params(Cfg=vars(Cfg)), train.py:209-210), restored as play.py's load_env restores them (play.py:35-46), build an
    environment whose simulator carries the same table"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from go1_gym.envs.wrappers.history_wrapper import HistoryWrapper
    from go1_gym_learn.ppo_cse import Runner
    from go1_gym_learn.ppo_cse.ppo import PPO_Args
    from ml_logger import logger
    from scripts.train_config import apply_train_config
    path = save_scripted(model_of(perturbed_table(9)), tmp_path / "retrained.pt")
    table = H.load_actuator_net(path)
    Cfg = apply_train_config(make_cfg(), num_envs=256)
    Cfg.control.actuator_net_file = path
    logger.configure("run_act", root=str(tmp_path))
    logger.print_summary = False
    logger.log_params(Cfg=vars(Cfg))
    PPO_Args.autocast_bf16 = True
    cwd = os.getcwd()
    try:
        env = HistoryWrapper(VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=Cfg))
        np.testing.assert_array_equal(env.env.sim.actuator_net(), table)
        os.chdir(tmp_path)
        runner = Runner(env, device="cuda:0")
        runner.learn(num_learning_iterations=2, init_at_random_ep_len=True, eval_freq=100)
        assert torch.isfinite(runner.alg.flat_param).all()
        assert _fatal(env.env.buffers) == 0
    finally:
        PPO_Args.autocast_bf16 = False
        os.chdir(cwd)
    del runner, env
    with open(tmp_path / "run_act" / "parameters.pkl", "rb") as f:
        stored = pickle.load(f)["Cfg"]
    assert stored["control"]["actuator_net_file"] == path
    Cfg2 = apply_train_config(make_cfg(), num_envs=64)
    for key, value in stored.items():                 # play.py:43-46
        if hasattr(Cfg2, key):
            for key2, value2 in value.items():
                setattr(getattr(Cfg2, key), key2, value2)
    Cfg2.env.num_envs = 64
    env2 = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=Cfg2)
    np.testing.assert_array_equal(env2.sim.actuator_net(), table)
    env2.reset()                                      # (reset_idx of every environment + one step, base_task.py:55-59)
    for _ in range(10):
        env2.step(torch.zeros(64, 12, device="cuda:0"))
    torch.cuda.synchronize()
    assert _fatal(env2.buffers) == 0
