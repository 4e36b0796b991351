"""The actuator network as a run-time input (include/go1sim.h Go1ActuatorTable, go1sim_host.load_actuator_net,
Cfg.control.actuator_net_file): TorchScript files shaped like the reference trainer's output (scripts/actuator_net/utils.py:66-72,
93, 144-145) load into the step library's table bit for bit, everything else is refused with a message that names the file, a
simulator that cannot take the table refuses the switch, and the product's device code (run by the SIMT emulator of tests/emu)
evaluates a loaded network as torch does in float64.  The networks are built and scripted here at run time."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import go1sim_host as H
from util import make_sim, randomize_dr

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))

ACT_DATA = os.path.join(os.path.dirname(__file__), "..", "walk-these-ways_amd", "csrc", "go1_actuator_data.h")


class Act(nn.Module):
    """modelled on the reference trainer's activation module (scripts/actuator_net/utils.py:25-64)"""

    def __init__(self, act, slope=0.05):
        super().__init__()
        self.act = act
        self.slope = slope
        self.shift = torch.log(torch.tensor(2.0)).item()

    def forward(self, input):
        if self.act == "relu":
            return F.relu(input)
        elif self.act == "elu":
            return F.elu(input, alpha=1.)
        elif self.act == "tanh":
            return torch.tanh(input)
        elif self.act == "softsign":
            return F.softsign(input)
        else:
            raise RuntimeError(f"Undefined activation called {self.act}")


def build_mlp(in_dim=6, units=32, layers=2, out_dim=1, act="softsign"):
    """the trainer's build_mlp (utils.py:66-76) without the layer-norm / final-activation options it leaves off"""
    mods = [nn.Linear(in_dim, units), Act(act)]
    for _ in range(layers - 1):
        mods += [nn.Linear(units, units), Act(act)]
    mods += [nn.Linear(units, out_dim)]
    return nn.Sequential(*mods)


def save_scripted(model, path):
    torch.jit.script(model).save(str(path))       # utils.py:144-145
    return str(path)


def table_of(model):
    return np.concatenate([p.detach().float().reshape(-1).numpy() for p in (model[0].weight, model[0].bias, model[2].weight,
                                                                           model[2].bias, model[4].weight, model[4].bias)])


def model_of(table, act_module=None):
    """the trainer's network carrying a table's weights"""
    m = build_mlp() if act_module is None else nn.Sequential(nn.Linear(6, 32), act_module(), nn.Linear(32, 32), act_module(), nn.Linear(32, 1))
    t = torch.from_numpy(np.asarray(table, np.float32))
    o = 0
    with torch.no_grad():
        for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias):
            p.copy_(t[o:o + p.numel()].reshape(p.shape))
            o += p.numel()
    return m


def builtin_table():
    """the GO1_ACT_* arrays of csrc/go1_actuator_data.h (printed exactly: each decimal is the float32 it came from)"""
    src = open(ACT_DATA).read()
    out = []
    for name in ("W0", "B0", "W1", "B1", "W2", "B2"):
        body = re.search(r"GO1_ACT_%s\b[^=]*=\s*([^;]*);" % name, src).group(1)
        out += [float(v) for v in re.findall(r"-?\d+\.\d*(?:[eE][-+]?\d+)?", body)]
    t = np.array(out, dtype=np.float32)
    assert t.size == H.ACT_TABLE_FLOATS
    assert all(float(np.float32(v)) == v for v in out[:64])          # exact float32 values, not rounded decimals
    return t


def random_table(seed):
    """a freshly initialised trainer network (torch's nn.Linear initialisation: the trainer's starting point)"""
    torch.manual_seed(seed)
    return table_of(build_mlp())


def perturbed_table(seed, rel=0.05):
    """the built-in network with ~5 % multiplicative noise on every parameter"""
    t = builtin_table().astype(np.float64)
    return (t * (1.0 + rel * np.random.default_rng(seed).standard_normal(t.size))).astype(np.float32)


def torch_reference_torques(path, B_before, B_after):
    """float64 torch evaluation of the scripted module on the inputs go1sim_compute_torques saw, rebuilt from the history buffers
    around the call (legged_robot.py:927-937: x = (err, err_last, err_last_last, vel, vel_last, vel_last_last)), times the motor
    strength and clipped as there: (12, N)"""
    x = torch.stack([B_after["joint_pos_err_last"], B_before["joint_pos_err_last"], B_before["joint_pos_err_last_last"],
                     B_after["joint_vel_last"], B_before["joint_vel_last"], B_before["joint_vel_last_last"]], dim=-1).double()
    m = torch.jit.load(path, map_location="cpu").double()
    with torch.no_grad():
        tq = m(x.reshape(-1, 6)).reshape(x.shape[:2])
    tq = tq * B_after["motor_strengths"].double()
    lim = B_after["torque_limits"].double()
    return torch.maximum(torch.minimum(tq, lim), -lim).numpy()


HISTORY = ("joint_pos_err_last", "joint_pos_err_last_last", "joint_vel_last", "joint_vel_last_last")


def snapshot(B, S):
    d = {k: B.tensors[k].detach().cpu().clone() for k in HISTORY + ("motor_strengths",)}
    d["torque_limits"] = torch.tensor(list(S.torque_limits)).unsqueeze(1)
    return d


# ---- loader ----------------------------------------------------------------------------------------------------------------
def test_trainer_network_round_trips(tmp_path):
    """the reference trainer's module structure (Linear / Act("softsign") / ...): the table holds its parameters bit for bit"""
    torch.manual_seed(1)
    m = build_mlp()
    path = save_scripted(m, tmp_path / "trainer.pt")
    t = H.load_actuator_net(path)
    assert t.dtype == np.float32 and t.shape == (H.ACT_TABLE_FLOATS,)
    np.testing.assert_array_equal(t, table_of(m))
    x = H.actuator_probe_inputs(256)
    with torch.no_grad():
        want = m.double()(torch.from_numpy(x)).numpy()[:, 0]
    np.testing.assert_allclose(H.actuator_net_eval(t, x), want, rtol=1e-12, atol=1e-12)


def test_sequential_softsign_network_round_trips(tmp_path):
    table = random_table(2)
    path = save_scripted(model_of(table, nn.Softsign), tmp_path / "softsign.pt")
    np.testing.assert_array_equal(H.load_actuator_net(path), table)


def test_builtin_weights_load_bit_equal(tmp_path):
    """a file carrying exactly the built-in GO1_ACT_* values (what the step library installs at go1sim_create) loads to them"""
    table = builtin_table()
    path = save_scripted(model_of(table), tmp_path / "builtin.pt")
    np.testing.assert_array_equal(H.load_actuator_net(path), table)


REFERENCE_ROOT = os.environ.get("WTW_REFERENCE_ROOT")


@pytest.mark.skipif(not REFERENCE_ROOT or not os.path.isfile(os.path.join(REFERENCE_ROOT, "resources", "actuator_nets", "unitree_go1.pt")),
                    reason="set WTW_REFERENCE_ROOT to a walk-these-ways checkout to compare with its unitree_go1.pt")
def test_reference_file_loads_bit_equal_to_the_builtin_table():
    t = H.load_actuator_net(os.path.join(REFERENCE_ROOT, "resources", "actuator_nets", "unitree_go1.pt"))
    np.testing.assert_array_equal(t, builtin_table())


class InputScaled(nn.Sequential):
    """the trainer's layers (same parameter names and shapes) behind a scaling of the inputs"""

    def forward(self, input):
        input = 2.0 * input
        for module in self:
            input = module(input)
        return input


@pytest.mark.parametrize("case", ["hidden_width", "three_hidden_layers", "elu", "nan_weight", "w1_out_of_range", "input_scaling"])
def test_networks_the_kernel_cannot_evaluate_are_refused(tmp_path, case):
    torch.manual_seed(3)
    if case == "hidden_width":
        m, msg = build_mlp(units=64), "shape"
    elif case == "three_hidden_layers":
        m, msg = build_mlp(layers=3), "parameters"
    elif case == "elu":
        m, msg = build_mlp(act="elu"), "not the softsign network"
    elif case == "nan_weight":
        m, msg = build_mlp(), "non-finite"
        with torch.no_grad():
            m[2].weight[3, 4] = float("nan")
    elif case == "w1_out_of_range":
        m, msg = build_mlp(), "fp16"
        with torch.no_grad():
            m[2].weight[0, 0] = 7.0e4
    else:
        m, msg = InputScaled(*build_mlp().children()), "not the softsign network"
    path = save_scripted(m, tmp_path / f"{case}.pt")
    with pytest.raises(ValueError) as exc:
        H.load_actuator_net(path)
    assert path in str(exc.value) and msg in str(exc.value), str(exc.value)


def test_missing_or_foreign_file_is_refused(tmp_path):
    missing = str(tmp_path / "nope.pt")
    with pytest.raises(FileNotFoundError, match=re.escape(missing)):
        H.load_actuator_net(missing)
    junk = tmp_path / "junk.pt"
    junk.write_bytes(b"not a torchscript archive")
    with pytest.raises(ValueError, match="not a TorchScript file"):
        H.load_actuator_net(str(junk))


# ---- environment switch --------------------------------------------------------------------------------------------------
def _small_env(monkeypatch, actuator_net_file, control_type="actuator_net"):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    Cfg = apply_train_config(make_cfg(), num_envs=16)
    Cfg.terrain.mesh_type = "plane"
    Cfg.control.control_type = control_type
    Cfg.control.actuator_net_file = actuator_net_file
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=Cfg)


def test_switch_is_off_by_default_and_travels_in_the_logged_parameters(tmp_path):
    """absent from the defaults (they stay the reference's): None.  Set, it is part of vars(Cfg), which scripts/train.py logs
    (logger.log_params(Cfg=vars(Cfg)), train.py:209-210) and play.py's load_env writes back (play.py:35-46)"""
    import pickle
    from go1_gym.envs.base.legged_robot_config import make_cfg
    assert getattr(make_cfg().control, "actuator_net_file", None) is None
    Cfg = make_cfg()
    Cfg.control.actuator_net_file = "/nets/retrained.pt"
    with open(tmp_path / "parameters.pkl", "wb") as f:
        pickle.dump({"Cfg": vars(Cfg)}, f)
    with open(tmp_path / "parameters.pkl", "rb") as f:
        stored = pickle.load(f)["Cfg"]
    Cfg2 = make_cfg()
    for key, value in stored.items():
        if hasattr(Cfg2, key):
            for key2, value2 in value.items():
                setattr(getattr(Cfg2, key), key2, value2)
    assert Cfg2.control.actuator_net_file == "/nets/retrained.pt"


def test_simulator_without_the_table_refuses_the_file(monkeypatch, tmp_path):
    """the oracle-backed stand-in only has the built-in network: it must not run silently with it"""
    path = save_scripted(model_of(perturbed_table(0)), tmp_path / "retrained.pt")
    with pytest.raises(RuntimeError, match="cannot load an actuator network"):
        _small_env(monkeypatch, path)


def test_file_is_read_only_for_the_actuator_net_torque_model(monkeypatch, tmp_path):
    """as in the reference, the network is only loaded when control_type == 'actuator_net' (a PD run ignores the switch) — and a
    bad file is refused before any simulator exists"""
    _small_env(monkeypatch, str(tmp_path / "absent.pt"), control_type="P")
    with pytest.raises(FileNotFoundError):
        _small_env(monkeypatch, str(tmp_path / "absent.pt"))


# ---- the product's device code, emulated on the CPU ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import emu_sim
    emu_sim.lib()
    return emu_sim


def test_emulated_handle_starts_with_the_builtin_table_and_restores_it(emu):
    cfg, S, meta, B = make_sim("train", 16)
    sim = emu.EmuSim(S, B)
    np.testing.assert_array_equal(sim.actuator_net(), builtin_table())
    p = perturbed_table(1)
    sim.set_actuator_net(p)
    np.testing.assert_array_equal(sim.actuator_net(), p)
    sim.set_config(S)                                   # a configuration change keeps the table
    np.testing.assert_array_equal(sim.actuator_net(), p)
    sim.set_actuator_net(None)
    np.testing.assert_array_equal(sim.actuator_net(), builtin_table())
    bad = p.copy()
    bad[H.ACT_TABLE_FLOATS - 1] = np.inf
    with pytest.raises(RuntimeError, match="go1sim_set_actuator_net failed: -7"):
        sim.set_actuator_net(bad)
    np.testing.assert_array_equal(sim.actuator_net(), builtin_table())


@pytest.mark.parametrize("N", [16, 40])          # 16: one full wavefront (matrix-core path); 40: + a partial one (actuator_net3)
@pytest.mark.parametrize("net", ["random", "perturbed"])
def test_emulated_torques_of_a_loaded_network_match_torch(emu, tmp_path, N, net):
    table = random_table(5) if net == "random" else perturbed_table(6)
    path = save_scripted(model_of(table), tmp_path / f"{net}.pt")
    cfg, S, meta, B = make_sim("train", N)
    randomize_dr(B, 3)
    sim = emu.EmuSim(S, B)
    sim.set_actuator_net(H.load_actuator_net(path))
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for _ in range(3):
        B.dof_pos.copy_(torch.tensor(list(S.default_dof_pos)).unsqueeze(1) + torch.empty(12, N).uniform_(-0.8, 0.8, generator=g))
        B.dof_vel.copy_(torch.empty(12, N).uniform_(-10, 10, generator=g))
        a = torch.empty(12, N).uniform_(-4, 4, generator=g)
        before = snapshot(B, S)
        sim.compute_torques(a.contiguous())
        want = torch_reference_torques(path, before, snapshot(B, S))
        np.testing.assert_allclose(B.torques.numpy(), want, rtol=1e-5, atol=2e-5)
        worst = max(worst, float(np.abs(B.torques.numpy() - want).max()))
    print(f"emulated torque parity {net} N={N}: max |dtau| = {worst:.2e} N m")
