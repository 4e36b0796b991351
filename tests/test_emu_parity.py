"""The product's DEVICE CODE (walk-these-ways_amd/csrc/*.h, go1sim.hip — unmodified) executed lane by lane on the CPU by the
SIMT emulator of tests/emu, against the fp64 oracle and against the reference-generated fixtures.  These are the same
comparisons as the `-m gpu` parity tests at sizes the emulator finishes in seconds; they run where there is no GPU (here
and in the driver's CPU tier).  The emulator is test infrastructure: the product only ever loads csrc/libgo1sim.so.

The self-collision, thigh-capsule, hip-capsule, limit-row and contact-heavy tests take their inputs and event counters from tests/scenarios.py;
tests/test_gpu_scenarios.py runs the same builders on the compiled kernel (the emulator implements DPP, the barriers and the LDS hand-overs
from a reading of them and computes without the HIP build's contraction: a pass here says the SOURCE is right).  Each prints its event counts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import go1sim_host as H  # noqa: E402
import scenarios  # noqa: E402
from test_gpu_parity import ATTRIBUTED_BOUND, RULE_B_FACTOR, RULE_B_FLOOR  # noqa: E402  (constants only: that module's tests need the GPU)
from golden.variants import FUZZ_VARIANTS, random_switches  # noqa: E402
from util import (GOLDEN, RESAMPLE_MODES, check_resample_against_reference, load_maps_fixture, load_resample_fixture, maps_fixture_stream, maps_keep,  # noqa: E402
                  make_sim, randomize_dr, standing_state)


@pytest.fixture(scope="module")
def emu():
    import emu_sim
    emu_sim.lib()
    return emu_sim


def pair(oracle_lib, emu, variant, N, seed=3, signature=False, **kw):
    cfg, S, meta, Bc = make_sim(variant, N, seed=seed, **kw)
    randomize_dr(Bc, seed)
    if signature:
        Bc.enable_contact_signature()
    orc = oracle_lib.Oracle(S, Bc)
    orc.reset_idx()
    Be = Bc.clone_to("cpu")
    return S, Bc, orc, Be, emu.EmuSim(S, Be)


def scenario_pair(oracle_lib, emu, name, signature=True):
    """a free-flight scenario of tests/scenarios.py (the inputs tests/test_gpu_scenarios.py runs on the MI355X), the fp64 oracle on its
    buffers and the emulated kernel on a copy; signature=False: the copy carries no signature buffer, so the emulator runs the instance
    without the signature code (the oracle keeps its record: the event counters read it)"""
    sc = scenarios.FREE_FLIGHT[name]()
    orc = oracle_lib.Oracle(sc.S, sc.Bc)
    Be = sc.Bc.clone_to("cpu")
    if not signature:
        Be.tensors["contact_signature"] = None
        Be.refresh_struct()
    return sc, sc.Bc, orc, Be, emu.EmuSim(sc.S, Be)


def resync(Bc, Be, sim, orc):
    for k, t in Bc.tensors.items():
        if t is not None and Be.tensors.get(k) is not None:
            Be.tensors[k].copy_(t)
    sim.set_counters(orc.ctr.common_step_counter, orc.ctr.lag_head)


class Shadow32:
    """the fp32 build of the oracle beside the fp64 one (same inputs every step): an environment the emulated kernel leaves the
    tolerances in with an IDENTICAL contact set must be one the fp32 oracle leaves the fp64 result in as well (ill-conditioned
    in fp32: tests/test_gpu_parity.py module docstring, attribution (b))"""

    def __init__(self, oracle_lib, S, Bc, orc):
        self.Bc, self.orc = Bc, orc
        self.B = Bc.clone_to("cpu")
        self.o = oracle_lib.Oracle(S, self.B, fp32=True)
        self.sync()

    def sync(self):
        for k, t in self.Bc.tensors.items():
            if t is not None and self.B.tensors.get(k) is not None:
                self.B.tensors[k].copy_(t)
        c, o = self.orc.ctr, self.o.ctr
        o.common_step_counter, o.lag_head, o.history_slot = c.common_step_counter, c.lag_head, c.history_slot


def env_ratio(Bx, Bc, tols, N):
    """(N,) worst |error| / (atol + rtol |ref|) over the listed quantities"""
    r = torch.zeros(N, dtype=torch.float64)
    for k, tol, rt in tols:
        a, b = Bx.tensors[k].double(), Bc.tensors[k].double()
        d = (a - b).abs() / (tol + rt * b.abs())
        r = torch.maximum(r, (d.reshape(N, -1).max(1).values if (a.dim() == 2 and a.shape[0] == N and k in ("obs_buf", "privileged_obs_buf")) else d.reshape(-1, N).max(0).values))
    return r


def assert_attributed(Be, Bc, B32, tols, N, where):
    r, r32 = env_ratio(Be, Bc, tols, N), env_ratio(B32, Bc, tols, N)
    bad = r > 1.0
    # rule (b) of tests/test_gpu_parity.py with ITS frozen constants (until round 5 this file had a private `r32 > 0.5 r`; the hardware suite's
    # rule is the one that was measured — 4096 envs x 40 steps x 3 instances — and one rule set is easier to audit than two)
    ok = (Be.contact_signature != Bc.contact_signature).any(0) | ((r32 > RULE_B_FLOOR) & (r <= RULE_B_FACTOR * r32))
    assert not bool((bad & ~ok).any()), (where, (bad & ~ok).nonzero().flatten().tolist(), r[bad & ~ok].tolist())
    assert float(r.max()) < ATTRIBUTED_BOUND, (where, float(r.max()))
    return int(bad.sum())


def diff(Be, Bc, k):
    return float((Be.tensors[k].double() - Bc.tensors[k].double()).abs().max())


@pytest.mark.parametrize("variant,N", [("train_noise", 32), ("alt", 16), ("train_noise", 8), ("dr", 16), ("train_noise", 1),
                                       ("dr", 21), ("alt2", 16)])
def test_emulated_kernel_full_step_matches_oracle(oracle_lib, emu, variant, N):
    """fp32 kernel vs fp64 oracle, identical state / action / RNG streams, re-synchronised every step: round-off only.
    N = 32: two wavefronts, matrix-core torque path; N = 8: a partial wavefront, plain-FMA torque path; N = 1: scripts/play.py's
    single environment (play.py:62); N = 21: a ragged second workgroup."""
    S, Bc, orc, Be, sim = pair(oracle_lib, emu, variant, N)
    rng = np.random.default_rng(0)
    for step in range(8):
        a = (rng.standard_normal((N, 12)) * (2.5 if step % 3 == 0 else 0.5)).astype(np.float32)
        orc.step(a)
        sim.step(torch.from_numpy(a))
        assert torch.equal(Be.reset_buf, Bc.reset_buf) and torch.equal(Be.time_out_buf, Bc.time_out_buf)
        for k, tol in (("dof_pos", 5e-6), ("dof_vel", 1e-3), ("root_states", 2e-4), ("contact_forces", 2e-2), ("torques", 1e-3),
                       ("obs_buf", 1e-4), ("rew_buf", 1e-5), ("commands", 1e-6), ("episode_sums", 1e-4), ("foot_positions", 1e-4),      # (world coordinates reach 150 m: 1.5e-5 per fp32 ulp)
                       # what the torque model carries from substep to substep and step to step (the step kernel keeps it in an
                       # LDS stash and writes it back once: the write-back must leave exactly what compute_torques() leaves)
                       ("joint_pos_err_last", 1e-5), ("joint_pos_err_last_last", 1e-5), ("joint_vel_last", 1e-3), ("joint_vel_last_last", 1e-3),
                       ("joint_pos_target", 1e-6), ("lag_buffer", 1e-6)):
            assert diff(Be, Bc, k) <= tol, (step, k, diff(Be, Bc, k))
        resync(Bc, Be, sim, orc)
    assert int(Be.fault_counts[:10].sum()) == 0


@pytest.mark.parametrize("scenario", ["flight", "standing", "dropped", "tumbling"])
def test_emulated_physics_substep_matches_oracle(oracle_lib, emu, scenario):
    N = 32
    S, Bc, orc, Be, sim = pair(oracle_lib, emu, "train", N, extra={"domain_rand": dict(randomize_gravity=False)})
    g = torch.Generator().manual_seed(1)
    if scenario == "flight":
        Bc.root_states[2] = 2.0
        Bc.dof_vel.uniform_(-5, 5, generator=g)
        Bc.root_states[7:13].uniform_(-2, 2, generator=g)
    elif scenario == "standing":
        standing_state(S, Bc, z=0.28)
    elif scenario == "dropped":
        Bc.root_states[2].uniform_(0.05, 0.3, generator=g)
        Bc.root_states[9] = -1.5
    else:
        q = torch.randn(4, N, generator=g)
        Bc.root_states[3:7] = q / q.norm(dim=0, keepdim=True)
        Bc.root_states[2].uniform_(0.08, 0.35, generator=g)
        Bc.root_states[7:13].uniform_(-2, 2, generator=g)
        Bc.dof_vel.uniform_(-5, 5, generator=g)
    Bc.torques.uniform_(-20, 20, generator=g)
    resync(Bc, Be, sim, orc)
    bad = torch.zeros(N, dtype=torch.bool)
    for it in range(5):
        orc.physics_substep()
        sim.physics_substep()
        for k, tol in (("root_states", 2e-4), ("dof_pos", 2e-5), ("dof_vel", 3e-3)):
            bad |= ((Be.tensors[k] - Bc.tensors[k]).abs() > tol).any(0)
        bad |= ((Be.contact_forces - Bc.contact_forces).abs() > 5e-2 + 2e-3 * Bc.contact_forces.abs()).any(0)
        resync(Bc, Be, sim, orc)
    assert int(bad.sum()) <= (0 if scenario in ("flight", "standing") else 1), int(bad.sum())      # contact-mode flips at thresholds
    if scenario != "flight":
        assert float(Bc.contact_forces.abs().max()) > 1.0


def test_emulated_limit_rows_conserve_momentum_and_match_oracle(oracle_lib, emu):
    """The root-cause scenario of round 1's non-finite rewards through the KERNEL code: zero gravity, free flight, 20 N m
    held against the hip velocity limit / the thigh stops.  The limit rows keep the base at rest (before: 1450 rad/s after
    50 substeps) and the kernel follows the oracle to round-off, so the rows are the same rows."""
    sc, Bc, orc, Be, sim = scenario_pair(oracle_lib, emu, "limit_rows", signature=False)
    ctr = scenarios.KernelCounters()                     # (resync() overwrites the kernel's fault counters with the oracle's zeros)
    for it in range(sc.substeps):
        orc.physics_substep()
        sim.physics_substep()
        for k, tol in (("root_states", 5e-4), ("dof_pos", 1e-4), ("dof_vel", 2e-2)):
            assert diff(Be, Bc, k) <= tol, (it, k, diff(Be, Bc, k))
        sc.events.substep(Bc)
        ctr.add(Be, Bc)
        resync(Bc, Be, sim, orc)
    print("events[limit_rows]", sc.events.free_flight())
    assert torch.isfinite(Be.root_states).all()
    assert float(Be.root_states[10:13, :12].norm(dim=0).max()) < 3.0 and float(Be.root_states[7:10, :12].norm(dim=0).max()) < 1.0
    assert bool(((Be.dof_pos >= scenarios.DOF_LO - 0.03) & (Be.dof_pos <= scenarios.DOF_HI + 0.03)).all())
    assert int(ctr.faults[:10].sum()) == 0 and int(ctr.faults[H.abi.GO1_FAULT_LIMIT_SAFETY]) == 0, ctr.faults.tolist()


@pytest.mark.parametrize("variant,fname", [("train", "maps_train.npz"), ("alt", "maps_alt_mild.npz"), ("alt2", "maps_alt2.npz"),
                                           ("alt2", "maps_alt2_mild.npz"), ("train_noise", "maps_train_noise_mild.npz")]
                                          + [(f"fuzz{k}", f"maps_fuzz{k}_mild.npz") for k in range(FUZZ_VARIANTS)])
def test_emulated_post_physics_maps_match_reference_golden(emu, variant, fname):
    """kernel code vs the reference's own Python (tests/golden/maps_*.npz), same bounds as the -m gpu version."""
    N = 48
    seed, counter = maps_fixture_stream(fname)
    cfg, S, meta, Bc = make_sim(variant, N, seed=seed)
    d = load_maps_fixture(fname, S, meta, Bc)
    sim = emu.EmuSim(S, Bc)
    sim.set_counters(counter, 0)
    sim.post_physics(d["gravity"])
    g = lambda k: Bc.tensors[k]
    reset = d["out_reset_buf"].astype(bool)
    keep = maps_keep(d, S)
    np.testing.assert_array_equal(g("reset_buf").numpy().astype(bool), reset)
    tol = dict(rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(g("base_lin_vel").t().numpy(), d["out_base_lin_vel"], **tol)
    np.testing.assert_allclose(g("clock_inputs").t().numpy(), d["out_clock_inputs"], rtol=1e-5, atol=3e-5)
    np.testing.assert_allclose(g("rew_buf").numpy(), d["out_rew_buf"], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(g("episode_sums").numpy()[:, keep], d["out_episode_sums"][:, keep], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(g("obs_buf").numpy()[keep], d["out_obs"][keep], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(g("privileged_obs_buf").numpy()[keep][:, :S.num_privileged_obs], d["out_priv"][keep], rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("variant", ["train", "alt", "act_nolag", "pd_lag"])
def test_emulated_torque_model_matches_reference_golden(emu, variant):
    d = np.load(os.path.join(GOLDEN, f"torques_{variant}.npz"))
    cfg, S, meta, B = make_sim(variant, 16)
    for k in ("motor_strengths", "motor_offsets", "Kp_factors", "Kd_factors"):
        getattr(B, k)[:] = torch.from_numpy(d[k]).t()
    sim = emu.EmuSim(S, B)
    for s_ in range(d["actions"].shape[0]):
        B.dof_pos.copy_(torch.from_numpy(d["dof_pos"][s_]).t())
        B.dof_vel.copy_(torch.from_numpy(d["dof_vel"][s_]).t())
        sim.compute_torques(torch.from_numpy(np.ascontiguousarray(d["actions"][s_].T)))
        np.testing.assert_allclose(B.torques.t().numpy(), d["torques"][s_], rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("mode", list(RESAMPLE_MODES))
def test_emulated_resample_and_curriculum_update_match_reference(emu, mode):
    d, S, meta, B = load_resample_fixture(mode)
    sim = emu.EmuSim(S, B)
    sim.set_counters(int(d["step"]), 0)
    sim.reset_idx(torch.from_numpy(d["env_ids"]))
    sim.curriculum_update()
    check_resample_against_reference(d, B)


def test_emulated_failed_state_is_contained(oracle_lib, emu):
    N = 16
    S, Bc, orc, Be, sim = pair(oracle_lib, emu, "train_noise", N, seed=23)
    z = torch.zeros(N, 12)
    sim.step(z)
    Be.root_states[2, 5] = float("nan")
    Be.dof_vel[7, 9] = float("inf")
    for _ in range(2):
        sim.step(z)
    for k, t in Be.tensors.items():
        if t is not None and t.is_floating_point() and k != "episode_log":
            assert torch.isfinite(t).all(), k
    assert int(Be.fault_flags[5]) & (1 << H.abi.GO1_FAULT_STATE_IN) and int(Be.fault_flags[9]) & H.FAULT_FATAL_MASK
    others = torch.ones(N, dtype=torch.bool)
    others[[5, 9]] = False
    assert int(Be.fault_flags[others].abs().sum()) == 0


def test_emulated_reward_guard_with_the_observations_on_the_helper(oracle_lib, emu):
    """tests/test_gpu_parity.py::test_failed_simulation_guard through the emulated kernel: a NaN in one environment's previous joint rate
    turns the dof_acc reward term non-finite — the only way an environment can reset AFTER the helper wavefront was sent off with the
    observations (csrc/go1_maps.h post_physics: S1 / S2).  The victim is re-initialised and observed again by the master, everything it
    leaves is finite, and the other environments (same workgroup, observed by the helper) are bit-identical to an undisturbed run."""
    N = 32
    S, Bc, orc, Be, sim = pair(oracle_lib, emu, "train_noise", N, seed=21)
    Br = Be.clone_to("cpu")
    ref = emu.EmuSim(S, Br)
    ref.set_counters(orc.ctr.common_step_counter, orc.ctr.lag_head)
    sim.set_counters(orc.ctr.common_step_counter, orc.ctr.lag_head)
    victim = 5
    Be.last_dof_vel[4, victim] = float("nan")
    for B in (Be, Br):            # the previous target differs from this step's: a second roll of the pair would show (advisor finding, round 5)
        B.last_joint_pos_target[:, victim] += 0.37
    z = torch.zeros(N, 12)
    sim.step(z)
    ref.step(z)
    for k in ("rew_buf", "episode_sums", "obs_buf", "obs_history", "privileged_obs_buf", "last_actions", "last_dof_vel"):
        assert torch.isfinite(Be.tensors[k]).all(), k
    assert int(Be.reset_buf[victim]) == 1 and int(Be.time_out_buf[victim]) == 0 and int(Be.episode_length_buf[victim]) == 0
    assert int(Be.fault_flags[victim]) & H.FAULT_FATAL_MASK == 1 << H.abi.GO1_FAULT_REWARD
    others = torch.arange(N) != victim
    assert int((Be.fault_flags[others] & H.FAULT_FATAL_MASK).sum()) == 0
    for k in ("rew_buf", "reset_buf", "obs_buf", "privileged_obs_buf", "last_actions", "last_last_actions", "last_dof_vel", "last_joint_pos_target"):
        a, b = Be.tensors[k], Br.tensors[k]
        per_env_first = a.shape[0] == N and k in ("obs_buf", "privileged_obs_buf")
        assert torch.equal(a[others] if (per_env_first or a.dim() == 1) else a[..., others], b[others] if (per_env_first or b.dim() == 1) else b[..., others]), k
    # the roll of the victim's joint position targets happened ONCE (the reset leaves the pair alone: the undisturbed run's values)
    for k in ("last_joint_pos_target", "last_last_joint_pos_target"):
        assert torch.equal(Be.tensors[k][:, victim], Br.tensors[k][:, victim]), k
    assert not torch.equal(Be.last_joint_pos_target[:, victim], Be.last_last_joint_pos_target[:, victim])
    # the victim's observation is that of the re-initialised environment: its joint-velocity columns are those of the reset state
    assert torch.isfinite(Be.obs_buf[victim]).all() and not torch.equal(Be.obs_buf[victim], Br.obs_buf[victim])


def test_emulated_self_collision_matches_oracle(oracle_lib, emu):
    """Self-collision through the KERNEL code: in free flight the hips swing the lower legs into each other (left-right and,
    with the thighs, front-rear) and fold the feet against the trunk; leg-leg rows carry two leg parts, trunk-leg rows one.
    Kernel and oracle agree to round-off on every substep, and contacts between bodies of the robot do occur."""
    sc, Bc, orc, Be, sim = scenario_pair(oracle_lib, emu, "self_collision", signature=False)
    ctr = scenarios.KernelCounters()                     # (resync() overwrites the kernel's fault counters with the oracle's zeros)
    for it in range(sc.substeps):
        orc.physics_substep()
        sim.physics_substep()
        for k, tol in (("root_states", 5e-4), ("dof_pos", 1e-4), ("dof_vel", 2e-2)):
            assert diff(Be, Bc, k) <= tol, (it, k, diff(Be, Bc, k))
        bad = ((Be.contact_forces - Bc.contact_forces).abs() > 5e-2 + 5e-3 * Bc.contact_forces.abs()).any(0)
        assert int(bad.sum()) == 0, (it, bad.nonzero().flatten().tolist())
        sc.events.substep(Bc)
        ctr.add(Be, Bc)
        resync(Bc, Be, sim, orc)
    print("events[self_collision]", sc.events.free_flight())
    leg_leg, trunk_leg = sc.events.leg_leg, sc.events.trunk_leg
    assert leg_leg > 200, (leg_leg, trunk_leg)      # (the trunk pairs are evaluated too, but the Go1's lower legs cannot reach
                                                    #  the trunk's capsule within the joint limits: they never fire on either side)
    assert int(ctr.faults[:10].sum()) == 0, ctr.faults.tolist()


def test_emulated_thigh_capsules_match_oracle(oracle_lib, emu):
    """Thigh capsules in the self-collision (pairs with a thigh: types 1-3 of the pair mask) through the KERNEL code: in free
    flight the front hips roll inwards, one thigh pitched forward and one back, and the thighs scissor into each other; kernel and oracle list the same pairs
    and agree to round-off, and a pair with a thigh does fire."""
    sc, Bc, orc, Be, sim = scenario_pair(oracle_lib, emu, "thigh_capsules")
    ctr = scenarios.KernelCounters()                     # (resync() overwrites the kernel's fault counters with the oracle's zeros)
    for it in range(sc.substeps):
        orc.physics_substep()
        sim.physics_substep()
        assert torch.equal(Be.contact_signature[:3], Bc.contact_signature[:3]), it
        for k, tol in (("root_states", 5e-4), ("dof_pos", 1e-4), ("dof_vel", 2e-2)):
            assert diff(Be, Bc, k) <= tol, (it, k, diff(Be, Bc, k))
        assert not bool(((Be.contact_forces - Bc.contact_forces).abs() > 5e-2 + 5e-3 * Bc.contact_forces.abs()).any()), it
        sc.events.substep(Bc)
        ctr.add(Be, Bc)
        resync(Bc, Be, sim, orc)
    print("events[thigh_capsules]", sc.events.free_flight())
    assert sc.events.thigh_pairs > 50, sc.events.thigh_pairs
    assert int(ctr.faults[:10].sum()) == 0, ctr.faults.tolist()


def test_emulated_hip_capsules_match_oracle(oracle_lib, emu):
    """Hip capsules in the self-collision (round 5: types 4 / 5 of a pair of legs, hip - the other leg's lower leg) through the KERNEL code: in
    free flight a fore lower leg (knee stretched) is swung back into the hind hip of its side (environments 0-7: left side, the lower-numbered
    leg carries the lower leg = type 5; environments 8-15: the hind lower leg swung FORWARD into the fore hip = type 4), every joint held by
    a PD torque; kernel and oracle list the same pairs and agree to round-off on every substep, and both types do fire."""
    sc, Bc, orc, Be, sim = scenario_pair(oracle_lib, emu, "hip_capsules")
    N = sc.N
    ctr = scenarios.KernelCounters()                     # (resync() overwrites the kernel's fault counters with the oracle's zeros)
    for it in range(sc.substeps):
        tau = sc.torque_fn(Bc)
        Bc.torques.copy_(tau)
        Be.torques.copy_(tau)
        orc.physics_substep()
        sim.physics_substep()
        assert torch.equal(Be.contact_signature[:3], Bc.contact_signature[:3]), it
        for k, tol in (("root_states", 5e-4), ("dof_pos", 1e-4), ("dof_vel", 2e-2)):
            assert diff(Be, Bc, k) <= tol, (it, k, diff(Be, Bc, k))
        assert not bool(((Be.contact_forces - Bc.contact_forces).abs() > 5e-2 + 5e-3 * Bc.contact_forces.abs()).any()), it
        sc.events.substep(Bc)
        ctr.add(Be, Bc)
        resync(Bc, Be, sim, orc)
    print("events[hip_capsules]", sc.events.free_flight())
    seen = sc.events.seen
    assert seen[5] > 50 and seen[6] > 50, seen
    hipf = Bc.contact_forces.view(17, 3, N)[[1, 9]].norm(dim=1)   # FL hip, RL hip: the forces are booked on the hip bodies
    assert float(hipf.max()) > 1.0
    assert int(ctr.faults[:10].sum()) == 0, ctr.faults.tolist()


def test_emulated_train_eval_split_matches_oracle(oracle_lib, emu):
    """eval_cfg (reference base_task.py:43-49, legged_robot.py:531-544 `_call_train_eval`): 16 training + 16 evaluation
    environments, the evaluation group with its own domain-randomisation ranges, push settings and reset distribution
    (include/go1sim.h go1sim_set_eval_config: second configuration block, selected per wavefront).  Kernel (emulated) vs
    oracle over steps full of resets; every freshly drawn parameter lies in ITS group's range; evaluation episodes stay out
    of the training episode log and their first finished episode lands in episode_sums_eval."""
    N, NT = 32, 16
    ev = {"domain_rand": dict(friction_range=[5.0, 5.5], restitution_range=[0.7, 0.8], added_mass_range=[4.0, 4.5],
                              motor_strength_range=[1.5, 1.6], motor_offset_range=[0.10, 0.11], push_robots=True, max_push_vel_xy=2.0,
                              randomize_rigids_after_start=True, randomize_friction=True, randomize_restitution=True, randomize_base_mass=True),
          "terrain": dict(yaw_init_range=0.1, x_offset=163)}            # (an evaluation terrain region 163 samples behind, terrain.py:51)
    cfg, S, meta, Bc = make_sim("dr", N, seed=5)
    _, S_ev_full, _, _ = make_sim("dr", N, seed=5, extra=ev)
    S_eval = H.make_eval_sim_config(S, S_ev_full)
    assert (S.teleport_x_offset, S_eval.teleport_x_offset) == (0.0, 16.0) and S.teleport_robots and S_eval.teleport_robots
    assert S_eval.num_envs == N and list(S_eval.friction_range) == [5.0, 5.5] and list(S.friction_range) != [5.0, 5.5]
    assert S_eval.num_rewards == S.num_rewards and S_eval.resample_interval == S.resample_interval
    randomize_dr(Bc, 5)
    Bc.episode_sums_eval.fill_(-1.0)
    orc = oracle_lib.Oracle(S, Bc)
    orc.set_eval_config(S_eval, NT)
    orc.reset_idx()
    Bc.episode_length_buf[:] = torch.randint(int(S.max_episode_length) - 6, int(S.max_episode_length) - 1, (N,), dtype=torch.int32,
                                             generator=torch.Generator().manual_seed(1))      # time-outs in the next steps
    # the teleport window of each group (`_teleport_robots` :1033-1038): x = 16.2 is inside the evaluation region's low edge zone
    # (16 + 0.4) and an interior point of the training terrain
    Bc.root_states[0, [3, NT + 3]] = 16.2
    Bc.root_states[0, [5, NT + 5]] = 0.2                    # below the training window's low edge, far below the evaluation one's
    x_before = Bc.root_states[0].clone()
    Be = Bc.clone_to("cpu")
    sim = emu.EmuSim(S, Be)
    sim.set_eval_config(S_eval, NT)
    sim.set_counters(orc.ctr.common_step_counter, orc.ctr.lag_head)
    with pytest.raises(RuntimeError):
        sim.set_eval_config(S_eval, 8)                       # not a multiple of 16: refused, nothing changes
    rng = np.random.default_rng(2)
    log_e = np.zeros(Bc.episode_log.shape[0])
    for step in range(8):
        a = (rng.standard_normal((N, 12)) * 0.5).astype(np.float32)
        Be.episode_log.zero_()
        orc.step(a)
        sim.step(torch.from_numpy(a))
        assert torch.equal(Be.reset_buf, Bc.reset_buf), step
        for k, tol in (("dof_pos", 5e-6), ("root_states", 2e-4), ("friction_coeffs", 1e-6), ("restitutions", 1e-6), ("payloads", 1e-6),
                       ("motor_strengths", 1e-6), ("motor_offsets", 1e-6), ("obs_buf", 1e-4), ("rew_buf", 1e-5), ("commands", 1e-6),
                       ("episode_sums", 1e-4), ("episode_sums_eval", 1e-4), ("episode_log", 1e-3)):
            assert diff(Be, Bc, k) <= tol, (step, k, diff(Be, Bc, k))
        if step == 0:
            jump = (Be.root_states[0] - x_before) / (S.terrain_length * (S.terrain_num_rows - 1))
            keep = ~Be.reset_buf.bool()
            want = torch.ones(N)                              # everything else starts near x = 0: below both low edges
            want[3] = 0.0                                     # 16.2 is interior for the training group, edge zone for NT + 3
            assert float((jump - want)[keep].abs().max()) < 0.01 and bool(keep[[3, NT + 3, 5, NT + 5]].all())
        log_e += Be.episode_log.numpy()
        resync(Bc, Be, sim, orc)
    done = Bc.episode_sums_eval[-1] != -1.0
    assert int(done[NT:].sum()) > 0 and int(done[:NT].sum()) == 0          # only evaluation environments write the snapshot
    assert 0 < log_e[-1] <= NT                                               # the training log counted training resets only
    fr, ms = Bc.friction_coeffs, Bc.motor_strengths
    assert bool(((fr[NT:] >= 5.0) & (fr[NT:] <= 5.5)).all()) and bool((fr[:NT] < 5.0).all())
    assert bool(((ms[:, NT:] >= 1.5) & (ms[:, NT:] <= 1.6)).all()) and bool((ms[:, :NT] < 1.5).all())
    assert bool(((Bc.payloads[NT:] >= 4.0) & (Bc.payloads[NT:] <= 4.5)).all())


@pytest.mark.parametrize("seed", [4] + list(range(100, 100 + int(os.environ.get("GO1_FUZZ_CONTACT", "2")))))
def test_emulated_full_step_in_the_contact_heavy_regime(oracle_lib, emu, seed):
    """The 4-wavefront step kernel (helper hand-overs: actuator tiles, the rows of the listed terrain contacts on the helper
    lanes) with robots thrown onto the ground in random orientations with folded / splayed legs: trunk, hip, thigh and calf
    contacts, lists far beyond round 2's cap of 8, leg-leg self-contacts — against the oracle, re-synchronised every step.  No
    environment leaves the tolerances unless its listed contact set differs (contact signature)."""
    N = 32
    S, Bc, orc, Be, sim = pair(oracle_lib, emu, "train", N, extra={"domain_rand": dict(randomize_gravity=False)}, signature=True)
    rng = scenarios.contact_heavy_state(Bc, seed)
    resync(Bc, Be, sim, orc)
    sh = Shadow32(oracle_lib, S, Bc, orc)
    ev = scenarios.Events()
    ctr = scenarios.KernelCounters()                     # (resync() overwrites the kernel's counters with the oracle's)
    tols = scenarios.CONTACT_HEAVY_TOL
    for step in range(scenarios.CONTACT_HEAVY_STEPS):
        a = scenarios.contact_heavy_actions(rng, N)
        orc.step(a)
        sh.o.step(a)
        sim.step(torch.from_numpy(a))
        assert torch.equal(Be.reset_buf, Bc.reset_buf), step
        assert_attributed(Be, Bc, sh.B, tols, N, step)
        ev.full_step(Bc)
        ctr.add(Be, Bc)
        assert int(Be.contact_drop_counts.sum()) == int(Bc.contact_drop_counts.sum()), step      # (both started the step from the same counts)
        resync(Bc, Be, sim, orc)
        sh.sync()
    print(f"events[contact_heavy, seed {seed}]", ev.contact_heavy())
    peak_listed, split_substeps = ev.peak_listed, ev.split_substeps
    assert peak_listed > 8, peak_listed                               # beyond what round 2 could solve
    assert split_substeps > 50, split_substeps                        # the mass-split leg phase ran (two or more legs with hip / thigh rows)
    assert int(ctr.faults[:10].sum()) == 0, ctr.faults.tolist()


@pytest.mark.parametrize("walls,above", [(False, False), (True, False), (False, True)])
def test_emulated_full_step_on_a_height_field(oracle_lib, emu, walls, above):
    """BASELINE config 3 through the emulated step kernel: rough int16 height field with a staircase strip (bilinear height,
    tilted contact normals), the 187-point height scan in the observation (257 columns), resets onto the field — against
    the oracle, re-synchronised every step (the GPU counterpart: tests/test_gpu_parity.py::test_full_step_on_height_field).
    walls: the same field as a `trimesh` terrain — the strip's 0.1 m risers are vertical faces (the kernel's WALLS instances);
    half of the robots start on the strip.  above: the non-reference `rewards.heights_above_terrain` switch (foot / base heights of the
    reward terms measured above the ground, include/go1sim.h reward_heights_above_terrain)."""
    N = 32
    pts_x = [round(-0.8 + 0.1 * i, 1) for i in range(17)]
    pts_y = [round(-0.5 + 0.1 * i, 1) for i in range(11)]
    ex = {"terrain": dict(measure_heights=True, measured_points_x=pts_x, measured_points_y=pts_y),
          "env": dict(observe_heights=True, num_observations=70 + 187),
          "domain_rand": dict(randomize_gravity=False)}
    if above:
        ex["rewards"] = dict(heights_above_terrain=True)
    cfg, S, meta, Bc = make_sim("train_noise", N, seed=13, extra=ex)
    assert bool(S.reward_heights_above_terrain) == above
    rng = np.random.default_rng(2)
    z = rng.uniform(-1, 1, (62, 62))
    z = np.kron(z, np.ones((4, 4)))[:240, :240]
    for _ in range(3):
        z = 0.25 * (np.roll(z, 1, 0) + np.roll(z, -1, 0) + np.roll(z, 1, 1) + np.roll(z, -1, 1))
    z = 0.08 * z / np.abs(z).max()
    z[:, 100:140] += 0.1 * (np.arange(40) // 4)[None, :] % 0.5
    hscale, vscale = 0.1, 0.005
    hs = np.rint(z / vscale).astype(np.int16)
    H.bind_height_field(S, Bc, hs, hscale, vscale, 0.0, slope_threshold=0.75 if walls else None)
    assert (S.hf_wall_units > 0) == walls
    randomize_dr(Bc, 13)
    Bc.enable_contact_signature()
    Bc.env_origins[0].uniform_(4.0, 19.0, generator=torch.Generator().manual_seed(1))
    Bc.env_origins[1].uniform_(4.0, 19.0, generator=torch.Generator().manual_seed(2))
    if walls:
        Bc.env_origins[1, ::2].uniform_(10.2, 13.8, generator=torch.Generator().manual_seed(3))
    ix, iy = (Bc.env_origins[0] / hscale).long(), (Bc.env_origins[1] / hscale).long()
    Bc.env_origins[2] = torch.from_numpy(hs.astype(np.float32))[ix, iy] * vscale + 0.05
    orc = oracle_lib.Oracle(S, Bc)
    orc.reset_idx()
    Bc.episode_length_buf[:8] = int(S.max_episode_length) - 3          # a few time-outs: resets onto the field
    Be = Bc.clone_to("cpu")
    sim = emu.EmuSim(S, Be)
    sim.set_counters(orc.ctr.common_step_counter, orc.ctr.lag_head)
    arng = np.random.default_rng(0)
    resets, wall_points = 0, 0
    sh = Shadow32(oracle_lib, S, Bc, orc)
    tols = (("root_states", 1e-3, 1e-3), ("dof_pos", 2e-4, 0), ("dof_vel", 1e-2, 1e-3), ("rew_buf", 1e-4, 0), ("torques", 5e-3, 0),
            ("measured_heights", 1e-4, 0), ("obs_buf", 2e-3, 0))
    for step in range(6):
        a = (arng.standard_normal((N, 12)) * (1.0 if step % 2 else 0.3)).astype(np.float32)
        orc.step(a)
        sh.o.step(a)
        sim.step(torch.from_numpy(a))
        assert torch.equal(Be.reset_buf, Bc.reset_buf), step
        assert_attributed(Be, Bc, sh.B, tols, N, step)
        wall_points += int((Bc.contact_signature.view(4, 4, N)[:, 1] & 0x1FFF != 0).sum())
        resets += int(Bc.reset_buf.sum())
        resync(Bc, Be, sim, orc)
        sh.sync()
    assert Bc.obs_buf.shape[1] == 257 and float(Bc.obs_buf[:, 70:].abs().max()) > 0.1
    assert resets >= 8, resets
    assert (wall_points > 0) == walls, wall_points
    assert int(Be.fault_counts[:10].sum()) == 0


@pytest.mark.parametrize("case", range(int(__import__("os").environ.get("GO1_FUZZ_CASES", "8"))))
def test_emulated_kernel_under_random_configurations(oracle_lib, emu, case):
    """configuration fuzz (fixed seeds): random consistent sets of the observation, privileged-observation, controller, reward,
    termination and command-sampling switches; emulated kernel vs oracle, three steps each, observation noise on."""
    rng = np.random.default_rng(1000 + case)
    extra = random_switches(rng)
    N = 16
    S, Bc, orc, Be, sim = pair(oracle_lib, emu, "train_noise", N, seed=40 + case, extra=extra)
    assert S.num_obs == extra["env"]["num_observations"]
    Bc.episode_length_buf[:] = torch.randint(0, int(S.max_episode_length), (N,), dtype=torch.int32, generator=torch.Generator().manual_seed(case))
    resync(Bc, Be, sim, orc)
    for step in range(3):
        a = (rng.standard_normal((N, 12)) * (2.0 if step == 1 else 0.5)).astype(np.float32)
        orc.step(a)
        sim.step(torch.from_numpy(a))
        assert torch.equal(Be.reset_buf, Bc.reset_buf) and torch.equal(Be.time_out_buf, Bc.time_out_buf), (case, step)
        for k, tol in (("dof_pos", 5e-6), ("dof_vel", 1e-3), ("root_states", 2e-4), ("torques", 1e-3), ("obs_buf", 1e-4),
                       ("privileged_obs_buf", 1e-4), ("rew_buf", 1e-5), ("commands", 1e-6), ("episode_sums", 1e-4), ("command_sums", 1e-4)):
            assert diff(Be, Bc, k) <= tol, (case, step, k, diff(Be, Bc, k), extra)
        resync(Bc, Be, sim, orc)


# ---- sweep order: the legs' terrain contacts side by side (the contract) against the list order (oracle switch only) ----------------------
def test_sweep_orders_converge_to_the_same_solve(oracle_lib):
    """the oracle's order switch (3 = the contract: a leg's terrain contacts side by side, hip / thigh rows mass-split; 1 = the same without
    splitting, round 4's study order; 0 = list order, the contract of rounds 1-4) is live (4 sweeps in list order and side by side differ
    beyond round-off) and on robots standing on their feet under random joint rates and torques the orders approach the same converged
    solve: 64 sweeps agree within 2e-3 rad/s, while 4 sweeps of EITHER order are 0.17 rad/s away from it (measured) — the order costs
    nothing in convergence there (tools/solver_order_study.py for the statistics; on its feet a robot has no hip / thigh contacts:
    orders 1 and 3 coincide)"""
    N = 16
    out = {}
    for order in (0, 1, 3):
        for sweeps in (4, 64):
            cfg, S, meta, B = make_sim("train", N, extra={"domain_rand": dict(randomize_gravity=False)})
            g = torch.Generator().manual_seed(2)
            standing_state(S, B, 0.28)
            B.dof_vel.uniform_(-3, 3, generator=g)
            B.root_states[7:13].uniform_(-0.5, 0.5, generator=g)
            B.torques.uniform_(-10, 10, generator=g)
            S.solver_iterations = sweeps
            orc = oracle_lib.Oracle(S, B)
            orc.L.go1_oracle_set_solver_order(order)
            try:
                for _ in range(3):
                    orc.physics_substep()
            finally:
                orc.L.go1_oracle_set_solver_order(3)
            out[(order, sweeps)] = torch.cat([B.root_states[7:13], B.dof_vel]).clone()
    assert float((out[(0, 4)] - out[(3, 4)]).abs().max()) > 1e-4
    assert float((out[(1, 4)] - out[(3, 4)]).abs().max()) < 1e-9
    assert float((out[(0, 64)] - out[(3, 64)]).abs().max()) < 2e-3
    for order in (0, 3):
        assert 0.05 < float((out[(order, 4)] - out[(0, 64)]).abs().max()) < 0.5


def test_hip_and_thigh_rows_are_mass_split_for_a_reason(oracle_lib):
    """why the contract splits the base for hip / thigh rows (order 3) instead of running plain block Jacobi over them (round 4's study
    order 1): a limp robot lying on its side (hips, thighs, calves and a trunk edge on the ground) comes to rest under the list order and
    under order 3, and keeps creeping at > 5 mm/s under order 1 — with 8 sweeps too (every leg stops the WHOLE base)."""
    creep = {}
    for order in (0, 1, 3):
        cfg, S, meta, B = make_sim("train", 1, extra={"domain_rand": dict(randomize_gravity=False)})
        S.solver_iterations = 8
        standing_state(S, B, 0.30)
        B.root_states[2, 0] = 0.12; B.root_states[3, 0] = np.sin(np.pi / 4); B.root_states[6, 0] = np.cos(np.pi / 4)
        orc = oracle_lib.Oracle(S, B)
        orc.L.go1_oracle_set_solver_order(order)
        B.torques.zero_()
        try:
            for _ in range(800):
                orc.physics_substep()
            v = 0.0
            for _ in range(40):
                orc.physics_substep()
                v = max(v, float(B.root_states[7:10].norm()))
        finally:
            orc.L.go1_oracle_set_solver_order(3)
        creep[order] = v
    assert creep[0] < 1e-3 and creep[3] < 1e-3 and creep[1] > 5e-3, creep
