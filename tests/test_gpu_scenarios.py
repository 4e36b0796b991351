"""The scenarios of tests/scenarios.py — leg-leg self-collision, thigh capsules, hip capsules, joint-limit rows, the contact-heavy regime — on
the COMPILED kernel, with the inputs tests/test_emu_parity.py runs through the SIMT emulator (same builders).  In the random rollouts and
`tumbling` states of tests/test_gpu_parity.py these code paths are reached by chance and a differing contact list is an admitted excuse
(rule (a)); here every scenario asserts from the oracle's record that its events happened, and — one substep at a time from identical state —
that the kernel LISTED what the oracle listed: the exchange of capsule segments between the four lanes of an environment through LDS, the quad
rotations and quad-wide OR of the pair masks (DPP), the emission hand-over between master and helper wavefronts and the rare branches of the pair geometry are the hardware's and the compiler's
here, not the emulator's reading of them.  (`cand_min_dpp` is NOT among them: only the walls instances call it, and these scenarios run on the plane.)

Bookkeeping, tolerances and the bulk gate against the fp32 build of the oracle are those of tests/test_gpu_parity.py (Attribution, SUBSTEP_TOL,
finish()); the measured figures of the run on the MI355X are committed as profiles/parity_scenarios.txt.

tools/dry_run_gpu_tests.py runs this file through the emulator (both instances: the emulator build has the signature-free ones too); the
contact-heavy cases then run 32 environments instead of 256 with the emulator test's thresholds (DRY below)."""
import os

import pytest
import torch

import go1sim_host as H
import scenarios
from test_gpu_parity import SUBSTEP_TOL, Attribution, ProductPair, Shadow32, gpu_pair, make_ratio, sync_from, to_gpu

pytestmark = pytest.mark.gpu

DRY = bool(os.environ.get("GO1_DRY_RUN_GPU_TESTS"))
STATE_OUT = ("root_states", "dof_pos", "dof_vel", "contact_forces")
# events of environments 0..15 a scenario must show (tests/test_emu_parity.py's thresholds; limit rows: 1900 of 1920 env-substeps measured
# with the CPU oracle)
REQUIRED = {"self_collision": dict(leg_leg=200), "thigh_capsules": dict(thigh_pairs=50), "hip_capsules": dict(hip_lower=50, lower_hip=50),
            "limit_rows": dict(limit_rows=1500)}
SIG_DIFFER_PER = 1000            # at most one env-substep in 1000 of a scenario may list another contact set than the oracle: the fp32 build of the
                                 # oracle lists the fp64 one's in all 9,920 env-substeps of the four scenarios at N = 16, and so does the emulated kernel


@pytest.mark.parametrize("instance", ["sig", "product"])
@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("name", list(scenarios.FREE_FLIGHT))
def test_free_flight_scenario_matches_oracle(name, N, instance):
    """One physics substep at a time (`physics_substep()` = mode 2 of the step kernel: the production structure of four wavefronts) from the
    oracle's state, fp32 oracle beside.  N = 40: two full workgroups and a ragged one of 8 environments, every environment e + 16 k a copy of
    environment e.  instance: the `_sig` twin, or the instance the product launches (no signature buffer) with the twin stepped beside it.
      * the scenario's events happened — counted from the oracle's record and again from the twin's own;
      * the kernel listed the oracle's contact points / self pairs / limit-row legs (signature words 0..2): at most 1 env-substep in 1000
        differs, each of those is attributed to the differing list, nothing is attributed to anything else;
      * the bulk gate of finish() against the fp32 oracle;
      * tiling invariance: after every substep every buffer of environment e + 16 k is bit-identical to environment e's;
      * limit_rows: finite, the base at rest, joints inside the limits, no limit-safety fault — on the kernel's own buffers; no faults anywhere.
    Bit-identity of the product instance with its twin is tallied per output and printed (ProductPair.note()), not asserted."""
    import pyoracle
    sc = scenarios.FREE_FLIGHT[name](N)
    S, Bc = sc.S, sc.Bc
    orc = pyoracle.Oracle(S, Bc)
    product = instance == "product"
    pp = ProductPair(S, Bc, orc, STATE_OUT) if product else None
    Bg, sim = (pp.Bg, pp.sim) if product else to_gpu(S, Bc)
    Bt = pp.Bt if product else Bg                                   # the buffers that carry the kernel's own signature
    sh = Shadow32(S, Bc, orc)
    att = Attribution(N)
    own = scenarios.Events()                                        # the events as the `_sig` instance itself recorded them
    kernels = {id(Bg): Bg, id(Bt): Bt}.values()                     # the kernel's buffer sets (product: the instance and its twin)
    counters = [scenarios.KernelCounters() for _ in kernels]
    differ = 0
    for it in range(sc.substeps):
        if sc.torque_fn is not None:
            tau = sc.torque_fn(Bc)
            for B in (Bc, sh.B, Bg, Bt):
                B.torques.copy_(tau)
        orc.physics_substep()
        sh.o.physics_substep()
        twin = None
        if product:
            twin = pp.substep()
        else:
            sim.physics_substep()
            torch.cuda.synchronize()
        att.step(make_ratio(att, SUBSTEP_TOL), Bg, Bc, sh.B, twin=twin)
        differ += int((Bt.contact_signature[:3].cpu() != Bc.contact_signature[:3]).any(0).sum())
        sc.events.substep(Bc)
        own.substep(Bt)
        for B, ctr in zip(kernels, counters):
            for k in STATE_OUT:
                assert bool(torch.isfinite(B.tensors[k]).all()), (it, k)
            odd = sc.not_tiled(B)                                   # equal inputs in different workgroups and in the ragged one: the same bits
            assert not odd, (it, odd)
            ctr.add(B, Bc)                                          # (the re-synchronisation below overwrites the kernel's counters)
        assert not sc.not_tiled(Bc, STATE_OUT), it                  # (the inputs of the next substep are tiled again)
        if name == "limit_rows" and it == sc.substeps - 1:          # the physical checks of the emulator test, before the state is the oracle's again
            rs, q = Bg.root_states.cpu(), Bg.dof_pos.cpu()
            rest = torch.arange(N) % scenarios.BASE < 12
            assert float(rs[10:13, rest].norm(dim=0).max()) < 3.0 and float(rs[7:10, rest].norm(dim=0).max()) < 1.0
            assert bool(((q >= scenarios.DOF_LO - 0.03) & (q <= scenarios.DOF_HI + 0.03)).all())
        pp.sync() if product else sync_from(Bc, Bg, sim, orc)
        sh.sync()
    ev, ev_own = sc.events.free_flight(), own.free_flight()
    att.note = (f"; events of envs 0..15, oracle: {ev}, `_sig` instance's own record: {ev_own}; listed signature words differ from the oracle's in "
                f"{differ} of {att.env_steps} env-substeps" + (pp.note() if product else ""))
    att.finish(f"scenario {name} [{instance} instance, {N} envs x {sc.substeps} substeps]")
    for k, least in REQUIRED[name].items():
        assert ev[k] > least and ev_own[k] > least, (k, ev, ev_own)
    assert differ * SIG_DIFFER_PER <= att.env_steps, (differ, att.env_steps)
    assert att.bad <= differ and att.bad == att.by_rule["a-list"], (att.bad, differ, att.by_rule)
    assert all(att.by_rule[k] == 0 for k in ("c", "a-active", "local", "b-fp32", "b-pert")), att.by_rule
    for ctr in counters:                                            # what the kernel counted over all substeps, not what the last re-synchronisation left
        assert int(ctr.faults[:10].sum()) == 0, ctr.faults.tolist()
        if name == "limit_rows":
            assert int(ctr.faults[H.abi.GO1_FAULT_LIMIT_SAFETY]) == 0, ctr.faults.tolist()


@pytest.mark.parametrize("seed", [4, 100, 101])
def test_full_step_in_the_contact_heavy_regime(seed):
    """tests/test_emu_parity.py::test_emulated_full_step_in_the_contact_heavy_regime on the compiled kernel at 256 environments: robots thrown
    onto the ground in random orientations, joint angles over the whole limit box — lists far beyond 8 contacts, leg-leg self-contacts, the
    mass-split leg phase of the sweep — six full steps against the oracle, re-synchronised every step, the emulator test's tolerances through
    Attribution with the fp32 oracle beside (measured with the CPU oracle: the fp32 oracle alone leaves them in 1 of 1536 env-steps per seed).
    Under tools/dry_run_gpu_tests.py: 32 environments and the emulator test's thresholds."""
    N = 32 if DRY else 256
    cfg, S, meta, Bc, orc = gpu_pair("train", N, extra={"domain_rand": dict(randomize_gravity=False)})
    rng = scenarios.contact_heavy_state(Bc, seed)
    Bg, sim = to_gpu(S, Bc)
    sync_from(Bc, Bg, sim, orc)
    sh = Shadow32(S, Bc, orc)
    att = Attribution(N)
    ev = scenarios.Events()
    ctr = scenarios.KernelCounters()
    drops = 0
    for step in range(scenarios.CONTACT_HEAVY_STEPS):
        a = scenarios.contact_heavy_actions(rng, N)
        orc.step(a)
        sh.o.step(a)
        sim.step(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        # (reset_key: a reset_buf that differs from the oracle's puts the environment outside the tolerances, where it must be attributed or fails)
        att.step(make_ratio(att, scenarios.CONTACT_HEAVY_TOL), Bg, Bc, sh.B, reset_key="reset_buf")
        ev.full_step(Bc)
        # the kernel's counters BEFORE the re-synchronisation overwrites them with the oracle's: both started this step from the same counts
        ctr.add(Bg, Bc)
        assert torch.equal(Bg.contact_drop_counts.cpu(), Bc.contact_drop_counts), (step, Bg.contact_drop_counts.tolist(), Bc.contact_drop_counts.tolist())
        drops = int(Bc.contact_drop_counts.sum())
        sync_from(Bc, Bg, sim, orc)
        sh.sync()
    att.note = f"; events (oracle): {ev.contact_heavy()}; contact points dropped for want of a solver slot (kernel = oracle, per class, every step): {drops}"
    att.finish(f"contact-heavy full step [seed {seed}, {N} envs x {scenarios.CONTACT_HEAVY_STEPS} steps]")
    assert int(ctr.faults[:10].sum()) == 0, ctr.faults.tolist()
    assert ev.peak_listed > 8, ev.contact_heavy()                   # beyond what the first list cap could solve
    if DRY:
        assert ev.split_substeps > 50, ev.contact_heavy()
    else:
        assert ev.split_substeps > 1000 and ev.self_pairs > 1000, ev.contact_heavy()
