"""The oracle in fp32 (oracle/_build/libgo1oracle32.so: the same C source with real = float, Makefile) against the fp64 build.

What separates the two is round-off only.  The parity tests (tests/test_gpu_parity.py, tests/test_emu_parity.py) allow an
environment outside the per-quantity tolerances only if its contact set differs or if THIS fp32 build leaves the fp64 result
there as well; here the fp32 build is measured on its own: on the train.py configuration under N(0,1) actions (robots
falling and tangling: the contact-heavy regime) it leaves the tolerances in far fewer than 1e-3 of the environment-steps, by a
bounded factor — so the 1-2 % outlier budgets of round 2 were not precision (they came from the 8-contact cap's dropped
points), and none is granted now."""
import numpy as np
import pytest
import torch

from util import make_sim, randomize_dr

TOL = (("root_states", 1e-3, 1e-3), ("dof_pos", 1e-3, 0), ("dof_vel", 2e-2, 1e-3), ("rew_buf", 2e-4, 1e-3), ("torques", 5e-3, 1e-3),
       ("contact_forces", 5e-2, 1e-2))          # (the full-step force tolerance of tests/test_gpu_parity.py FULL_STEP_TOL)


def test_fp32_build_of_the_oracle_stays_within_the_parity_tolerances(oracle_lib):
    N, steps = 1024, 30
    cfg, S, meta, B64 = make_sim("train_noise", N, seed=11)
    randomize_dr(B64, 11)
    B64.enable_contact_signature()
    o64 = oracle_lib.Oracle(S, B64)
    o64.reset_idx()
    B64.episode_length_buf[:] = torch.randint(0, S.max_episode_length, (N,), dtype=torch.int32, generator=torch.Generator().manual_seed(2))
    B32 = B64.clone_to("cpu")
    o32 = oracle_lib.Oracle(S, B32, fp32=True)
    rng = np.random.default_rng(0)
    bad_total, worst, worst_force_flip, flips = 0, 0.0, 0.0, 0
    for step in range(steps):
        a = (rng.standard_normal((N, 12)) * (1.0 if step % 2 else 0.3)).astype(np.float32)
        o64.step(a)
        o32.step(a)
        ratio = torch.zeros(N, dtype=torch.float64)          # every quantity but the forces
        for k, tol, rt in TOL:
            d = (B32.tensors[k].double() - B64.tensors[k].double()).abs() / (tol + rt * B64.tensors[k].double().abs())
            d = d.reshape(-1, N).max(0).values
            if k == "contact_forces":
                force = d
            else:
                ratio = torch.maximum(ratio, d)
        bad = (ratio > 1.0) | (force > 1.0)
        bad_total += int(bad.sum())
        flip = (B32.contact_signature != B64.contact_signature).any(0)
        worst = max(worst, float(ratio.max()), float(force[~flip].max()))
        worst_force_flip = max(worst_force_flip, float(force[flip].max()) if bool(flip.any()) else 0.0)
        flips += int(flip.sum())
        for k, t in B64.tensors.items():           # re-synchronise: one step is compared at a time
            if t is not None and B32.tensors.get(k) is not None:
                B32.tensors[k].copy_(t)
        o32.ctr.common_step_counter, o32.ctr.lag_head, o32.ctr.history_slot = o64.ctr.common_step_counter, o64.ctr.lag_head, o64.ctr.history_slot
    rate = bad_total / (N * steps)
    print(f"fp32 oracle vs fp64 oracle: {N * steps} env-steps, {bad_total} outside the tolerances (rate {rate:.1e}), worst x{worst:.1f}, "
          f"{flips} contact-set flips (forces there: worst x{worst_force_flip:.1f})")
    assert float(B64.contact_forces.abs().max()) > 50.0 and int(B64.reset_buf.sum()) >= 0
    # x50 (the hardware suite's ATTRIBUTED_BOUND) for every quantity in every environment-step, and for the forces wherever both builds list the
    # same contact and active sets; where they do not, a contact impulse enters or leaves the net force of a body, and the FORCES alone get the
    # suite's bound for that case, RULE_A_BOUND = x500 (the one such step of this run: x90 of 5e-2 N + 1 %, x2 in everything else; at 512
    # environments, where the force tolerance was measured, there is none)
    assert rate <= 1e-3 and worst <= 50.0 and worst_force_flip <= 500.0, (rate, worst, worst_force_flip)


def env_ratio(Bx, Bref, tols, N):
    ratio = torch.zeros(N, dtype=torch.float64)
    for k, tol, rt in tols:
        d = (Bx.tensors[k].double() - Bref.tensors[k].double()).abs() / (tol + rt * Bref.tensors[k].double().abs())
        ratio = torch.maximum(ratio, d.reshape(-1, N).max(0).values)
    return ratio


@pytest.mark.parametrize("walls", [False, True])
def test_fp32_build_of_the_oracle_on_the_relief(oracle_lib, walls):
    """The same measurement on the relief of the parity tests (rough_field(seed=2), height scan observed; walls: vertical risers), with the
    relief's tolerances, contact forces included: the fp32 oracle leaves them at a rate within RULE_BC_RATE = 4e-3 — the budget the hardware
    suite grants precision — and the force tolerance ALONE (everything else inside) in at most 1e-3 of the environment-steps: 0.5 N was chosen
    for that (with 5e-2 N: 22 of 15,360 without walls, 8 with)."""
    from test_gpu_parity import RELIEF_TOL, RULE_BC_RATE, relief_pair          # (helpers and constants only: that module's tests need the GPU)
    N, steps = 512, 30
    S, B64, o64 = relief_pair(walls, N)
    B32 = B64.clone_to("cpu")
    o32 = oracle_lib.Oracle(S, B32, fp32=True)
    rng = np.random.default_rng(0)
    rest = tuple(t for t in RELIEF_TOL if t[0] != "contact_forces")
    force = tuple(t for t in RELIEF_TOL if t[0] == "contact_forces")
    assert force == (("contact_forces", 0.5, 1e-2),) and RULE_BC_RATE == 4e-3
    bad_total = force_only = 0
    peak = side = 0.0
    for step in range(steps):
        a = (rng.standard_normal((N, 12)) * (1.0 if step % 2 else 0.3)).astype(np.float32)
        o64.step(a)
        o32.step(a)
        r_rest, r_force = env_ratio(B32, B64, rest, N), env_ratio(B32, B64, force, N)
        differ = B32.reset_buf.bool() != B64.reset_buf.bool()
        bad_total += int(((r_rest > 1.0) | (r_force > 1.0) | differ).sum())
        force_only += int(((r_force > 1.0) & (r_rest <= 1.0) & ~differ).sum())
        cf = B64.contact_forces.view(17, 3, N)
        peak, side = max(peak, float(cf[:, 2].max())), max(side, float(cf[:, :2].abs().max()))
        for k, t in B64.tensors.items():           # re-synchronise: one step is compared at a time
            if t is not None and B32.tensors.get(k) is not None:
                B32.tensors[k].copy_(t)
        o32.ctr.common_step_counter, o32.ctr.lag_head, o32.ctr.history_slot = o64.ctr.common_step_counter, o64.ctr.lag_head, o64.ctr.history_slot
    n = N * steps
    print(f"fp32 oracle vs fp64 oracle on the relief (walls={walls}): {n} env-steps, {bad_total} outside the tolerances (rate {bad_total / n:.1e}), "
          f"{force_only} outside the force tolerance alone (rate {force_only / n:.1e}); largest normal force {peak:.0f} N, horizontal {side:.0f} N")
    assert peak > 50.0 and side > 0.5
    assert bad_total / n <= 4e-3, (bad_total, n)
    assert force_only / n <= 1e-3, (force_only, n)
