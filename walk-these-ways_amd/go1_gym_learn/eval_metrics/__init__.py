"""Evaluation of trained policies: the reference's metric functions and domain-randomisation presets under their own names
(`metrics.METRICS_FNS`, `domain_randomization.DR_SETTINGS`), and `sweep.run_sweep`, which measures the ten scalar metrics on
the device (include/go1eval.h) over a grid of commands.  `behaviour` adds the second table: gait and behaviour tracking
(`BEHAVIOUR_FNS`, `StrideTracker`, `run_behaviour_sweep`) over a product of the other commands' values.  `response` measures the
step response to a command switch from a trace recorded on the device, `recovery` the recovery from a push (`run_push_sweep`), `terrain`
which tiles of a generated terrain a policy crosses, and how (`run_terrain_sweep`), `joints` how every joint's actuator is used
(`joint_terms`, `run_joint_sweep`, `plot_envelope`), `feet` what every foot puts into the ground (`foot_terms`, `run_foot_sweep`, `plot_grf`;
include/go1feet.h), `trunk` what the trunk does: tilt, accelerations, support margin and path drift (`trunk_terms`, `run_trunk_sweep`,
`plot_tilt`; include/go1trunk.h), `gait` how the legs move relative to one another and which gait that is (`run_gait_sweep`, `classify`,
`plot_gait`; include/go1gait.h), `spectrum` where in frequency the actions, torques, joint speeds and trunk rates carry their energy
(`run_spectrum_sweep`, `gait_locked`, `plot_spectrum`; include/go1spectrum.h), `placement` where every foot lands against its nominal stance
point and the Raibert heuristic's target, and the stride length and track width the robot realises (`placement_errors`, `run_placement_sweep`,
`plot_footprints`; include/go1place.h), `episodes` what whole episodes come to: return, length, time to a fall, distance and the survival
curve with the episodes still open as censored observations (`run_episode_sweep`, `kaplan_meier`, `episode_to_json`,
`episode_markdown_table`, `plot_survival`; include/go1episode.h), `sensitivity` how a policy holds up as the randomised dynamics move:
exposure, falls, tracking errors and power per bin of friction, restitution, payload, centre-of-mass displacement and motor strength
(`run_sensitivity_sweep`, `hazard`, `wilson`, `effect`, `rank_parameters`, `plot_sensitivity`; include/go1sens.h), `observations` what the
policy is fed: moments, histogram, tails, clip share and step-to-step change of every observation column, and how two such profiles differ
(`run_observation_sweep`, `channel_names`, `profile`, `profile_from_array`, `shift`, `rank_channels`, `plot_observations`; include/go1obs.h)."""
