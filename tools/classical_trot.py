"""Close the classical loop on flat ground: leg-odometry estimator -> gait planner -> convex centroidal MPC -> whole-body controller
(task QP) -> set_dof_forces -> simulate, every layer one HIP launch, and report what happened. Nothing here is tuned: the gains are the
defaults of BaseStateEstimator, FootstepPlanner, CentroidalMPC and whole_body_controller.

  python tools/classical_trot.py [--envs 64] [--seconds 4] [--speed 0.3] [--gait trot] [--detector] [--controller qp|leg] [--height H]
                                 [--attitude [--gyro-bias B]] [--ground] [--slip] [--friction MU]

Prints, once per simulated second and at the end: the share of envs still upright (trunk z axis within 0.5 rad of vertical and the trunk
above 0.15 m), the mean forward speed of the upright envs against the command, and the MPC / QP / planner status counts.

--detector (default off) puts the contact detector (env.contact_detector: momentum observer + wbc_sim_contact_detect) into the loop: the
estimator takes det.prob instead of the planner's schedule and the whole-body controller det.stance instead of planner.stance. It then
also prints how often det.contact agrees with env.get_foot_contacts() and the counts of EARLY / LATE foot-steps. Feeding the touchdown
events back into the planner's clock is not covered: the planner still swings and places the feet by its own schedule.

--controller leg (default qp) replaces the whole-body task QP by the leg controller (env.leg_controller: wbc_sim_leg_control), the layer the
MPC's source paper runs: stance legs push with mpc.forces (tau = -J^T f), swing legs follow planner.swing_ref by a Cartesian impedance
with the acceleration feed-forward, the arm holds its default posture; the stance weights are planner.contact, or det.prob with
--detector. It then prints the counts of the controller's info bits instead of the QP's status. --height H hands the MPC a reference
height of the centre of mass (default: the current one, so that nothing pulls a sagging trunk back up).

--attitude (default off) puts the attitude filter (env.attitude_estimator: wbc_sim_attitude_filter) into the loop on an IMU model
(env.imu: gyro noise 0.002 rad/s, accelerometer noise 0.05 m/s^2, a heading vector with noise 0.01, and --gyro-bias B rad/s on every
axis): the leg-odometry estimator takes att.quat, att.gyro and the IMU's accelerometer instead of the sim's true orientation and angular
velocity. The planner, the detector and the controllers keep reading the sim's quaternion. It then also prints, once per simulated
second, the tilt and heading errors of att.quat against the sim's quaternion and the bias error.

--ground (default off) puts the blind terrain estimate (env.ground_estimator: wbc_sim_ground_estimate) into the loop, on the planner's
contact (det.prob with --detector) and the estimator's position: the leg odometry takes gnd.ground as foot_height, the detector
gnd.ground and gnd.normal, the task QP gnd.normal, and with --height H the MPC's reference height is gnd.trunk[:, 0] + H, H above the
estimated plane under the trunk (without --height the MPC keeps the current height as before). It then also prints, once per simulated
second, the estimated slope and the error of the feet's clearance gnd.ground - est z against the truth (the plane: the foot sphere's
radius above z = 0, less the trunk's true height); the loop of estimator and plane has no absolute height, so only that difference means
anything.

--friction MU (default: the env's randomised draws) makes MU the coefficient that the step kernel's contact law applies between every
env's feet and the terrain: the law combines the env's WBC_T_FRICTION with the cfg's terrain_friction by their mean (DESIGN.md section
3), so every env's WBC_T_FRICTION is set to 2 MU - terrain_friction, through set_env_params.

--slip (default off) puts the slip detector and friction estimate (env.slip_detector: wbc_sim_slip_detect) into the loop, on the
planner's contact (det.prob with --detector), the estimator's velocity, att.gyro with --attitude, gnd.normal with --ground and the foot
forces (det.foot_forces with --detector, otherwise the sim's net contact forces on the feet): the leg odometry and the ground estimator
take slip.weight as contact and the task QP slip.mu as its friction coefficient. It then also prints, once per simulated second, the
share of stance foot-steps flagged as slipping so far and, over the upright envs with a MU_VALID foot, the median and the 90th
percentile of |mu_env - mu_true| / mu_true, mu_true the coefficient the contact law applies (MU with --friction)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=64)
ap.add_argument("--seconds", type=float, default=4.0)
ap.add_argument("--speed", type=float, default=0.3)
ap.add_argument("--gait", default="trot")
ap.add_argument("--settle", type=float, default=0.5, help="seconds of standing (gait stand) before the gait starts")
ap.add_argument("--detector", action="store_true", help="contact flags from proprioception instead of the planner's schedule")
ap.add_argument("--controller", choices=("qp", "leg"), default="qp", help="whole-body task QP, or the leg controller on the MPC's forces")
ap.add_argument("--height", type=float, default=None, help="reference height of the centre of mass for the MPC (default: the current one)")
ap.add_argument("--attitude", action="store_true", help="orientation and gyro for the leg odometry from the attitude filter on an IMU model")
ap.add_argument("--gyro-bias", type=float, default=0.0, help="constant gyro bias of the IMU model, rad/s on every axis (with --attitude)")
ap.add_argument("--ground", action="store_true", help="foot heights, normals and the MPC's reference height from the blind terrain estimate")
ap.add_argument("--slip", action="store_true", help="slip detector in the loop: its weight for the estimators, its mu for the task QP")
ap.add_argument("--friction", type=float, default=None, help="the foot-terrain friction coefficient of every env (default: the randomised draws)")
a = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import math  # noqa: E402
from collections import Counter  # noqa: E402

import torch  # noqa: E402

from wbc_amd import abi  # noqa: E402
from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
env.reset()
env.reset_buf.zero_()                                                              # no env.step() follows: nothing below is to be reset by a stale flag
n, dev = a.envs, env.device
est = env.base_state_estimator()
stand = env.gait_planner("stand", horizon=10)
walk = env.gait_planner(a.gait, period=0.5, duty=0.5, horizon=10)
mpc = env.centroidal_mpc(horizon=10)
zero = torch.zeros(n, 2, device=dev)
cmd = torch.tensor([[a.speed, 0.0]], device=dev).expand(n, 2).contiguous()
wz = torch.zeros(n, device=dev)
decimation = int(env.cfg.control.decimation)
steps, settle = int(round(a.seconds / env.dt)), int(round(a.settle / env.dt))
counts = dict(mpc=Counter(), qp=Counter(), no_safe=0, failed=0, leg=Counter())
ctl = env.leg_controller() if a.controller == "leg" else None
dets = {id(stand): env.contact_detector(planner=stand), id(walk): env.contact_detector(planner=walk)} if a.detector else None
agree, events, tau = [0, 0], dict(early=0, late=0, touchdown=0, liftoff=0), None
att = env.attitude_estimator() if a.attitude else None
imu = env.imu(gyro_bias=a.gyro_bias, gyro_noise=0.002, accel_noise=0.05, heading_noise=0.01, seed=2) if a.attitude else None
gnd = env.ground_estimator() if a.ground else None
terrain_mu = float(env.cfg.terrain.static_friction)
if a.friction is not None:
    env.sim.set_env_params(friction=[2.0 * a.friction - terrain_mu] * n)
mu_true = ((env.friction_coeffs_tensor.reshape(n).to(torch.float32) + terrain_mu) / 2).clamp(min=0.0)   # the contact law's coefficient
slip = env.slip_detector() if a.slip else None
slipped = [0, 0]
h_nominal = None
x_start = env.root_states[:, 0].clone()


def upright():
    q = env.root_states[:, 3:7]
    zz = 1 - 2 * (q[:, 0] ** 2 + q[:, 1] ** 2)                                         # R_22: the trunk's z axis against the world's
    return (zz > math.cos(0.5)) & (env.root_states[:, 2] > 0.15)


def report(label, k):
    up = upright()
    vx = env.root_states[:, 7][up].mean().item() if bool(up.any()) else float("nan")
    print(f"{label}: upright {float(up.float().mean()):.3f}, mean forward speed of the upright envs {vx:.3f} m/s (command {a.speed if k >= settle else 0.0:.2f}), "
          f"mean trunk height {env.root_states[:, 2].mean().item():.3f} m, travelled {float((env.root_states[:, 0] - x_start).mean()):.3f} m", flush=True)
    if att is not None:
        qe, qs = att.quat[up], env.root_states[:, 3:7][up]

        def zx(q):                                                                      # R^T z (the tilt) and the heading of R's x axis
            x, y, z, w = q.unbind(-1)
            return (torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1),
                    torch.atan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z)))
        (ze, he), (zs, hs) = zx(qe), zx(qs)
        tilt = torch.acos((ze * zs).sum(-1).clamp(-1, 1))
        head = torch.atan2(torch.sin(he - hs), torch.cos(he - hs)).abs()
        berr = (att.bias[up] - a.gyro_bias).abs().max(dim=-1).values
        stat = lambda t: f"mean {t.mean().item():.4f} max {t.max().item():.4f}" if t.numel() else "no upright env"
        print(f"    attitude of the upright envs: tilt error {stat(tilt)} rad, heading error {stat(head)} rad, bias error {stat(berr)} rad/s", flush=True)
    if gnd is not None and bool(up.any()):
        slope = gnd.plane[up][:, 3:5].norm(dim=1)
        gerr = ((gnd.ground - est.position[:, 2:3]) - (abi.FOOT_RADIUS - env.root_states[:, 2:3]))[up].abs()
        print(f"    ground estimate of the upright envs: slope mean {slope.mean().item():.4f} max {slope.max().item():.4f} (truth 0), error of the feet's "
              f"clearance below the trunk mean {gerr.mean().item() * 1e3:.2f} max {gerr.max().item() * 1e3:.2f} mm, |residual| max "
              f"{gnd.residual[up].abs().max().item() * 1e3:.2f} mm, estimator z - true z mean "
              f"{(est.position[:, 2] - env.root_states[:, 2])[up].mean().item() * 1e3:.2f} mm", flush=True)
    if slip is not None:
        have = up & (((slip.info >> 16) & 15) != 0)
        err = ((slip.mu_env[:, 0] - mu_true).abs() / mu_true.clamp(min=1e-6))[have]
        q = lambda p: f"{torch.quantile(err, p).item():.3f}" if err.numel() else "none"
        print(f"    slip: {slipped[0] / max(slipped[1], 1):.4f} of the stance foot-steps flagged ({slipped[0]} of {slipped[1]}); {int(have.sum())} upright envs "
              f"with MU_VALID, |mu_env - mu_true| / mu_true median {q(0.5)} 90 % {q(0.9)} (mu_true mean {mu_true.mean().item():.3f}, mu_env mean "
              f"{slip.mu_env[:, 0].mean().item():.3f})", flush=True)


planner = stand
for k in range(steps):
    if k == settle:
        planner = walk
        planner.reset()
        if a.detector:
            dets[id(walk)].reset()
        if gnd is not None and a.height is not None:
            h_nominal = a.height
    c = cmd if k >= settle else zero
    ekw = {}
    if att is not None:
        gyro, accel, heading = imu.read()
        att.update(gyro=gyro, accel=accel, aux=(heading, imu.heading_world, 0.05))
        ekw = dict(quat=att.quat, gyro=att.gyro, accel=accel)
    gkw, height = {}, a.height
    contact_in = dets[id(planner)].prob if a.detector else planner.contact            # of the step before
    if slip is not None:
        force = dets[id(planner)].foot_forces if a.detector else env.contact_forces[:, env.feet_indices, :]
        slip.update(contact_in, foot_force=force, normal=gnd.normal if gnd is not None and k > 0 else None, state=est,
                    gyro=att.gyro if att is not None else None)
        contact_in = slip.weight
        if k >= settle:
            stance_now = slip.last_inputs["contact"] >= slip.cfg.c_on
            slipped[0] += int((slip.slip.bool() & stance_now).sum()); slipped[1] += int(stance_now.sum())
    if gnd is not None:                                                                # on the contact and the position of the step before
        gnd.update(contact_in, base_pos=est.position)
        ekw["foot_height"] = gnd.ground
        gkw = dict(ground=gnd.ground, normal=gnd.normal)
        if h_nominal is not None:
            height = gnd.trunk[:, 0] + h_nominal
    if a.detector:
        det = dets[id(planner)]
        det.update(torques=tau, **gkw)                                                 # tau: what the last simulate calls applied (None at the start: env.torques)
        est.update(contact=slip.weight if slip is not None else det.prob, **ekw)
    else:
        est.update(contact=slip.weight if slip is not None else planner.contact, **ekw)
    planner.update(c, wz, state=est)
    mpc.solve(planner.contact_schedule, c, wz, height=height, foot_positions=planner.foot_positions, state=est)
    if ctl is not None:
        tau = ctl.update(forces=mpc.forces, swing_ref=planner.swing_ref, stance=det.prob if a.detector else planner.contact, state=est)
    else:
        tau, nudot, lam, info = env.whole_body_controller(base_acc=mpc.base_acc, swing_acc=planner.swing_acc,
                                                          stance=det.stance if a.detector else planner.stance,
                                                          normal=gnd.normal if gnd is not None else None,
                                                          **(dict(mu=slip.mu) if slip is not None else {}))
    env.sim.set_dof_forces(tau.contiguous())
    for _ in range(decimation):
        env.sim.simulate()
    counts["mpc"].update(mpc.status.cpu().tolist())
    if ctl is not None:
        word = ctl.info
        counts["leg"].update(dict(failed=int((word & 2 != 0).sum()), ff_singular=int(((word >> 8) & 15 != 0).sum()),
                                  saturated_leg=int(((word >> 12) & 15 != 0).sum()), saturated_arm=int(((word >> 16) & 1 != 0).sum())))
    else:
        counts["qp"].update(info["status"].cpu().tolist())
    counts["no_safe"] += int(((planner.info >> 4) & 15 != 0).sum())
    counts["failed"] += int((planner.info & 2 != 0).sum())
    if a.detector and k >= settle:
        up = upright()
        agree[0] += int((det.contact.bool() == env.get_foot_contacts())[up].sum()); agree[1] += 4 * int(up.sum())
        for name, shift in (("touchdown", 4), ("liftoff", 8), ("early", 12), ("late", 16)):
            events[name] += int(sum(((det.info >> (shift + i)) & 1).sum() for i in range(4)))
    if (k + 1) % int(round(1.0 / env.dt)) == 0:
        report(f"t = {(k + 1) * env.dt:.2f} s", k)
report("end", steps - 1)
second = (f"leg controller, env-steps with the bit: {dict(counts['leg'])}" if ctl is not None else
          f"QP status counts (0 optimal, 1 / 2 clamped): {dict(counts['qp'])}")
print(f"MPC status counts (0 ok, 1 iterations, 2 failed): {dict(counts['mpc'])}; {second}; "
      f"planner: {counts['no_safe']} env-steps with NO_SAFE, {counts['failed']} FAILED", flush=True)
if a.detector:
    print(f"detector: det.contact equals get_foot_contacts() in {agree[0] / max(agree[1], 1):.3f} of the upright foot-steps; foot-steps flagged "
          f"EARLY {events['early']}, LATE {events['late']}; TOUCHDOWN events {events['touchdown']}, LIFTOFF events {events['liftoff']}", flush=True)
