"""The HIP substep (physics_substep of csrc/wbc_step_kernel.hip, through wbc_simulate_kernel and wbc_step_kernel) held to the fp64
equations of motion, row by row: tests/forward_dynamics_reference.py puts the state the kernel stored before and after a substep
into  ID_ref(q0, nu0, a) + armature a - (0, tau + t_limit) - sum J_foot^T wrench  and every live row of every eligible env has to
satisfy |res_k| <= C 2^-24 scale_k. Everything goes through the C-ABI (helpers.make_gpu) with per-env randomised body parameters,
the box parked 50 m away. The states, seeds and n are those tests/test_forward_dynamics.py runs through the C oracle on the CPU.

Constants: C = 4 x K_ref rounded up to a power of two, K_ref the fp32 ORACLE's largest ratio on exactly these states (measured and
asserted on the CPU by tests/test_forward_dynamics.py, never taken from the kernel), capped at 1024.

    family                          K_ref    C     kernel's largest ratio on an MI355X     kernel / K_ref
    airborne (n = 1, 13, 256)        6.61    32    6.84                         1.03
    feet in contact (3 substeps)     9.51    64    12.24                          1.29
    limit stop                       5.01    32    3.90                            0.78
    step kernel (decimation = 1)    14.06    64    16.66                             1.18
    integrator (all of the above)    3.82    16    2.94                            0.77

The kernel's maxima all sit on row 21 (the forearm roll, the lightest joint of the tree): airborne-256 env 84; contact-256 third
substep env 167; limit-128 env 88; step-2560 fourth step env 1770. No row comes closer to its C than a factor of 3.8.
The step kernel runs decimation = 1 here; its decimation loop (substeps 2 to 4 of a launch) is held by tests/test_gpu_step_decimation.py.
"""
import numpy as np
import pytest

import forward_dynamics_reference as fdr
import helpers

pytestmark = pytest.mark.gpu

LIVE, FINGERS = fdr.LIVE, fdr.FINGERS


class GpuAdapter:
    """WbcSim (the C-ABI) behind the load / simulate / step / get interface of forward_dynamics_reference."""

    def __init__(self, g):
        import torch
        self.g, self.torch = g, torch

    def get(self, name):
        self.torch.cuda.synchronize()
        return self.g.tensor(name).detach().cpu().numpy().astype(np.float64)

    def load(self, root, dof, tau):
        self.g.tensor("ROOT_STATES").copy_(self.torch.from_numpy(root))
        self.g.tensor("DOF_STATE").copy_(self.torch.from_numpy(dof))
        self.g.set_dof_forces(self.torch.from_numpy(tau).cuda())

    def simulate(self):
        self.g.simulate()

    def reset_all(self):
        self.g.reset_all()

    def set_step_counter(self, v):
        self.g.step_counter = v

    def step(self, a):
        self.g.step(self.torch.from_numpy(a).cuda())


def _assert_within(name, family, outs, envs=None):
    """Element-wise bound, eligibility caps, finger rows, coverage of the rows, integrator."""
    C, C_int = fdr.bound(family), fdr.bound("integrator")
    n = len(outs[0]["elig"])
    envs = list(range(n)) if envs is None else envs
    worst = worst_int = 0.0
    for i, o in enumerate(outs):
        elig = np.zeros(n, bool)
        elig[envs] = o["elig"][envs]
        assert elig.sum() >= fdr.MIN_ELIGIBLE[family] * len(envs), (name, i, int(elig.sum()))
        r, s = o["ratio"][elig], o["scale"][elig]
        assert np.isfinite(s).all() and not np.isnan(r).any()
        assert np.all(r[:, FINGERS] == 0) and np.all(s[:, FINGERS] == 0)              # the locked fingers do not move
        assert np.all(s[:, LIVE].max(axis=0) > 0)                                     # every live row is exercised
        integ = o["integ"][envs]
        worst, worst_int = max(worst, float(r[:, LIVE].max())), max(worst_int, float(integ.max()))
        e, k = np.unravel_index(np.argmax(r[:, LIVE]), r[:, LIVE].shape)
        print(f"{name} substep {i}: {int(elig.sum())} of {len(envs)} eligible, {o['contacts']} foot contacts, largest |res| / (2^-24 scale) "
              f"= {r[:, LIVE].max():.3f} (env {np.flatnonzero(elig)[e]}, row {LIVE[k]}), integrator {integ.max():.3f}")
    for i, o in enumerate(outs):
        elig = np.zeros(n, bool)
        elig[envs] = o["elig"][envs]
        r = o["ratio"][elig][:, LIVE]
        bad = np.argwhere(r > C)
        assert bad.size == 0, (f"{name} substep {i}: {len(bad)} rows beyond C = {C}: " +
                               "; ".join(f"env {np.flatnonzero(elig)[e]} row {LIVE[k]}: {r[e, k]:.1f}" for e, k in bad[:8]))
        assert np.all(o["integ"][envs] <= C_int), (name, i, float(o["integ"][envs].max()))
    if family == "contact":
        assert sum(o["contacts"] for o in outs) >= n
    if family in ("airborne", "limit"):
        assert all(o["contacts"] == 0 for o in outs)
    return worst, worst_int


@pytest.mark.parametrize("family,name,n,seed,gravity,substeps", fdr.SUBSTEP_CASES, ids=[c[1] for c in fdr.SUBSTEP_CASES])
def test_simulate_kernel_satisfies_the_equations_of_motion(robot, family, name, n, seed, gravity, substeps):
    """wbc_simulate_kernel: airborne (one case under a tilted gravity), feet in contact over three consecutive substeps (each
    checked from the kernel's own previous state; friction from the randomised range, clamped values included), joints beyond
    their limits with both signs of approach."""
    tc = fdr.with_cfg(robot["tcfg"], gravity=gravity)
    params = helpers.random_env_params(n, seed=seed)
    g = helpers.make_gpu(robot, n, params, tcfg=tc)
    sim = GpuAdapter(g)
    bp = sim.get("BODY_PARAMS")
    if n > 1:
        assert np.ptp(bp[:, 0]) > 0 and np.ptp(bp[:, 1:4], axis=0).max() > 0 and np.ptp(bp[:, 10]) > 0     # randomised per env
    if family == "contact":
        assert (params["friction"] < 0).any() and (params["friction"] > 1).any()
    root, dof, tau = fdr.case_states(family, robot["wmodel"], tc, n, seed)
    outs = fdr.run_substeps(sim, robot["model"], robot["wmodel"], tc, family, root, dof, tau, substeps)
    _assert_within(name, family, outs)
    g.close()


@pytest.mark.parametrize("n,seed", fdr.STEP_CASES, ids=[f"step-{n}" for n, _ in fdr.STEP_CASES])
def test_step_kernel_satisfies_the_equations_of_motion(robot, n, seed):
    """wbc_step_kernel with decimation = 1 (one substep per step, its torques in TORQUES): five steps from reset_all under
    0.6-sigma actions; n = 13 (the grid is rounded up to 8) and n = 2560 (the envs are dealt to the XCDs from 2048 on; every tenth
    env plus the last is checked). Envs that reset in a step are left out; the step counter keeps the push away. Five steps from
    the spawn height of 0.42 m end before a foot reaches the ground: 0 foot contacts are expected here, the tier is the step
    kernel's airborne substep under the PD torques of its own torque stage; contact is held through wbc_simulate_kernel."""
    tc = fdr.with_cfg(robot["tcfg"], decimation=1)
    g = helpers.make_gpu(robot, n, helpers.random_env_params(n, seed=seed), tcfg=tc)
    envs = fdr.step_envs(n)
    assert envs[-1] == n - 1 and (n <= 256 or len(envs) == n // 10 + 1)
    outs = fdr.run_steps(GpuAdapter(g), robot["model"], robot["wmodel"], tc, fdr.step_actions(n, seed), envs)
    _assert_within(f"step-{n}", "step", outs, envs)
    g.close()


def test_velocity_clamp(robot):
    """Arm torques of 10 N m take the wrist joints beyond pi rad/s within one substep. Where the fp64 unclamped prediction
    qd0 + dt a_ref is beyond the limit by more than 1 % the stored velocity is bit-exactly +-qd_limit; where it is inside by more
    than 1 % the stored velocity is inside; q1 = q0 + dt qd1 with the CLAMPED velocity, to the integrator's bound. The other
    joints of such an env are not held to the equations of motion (the clamp removes momentum)."""
    n = fdr.CLAMP_CASE["n"]
    g = helpers.make_gpu(robot, n, helpers.random_env_params(n, seed=fdr.CLAMP_CASE["seed"]))
    clamped, free, stored, limit, integ = fdr.clamp_check(GpuAdapter(g), robot["model"], robot["wmodel"], robot["tcfg"])
    print(f"velocity clamp: {int(clamped.sum())} joints of {int(clamped.any(1).sum())} envs predicted beyond the limit, "
          f"integrator {integ.max():.3f}")
    assert clamped.sum() >= n and clamped[:, 12:18].any(0).sum() >= 4
    assert np.all(stored[clamped] == limit[clamped])
    bounded = free & (limit != 0)
    assert np.all(np.abs(stored[bounded]) < np.abs(limit[bounded]))
    assert np.all(integ <= fdr.bound("integrator"))
    g.close()
