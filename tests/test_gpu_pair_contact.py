"""The pair contacts of the HIP substep (physics_substep of csrc/wbc_step_kernel.hip, through wbc_simulate_kernel and wbc_step_kernel) held
to the fp64 statements of tests/pair_contact_reference.py: which rigid-body rows may carry a force and that a lone pair's two rows are
minus each other bit for bit (exactly), the velocity-level law of every single-contact env (a limb pair or an arm sphere against the
trunk box: the law iterated through the spec's four block-Jacobi sweeps; a robot sphere against the free box or a box corner against the
terrain: the converged law), friction cone and sign, the force sensor of a foot pushed by the box or by another limb, every row of the
robot's equations of motion with J_rel^T f, the box's Newton-Euler rows and integrator, and the sleeping box bit for bit. Everything goes
through the C-ABI (helpers.make_gpu) with per-env randomised body parameters, friction (negative and > 1 draws included) and box mass. The
states, seeds and n are those tests/test_pair_contact.py runs through the C oracle on the CPU.

Cases: L one of 42 candidate limb pairs alone in contact (n = 1, 13, 264); T gripper tip or wrist against the trunk box (n = 96; face,
edge and corner regions, centre inside); B the free box against one of the 17 spheres that can touch it (n = 255; face, edge, corner, centre inside;
static and promoted slots); K the box alone on one corner over the plane / a rough grid (n = 128); S the sleeping box (n = 64, half of
them woken by a foot); M 256 tangled robots, a box at every third, two substeps (activation, cone, sensors, root rows, box rows with any number of
contacts); E wbc_step_kernel with decimation = 1 from the staged states of L and of B under 0.3-sigma actions (n = 13 and 2560).

Constants: C = 4 x K_ref rounded up to a power of two, K_ref the fp32 ORACLE's largest ratio on exactly these states (measured and
asserted on the CPU by tests/test_pair_contact.py, never taken from the kernel), capped at 1024. Every ratio is residual / (2^-24 scale).

    tier                                     K_ref     C    fp64 oracle   kernel's largest ratio on an MI355X (case, env)   kernel / K_ref
    velocity law (tree: W_u (f dt - lam_4))   2.86     16   0.053          2.12  (K-128, env 26)                             0.74
    cone / slide magnitude, sign of f.n       0.94      4   0.503          1.94  (M-256, second substep, env 90)             2.06
    slide direction                           0.572     4   0.203          0.592 (K-128-grid, env 123)                       1.04
    force sensors                             2.14     16   4e-09          2.23  (L-13, env 1)                               1.04
    root rows of the equations of motion      3.93     16   1e-08          2.86  (K-128, env 71)                             0.73
    joint rows                               14.81     64   2e-08         11.91  (E-2560-box, env 2460)                      0.80
    box Newton-Euler and integrator rows      5.69     32   7e-09          2.63  (S-64, env 49)                              0.46

K_ref sits on E-2560 env 2550 (velocity), T-96 env 73 (cone), K-128-grid env 123 (direction), E-2560 env 700 (sensors), K-128 env 74
(root rows), E-2560-box env 790 (joint rows), S-64 env 62 (box). Counts and classes: DESIGN.md section 3. Largest contraction
|1 - W_t W_u^-1|: 1.00.
The box row of NET_CONTACT_FORCE is the row reduction's sum itself, so a lone pair's two rows are exact negatives.
Case E runs decimation = 1; the step kernel's decimation loop (substeps 2 to 4 of a launch) is held by tests/test_gpu_step_decimation.py.
"""
import numpy as np
import pytest

import contact_law_reference as clr
import helpers
import pair_contact_reference as pcr

pytestmark = pytest.mark.gpu


class GpuAdapter:
    """WbcSim (the C-ABI) behind the load / set / simulate / step / get interface of pair_contact_reference."""

    def __init__(self, g):
        import torch
        self.g, self.torch = g, torch

    def get(self, name):
        self.torch.cuda.synchronize()
        return self.g.tensor(name).detach().cpu().numpy().astype(np.float64)

    def set(self, name, value):
        t = self.g.tensor(name)
        t.copy_(self.torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(t.dtype))

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


def _sim(robot, name):
    rb = pcr.case_robot(robot)
    case = pcr.CASES.get(name) or pcr.STEP_CASES[name]
    tc, ter = (pcr.case_states(rb, name) if name in pcr.CASES else pcr.step_states(rb, name))[:2]
    params = pcr.case_params(name)
    if case["n"] >= 64:
        assert (params["friction"] < 0).any() and (params["friction"] > 1).any()
    g = helpers.make_gpu(rb, case["n"], params, tcfg=tc)
    if ter is not None:
        g.set_heightfield(*clr.heightfield_args(ter))
    sim = GpuAdapter(g)
    if case["n"] > 1:
        bp = sim.get("BODY_PARAMS")
        assert np.ptp(bp[:, 0]) > 0 and np.ptp(bp[:, 10]) > 0 and np.ptp(sim.get("BOX_MASS")) > 0                # randomised per env
    return rb, g, sim, params


def _assert_within(name, s):
    """Every figure first, then: no exact requirement violated, every tier within its C, the caps and the coverage."""
    print(pcr.report(name + " kernel", s))
    assert s["exact"] == [], s["exact"][:8]
    for t in pcr.TIERS:
        assert s["worst"][t][0] <= pcr.bound(t), (name, t, s["worst"][t], pcr.bound(t))
    pcr.assert_caps_and_coverage(name, s)


@pytest.mark.parametrize("name", list(pcr.CASES))
def test_simulate_kernel_obeys_the_pair_contact_checks(robot, name):
    """wbc_simulate_kernel: cases L, T, B, K and S. In S-64 the bit-exact statements (pose unchanged, velocity and box row exactly 0, timer
    kept; woken: timer 0) are among the exact requirements."""
    rb, g, sim, params = _sim(robot, name)
    out, st = pcr.run_case(sim, rb, name, params)
    s = pcr.summarise(out)
    _assert_within(name, s)
    if name == "S-64":
        n = len(out)
        assert np.array_equal(st["root1"][: n // 2, 1, 0:7], st["root0"][: n // 2, 1, 0:7]) and not np.any(st["root1"][: n // 2, 1, 7:13] != 0)
        assert not np.any(st["ncf"][: n // 2, pcr.BOX_ROW] != 0) and np.all(st["timer1"][: n // 2] == st["timer0"][: n // 2])
        assert np.all(st["timer1"][n // 2:] == 0)
    g.close()


@pytest.mark.parametrize("name", list(pcr.STEP_CASES))
def test_step_kernel_obeys_the_pair_contact_checks(robot, name):
    """wbc_step_kernel with decimation = 1 (one substep per step). Envs that reset in the step are left out; the step counter keeps the
    push away; n = 2560: every tenth env plus the last."""
    rb, g, sim, params = _sim(robot, name)
    n = pcr.STEP_CASES[name]["n"]
    out, _ = pcr.run_step(sim, rb, name, params)
    s = pcr.summarise(out)
    _assert_within(name, s)
    assert s["n"] == (n if n <= 256 else n // 10 + 1) and s["single"] >= 0.8 * s["n"]
    g.close()
