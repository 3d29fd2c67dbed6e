"""The contact stage of the HIP substep (physics_substep of csrc/wbc_step_kernel.hip, through wbc_simulate_kernel and wbc_step_kernel)
held to the fp64 contact law of tests/contact_law_reference.py: which spheres may carry a force (exactly), the velocity-level law of
every single-contact env (separating / stick / slide / frictionless fallback, classified in fp64), the friction cone and the sign of
every foot's force, the force sensors, and the root rows of the equations of motion (the size of the force). Everything goes through
the C-ABI (helpers.make_gpu) with per-env randomised body parameters and friction (negative and > 1 draws included), the box parked
50 m away in the air. The states, seeds and n are those tests/test_contact_law.py runs through the C oracle on the CPU.

Cases: A plane, one foot (n = 1, 13, 256); B plane, one of the 20 other spheres that can touch a plane alone (n = 192, joints over
their whole range); C a rough int16 height grid translated by 20 m, one foot, knee or mid-shank (n = 256; 12 % of the spheres within
1e-3 cell of a border or the diagonal, 15 % beyond the grid's edge); D fdr.contact_states, two to four feet down, three consecutive
substeps (activation, cone, sensors, linear momentum); E wbc_step_kernel with decimation = 1 from the staged states of A and C under
0.6-sigma actions (n = 13: the grid is rounded up to 8; n = 2560: the envs are dealt to the XCDs, every tenth env plus the last).

Constants: C = 4 x K_ref rounded up to a power of two, K_ref the fp32 ORACLE's largest ratio on exactly these states (measured and
asserted on the CPU by tests/test_contact_law.py, never taken from the kernel), capped at 1024. Every ratio is residual / (2^-24 scale).

    tier                                   K_ref     C    fp64 oracle   kernel's largest ratio on an MI355X (case, env)
    velocity law (n.v+, stick: v+)         16.09    128   0.374         10.92  (B-192, env 182)
    cone / slide magnitude, sign of f.n     1.89      8   0.461          1.15  (D-256, first substep, env 100)
    slide direction                         1.21      8   0.444          0.67  (C-256, env 151)
    force sensors                           3.02     16   6.4e-09        3.28  (E-2560, env 1130)
    momentum (root rows, size of f)         3.15     16   7.3e-09        6.21  (A-256, env 150)

K_ref sits on A-256 env 114 (velocity: a speculative contact that closes at 0.92 m/s), D-256 env 49 (cone), A-256 env 126 (direction),
D-256 env 67 (sensors), B-192 env 63 (momentum). No exact requirement is violated by either oracle or by the kernel, and no kernel
ratio comes closer to its C than a factor of 2.6 (momentum), 4.9 (sensors), 7 (cone) and 11.7 (velocity, direction).

Counts per class (checked single-contact envs; separating / stick / slide / fallback; mu = 0; vn_tgt speculative / erp / cap), the same
on the fp64 oracle, the fp32 oracle and the kernel: A-256 54 / 113 / 89 / 0, 32, 53 / 139 / 64; B-192 41 / 81 / 67 / 0, 17, 78 / 83 / 28;
C-256 54 / 86 / 106 / 1, 23, 99 / 108 / 40 (triangles 121 / 126, 28 clipped indices; 7 envs left out for a velocity clamp, 2 for a
cell border). The step tier, the same on all three: E-2560 82 / 63 / 104 / 0 of 249 checked (8 left out for a velocity clamp),
E-2560-grid 72 / 41 / 121 / 1 of 235 (22 left out). No env of any case sits in a decision band or at the margin. The frictionless
fallback is produced once per grid case by the fp64 oracle and by the kernel alike (reported, not asserted as a count).
Case E runs decimation = 1; the step kernel's decimation loop (substeps 2 to 4 of a launch) is held by tests/test_gpu_step_decimation.py.
"""
import numpy as np
import pytest

import contact_law_reference as clr
import helpers

pytestmark = pytest.mark.gpu

SINGLE = [k for k, c in clr.CASES.items() if c["kind"] == "single"]


class GpuAdapter:
    """WbcSim (the C-ABI) behind the load / simulate / step / get interface of contact_law_reference."""

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


def _sim(robot, name):
    case = clr.CASES.get(name) or clr.STEP_CASES[name]
    tc, ter = (clr.case_states(robot, name) if name in clr.CASES else clr.step_states(robot, name))[:2]
    params = helpers.random_env_params(case["n"], seed=case["seed"])
    if case["n"] > 1:
        assert (params["friction"] < 0).any() and (params["friction"] > 1).any()
    g = helpers.make_gpu(robot, case["n"], params, tcfg=tc)
    if ter is not None:
        g.set_heightfield(*clr.heightfield_args(ter))
    sim = GpuAdapter(g)
    if case["n"] > 1:
        bp = sim.get("BODY_PARAMS")
        assert np.ptp(bp[:, 0]) > 0 and np.ptp(bp[:, 1:4], axis=0).max() > 0 and np.ptp(bp[:, 10]) > 0     # randomised per env
    return g, sim, params


def _assert_within(name, s):
    """Every figure first, then: no exact requirement violated, every tier within its C, eligibility, what may be left out, coverage."""
    print(clr.report(name + " kernel", s))
    assert s["exact"] == [], s["exact"][:8]
    for t in clr.TIERS:
        assert s["worst"][t][0] <= clr.bound(t), (name, t, s["worst"][t], clr.bound(t))
    assert s["checked"] >= clr.MIN_ELIGIBLE * s["n"], (name, s["checked"], s["n"], s["left_out"])
    assert s["left_out"].get("border", 0) <= clr.MAX_LEFT_OUT * s["n"] and s["near"] <= clr.MAX_LEFT_OUT * max(s["n"], 50)
    if name in SINGLE:
        assert s["left_out"].get("margin", 0) == 0 and s["left_out"].get("self", 0) == 0
        assert s["single"] == s["checked"]
    if name in clr.COVERED:
        assert min(s["classes"][c] for c in ("separating", "stick", "slide")) >= clr.MIN_COUNT, s["classes"]
        assert s["mu0"] >= clr.MIN_COUNT and min(s["branches"]) >= clr.MIN_COUNT, (s["mu0"], s["branches"])
    if name == "C-256":
        assert min(s["tri"]) >= clr.MIN_COUNT and s["clipped"] >= clr.MIN_COUNT, (s["tri"], s["clipped"])


@pytest.mark.parametrize("name", list(clr.CASES))
def test_simulate_kernel_obeys_the_contact_law(robot, name):
    """wbc_simulate_kernel: tiers A to D, each substep checked from the kernel's own previous state."""
    g, sim, params = _sim(robot, name)
    outs, _ = clr.run_case(sim, robot, name, params["friction"])
    s = clr.summarise(outs)
    _assert_within(name, s)
    if name == "D-256":
        assert s["single"] == 0 and s["worst"]["sensor"][0] > 0                 # feet on the ground, their sensors live
    g.close()


@pytest.mark.parametrize("name", list(clr.STEP_CASES))
def test_step_kernel_obeys_the_contact_law(robot, name):
    """wbc_step_kernel with decimation = 1 (one substep per step): tier E. Envs that reset in the step are left out; the step counter
    keeps the push away."""
    g, sim, params = _sim(robot, name)
    n = clr.STEP_CASES[name]["n"]
    envs = clr.step_envs(n)
    assert envs[-1] == n - 1 and (n <= 256 or len(envs) == n // 10 + 1)
    outs, _ = clr.run_step(sim, robot, name, params["friction"])
    s = clr.summarise(outs)
    _assert_within(name, s)
    assert s["n"] == len(envs) and s["left_out"].get("reset", 0) <= 0.05 * s["n"] and s["single"] >= 0.8 * s["n"]
    g.close()
