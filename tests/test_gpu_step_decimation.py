"""The decimation loop of wbc_step_kernel (csrc/wbc_step_kernel.hip: `for (t = 0; t < dec; ++t) { torque_pass; WSYNC;
physics_substep(..., t == dec - 1); }`) held to the one-substep fp64 tier, through the C-ABI (helpers.make_gpu) and the driver of
tests/decimation_reference.py. The fp64 tests of the substep (test_gpu_forward_dynamics.py, test_gpu_contact_law.py,
test_gpu_pair_contact.py, test_gpu_step_state.py) all run decimation = 1; the shipped configuration and bench.py run 4. Per case:

  R1  one step at decimation D leaves the same bits as D steps at decimation 1 under the same action on ROOT_STATES (both rows),
      DOF_STATE, TORQUES, NET_CONTACT_FORCE, FORCE_SENSOR, RIGID_BODY_STATE, BASE_LIN_VEL, BASE_ANG_VEL, BOX_SLEEP_TIMER and the
      increment of DROPPED_HITS: whatever substeps 2 .. D carry in LDS (the dyn_dirty restore of the per-body contact masks, the
      aliased IA / U / pA / c regions, q / qd for torque_pass, bxtimer, dropped) leaves no trace.
  R2  the same chain through wbc_simulate_kernel (set_dof_forces with the k-th step's TORQUES, simulate()), bit for bit after every
      link on ROOT_STATES, DOF_STATE, NET_CONTACT_FORCE, FORCE_SENSOR, BOX_SLEEP_TIMER: the substep of the simulate kernel, which
      the contact tiers A to D, M and S run through, is the step kernel's own.
  R3  every link of the decimation-1 chain within the existing C of the fp64 checkers (equations of motion and integrator, contact
      law, pair contacts, PD torques): substeps 2 .. D start from the kernel's own contact-rich states.
  and the transitions between consecutive links that the case has to exercise (decimation_reference.CASES: a dynamic slot on -> off
  and off -> on, a foot contact opening and closing, the box woken inside the launch), counted on the kernel's own chain from the
  fp64 restatement of its states, in at least 8 envs each.

The cases, seeds and n are those tests/test_step_decimation.py runs through the C oracle in both precisions (R1 and R2 hold bit for
bit there; the fp32 oracle stays within C / 4 on every link). The largest ratios per tier and link are printed; DESIGN.md section 4
lists them beside K_ref and C."""
import numpy as np
import pytest

import contact_law_reference as clr
import decimation_reference as dr
import helpers

pytestmark = pytest.mark.gpu


class GpuAdapter:
    """WbcSim (the C-ABI) behind the interface of decimation_reference.run."""

    def __init__(self, g):
        import torch
        self.g, self.torch = g, torch

    def get(self, name):
        self.torch.cuda.synchronize()
        return self.g.tensor(name).detach().cpu().numpy().astype(np.float64)

    def set(self, name, value):
        t = self.g.tensor(name)
        t.copy_(self.torch.from_numpy(np.ascontiguousarray(value, dtype=np.float64)).to(t.dtype))

    def set_torques(self, tau):
        self.g.set_dof_forces(self.torch.from_numpy(np.ascontiguousarray(tau, dtype=np.float32)).cuda())

    def simulate(self):
        self.g.simulate()

    def reset_all(self):
        self.g.reset_all()

    def set_step_counter(self, v):
        self.g.step_counter = v

    def step(self, a):
        self.g.step(self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda())


@pytest.mark.parametrize("name,D", dr.RUNS, ids=[f"{n}-D{d}" for n, d in dr.RUNS])
def test_one_step_at_D_is_D_steps_at_1(robot, name, D):
    sims = []

    def make(rb, tcfg, n, params, ter):
        g = helpers.make_gpu(rb, n, params, tcfg=tcfg)
        if ter is not None:
            g.set_heightfield(*clr.heightfield_args(ter))
        sims.append(g)
        return GpuAdapter(g)

    try:
        r = dr.run(make, robot, name, D)
    finally:
        for g in sims:
            g.close()
    dr.assert_case(name, D, "kernel", r, dr.check_r3(r))
