"""An asset loaded from the URDF by wbc_asset_load_urdf drives the existing kernels exactly as the packaged asset does, and edits of
the URDF reach them: a heavier trunk in the mass matrix and the trajectory, a changed effort limit in the torque clip."""
import ctypes as C
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

from wbc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URDF = os.path.join(ROOT, "tests", "golden", "widowGo1.urdf")
N = 4096


def _edited(tmp_path, name, anchor, old, new):
    text = open(URDF).read()
    j = text.index(old, text.index(anchor))
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write(text[:j] + new + text[j + len(old):])
    return p


def _packaged():
    """wbc_model, wbc_task_cfg and the curriculum after the first update, read from the packaged .wbcasset (include/wbc_sim.h)."""
    with open(abi.DEFAULT_ASSET, "rb") as f:
        raw = f.read()
    off = 30                                                                 # magic + the five header words
    model = abi.WbcModel.from_buffer_copy(raw, off)
    off += C.sizeof(abi.WbcModel)
    cfg = abi.WbcTaskCfg.from_buffer_copy(raw, off)
    off += C.sizeof(abi.WbcTaskCfg) + C.sizeof(abi.WbcCurriculum)
    return model, cfg, abi.WbcCurriculum.from_buffer_copy(raw, off)


def _sim(model, cfg, cur, n=N, seed=11):
    from wbc_amd.sim import WbcSim
    sim = WbcSim(model, cfg, n, torch.device("cuda:0"), seed=seed)
    sim.set_curriculum(cur)
    zeros = np.zeros(n, dtype=np.float32)
    sim.set_env_params(base_dmass=zeros, base_dcom=np.zeros((n, 3), dtype=np.float32), gripper_dmass=zeros)
    sim.reset_all()
    return sim


def _run(sim, steps, seed=3, actions=None):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    for _ in range(steps):
        a = actions if actions is not None else torch.randn(sim.num_envs, abi.NACT, device="cuda", generator=g) * 0.5
        sim.step(a.contiguous())
    torch.cuda.synchronize()


def _dynamics(sim):
    n, ncol = sim.num_envs, 6 + abi.NDOF
    J = torch.empty(n, abi.NRB, 6, ncol, dtype=torch.float32, device="cuda")
    M = torch.empty(n, ncol, ncol, dtype=torch.float32, device="cuda")
    sim.body_dynamics(jac=J, mm=M)
    torch.cuda.synchronize()
    return J, M


@pytest.mark.gpu
def test_urdf_asset_drives_the_kernels_bit_identically():
    model, cfg, cur = _packaged()
    u = abi.load_urdf_asset(URDF, template=abi.DEFAULT_ASSET)
    a, b = _sim(model, cfg, cur), _sim(u.model, u.task_cfg, u.curricula[1])
    _run(a, 50)
    _run(b, 50)
    for name in abi.TENSOR_IDS:
        ta, tb = a.tensor(name), b.tensor(name)
        assert torch.equal(ta.contiguous().view(torch.uint8), tb.contiguous().view(torch.uint8)), name
    Ja, Ma = _dynamics(a)
    Jb, Mb = _dynamics(b)
    assert torch.equal(Ja.view(torch.uint8), Jb.view(torch.uint8)) and torch.equal(Ma.view(torch.uint8), Mb.view(torch.uint8))
    assert torch.isfinite(Ja).all() and torch.isfinite(Ma).all()
    a.close()
    b.close()


@pytest.mark.gpu
def test_heavier_trunk_reaches_mass_matrix_and_trajectory(tmp_path):
    path = _edited(tmp_path, "heavy.urdf", '<link name="trunk">', '<mass value="5.204"/>', '<mass value="7.204"/>')
    root = ET.parse(path).getroot()
    total = sum(float(le.find("inertial/mass").attrib["value"]) for le in root.findall("link") if le.find("inertial") is not None)
    assert abs(total - (14.150879 + 2.0)) < 1e-9
    model, cfg, cur = _packaged()
    h = abi.load_urdf_asset(path, template=abi.DEFAULT_ASSET)
    heavy = _sim(h.model, h.task_cfg, h.curricula[1], n=1024)
    bp = heavy.tensor("BODY_PARAMS").cpu().numpy()
    np.testing.assert_allclose(bp[:, 0], h.model.base_rest_mass + h.model.base_piece_mass, rtol=1e-6)   # the per-env deltas are zero
    _, M = _dynamics(heavy)
    Mt = M[:, 0:3, 0:3].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(Mt, np.broadcast_to(total * np.eye(3), Mt.shape), rtol=0, atol=4e-6 * total)
    plain = _sim(model, cfg, cur, n=1024)
    _run(heavy, 20)
    _run(plain, 20)
    ra, rb = heavy.tensor("ROOT_STATES")[:, 0].cpu().numpy(), plain.tensor("ROOT_STATES")[:, 0].cpu().numpy()
    assert np.isfinite(ra).all() and np.abs(ra - rb).max() > 1e-4
    heavy.close()
    plain.close()


@pytest.mark.gpu
def test_edited_effort_limit_clips_the_torques(tmp_path):
    path = _edited(tmp_path, "effort.urdf", '<joint name="FR_calf_joint"', 'effort="23.7"', 'effort="12.5"')
    u = abi.load_urdf_asset(path, template=abi.DEFAULT_ASSET)
    j = u.dof_names.index("FR_calf_joint")
    lim = np.array([p.effort for p in u.dof_props], dtype=np.float32)
    assert lim[j] == np.float32(12.5) and np.float32(u.task_cfg.torque_limits[j]) == np.float32(12.5)
    sim = _sim(u.model, u.task_cfg, u.curricula[1], n=1024)
    sign = torch.where(torch.arange(1024, device="cuda") % 2 == 0, 1.0, -1.0)[:, None]
    actions = (100.0 * sign).expand(1024, abi.NACT).contiguous()
    resets = []
    for _ in range(8):
        sim.step(actions)
        resets.append(sim.tensor("RESET_BUF").cpu().numpy() != 0)
    tau = sim.tensor("TORQUES").cpu().numpy()
    # the torques of the last step use the actions of two steps before (action_delay = 2, WG:1162-1168), and a reset clears that
    # FIFO: an env counts if it was not reset during the last four steps
    live = ~np.any(resets[-4:], axis=0)
    assert live.sum() > 64
    assert np.all(np.abs(tau) <= lim[None, :])
    assert np.all(np.abs(tau[live, j]) == np.float32(12.5))                  # clipped at exactly the new limit
    driven = [i for i in range(abi.NACT) if u.task_cfg.action_scale[i] != 0 and u.task_cfg.p_gains[i] != 0]
    assert j in driven and len(driven) >= 13
    for i in driven:
        assert np.all(np.abs(tau[live, i]) == lim[i]), u.dof_names[i]
    sim.close()
