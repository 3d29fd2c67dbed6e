"""`WbcSim`: the torch-facing handle of one `wbc_sim` (include/wbc_sim.h). torch provides the
device arena, the stream and zero-copy tensor views; every computation is a kernel in libwbc_amd.so.

This is the layer that stands where `isaacgym.gymapi` + `gymtorch.wrap_tensor` stand in the
reference (legged_gym/envs/widowGo1/widowGo1.py:505-551)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import abi
from .native import check, lib

_TORCH_DT = {"f32": torch.float32, "i64": torch.int64, "u8": torch.uint8}


class SideJob:
    """A wbc_side_job plus the tensors it points into (kept alive until it has run)."""

    def __init__(self, L, keep):
        self.L, self.keep, self.c, self.done = L, keep, abi.WbcSideJob(), False

    def run(self, stream: int) -> None:
        """Stand-alone execution (nobody carried it)."""
        if not self.done:
            check(self.L.wbc_side_job_run(C.byref(self.c), stream), "wbc_side_job_run")
            self.done = True


class WbcSim:
    def __init__(self, model: abi.WbcModel, cfg: abi.WbcTaskCfg, num_envs: int, device: torch.device, seed: int = 1):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("WbcSim needs a ROCm device: the rollout step only exists as HIP kernels")
        if device.index is not None and device.index != torch.cuda.current_device():
            raise RuntimeError(f"WbcSim on {device} while torch's current device is cuda:{torch.cuda.current_device()}: call "
                               "torch.cuda.set_device(device) first (one process per GPU; the C-ABI launches on the caller's "
                               "current stream and does not switch devices behind torch's back)")
        self.L = lib()
        self.device = device
        self.num_envs = num_envs
        self.model, self.cfg = model, cfg
        nbytes = self.L.wbc_sim_arena_bytes(num_envs)
        self.arena = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        h = C.c_void_p()
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        check(self.L.wbc_sim_create(C.byref(model), C.byref(cfg), num_envs, dev_index, seed,
                                    self.arena.data_ptr(), nbytes, C.byref(h)), "wbc_sim_create")
        self.h = h
        self._views: Dict[str, torch.Tensor] = {}
        base = self.arena.data_ptr()
        for name in abi.TENSOR_IDS:
            p, shape, nd, dt = C.c_void_p(), (C.c_int64 * 4)(), C.c_int(), C.c_int()
            check(self.L.wbc_sim_get_tensor(self.h, abi.T[name], C.byref(p), shape, C.byref(nd), C.byref(dt)), "wbc_sim_get_tensor")
            dims = [int(shape[i]) for i in range(nd.value)]
            tdt = _TORCH_DT[["f32", "i64", "u8"][dt.value]]
            off = p.value - base
            nb = int(np.prod(dims)) * torch.empty((), dtype=tdt).element_size()
            self._views[name] = self.arena[off:off + nb].view(tdt).view(dims)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            torch.cuda.synchronize(self.device)
            self.L.wbc_sim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tensors ---------------------------------------------------------------------------
    def tensor(self, name: str) -> torch.Tensor:
        """Zero-copy view of a device tensor (names: abi.TENSOR_IDS)."""
        return self._views[name]

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- setup -----------------------------------------------------------------------------
    def set_env_params(self, friction=None, base_dmass=None, base_dcom=None, gripper_dmass=None, motor_strength=None,
                       env_origins=None, box_delta_y=None, traj_timesteps=None, traj_total_timesteps=None, box_dmass=None):
        n = self.num_envs
        keep = []

        def ptr(x, cols):
            if x is None:
                return None
            a = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(n * cols))
            keep.append(a)
            return a.ctypes.data
        torch.cuda.synchronize(self.device)
        check(self.L.wbc_sim_set_env_params(self.h, ptr(friction, 1), ptr(base_dmass, 1), ptr(base_dcom, 3), ptr(gripper_dmass, 1),
                                            ptr(motor_strength, 18), ptr(env_origins, 3), ptr(box_delta_y, 1),
                                            ptr(traj_timesteps, 1), ptr(traj_total_timesteps, 1), ptr(box_dmass, 1)),
              "wbc_sim_set_env_params")

    def set_curriculum(self, cur: abi.WbcCurriculum):
        check(self.L.wbc_sim_set_curriculum(self.h, C.byref(cur)), "wbc_sim_set_curriculum")

    def set_heightfield(self, heights: Optional[np.ndarray], hscale=0.0, vscale=0.0, tx=0.0, ty=0.0, tz=0.0):
        if heights is None:
            check(self.L.wbc_sim_set_heightfield(self.h, None, 0, 0, 0, 0, 0, 0, 0), "wbc_sim_set_heightfield")
            return
        h = np.ascontiguousarray(heights, dtype=np.int16)
        check(self.L.wbc_sim_set_heightfield(self.h, h.ctypes.data, h.shape[0], h.shape[1], hscale, vscale, tx, ty, tz),
              "wbc_sim_set_heightfield")

    @property
    def step_counter(self) -> int:
        v = C.c_int64()
        check(self.L.wbc_sim_get_step_counter(self.h, C.byref(v)))
        return v.value

    @step_counter.setter
    def step_counter(self, v: int):
        check(self.L.wbc_sim_set_step_counter(self.h, int(v)))

    # ---- stepping --------------------------------------------------------------------------
    def step(self, actions: torch.Tensor, obs_out: torch.Tensor = None, store=None) -> None:
        """One env step. obs_out (f32 [N, 860], contiguous, same device): write the observations there instead of OBS_BUF.
        store = (values f32 [N,2], gamma, out_rewards f32 [N,2], out_dones u8 [N,1] or [N]): also write this transition's
        rollout-storage reward (with the time-out bootstrap) and done slots (wbc_sim_step_rollout)."""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert actions.shape == (self.num_envs, abi.NACT)
        if obs_out is not None:
            assert (obs_out.is_cuda and obs_out.device == actions.device and obs_out.dtype == torch.float32 and obs_out.is_contiguous()
                    and obs_out.shape == (self.num_envs, abi.NOBS))
        if obs_out is None and store is None:
            check(self.L.wbc_sim_step(self.h, actions.data_ptr(), self._stream()), "wbc_sim_step")
        elif store is None:
            check(self.L.wbc_sim_step_to(self.h, actions.data_ptr(), obs_out.data_ptr(), self._stream()), "wbc_sim_step_to")
        else:
            values, gamma, rewards, dones = store
            n = self.num_envs
            assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.shape == (n, 2)
            assert rewards.is_cuda and rewards.dtype == torch.float32 and rewards.is_contiguous() and rewards.shape == (n, 2)
            assert dones.is_cuda and dones.dtype == torch.uint8 and dones.is_contiguous() and dones.numel() == n
            check(self.L.wbc_sim_step_rollout(self.h, actions.data_ptr(), obs_out.data_ptr() if obs_out is not None else None,
                                              values.data_ptr(), float(gamma), rewards.data_ptr(), dones.data_ptr(), self._stream()),
                  "wbc_sim_step_rollout")

    def reset_all(self) -> None:
        check(self.L.wbc_sim_reset_all(self.h, self._stream()), "wbc_sim_reset_all")

    def arm_dynamics(self, link_rb9, link_mass9):
        """(mm [N,6,6], ee Jacobian [N,6,6], gravity torques [N,6]) of the arm from the current state: what the
        reference reads from Isaac Gym's mass-matrix / Jacobian tensors (WG:550-558, 1201-1207)."""
        n = self.num_envs
        mm = torch.empty(n, 6, 6, dtype=torch.float32, device=self.device)
        jac = torch.empty(n, 6, 6, dtype=torch.float32, device=self.device)
        gt = torch.empty(n, 6, dtype=torch.float32, device=self.device)
        rb = (C.c_int * 9)(*[int(x) for x in link_rb9])
        ms = (C.c_float * 9)(*[float(x) for x in link_mass9])
        check(self.L.wbc_sim_arm_dynamics(self.h, rb, ms, mm.data_ptr(), jac.data_ptr(), gt.data_ptr(), self._stream()), "wbc_sim_arm_dynamics")
        return mm, jac, gt

    # ---- whole-body Jacobian / mass matrix (gym.acquire_jacobian_tensor / acquire_mass_matrix_tensor, WG:509-510, 550-558) ----
    def acquire_jacobian_tensor(self) -> torch.Tensor:
        """The persistent f32 [N, 27, 6, 26] Jacobian of every robot rigid body's origin w.r.t. (v_root, omega_root, qd), world
        frame (include/wbc_sim.h: wbc_sim_body_dynamics). The same tensor on every call; refresh_jacobian_tensors() fills it."""
        if self.__dict__.get("_jacobian") is None:
            self._jacobian = torch.zeros(self.num_envs, abi.NRB, 6, 6 + abi.NDOF, dtype=torch.float32, device=self.device)
        return self._jacobian

    def acquire_mass_matrix_tensor(self) -> torch.Tensor:
        """The persistent f32 [N, 26, 26] mass matrix in the same coordinates; refresh_mass_matrix_tensors() fills it."""
        if self.__dict__.get("_mass_matrix") is None:
            self._mass_matrix = torch.zeros(self.num_envs, 6 + abi.NDOF, 6 + abi.NDOF, dtype=torch.float32, device=self.device)
        return self._mass_matrix

    def body_dynamics(self, jac: Optional[torch.Tensor] = None, mm: Optional[torch.Tensor] = None) -> None:
        """One wbc_sim_body_dynamics launch on the current stream into caller-owned buffers (either may be None)."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        for t, shape in ((jac, (n, abi.NRB, 6, ncol)), (mm, (n, ncol, ncol))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        check(self.L.wbc_sim_body_dynamics(self.h, jac.data_ptr() if jac is not None else None,
                                           mm.data_ptr() if mm is not None else None, self._stream()), "wbc_sim_body_dynamics")

    def refresh_jacobian_tensors(self) -> None:
        """Recompute the acquired Jacobian in place from the current root / DoF state (views of it see the new values)."""
        self.body_dynamics(jac=self.acquire_jacobian_tensor())

    def refresh_mass_matrix_tensors(self) -> None:
        """Recompute the acquired mass matrix in place from the current state and per-env body parameters."""
        self.body_dynamics(mm=self.acquire_mass_matrix_tensor())

    # ---- whole-body inverse dynamics / bias forces: the h of M nudot + h = S^T tau + sum J_c^T f_c, same coordinates ----------
    def acquire_bias_force_tensor(self) -> torch.Tensor:
        """The persistent f32 [N, 26] bias vector h = C nu + g (include/wbc_sim.h: wbc_sim_inverse_dynamics with nudot = NULL).
        The same tensor on every call; refresh_bias_force_tensors() fills it."""
        if self.__dict__.get("_bias_force") is None:
            self._bias_force = torch.zeros(self.num_envs, 6 + abi.NDOF, dtype=torch.float32, device=self.device)
        return self._bias_force

    def inverse_dynamics(self, nudot: Optional[torch.Tensor] = None, tau: Optional[torch.Tensor] = None,
                         grav: Optional[torch.Tensor] = None) -> None:
        """One wbc_sim_inverse_dynamics launch on the current stream into caller-owned [N, 26] buffers: tau = M nudot + C nu + g
        (nudot None: zeros, i.e. tau = h) and / or grav = g(q); either output may be None, not both."""
        shape = (self.num_envs, 6 + abi.NDOF)
        for t in (nudot, tau, grav):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        check(self.L.wbc_sim_inverse_dynamics(self.h, nudot.data_ptr() if nudot is not None else None,
                                              tau.data_ptr() if tau is not None else None,
                                              grav.data_ptr() if grav is not None else None, self._stream()), "wbc_sim_inverse_dynamics")

    def refresh_bias_force_tensors(self) -> None:
        """Recompute the acquired bias vector in place from the current state and per-env body parameters."""
        self.inverse_dynamics(tau=self.acquire_bias_force_tensor())

    # ---- M^-1: mass-matrix solves and forward dynamics, same coordinates (include/wbc_sim.h: wbc_sim_mass_solve) ------------------
    def mass_solve(self, rhs: torch.Tensor, out: Optional[torch.Tensor] = None, armature: bool = False) -> torch.Tensor:
        """One wbc_sim_mass_solve launch on the current stream: out[e, k] = M_e^-1 rhs[e, k] at the current state. rhs f32 [N, 26]
        or [N, K, 26] (K <= 32) whose last two dims are contiguous, with any env stride (a view such as jacobian[:, r] is passed as
        it stands); returns (or fills) [N, K, 26], [N, 26] for a [N, 26] rhs. armature: solve with M + diag(0_6, joint_armature)."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        flat = rhs.dim() == 2
        r3 = rhs.unsqueeze(1) if flat else rhs
        assert r3.dim() == 3 and r3.shape[0] == n and r3.shape[2] == ncol and 1 <= r3.shape[1] <= 32, tuple(rhs.shape)
        assert rhs.device == self.arena.device and rhs.dtype == torch.float32
        k = r3.shape[1]
        assert r3.stride(2) == 1 and (k == 1 or r3.stride(1) == ncol), "the last two dims of rhs must be contiguous"
        stride = r3.stride(0) if n > 1 else k * ncol
        assert stride >= k * ncol, "rhs rows of different envs overlap"
        if out is None:
            out = torch.empty((n, ncol) if flat else (n, k, ncol), dtype=torch.float32, device=self.device)
        assert out.device == self.arena.device and out.dtype == torch.float32 and out.is_contiguous()
        assert tuple(out.shape) == ((n, ncol) if flat else (n, k, ncol))
        r0, o0 = rhs.data_ptr(), out.data_ptr()
        assert r0 + 4 * ((n - 1) * stride + k * ncol) <= o0 or o0 + 4 * n * k * ncol <= r0, "out overlaps rhs"
        check(self.L.wbc_sim_mass_solve(self.h, rhs.data_ptr(), stride, k, out.data_ptr(), 1 if armature else 0, self._stream()),
              "wbc_sim_mass_solve")
        return out

    def forward_dynamics(self, tau: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         armature: bool = False) -> torch.Tensor:
        """wbc_sim_forward_dynamics on the current stream: nudot = M^-1 (tau - h), f32 [N, 26] (tau None: zeros)."""
        shape = (self.num_envs, 6 + abi.NDOF)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        for t in (tau, out):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        assert tau is None or abs(tau.data_ptr() - out.data_ptr()) >= 4 * out.numel(), "out overlaps tau"
        check(self.L.wbc_sim_forward_dynamics(self.h, tau.data_ptr() if tau is not None else None, out.data_ptr(),
                                              1 if armature else 0, self._stream()), "wbc_sim_forward_dynamics")
        return out

    # ---- rigid-body accelerations and contact-constrained forward dynamics (include/wbc_sim.h) --------------------------------------
    def body_accelerations(self, nudot: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wbc_sim_body_accelerations on the current stream: f32 [N, 27, 6] = J nudot + Jdot nu of every rigid-body origin (rows
        linear, angular; world frame). nudot f32 [N, 26] in the convention of inverse_dynamics, None: zeros (the result is Jdot nu)."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        if out is None:
            out = torch.empty((n, abi.NRB, 6), dtype=torch.float32, device=self.device)
        assert out.device == self.arena.device and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n, abi.NRB, 6)
        if nudot is not None:
            assert nudot.device == self.arena.device and nudot.dtype == torch.float32 and nudot.is_contiguous()
            assert tuple(nudot.shape) == (n, ncol), tuple(nudot.shape)
        check(self.L.wbc_sim_body_accelerations(self.h, nudot.data_ptr() if nudot is not None else None, out.data_ptr(), self._stream()),
              "wbc_sim_body_accelerations")
        return out

    def constrained_dynamics(self, rigid_bodies, tau: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                             acc_des: Optional[torch.Tensor] = None, damping: float = 0.0, armature: bool = False, out=None):
        """wbc_sim_constrained_dynamics on the current stream: forward dynamics with the origins of the listed rigid bodies (1..5
        indices) held at the linear accelerations acc_des [N, K, 3] (None: zeros) where active [N, K] (bool or uint8; None: all).
        Returns (nudot [N, 26], lam [N, K, 3]): lam is the force applied TO the robot at each origin, world axes, exactly 0 where
        inactive. out: an optional (nudot, lam) pair to fill. The workspace is cached per number of bodies."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        rbs = [int(r) for r in (rigid_bodies.tolist() if isinstance(rigid_bodies, torch.Tensor) else rigid_bodies)]
        k = len(rbs)
        assert 1 <= k <= 5, k
        nudot, lam = out if out is not None else (None, None)
        if nudot is None:
            nudot = torch.empty((n, ncol), dtype=torch.float32, device=self.device)
        if lam is None:
            lam = torch.empty((n, k, 3), dtype=torch.float32, device=self.device)
        for t, shape in ((tau, (n, ncol)), (acc_des, (n, k, 3)), (nudot, (n, ncol)), (lam, (n, k, 3))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, tuple(t.shape)
        if active is not None:
            assert active.device == self.arena.device and active.dtype in (torch.bool, torch.uint8) and tuple(active.shape) == (n, k)
            active = active.contiguous()
            if active.dtype == torch.bool:
                active = active.view(torch.uint8)
        cache = self.__dict__.setdefault("_constr_ws", {})
        if k not in cache:
            cache[k] = torch.empty(int(self.L.wbc_sim_constrained_dynamics_workspace_floats(n, k)), dtype=torch.float32, device=self.device)
        idx = (C.c_int32 * k)(*rbs)
        check(self.L.wbc_sim_constrained_dynamics(self.h, idx, k, active.data_ptr() if active is not None else None,
                                                  tau.data_ptr() if tau is not None else None,
                                                  acc_des.data_ptr() if acc_des is not None else None, float(damping),
                                                  1 if armature else 0, nudot.data_ptr(), lam.data_ptr(), cache[k].data_ptr(),
                                                  self._stream()), "wbc_sim_constrained_dynamics")
        return nudot, lam

    def impulse_dynamics(self, rigid_bodies, active: Optional[torch.Tensor] = None, restitution=None,
                         vel_des: Optional[torch.Tensor] = None, impulse_ext: Optional[torch.Tensor] = None, damping: float = 0.0,
                         armature: bool = False, want_map: bool = False, want_energy: bool = False,
                         workspace: Optional[torch.Tensor] = None) -> dict:
        """wbc_sim_impulse_dynamics on the current stream: the velocity jump when the origins of the listed rigid bodies (1..5
        indices) meet surfaces that move at vel_des [N, K, 3] (None: zeros) with Newton restitution [N, K] (a Python float is
        broadcast; None: 0, plastic) where active [N, K] (bool or uint8; None: all), and / or the generalised impulse impulse_ext
        [N, 26] acts. Returns a dict: nu_plus [N, 26], impulse [N, K, 3] (N s, applied TO the robot, exactly 0 where inactive), and
        denergy [N] (want_energy) / dnu_dnu [N, 26, 26] (want_map). workspace: f32, at least
        wbc_sim_impulse_dynamics_workspace_floats(N, K) elements; None: cached per number of bodies, as in constrained_dynamics."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        rbs = [int(r) for r in (rigid_bodies.tolist() if isinstance(rigid_bodies, torch.Tensor) else rigid_bodies)]
        k = len(rbs)
        assert 1 <= k <= 5, k
        if restitution is not None and not isinstance(restitution, torch.Tensor):
            restitution = torch.full((n, k), float(restitution), dtype=torch.float32, device=self.device)
        for t, shape in ((restitution, (n, k)), (vel_des, (n, k, 3)), (impulse_ext, (n, ncol))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, tuple(t.shape)
        if active is not None:
            assert active.device == self.arena.device and active.dtype in (torch.bool, torch.uint8) and tuple(active.shape) == (n, k)
            active = active.contiguous()
            if active.dtype == torch.bool:
                active = active.view(torch.uint8)
        need = int(self.L.wbc_sim_impulse_dynamics_workspace_floats(n, k))
        if workspace is None:
            cache = self.__dict__.setdefault("_impulse_ws", {})
            if k not in cache:
                cache[k] = torch.empty(need, dtype=torch.float32, device=self.device)
            workspace = cache[k]
        assert workspace.device == self.arena.device and workspace.dtype == torch.float32 and workspace.is_contiguous()
        assert workspace.numel() >= need, (workspace.numel(), need)
        out = dict(nu_plus=torch.empty((n, ncol), dtype=torch.float32, device=self.device),
                   impulse=torch.empty((n, k, 3), dtype=torch.float32, device=self.device))
        if want_energy:
            out["denergy"] = torch.empty((n,), dtype=torch.float32, device=self.device)
        if want_map:
            out["dnu_dnu"] = torch.empty((n, ncol, ncol), dtype=torch.float32, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        check(self.L.wbc_sim_impulse_dynamics(self.h, (C.c_int32 * k)(*rbs), k, ptr(active), ptr(restitution), ptr(vel_des), ptr(impulse_ext),
                                              float(damping), 1 if armature else 0, out["nu_plus"].data_ptr(), out["impulse"].data_ptr(),
                                              ptr(out.get("denergy")), ptr(out.get("dnu_dnu")), workspace.data_ptr(), self._stream()),
              "wbc_sim_impulse_dynamics")
        return out

    # ---- whole-body inverse kinematics with joint limits (include/wbc_sim.h: wbc_sim_inverse_kinematics) ------------------------------
    def inverse_kinematics(self, bodies, target_pos: torch.Tensor, target_quat: Optional[torch.Tensor] = None,
                           w_pos: Optional[torch.Tensor] = None, w_ori: Optional[torch.Tensor] = None,
                           root_init: Optional[torch.Tensor] = None, dof_init: Optional[torch.Tensor] = None,
                           q_ref: Optional[torch.Tensor] = None, posture: float = 1e-2, damping: float = 1e-3, step_tol: float = 1e-4,
                           max_iter: int = 0):
        """wbc_sim_inverse_kinematics on the current stream, one launch: the configuration that puts the origins of the listed rigid
        bodies (1..6 indices) at target_pos [N, K, 3] and, where target_quat [N, K, 4] (xyzw) is given, their frames at those
        orientations, weighted by w_pos [N, K, 3] / w_ori [N, K] (None: ones; a row of weight 0 is skipped), regularised towards q_ref
        [N, 20] (None: the start) with weight `posture` and kept inside the model's joint limits. The start is root_init [N, 7] /
        dof_init [N, 20], None: the sim's current state, which is read and never written. damping: the initial Levenberg-Marquardt
        factor; step_tol: metres / radians; max_iter: 0 = abi.IK_MAX_ITER. Returns (root_pose [N, 7], dof_pos [N, 20], info) with
        info["status"] int32 [N] (0 converged, 1 iteration cap, 2 no descent: stationary or out of reach, 3 non-finite input),
        info["iterations"] int32 [N], info["cost"] [N, 2] (start, output) and info["residual"] [N, K, 6] (target - x, phi)."""
        n = self.num_envs
        rbs = [int(r) for r in (bodies.tolist() if isinstance(bodies, torch.Tensor) else bodies)]
        k = len(rbs)
        assert 1 <= k <= abi.IK_MAX_TARGETS, k
        for t, shape in ((target_pos, (n, k, 3)), (target_quat, (n, k, 4)), (w_pos, (n, k, 3)), (w_ori, (n, k)), (root_init, (n, 7)),
                         (dof_init, (n, abi.NDOF)), (q_ref, (n, abi.NDOF))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, tuple(t.shape)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=self.device)   # noqa: E731
        root, dof = new((n, 7)), new((n, abi.NDOF))
        info = dict(status=new((n,), torch.int32), iterations=new((n,), torch.int32), cost=new((n, 2)), residual=new((n, k, 6)))
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        opts = abi.WbcIkOpts(float(posture), float(damping), float(step_tol), int(max_iter))
        check(self.L.wbc_sim_inverse_kinematics(self.h, (C.c_int32 * k)(*rbs), k, target_pos.data_ptr(), ptr(target_quat), ptr(w_pos), ptr(w_ori),
                                                ptr(root_init), ptr(dof_init), ptr(q_ref), C.byref(opts), root.data_ptr(), dof.data_ptr(),
                                                info["residual"].data_ptr(), info["cost"].data_ptr(), info["status"].data_ptr(),
                                                info["iterations"].data_ptr(), self._stream()), "wbc_sim_inverse_kinematics")
        return root, dof, info

    # ---- whole-body inverse dynamics for task-space accelerations (include/wbc_sim.h: wbc_sim_task_inverse_dynamics) ------------------
    def task_inverse_dynamics(self, stance_bodies=(), task_bodies=(), task_acc: Optional[torch.Tensor] = None,
                              task_weight: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                              stance_acc: Optional[torch.Tensor] = None, nudot_ref: Optional[torch.Tensor] = None,
                              posture: float = 1e-2, force: float = 1e-4, torque: float = 1e-3, damping: float = 0.0,
                              armature: bool = False, out=None):
        """wbc_sim_task_inverse_dynamics on the current stream: the joint torques that give the origins of task_bodies (0..6 rigid-body
        indices) the accelerations task_acc [N, T, 6] (linear, angular; per-row weights task_weight [N, T, 6] >= 0, None: ones) while
        the origins of stance_bodies (0..4 indices) keep the linear accelerations stance_acc [N, K, 3] (None: zeros) where active
        [N, K] (bool or uint8; None: all), in the weighted least-squares sense of include/wbc_sim.h with the scalar weights posture
        (towards nudot_ref [N, 26], None: zeros), force, torque (> 0) and the Delassus damping. No inequalities: clamp the result, or
        call task_inverse_dynamics_qp, which solves with torque limits and friction pyramids.
        Returns (tau [N, 26], nudot [N, 26], lam [N, K, 3]): tau[:, 6:] is what set_dof_forces takes, rows 0:6 and the fingers are
        exactly 0. out: an optional (tau, nudot, lam) triple to fill. The workspace is cached per (K, T)."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        srb = [int(r) for r in (stance_bodies.tolist() if isinstance(stance_bodies, torch.Tensor) else stance_bodies)]
        trb = [int(r) for r in (task_bodies.tolist() if isinstance(task_bodies, torch.Tensor) else task_bodies)]
        k, t = len(srb), len(trb)
        assert 0 <= k <= 4 and 0 <= t <= 6, (k, t)
        assert t == 0 or task_acc is not None, "task_acc is needed with task bodies"
        tau, nudot, lam = out if out is not None else (None, None, None)
        if tau is None:
            tau = torch.empty((n, ncol), dtype=torch.float32, device=self.device)
        if nudot is None:
            nudot = torch.empty((n, ncol), dtype=torch.float32, device=self.device)
        if lam is None:
            lam = torch.empty((n, k, 3), dtype=torch.float32, device=self.device)
        for x, shape in ((task_acc, (n, t, 6)), (task_weight, (n, t, 6)), (stance_acc, (n, k, 3)), (nudot_ref, (n, ncol)), (tau, (n, ncol)),
                         (nudot, (n, ncol)), (lam, (n, k, 3))):
            if x is not None:
                assert x.device == self.arena.device and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == shape, tuple(x.shape)
        if active is not None:
            assert active.device == self.arena.device and active.dtype in (torch.bool, torch.uint8) and tuple(active.shape) == (n, k)
            active = active.contiguous()
            if active.dtype == torch.bool:
                active = active.view(torch.uint8)
        cache = self.__dict__.setdefault("_taskid_ws", {})
        if (k, t) not in cache:
            cache[(k, t)] = torch.empty(int(self.L.wbc_sim_task_inverse_dynamics_workspace_floats(n, k, t)), dtype=torch.float32,
                                        device=self.device)
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() > 0 else None
        w = abi.WbcTaskIdWeights(float(posture), float(force), float(torque), float(damping))
        check(self.L.wbc_sim_task_inverse_dynamics(self.h, (C.c_int32 * max(k, 1))(*srb), k, ptr(active), ptr(stance_acc),
                                                   (C.c_int32 * max(t, 1))(*trb), t, ptr(task_acc), ptr(task_weight), ptr(nudot_ref),
                                                   C.byref(w), 1 if armature else 0, tau.data_ptr(), nudot.data_ptr(), ptr(lam),
                                                   cache[(k, t)].data_ptr(), self._stream()), "wbc_sim_task_inverse_dynamics")
        return tau, nudot, lam

    # ---- the same with torque limits and friction pyramids (include/wbc_sim.h: wbc_sim_task_inverse_dynamics_qp) -----------------------
    def task_inverse_dynamics_qp(self, stance_bodies=(), task_bodies=(), task_acc: Optional[torch.Tensor] = None,
                                 task_weight: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                                 stance_acc: Optional[torch.Tensor] = None, nudot_ref: Optional[torch.Tensor] = None,
                                 posture: float = 1e-2, force: float = 1e-4, torque: float = 1e-3, damping: float = 0.0,
                                 armature: bool = False, mu=0.5, fn_min: float = 0.0, tau_limit: Optional[torch.Tensor] = None,
                                 normal: Optional[torch.Tensor] = None, max_iter: int = 0, out=None):
        """wbc_sim_task_inverse_dynamics_qp on the current stream: task_inverse_dynamics' problem and arguments, further subject to
        |tau_j| <= tau_limit [N, 18] (None: the config's torque_limits of the 18 revolute joints, in the order of tau[:, 6:24]) and, per
        active stance body, normal force >= fn_min and the friction pyramid |t . lam| <= mu n . lam along two tangents (mu: a float, or
        a tensor [N, K]; normal [N, K, 3], None: world z; tangent rule in include/wbc_sim.h). max_iter: 0 = the default, at most
        abi.TASKQP_MAX_ITER. Returns (tau [N, 26], nudot [N, 26], lam [N, K, 3], info): info["status"] int32 [N] (0 optimal, 1 the
        iteration cap, 2 no point satisfies the rows; 1 and 2 carry the unconstrained optimum clamped to the box), info["active_set"]
        int64 [N] (bits: header) and info["iterations"] int32 [N]. out: an optional (tau, nudot, lam, status, active_set, iterations)
        tuple to fill. The workspace is cached per (K, T) and shared with nothing else."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        srb = [int(r) for r in (stance_bodies.tolist() if isinstance(stance_bodies, torch.Tensor) else stance_bodies)]
        trb = [int(r) for r in (task_bodies.tolist() if isinstance(task_bodies, torch.Tensor) else task_bodies)]
        k, t = len(srb), len(trb)
        assert 0 <= k <= 4 and 0 <= t <= 6, (k, t)
        assert t == 0 or task_acc is not None, "task_acc is needed with task bodies"
        tau, nudot, lam, status, aset, iters = out if out is not None else (None,) * 6
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
        tau = new((n, ncol), torch.float32) if tau is None else tau
        nudot = new((n, ncol), torch.float32) if nudot is None else nudot
        lam = new((n, k, 3), torch.float32) if lam is None else lam
        status = new((n,), torch.int32) if status is None else status
        aset = new((n,), torch.int64) if aset is None else aset
        iters = new((n,), torch.int32) if iters is None else iters
        mu_t = mu if isinstance(mu, torch.Tensor) else None
        for x, shape, dtype in ((task_acc, (n, t, 6), torch.float32), (task_weight, (n, t, 6), torch.float32), (stance_acc, (n, k, 3), torch.float32),
                                (nudot_ref, (n, ncol), torch.float32), (tau, (n, ncol), torch.float32), (nudot, (n, ncol), torch.float32),
                                (lam, (n, k, 3), torch.float32), (tau_limit, (n, abi.NJ), torch.float32), (normal, (n, k, 3), torch.float32),
                                (mu_t, (n, k), torch.float32), (status, (n,), torch.int32), (aset, (n,), torch.int64), (iters, (n,), torch.int32)):
            if x is not None:
                assert x.device == self.arena.device and x.dtype == dtype and x.is_contiguous() and tuple(x.shape) == shape, tuple(x.shape)
        if active is not None:
            assert active.device == self.arena.device and active.dtype in (torch.bool, torch.uint8) and tuple(active.shape) == (n, k)
            active = active.contiguous()
            if active.dtype == torch.bool:
                active = active.view(torch.uint8)
        cache = self.__dict__.setdefault("_taskqp_ws", {})
        if (k, t) not in cache:
            cache[(k, t)] = torch.empty(int(self.L.wbc_sim_task_inverse_dynamics_qp_workspace_floats(n, k, t)), dtype=torch.float32,
                                        device=self.device)
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() > 0 else None
        w = abi.WbcTaskIdWeights(float(posture), float(force), float(torque), float(damping))
        lim = abi.WbcTaskQpLimits(1.0 if mu_t is not None else float(mu), float(fn_min), int(max_iter))
        check(self.L.wbc_sim_task_inverse_dynamics_qp(self.h, (C.c_int32 * max(k, 1))(*srb), k, ptr(active), ptr(stance_acc),
                                                      (C.c_int32 * max(t, 1))(*trb), t, ptr(task_acc), ptr(task_weight), ptr(nudot_ref),
                                                      C.byref(w), C.byref(lim), ptr(tau_limit), ptr(normal), ptr(mu_t), 1 if armature else 0,
                                                      tau.data_ptr(), nudot.data_ptr(), ptr(lam), status.data_ptr(), aset.data_ptr(),
                                                      iters.data_ptr(), cache[(k, t)].data_ptr(), self._stream()),
              "wbc_sim_task_inverse_dynamics_qp")
        return tau, nudot, lam, {"status": status, "active_set": aset, "iterations": iters}

    # ---- centre of mass, centroidal momentum and its matrix (include/wbc_sim.h: wbc_sim_centroidal) ----------------------------------
    def centroidal(self, nudot: Optional[torch.Tensor] = None, com: Optional[torch.Tensor] = None, mom: Optional[torch.Tensor] = None,
                   cmm: Optional[torch.Tensor] = None, inertia: Optional[torch.Tensor] = None):
        """One wbc_sim_centroidal launch on the current stream. Returns (com [N, 9], mom [N, 12], cmm [N, 6, 26], inertia [N, 7]):
        (c - p_root, v_com, a_com), (h_G, hdot_G), A_G and (m, I_G as xx yy zz xy xz yz), world axes, angular rows about the centre of
        mass. Outputs that are not passed are allocated; nudot f32 [N, 26] in the convention of inverse_dynamics, None: zeros (a_com
        and hdot_G are then the bias parts). A launch that writes fewer outputs goes through the C-ABI with NULL pointers."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        shapes = ((n, 9), (n, 12), (n, 6, ncol), (n, 7))
        outs = [torch.empty(sh, dtype=torch.float32, device=self.device) if t is None else t for t, sh in zip((com, mom, cmm, inertia), shapes)]
        for t, sh in zip([nudot] + outs, ((n, ncol),) + shapes):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        check(self.L.wbc_sim_centroidal(self.h, nudot.data_ptr() if nudot is not None else None, *[t.data_ptr() for t in outs],
                                        self._stream()), "wbc_sim_centroidal")
        return tuple(outs)

    # ---- Coriolis matrix, dM/dt, generalised momentum and the momentum observer (include/wbc_sim.h: wbc_sim_coriolis) -------------------
    def coriolis(self, cmat: Optional[torch.Tensor] = None, mdot: Optional[torch.Tensor] = None, vec: Optional[torch.Tensor] = None):
        """One wbc_sim_coriolis launch on the current stream into the tensors that are passed; returns the tensors it filled, in the
        order (cmat [N, 26, 26] = C(q, nu), mdot [N, 26, 26] = dM/dt = C + C^T, vec [N, 2, 26] = (M nu, C^T nu)). With none passed all
        three are allocated and filled. vec alone takes the vector kernel, which forms nothing 26 x 26."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        shapes = ((n, ncol, ncol), (n, ncol, ncol), (n, 2, ncol))
        outs = [cmat, mdot, vec]
        if all(t is None for t in outs):
            outs = [torch.empty(sh, dtype=torch.float32, device=self.device) for sh in shapes]
        for t, sh in zip(outs, shapes):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        check(self.L.wbc_sim_coriolis(self.h, *[t.data_ptr() if t is not None else None for t in outs], self._stream()), "wbc_sim_coriolis")
        return tuple(t for t in outs if t is not None)

    def momentum_observer(self, tau: Optional[torch.Tensor], gain: float, dt: float, state: Optional[torch.Tensor] = None,
                          reset: bool = False) -> torch.Tensor:
        """One wbc_sim_momentum_observer update on the current stream at the sim's current state; returns state f32 [N, 2, 26] (the
        integral, then the residual: the estimate of the generalised forces that tau [N, 26] does not hold; tau None: zeros). state None:
        the observer's own tensor, allocated on first use (and then reset, whatever `reset` says) and kept. gain > 0, dt > 0,
        gain dt < 1. Uses the sim's bias-force scratch: one stream at a time per sim."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        if state is None:
            state = self.__dict__.get("_observer_state")
            if state is None:
                state = self._observer_state = torch.zeros((n, 2, ncol), dtype=torch.float32, device=self.device)
                reset = True
        for t, sh in ((tau, (n, ncol)), (state, (n, 2, ncol))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        check(self.L.wbc_sim_momentum_observer(self.h, tau.data_ptr() if tau is not None else None, float(gain), float(dt),
                                               abi.OBSERVER_RESET if reset else 0, state.data_ptr(), self._stream()),
              "wbc_sim_momentum_observer")
        return state

    # ---- self-collision proximity: gaps, witness points and gap Jacobians (include/wbc_sim.h: wbc_sim_proximity) ------------------------
    @property
    def proximity_pair_ids(self) -> np.ndarray:
        """int32 [P, 4]: (kind, a, b, 0) per pair as wbc_sim_proximity_pairs lists them (abi.PR_LIMBS: limb ids; abi.PR_STATIC: the
        sphere's compact index and the box's rigid body). P = 0 for a model without self-collisions."""
        ids = self.__dict__.get("_proximity_pair_ids")
        if ids is None:
            p = self.L.wbc_sim_proximity_pair_count(self.h)
            if p < 0:
                check(p, "wbc_sim_proximity_pair_count")
            buf = (C.c_int32 * (4 * max(p, 1)))()
            if p > 0 and self.L.wbc_sim_proximity_pairs(self.h, buf) != p:
                check(-1, "wbc_sim_proximity_pairs")
            ids = self._proximity_pair_ids = np.array(buf[:4 * p], dtype=np.int32).reshape(p, 4)
        return ids

    @property
    def proximity_pairs(self):
        """[(name_a, name_b)] per pair, in the order of every output of proximity(): collision_set's limb names for a limb pair, the
        sphere's name and "trunk" for a sphere against the trunk box."""
        name = lambda table, i, what: table[i] if 0 <= i < len(table) else f"{what}{i}"
        return [(name(abi.LIMB_NAMES, a, "limb"), name(abi.LIMB_NAMES, b, "limb")) if kind == abi.PR_LIMBS
                else (name(abi.SPHERE_NAMES, a, "sphere"), "trunk") for kind, a, b, _ in self.proximity_pair_ids.tolist()]

    def proximity(self, gap: Optional[torch.Tensor] = None, normal: Optional[torch.Tensor] = None, witness: Optional[torch.Tensor] = None,
                  jac: Optional[torch.Tensor] = None, k_nearest: int = 0, nearest: Optional[torch.Tensor] = None):
        """One wbc_sim_proximity launch on the current stream into the tensors that are passed; returns the tensors it filled, in the
        order (gap [N, P], normal [N, P, 3], witness [N, P, 2, 3], jac [N, P, 26], nearest int32 [N, k_nearest]): the signed distances
        of the robot's own collision pairs (proximity_pairs), the unit vectors from b's closest point to a's, the two surface points
        relative to the root's origin (world axes) and d gap / d q with d gap / dt = jac . nu. With no float tensor passed all four
        are allocated and filled; k_nearest in 1 .. 8 (or a `nearest` tensor) adds the indices of the k smallest gaps per env."""
        n, ncol, p = self.num_envs, 6 + abi.NDOF, len(self.proximity_pair_ids)
        shapes = ((n, p), (n, p, 3), (n, p, 2, 3), (n, p, ncol))
        outs = [gap, normal, witness, jac]
        if all(t is None for t in outs) and nearest is None and p > 0:
            outs = [torch.empty(sh, dtype=torch.float32, device=self.device) for sh in shapes]
        if nearest is None and k_nearest:
            nearest = torch.empty((n, int(k_nearest)), dtype=torch.int32, device=self.device)
        for t, sh in zip(outs, shapes):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        if nearest is not None:
            assert nearest.device == self.arena.device and nearest.dtype == torch.int32 and nearest.is_contiguous()
            assert nearest.dim() == 2 and nearest.shape[0] == n, tuple(nearest.shape)
        check(self.L.wbc_sim_proximity(self.h, *[t.data_ptr() if t is not None else None for t in outs + [nearest]],
                                       int(nearest.shape[1]) if nearest is not None else 0, self._stream()), "wbc_sim_proximity")
        return tuple(t for t in outs + [nearest] if t is not None)

    # ---- leg-odometry Kalman filter (include/wbc_sim.h: wbc_sim_leg_odometry) --------------------------------------------------------------
    def leg_odometry(self, cfg: "abi.WbcEstimatorCfg", x: torch.Tensor, P: torch.Tensor, contact: torch.Tensor,
                     quat: Optional[torch.Tensor] = None, gyro: Optional[torch.Tensor] = None, dof: Optional[torch.Tensor] = None,
                     accel: Optional[torch.Tensor] = None, foot_height: Optional[torch.Tensor] = None,
                     reset_mask: Optional[torch.Tensor] = None, p_init: Optional[torch.Tensor] = None, reset: bool = False,
                     vel_body: Optional[torch.Tensor] = None, nis: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
        """One wbc_sim_leg_odometry launch on the current stream: one predict + correct of the caller-owned state x f32 [N, 18] = (p, v,
        four foot origins) and covariance P f32 [N, 18, 18], in place. contact f32 [N, 4] in [0, 1]; quat [N, 4] (xyzw), gyro [N, 3]
        (trunk axes) and dof [N, 20, 2], None: the sim's current state; accel [N, 3] the specific force in trunk axes (None: constant
        velocity); foot_height [N, 4] the ground's world height under each foot (None: no height rows). reset=True resets every env,
        reset_mask int32 [N] the envs whose entry is not 0, to p_init [N, 3] (None: 0). Returns the tensors it filled, in the order
        (x, P, vel_body [N, 3] = R^T v, nis [N], status int32 [N]); with none of the last three passed all three are allocated."""
        n = self.num_envs
        outs = [vel_body, nis, status]
        if all(t is None for t in outs):
            outs = [torch.empty((n, 3), dtype=torch.float32, device=self.device), torch.empty((n,), dtype=torch.float32, device=self.device),
                    torch.empty((n,), dtype=torch.int32, device=self.device)]
        f32, i32 = torch.float32, torch.int32
        for t, sh, dt in ((x, (n, abi.ESTIMATOR_NX), f32), (P, (n, abi.ESTIMATOR_NX, abi.ESTIMATOR_NX), f32), (contact, (n, 4), f32),
                          (quat, (n, 4), f32), (gyro, (n, 3), f32), (dof, (n, abi.NDOF, 2), f32), (accel, (n, 3), f32),
                          (foot_height, (n, 4), f32), (reset_mask, (n,), i32), (p_init, (n, 3), f32), (outs[0], (n, 3), f32),
                          (outs[1], (n,), f32), (outs[2], (n,), i32)):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        assert x is not None and P is not None and contact is not None
        ptr = lambda t: t.data_ptr() if t is not None else None
        check(self.L.wbc_sim_leg_odometry(self.h, C.byref(cfg), ptr(quat), ptr(gyro), ptr(dof), ptr(accel), ptr(contact), ptr(foot_height),
                                          ptr(reset_mask), ptr(p_init), abi.ESTIMATOR_RESET if reset else 0, x.data_ptr(), P.data_ptr(),
                                          ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), self._stream()), "wbc_sim_leg_odometry")
        return tuple(t for t in [x, P] + outs if t is not None)

    # ---- convex centroidal MPC of the foot forces (include/wbc_sim.h: wbc_sim_centroidal_mpc) ----------------------------------------------
    def centroidal_mpc(self, cfg: "abi.WbcMpcCfg", contact: torch.Tensor, x_ref: torch.Tensor, x0: Optional[torch.Tensor] = None,
                       mass: Optional[torch.Tensor] = None, inertia: Optional[torch.Tensor] = None, foot_pos: Optional[torch.Tensor] = None,
                       warm: Optional[torch.Tensor] = None, cold: bool = False, shift: bool = False, forces: Optional[torch.Tensor] = None,
                       u: Optional[torch.Tensor] = None, x_pred: Optional[torch.Tensor] = None, base_acc: Optional[torch.Tensor] = None,
                       res: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
        """One wbc_sim_centroidal_mpc launch on the current stream (two when x0, mass or inertia is None: wbc_centroidal_kernel fills the
        workspace first). contact u8 [N, H, 4] and x_ref f32 [N, H, 12] (stages 1..H) with H = cfg.horizon; x0 [N, 12], mass [N],
        inertia [N, 3, 3], foot_pos [N, 1 or H, 4, 3], None: the sim's current state; warm f32 [N, 2, H, 20] (z then y) is read and
        written unless cold (None: a cold start, nothing kept); shift moves it one stage to the left first. Returns the tensors it
        filled, in the order (forces [N, 4, 3], u [N, H, 12], x_pred [N, H, 12], base_acc [N, 6], res [N, 2], status int32 [N]); with
        none of them passed all six are allocated. workspace: f32 of wbc_sim_centroidal_mpc_workspace_floats(N) floats, allocated here
        when it is needed and not passed."""
        n, H = self.num_envs, int(cfg.horizon)
        f32, i32 = torch.float32, torch.int32
        shapes = ((n, 4, 3), (n, H, abi.MPC_NU), (n, H, abi.MPC_NX), (n, 6), (n, 2), (n,))
        outs = [forces, u, x_pred, base_acc, res, status]
        if all(t is None for t in outs):
            outs = [torch.empty(sh, dtype=i32 if k == 5 else f32, device=self.device) for k, sh in enumerate(shapes)]
        stages = int(foot_pos.shape[1]) if foot_pos is not None and foot_pos.dim() == 4 else 1
        need_ws = x0 is None or mass is None or inertia is None
        if need_ws and workspace is None:
            workspace = torch.empty((int(self.L.wbc_sim_centroidal_mpc_workspace_floats(n)),), dtype=f32, device=self.device)
        for t, sh, dt in [(contact, (n, H, 4), torch.uint8), (x_ref, (n, H, abi.MPC_NX), f32), (x0, (n, abi.MPC_NX), f32), (mass, (n,), f32),
                          (inertia, (n, 3, 3), f32), (foot_pos, (n, stages, 4, 3), f32), (warm, (n, 2, H, abi.MPC_NZ), f32)] + [
                              (t, sh, i32 if k == 5 else f32) for k, (t, sh) in enumerate(zip(outs, shapes))]:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        assert contact is not None and x_ref is not None
        if workspace is not None:
            assert workspace.device == self.arena.device and workspace.dtype == f32 and workspace.is_contiguous()
            assert not need_ws or workspace.numel() >= int(self.L.wbc_sim_centroidal_mpc_workspace_floats(n))
        ptr = lambda t: t.data_ptr() if t is not None else None
        flags = (abi.MPC_COLD if cold else 0) | (abi.MPC_SHIFT if shift else 0)
        check(self.L.wbc_sim_centroidal_mpc(self.h, C.byref(cfg), ptr(x0), ptr(mass), ptr(inertia), ptr(foot_pos), stages, ptr(contact),
                                            ptr(x_ref), ptr(warm), flags, *[ptr(t) for t in outs], ptr(workspace), self._stream()),
              "wbc_sim_centroidal_mpc")
        return tuple(t for t in outs if t is not None)

    # ---- gait clock, footholds and swing references (include/wbc_sim.h: wbc_sim_footstep_plan) ------------------------------------------------
    FOOTSTEP_OUTPUTS = ("stance", "contact", "schedule", "foot_pos", "foothold", "swing_ref", "swing_acc", "info")

    def footstep_plan(self, cfg: "abi.WbcFootstepCfg", state: torch.Tensor, base_pos: Optional[torch.Tensor] = None,
                      base_vel: Optional[torch.Tensor] = None, quat: Optional[torch.Tensor] = None, dof: Optional[torch.Tensor] = None,
                      vel_cmd: Optional[torch.Tensor] = None, yaw_rate: Optional[torch.Tensor] = None,
                      reset_mask: Optional[torch.Tensor] = None, phase_init: Optional[torch.Tensor] = None, reset: bool = False,
                      hold: bool = False, **outputs) -> None:
        """One wbc_sim_footstep_plan launch on the current stream: one control step of the gait clock, the footholds and the swing
        references on the caller-owned state f32 [N, 32], in place. base_pos, base_vel [N, 3], quat [N, 4] (xyzw) and dof [N, 20, 2],
        None: the sim's current state; vel_cmd [N, 2] (heading frame) and yaw_rate [N], None: 0. reset=True resets every env,
        reset_mask int32 [N] the envs whose entry is not 0, to the phase phase_init [N] (None: 0); hold=True leaves the clock where it is.
        Outputs by keyword, each a caller-owned tensor that is filled (FOOTSTEP_OUTPUTS): stance u8 [N, 4], contact [N, 4], schedule u8
        [N, H, 4], foot_pos [N, H, 4, 3], foothold [N, 4, 3], swing_ref [N, 4, 9], swing_acc [N, 4, 3], info int32 [N]."""
        n, H = self.num_envs, int(cfg.horizon)
        unknown = set(outputs) - set(self.FOOTSTEP_OUTPUTS)
        assert not unknown, f"unknown outputs: {sorted(unknown)}"
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        shapes = dict(stance=((n, 4), u8), contact=((n, 4), f32), schedule=((n, H, 4), u8), foot_pos=((n, H, 4, 3), f32),
                      foothold=((n, 4, 3), f32), swing_ref=((n, 4, 9), f32), swing_acc=((n, 4, 3), f32), info=((n,), i32))
        checks = [(state, (n, abi.FOOTSTEP_NS), f32), (base_pos, (n, 3), f32), (base_vel, (n, 3), f32), (quat, (n, 4), f32),
                  (dof, (n, abi.NDOF, 2), f32), (vel_cmd, (n, 2), f32), (yaw_rate, (n,), f32), (reset_mask, (n,), i32), (phase_init, (n,), f32)]
        checks += [(outputs.get(k),) + shapes[k] for k in self.FOOTSTEP_OUTPUTS]
        for t, sh, dt in checks:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, (tuple(t.shape), sh)
        assert state is not None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        flags = (abi.FOOTSTEP_RESET if reset else 0) | (abi.FOOTSTEP_HOLD if hold else 0)
        check(self.L.wbc_sim_footstep_plan(self.h, C.byref(cfg), ptr(base_pos), ptr(base_vel), ptr(quat), ptr(dof), ptr(vel_cmd), ptr(yaw_rate),
                                           ptr(reset_mask), ptr(phase_init), flags, state.data_ptr(),
                                           *[ptr(outputs.get(k)) for k in self.FOOTSTEP_OUTPUTS], self._stream()), "wbc_sim_footstep_plan")

    # ---- contact detection from proprioception (include/wbc_sim.h: wbc_sim_contact_detect) -------------------------------------------------
    CONTACT_OUTPUTS = ("prob", "contact", "stance", "force", "terms", "info")

    def contact_detect(self, cfg: "abi.WbcContactCfg", state: torch.Tensor, quat: Optional[torch.Tensor] = None,
                       dof: Optional[torch.Tensor] = None, base_pos: Optional[torch.Tensor] = None, tau_ext: Optional[torch.Tensor] = None,
                       foot_force: Optional[torch.Tensor] = None, normal: Optional[torch.Tensor] = None, ground: Optional[torch.Tensor] = None,
                       phase: Optional[torch.Tensor] = None, reset_mask: Optional[torch.Tensor] = None, p_init: Optional[torch.Tensor] = None,
                       reset: bool = False, **outputs) -> None:
        """One wbc_sim_contact_detect launch on the current stream: one control step of the probabilistic contact detector on the
        caller-owned state f32 [N, 16] = (p, c, t, 0) per foot, in place. quat [N, 4] (xyzw), dof [N, 20, 2] and base_pos [N, 3], None:
        the sim's current state. tau_ext [N, 26]: the external generalised forces, rows contiguous and the envs any stride >= 26 apart, so
        that a momentum observer's state[:, 1] is taken as it stands, without a copy; or foot_force [N, 4, 3] (world), not both; normal
        [N, 4, 3] (None: world z); ground [N, 4]: the height of a resting foot's origin (None: no height term); phase [N], the envs any
        stride apart (a FootstepPlanner's state[:, 0] fits; None: no gait prior, no EARLY / LATE). reset=True resets every env, reset_mask
        int32 [N] the envs whose entry is not 0, to p_init [N, 4] (None: 1). Outputs by keyword, each a caller-owned tensor that is filled
        (CONTACT_OUTPUTS): prob [N, 4], contact u8 [N, 4], stance u8 [N, 4], force [N, 4, 3], terms [N, 4, 4], info int32 [N]."""
        n = self.num_envs
        unknown = set(outputs) - set(self.CONTACT_OUTPUTS)
        assert not unknown, f"unknown outputs: {sorted(unknown)}"
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        shapes = dict(prob=((n, 4), f32), contact=((n, 4), u8), stance=((n, 4), u8), force=((n, 4, 3), f32), terms=((n, 4, 4), f32), info=((n,), i32))
        checks = [(state, (n, abi.CONTACT_NS), f32), (quat, (n, 4), f32), (dof, (n, abi.NDOF, 2), f32), (base_pos, (n, 3), f32),
                  (foot_force, (n, 4, 3), f32), (normal, (n, 4, 3), f32), (ground, (n, 4), f32), (reset_mask, (n,), i32), (p_init, (n, 4), f32)]
        checks += [(outputs.get(k),) + shapes[k] for k in self.CONTACT_OUTPUTS]
        for t, sh, dt in checks:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, (tuple(t.shape), sh)
        assert state is not None
        ncol = 6 + abi.NDOF
        tau_stride = phase_stride = 0
        if tau_ext is not None:                                                        # rows contiguous, envs any stride >= 26 apart
            assert tau_ext.device == self.arena.device and tau_ext.dtype == f32 and tuple(tau_ext.shape) == (n, ncol), tuple(tau_ext.shape)
            assert tau_ext.stride(1) == 1 and (n == 1 or tau_ext.stride(0) >= ncol), tau_ext.stride()
            tau_stride = int(tau_ext.stride(0)) if n > 1 else ncol
        if phase is not None:
            assert phase.device == self.arena.device and phase.dtype == f32 and tuple(phase.shape) == (n,), tuple(phase.shape)
            assert n == 1 or phase.stride(0) >= 1, phase.stride()
            phase_stride = int(phase.stride(0)) if n > 1 else 1
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        check(self.L.wbc_sim_contact_detect(self.h, C.byref(cfg), ptr(quat), ptr(dof), ptr(base_pos), ptr(tau_ext), tau_stride, ptr(foot_force),
                                            ptr(normal), ptr(ground), ptr(phase), phase_stride, ptr(reset_mask), ptr(p_init),
                                            abi.CONTACT_RESET if reset else 0, state.data_ptr(),
                                            *[ptr(outputs.get(k)) for k in self.CONTACT_OUTPUTS], self._stream()), "wbc_sim_contact_detect")

    # ---- leg controller (include/wbc_sim.h: wbc_sim_leg_control) ----------------------------------------------------------------------------
    LEGCTL_OUTPUTS = ("tau", "leg_force", "foot", "info")

    def leg_control(self, cfg: "abi.WbcLegControlCfg", quat: Optional[torch.Tensor] = None, dof: Optional[torch.Tensor] = None,
                    base_pos: Optional[torch.Tensor] = None, base_vel: Optional[torch.Tensor] = None, ang_vel: Optional[torch.Tensor] = None,
                    forces: Optional[torch.Tensor] = None, swing_ref: Optional[torch.Tensor] = None, stance: Optional[torch.Tensor] = None,
                    tau_bias: Optional[torch.Tensor] = None, mass_matrix: Optional[torch.Tensor] = None, acc_bias: Optional[torch.Tensor] = None,
                    arm_q_des: Optional[torch.Tensor] = None, tau_limit: Optional[torch.Tensor] = None, clip: bool = False, **outputs) -> None:
        """One wbc_sim_leg_control launch on the current stream: the joint torques of the stance legs from the planned foot forces
        (-J^T f), of the swing legs from a Cartesian impedance on swing_ref with the acceleration feed-forward, and of the arm from a joint
        PD. quat [N, 4] (xyzw), dof [N, 20, 2], base_pos, base_vel and ang_vel [N, 3] (world), None: the sim's current state. forces
        [N, 4, 3] (None: 0), swing_ref [N, 4, 9] (None: no swing term), stance f32 [N, 4] weights in [0, 1] (None: 1). tau_bias [N, 26],
        mass_matrix [N, 26, 26] and acc_bias [N, 27, 6] are taken as they stand: an env's rows contiguous, the envs any stride at or
        above the size apart (a plane of a wider buffer, env.mm_whole, body_accelerations(None)). arm_q_des [N, 6] (None: the cfg's
        default), tau_limit [N, 18] (None: no clamp); clip=True clips the forces to the cfg's pyramid first. Outputs by keyword, each a
        caller-owned tensor that is filled (LEGCTL_OUTPUTS): tau [N, 20], leg_force [N, 4, 3], foot [N, 4, 6], info int32 [N]."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        unknown = set(outputs) - set(self.LEGCTL_OUTPUTS)
        assert not unknown, f"unknown outputs: {sorted(unknown)}"
        f32, i32 = torch.float32, torch.int32
        shapes = dict(tau=((n, abi.NDOF), f32), leg_force=((n, 4, 3), f32), foot=((n, 4, 6), f32), info=((n,), i32))
        checks = [(quat, (n, 4), f32), (dof, (n, abi.NDOF, 2), f32), (base_pos, (n, 3), f32), (base_vel, (n, 3), f32), (ang_vel, (n, 3), f32),
                  (forces, (n, 4, 3), f32), (swing_ref, (n, 4, 9), f32), (stance, (n, 4), f32), (arm_q_des, (n, 6), f32), (tau_limit, (n, 18), f32)]
        checks += [(outputs.get(k),) + shapes[k] for k in self.LEGCTL_OUTPUTS]
        for t, sh, dt in checks:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, (tuple(t.shape), sh)
        strides = {}
        for name, t, sh in (("tau_bias", tau_bias, (ncol,)), ("mass_matrix", mass_matrix, (ncol, ncol)), ("acc_bias", acc_bias, (abi.NRB, 6))):
            strides[name] = 0
            if t is not None:                                                          # an env's rows contiguous, the envs any stride >= the size apart
                size = int(torch.Size(sh).numel())
                assert t.device == self.arena.device and t.dtype == f32 and tuple(t.shape) == (n,) + sh, (name, tuple(t.shape))
                assert t[0].is_contiguous() and (n == 1 or t.stride(0) >= size), (name, t.stride())
                strides[name] = int(t.stride(0)) if n > 1 else size
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        check(self.L.wbc_sim_leg_control(self.h, C.byref(cfg), ptr(quat), ptr(dof), ptr(base_pos), ptr(base_vel), ptr(ang_vel), ptr(forces),
                                         ptr(swing_ref), ptr(stance), ptr(tau_bias), strides["tau_bias"], ptr(mass_matrix), strides["mass_matrix"],
                                         ptr(acc_bias), strides["acc_bias"], ptr(arm_q_des), ptr(tau_limit), abi.LEGCTL_CLIP if clip else 0,
                                         *[ptr(outputs.get(k)) for k in self.LEGCTL_OUTPUTS], self._stream()), "wbc_sim_leg_control")

    # ---- attitude filter (include/wbc_sim.h: wbc_sim_attitude_filter) ------------------------------------------------------------------------
    ATTITUDE_OUTPUTS = ("gyro_out", "gravity_body", "nis", "status")

    def attitude_filter(self, cfg: "abi.WbcAttitudeCfg", q: torch.Tensor, b: torch.Tensor, P: torch.Tensor,
                        gyro: Optional[torch.Tensor] = None, accel: Optional[torch.Tensor] = None, aux_body: Optional[torch.Tensor] = None,
                        aux_world: Optional[torch.Tensor] = None, aux_sigma: Optional[torch.Tensor] = None,
                        reset_mask: Optional[torch.Tensor] = None, q_init: Optional[torch.Tensor] = None, reset: bool = False, **outputs) -> None:
        """One wbc_sim_attitude_filter launch on the current stream: one predict + correct of the caller-owned orientation q f32 [N, 4]
        (xyzw), gyro bias b f32 [N, 3] and covariance P f32 [N, 6, 6] of the error state (dtheta, db), in place. gyro [N, 3] in trunk axes
        (None: the sim's angular velocity, no bias); accel [N, 3] the specific force in trunk axes (None: no gravity row); aux_body and
        aux_world [N, K, 3] with aux_sigma [N, K], K <= 4: further directions measured in trunk axes and known in world axes (sigma <= 0:
        skipped). reset=True resets every env, reset_mask int32 [N] the envs whose entry is not 0, to q_init [N, 4] (None: from accel, or
        the identity). Outputs by keyword, each a caller-owned tensor that is filled (ATTITUDE_OUTPUTS): gyro_out [N, 3] = gyro - b,
        gravity_body [N, 3], nis [N, 1 + K], status int32 [N]."""
        n = self.num_envs
        unknown = set(outputs) - set(self.ATTITUDE_OUTPUTS)
        assert not unknown, f"unknown outputs: {sorted(unknown)}"
        f32, i32 = torch.float32, torch.int32
        k = 0 if aux_sigma is None else int(aux_sigma.shape[1])
        assert (aux_body is None) == (aux_world is None) == (aux_sigma is None), "aux_body, aux_world and aux_sigma go together"
        shapes = dict(gyro_out=((n, 3), f32), gravity_body=((n, 3), f32), nis=((n, 1 + k), f32), status=((n,), i32))
        checks = [(q, (n, 4), f32), (b, (n, 3), f32), (P, (n, 6, 6), f32), (gyro, (n, 3), f32), (accel, (n, 3), f32), (aux_body, (n, k, 3), f32),
                  (aux_world, (n, k, 3), f32), (aux_sigma, (n, k), f32), (reset_mask, (n,), i32), (q_init, (n, 4), f32)]
        checks += [(outputs.get(name),) + shapes[name] for name in self.ATTITUDE_OUTPUTS]
        for t, sh, dt in checks:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, (tuple(t.shape), sh)
        assert q is not None and b is not None and P is not None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        check(self.L.wbc_sim_attitude_filter(self.h, C.byref(cfg), ptr(gyro), ptr(accel), ptr(aux_body), ptr(aux_world), ptr(aux_sigma), k,
                                             ptr(reset_mask), ptr(q_init), abi.ATTITUDE_RESET if reset else 0, q.data_ptr(), b.data_ptr(),
                                             P.data_ptr(), *[ptr(outputs.get(name)) for name in self.ATTITUDE_OUTPUTS], self._stream()),
              "wbc_sim_attitude_filter")

    # ---- ground plane from the footholds (include/wbc_sim.h: wbc_sim_ground_estimate) ------------------------------------------------------
    GROUND_OUTPUTS = ("normal", "ground", "residual", "trunk", "theta_ref", "query_z", "info")

    def ground_estimate(self, cfg: "abi.WbcGroundCfg", state: torch.Tensor, contact: torch.Tensor, quat: Optional[torch.Tensor] = None,
                        dof: Optional[torch.Tensor] = None, base_pos: Optional[torch.Tensor] = None, reset_mask: Optional[torch.Tensor] = None,
                        query_xy: Optional[torch.Tensor] = None, reset: bool = False, **outputs) -> None:
        """One wbc_sim_ground_estimate launch on the current stream: one control step of the blind terrain estimate, a plane through the
        most recent footholds, on the caller-owned state f32 [N, 32] (per foot the last contact point, its age and a 0; the anchor at 20,
        the plane (a0, a1, a2) at 22), in place. contact f32 [N, 4]: a foot stands iff its entry is >= cfg.c_on. quat [N, 4] (xyzw), dof
        [N, 20, 2] and base_pos [N, 3], None: the sim's current state. query_xy [N, Q, 2]: world points at which the plane is evaluated.
        reset=True resets every env, reset_mask int32 [N] the envs whose entry is not 0. Outputs by keyword, each a caller-owned tensor
        that is filled (GROUND_OUTPUTS): normal [N, 4, 3], ground [N, 4], residual [N, 4], trunk [N, 6], theta_ref [N, 3], query_z
        [N, Q], info int32 [N]."""
        n = self.num_envs
        unknown = set(outputs) - set(self.GROUND_OUTPUTS)
        assert not unknown, f"unknown outputs: {sorted(unknown)}"
        f32, i32 = torch.float32, torch.int32
        nq = 0 if query_xy is None else int(query_xy.shape[1])
        assert query_xy is None or nq > 0, "query_xy needs at least one point per env"
        shapes = dict(normal=((n, 4, 3), f32), ground=((n, 4), f32), residual=((n, 4), f32), trunk=((n, 6), f32), theta_ref=((n, 3), f32),
                      query_z=((n, nq), f32), info=((n,), i32))
        checks = [(state, (n, abi.GROUND_NS), f32), (contact, (n, 4), f32), (quat, (n, 4), f32), (dof, (n, abi.NDOF, 2), f32),
                  (base_pos, (n, 3), f32), (reset_mask, (n,), i32), (query_xy, (n, nq, 2), f32)]
        checks += [(outputs.get(k),) + shapes[k] for k in self.GROUND_OUTPUTS]
        for t, sh, dt in checks:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, (tuple(t.shape), sh)
        assert state is not None and contact is not None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        check(self.L.wbc_sim_ground_estimate(self.h, C.byref(cfg), ptr(quat), ptr(dof), ptr(base_pos), ptr(contact), ptr(reset_mask), ptr(query_xy),
                                             nq, abi.GROUND_RESET if reset else 0, state.data_ptr(),
                                             *[ptr(outputs.get(k)) for k in self.GROUND_OUTPUTS], self._stream()), "wbc_sim_ground_estimate")

    # ---- foot slip detection and friction estimate (include/wbc_sim.h: wbc_sim_slip_detect) -------------------------------------------------
    SLIP_OUTPUTS = ("prob", "slip", "weight", "foot_vel", "speed", "distance", "mu", "mu_lower", "mu_env", "info")

    def slip_detect(self, cfg: "abi.WbcSlipCfg", state: torch.Tensor, contact: torch.Tensor, quat: Optional[torch.Tensor] = None,
                    dof: Optional[torch.Tensor] = None, base_vel: Optional[torch.Tensor] = None, ang_vel: Optional[torch.Tensor] = None,
                    foot_force: Optional[torch.Tensor] = None, normal: Optional[torch.Tensor] = None,
                    reset_mask: Optional[torch.Tensor] = None, mu_init: Optional[torch.Tensor] = None, reset: bool = False, **outputs) -> None:
        """One wbc_sim_slip_detect launch on the current stream: one control step of the foot slip detector and friction estimate on the
        caller-owned state f32 [N, 4, 8] (per foot p, s, t, c_prev, d, mu_i, w_i, m_i), in place. contact f32 [N, 4]: a foot stands iff
        its entry, clamped to [0, 1], is >= cfg.c_on. quat [N, 4] (xyzw), dof [N, 20, 2], base_vel [N, 3] (world) and ang_vel [N, 3]
        (trunk axes), None: the sim's current state. foot_force [N, 4, 3] (world), None: no friction update. normal [N, 4, 3], None:
        world z. reset=True resets every env, reset_mask int32 [N] the envs whose entry is not 0, to mu_init [N, 4] (None: cfg.mu_prior).
        Outputs by keyword, each a caller-owned tensor that is filled (SLIP_OUTPUTS): prob, weight, speed, distance, mu, mu_lower
        [N, 4], slip u8 [N, 4], foot_vel [N, 4, 3], mu_env [N, 2], info int32 [N]."""
        n = self.num_envs
        unknown = set(outputs) - set(self.SLIP_OUTPUTS)
        assert not unknown, f"unknown outputs: {sorted(unknown)}"
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        shapes = dict(prob=((n, 4), f32), slip=((n, 4), u8), weight=((n, 4), f32), foot_vel=((n, 4, 3), f32), speed=((n, 4), f32),
                      distance=((n, 4), f32), mu=((n, 4), f32), mu_lower=((n, 4), f32), mu_env=((n, 2), f32), info=((n,), i32))
        checks = [(state, (n, 4, abi.SLIP_NS), f32), (contact, (n, 4), f32), (quat, (n, 4), f32), (dof, (n, abi.NDOF, 2), f32),
                  (base_vel, (n, 3), f32), (ang_vel, (n, 3), f32), (foot_force, (n, 4, 3), f32), (normal, (n, 4, 3), f32),
                  (reset_mask, (n,), i32), (mu_init, (n, 4), f32)]
        checks += [(outputs.get(k),) + shapes[k] for k in self.SLIP_OUTPUTS]
        for t, sh, dt in checks:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == sh, (tuple(t.shape), sh)
        assert state is not None and contact is not None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        check(self.L.wbc_sim_slip_detect(self.h, C.byref(cfg), ptr(quat), ptr(dof), ptr(base_vel), ptr(ang_vel), ptr(contact), ptr(foot_force),
                                         ptr(normal), ptr(reset_mask), ptr(mu_init), abi.SLIP_RESET if reset else 0, state.data_ptr(),
                                         *[ptr(outputs.get(k)) for k in self.SLIP_OUTPUTS], self._stream()), "wbc_sim_slip_detect")

    def proximity_damper_rows(self, gap: torch.Tensor, jac: torch.Tensor, d_safe: float, d_influence: float, xi: float, dt: float,
                              nu: Optional[torch.Tensor] = None):
        """The velocity damper of the pairs inside the influence distance as rows on the accelerations, torch ops only: the gap rate
        after one step, jac . (nu + dt nudot), may not fall below -xi (gap - d_safe) / (d_influence - d_safe), i.e. A nudot >= b with
        A = dt jac [N, P, 26] and b = -xi (gap - d_safe) / (d_influence - d_safe) - jac . nu [N, P]. A pair with gap >= d_influence has
        its row zeroed and b = -inf (never binding). nu f32 [N, 26] in the coordinates of jac; None: the sim's current velocities.
        Handing the rows to the task-space QP (wbc_sim_task_inverse_dynamics_qp takes no extra rows yet) is the follow-up."""
        assert d_influence > d_safe and dt > 0
        if nu is None:
            nu = torch.cat([self.tensor("ROOT_STATES")[:, 0, 7:13], self.tensor("DOF_STATE")[:, :, 1]], dim=1)
        near = gap < d_influence
        a = torch.where(near.unsqueeze(-1), jac * dt, torch.zeros_like(jac))
        b = -xi * (gap - d_safe) / (d_influence - d_safe) - torch.einsum("npc,nc->np", jac, nu)
        return a, torch.where(near, b, torch.full_like(b, float("-inf")))

    # ---- analytic derivatives of inverse and forward dynamics (include/wbc_sim.h: wbc_sim_inverse_dynamics_derivatives) ----------------
    def inverse_dynamics_derivatives(self, nudot: Optional[torch.Tensor] = None, dq: Optional[torch.Tensor] = None,
                                     dnu: Optional[torch.Tensor] = None, transposed: bool = False):
        """One wbc_sim_inverse_dynamics_derivatives launch on the current stream. Returns (dtau_dq, dtau_dnu), f32 [N, 26, 26] with
        [e, i, j] = d tau_i / d x_j ([e, j, i] with transposed: one direction's 26 values contiguous, what mass_solve reads), in the
        tangent convention of include/wbc_sim.h (world-frame rotation vector, world components of nu / nudot held fixed). Outputs that
        are not passed are allocated; nudot f32 [N, 26] in the convention of inverse_dynamics, None: zeros. A launch that writes one
        output goes through the C-ABI with a NULL pointer."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        outs = [torch.empty((n, ncol, ncol), dtype=torch.float32, device=self.device) if t is None else t for t in (dq, dnu)]
        for t, sh in zip([nudot] + outs, ((n, ncol), (n, ncol, ncol), (n, ncol, ncol))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        check(self.L.wbc_sim_inverse_dynamics_derivatives(self.h, nudot.data_ptr() if nudot is not None else None, outs[0].data_ptr(),
                                                          outs[1].data_ptr(), 2 if transposed else 0, self._stream()),
              "wbc_sim_inverse_dynamics_derivatives")
        return tuple(outs)

    def forward_dynamics_derivatives(self, tau: Optional[torch.Tensor] = None, nudot: Optional[torch.Tensor] = None,
                                     dq: Optional[torch.Tensor] = None, dnu: Optional[torch.Tensor] = None,
                                     minv: Optional[torch.Tensor] = None, armature: bool = False, transposed: bool = False):
        """wbc_sim_forward_dynamics_derivatives on the current stream. Returns (nudot [N, 26], dnudot_dq, dnudot_dnu, minv [N, 26, 26]):
        nudot = M^-1 (tau - h) (tau None: zeros), its partial derivatives in the layout and tangent convention of
        inverse_dynamics_derivatives, and d nudot / d tau = M^-1. armature: M + diag(0_6, joint_armature) throughout. Outputs that are
        not passed are allocated; the workspace is cached on the sim."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        if nudot is None:
            nudot = torch.empty((n, ncol), dtype=torch.float32, device=self.device)
        outs = [torch.empty((n, ncol, ncol), dtype=torch.float32, device=self.device) if t is None else t for t in (dq, dnu, minv)]
        for t, sh in zip([tau, nudot] + outs, ((n, ncol), (n, ncol)) + ((n, ncol, ncol),) * 3):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        assert tau is None or abs(tau.data_ptr() - nudot.data_ptr()) >= 4 * nudot.numel(), "nudot overlaps tau"
        if "_fdd_ws" not in self.__dict__:
            self._fdd_ws = torch.empty(int(self.L.wbc_sim_forward_dynamics_derivatives_workspace_floats(n)), dtype=torch.float32,
                                       device=self.device)
        check(self.L.wbc_sim_forward_dynamics_derivatives(self.h, tau.data_ptr() if tau is not None else None, nudot.data_ptr(),
                                                          *[t.data_ptr() for t in outs], (1 if armature else 0) | (2 if transposed else 0),
                                                          self._fdd_ws.data_ptr(), self._stream()), "wbc_sim_forward_dynamics_derivatives")
        return (nudot,) + tuple(outs)

    # ---- body-parameter regressor of inverse dynamics (include/wbc_sim.h: wbc_sim_inverse_dynamics_regressor) ---------------------------
    def _regressor_bodies(self, bodies):
        """(host index array or None, its length for the C-ABI, the number of bodies in the output)."""
        if bodies is None:
            return None, 0, abi.NB
        idx = [int(b) for b in (bodies.tolist() if isinstance(bodies, torch.Tensor) else bodies)]
        return (C.c_int32 * max(len(idx), 1))(*idx), len(idx), len(idx)

    def inverse_dynamics_regressor(self, bodies=None, nudot: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                                   native: bool = False, transposed: bool = False) -> torch.Tensor:
        """One wbc_sim_inverse_dynamics_regressor launch on the current stream: Y f32 [N, 26, K, 10] with [e, i, b, k] =
        d tau_i / d (parameter k of bodies[b]) of inverse_dynamics(nudot) at the current state; bodies: distinct moving-body indices
        (None: all nineteen, in order). Columns: the linear parameters (m, m c, inertia about the body origin; abi.linear_body_params),
        so that sum_b Y[:, :, b] @ pi_b is tau; native: (m, c, inertia about the centre of mass), the parametrisation of BODY_PARAMS.
        transposed: [N, K * 10, 26], what mass_solve reads. nudot f32 [N, 26], None: zeros. out: filled if given, else allocated."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        idx, k, nb = self._regressor_bodies(bodies)
        shape = (n, nb * abi.NPARAM, ncol) if transposed else (n, ncol, nb, abi.NPARAM)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        for t, sh in ((nudot, (n, ncol)), (out, shape)):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        flags = (abi.DERIV_TRANSPOSED if transposed else 0) | (abi.REGRESSOR_NATIVE if native else 0)
        check(self.L.wbc_sim_inverse_dynamics_regressor(self.h, idx, k, nudot.data_ptr() if nudot is not None else None, out.data_ptr(),
                                                        flags, self._stream()), "wbc_sim_inverse_dynamics_regressor")
        return out

    def forward_dynamics_sensitivity(self, bodies=None, tau: Optional[torch.Tensor] = None, armature: bool = False, native: bool = False,
                                     nudot: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                                     workspace: Optional[torch.Tensor] = None):
        """wbc_sim_forward_dynamics_sensitivity on the current stream. Returns (nudot [N, 26], dnudot_dpi [N, K * 10, 26]): nudot =
        M^-1 (tau - h) (tau None: zeros; the bits of forward_dynamics) and [e, b * 10 + k, i] = d nudot_i / d (parameter k of
        bodies[b]) = -M^-1 Y, parameter-major. bodies, native: as inverse_dynamics_regressor; armature: M + diag(0_6, joint_armature)
        in every solve. Outputs that are not passed are allocated. workspace: a caller-owned f32 tensor of the shape of dnudot_dpi;
        None: one buffer kept on the sim, as large as the largest request so far (81 MB for all bodies at 4096 envs;
        release_sensitivity_workspace() frees it)."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        idx, k, nb = self._regressor_bodies(bodies)
        shape = (n, nb * abi.NPARAM, ncol)
        if nudot is None:
            nudot = torch.empty((n, ncol), dtype=torch.float32, device=self.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        for t, sh in ((tau, (n, ncol)), (nudot, (n, ncol)), (out, shape)):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        assert tau is None or abs(tau.data_ptr() - nudot.data_ptr()) >= 4 * nudot.numel(), "nudot overlaps tau"
        if workspace is None:
            if "_fds_ws" not in self.__dict__ or self._fds_ws.numel() < out.numel():
                self._fds_ws = torch.empty(out.numel(), dtype=torch.float32, device=self.device)
            workspace = self._fds_ws
        else:
            assert workspace.device == self.arena.device and workspace.dtype == torch.float32 and workspace.is_contiguous()
            assert tuple(workspace.shape) == shape, tuple(workspace.shape)
        flags = (abi.SOLVE_ARMATURE if armature else 0) | (abi.REGRESSOR_NATIVE if native else 0)
        check(self.L.wbc_sim_forward_dynamics_sensitivity(self.h, idx, k, tau.data_ptr() if tau is not None else None, nudot.data_ptr(),
                                                          out.data_ptr(), workspace.data_ptr(), flags, self._stream()),
              "wbc_sim_forward_dynamics_sensitivity")
        return nudot, out

    def release_sensitivity_workspace(self) -> None:
        """Drop the buffer forward_dynamics_sensitivity keeps between calls (the next call without a workspace allocates again)."""
        self.__dict__.pop("_fds_ws", None)

    # ---- recursive identification of inertial parameters (include/wbc_sim.h: wbc_sim_identification_accumulate) ---------------------------
    def identification_accumulate(self, bodies, tau_gen: torch.Tensor, nudot: Optional[torch.Tensor] = None,
                                  row_weight: Optional[torch.Tensor] = None, forget: float = 1.0, info_mat: Optional[torch.Tensor] = None,
                                  info_vec: Optional[torch.Tensor] = None, stat: Optional[torch.Tensor] = None, target=None,
                                  reset: bool = False):
        """One wbc_sim_identification_accumulate launch on the current stream: A <- forget A + Phi^T W Phi, b <- forget b + Phi^T W z,
        stat <- forget stat + (sum w z^2, rows with w > 0) for the linear parameters of `bodies` (1..3 distinct moving-body indices) at
        the current state. tau_gen f32 [N, 26]: the net generalised force; nudot, row_weight f32 [N, 26] or None (zeros; 1 on the live
        rows). info_mat f32 [N, P, P], info_vec [N, P], stat [N, 2], P = 10 len(bodies): updated in place; the three are passed together,
        or all left out: then they are allocated and the call resets. reset: the incoming three are taken as zero. target f32 [N, 26]:
        z (None: allocated; False: not written). Returns (info_mat, info_vec, stat, target)."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        idx, k, nb = self._regressor_bodies(bodies)
        assert idx is not None and 1 <= k <= abi.IDENT_MAX_BODIES, bodies
        p = nb * abi.NPARAM
        state = (info_mat, info_vec, stat)
        assert all(t is None for t in state) or all(t is not None for t in state), "info_mat, info_vec and stat go together"
        if info_mat is None:
            info_mat = torch.empty((n, p, p), dtype=torch.float32, device=self.device)
            info_vec = torch.empty((n, p), dtype=torch.float32, device=self.device)
            stat = torch.empty((n, 2), dtype=torch.float32, device=self.device)
            reset = True
        if target is None:
            target = torch.empty((n, ncol), dtype=torch.float32, device=self.device)
        elif target is False:
            target = None
        for t, sh in ((tau_gen, (n, ncol)), (nudot, (n, ncol)), (row_weight, (n, ncol)), (info_mat, (n, p, p)), (info_vec, (n, p)),
                      (stat, (n, 2)), (target, (n, ncol))):
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        ptr = lambda x: x.data_ptr() if x is not None else None
        check(self.L.wbc_sim_identification_accumulate(self.h, idx, k, ptr(nudot), tau_gen.data_ptr(), ptr(row_weight), float(forget),
                                                       info_mat.data_ptr(), info_vec.data_ptr(), stat.data_ptr(), ptr(target),
                                                       abi.IDENT_RESET if reset else 0, self._stream()), "wbc_sim_identification_accumulate")
        return info_mat, info_vec, stat, target

    IDENT_OUTPUTS = ("pi_hat", "theta_hat", "cov_diag", "sse", "status")

    def identification_solve(self, info_mat: torch.Tensor, info_vec: torch.Tensor, stat: Optional[torch.Tensor] = None,
                             prior: Optional[torch.Tensor] = None, prior_weight: Optional[torch.Tensor] = None, pivot_tol: float = 1e-5,
                             want=IDENT_OUTPUTS, out=None):
        """One wbc_sim_identification_solve launch on the current stream: (A + diag(prior_weight)) pi_hat = b + prior_weight * prior per
        env, equilibrated, by fp32 Cholesky. info_mat [N, P, P], info_vec [N, P], stat [N, 2] as identification_accumulate leaves them;
        prior, prior_weight f32 [N, P / 10, 10] or None. Returns a dict with the names in `want` (a subset of IDENT_OUTPUTS, pi_hat
        always): pi_hat, theta_hat (m, c, I_c), cov_diag f32 [N, P / 10, 10], sse f32 [N] (needs stat), status int32 [N, P / 10] (bit 0:
        not solvable, the prior is returned; 1: m <= 0; 2: I_c not positive definite; 3: triangle inequality). out: an optional dict
        of caller-owned tensors under the same names."""
        n = self.num_envs
        assert info_mat.dim() == 3 and info_mat.shape[1] % abi.NPARAM == 0, tuple(info_mat.shape)
        p = int(info_mat.shape[1])
        nb = p // abi.NPARAM
        assert 1 <= nb <= abi.IDENT_MAX_BODIES, nb
        want = tuple(dict.fromkeys(("pi_hat",) + tuple(want)))
        assert all(w in self.IDENT_OUTPUTS for w in want), want
        assert "sse" not in want or stat is not None, "sse needs stat"
        out = dict(out) if out is not None else {}
        assert all(key in want for key in out), tuple(out)
        shapes = {"pi_hat": (n, nb, abi.NPARAM), "theta_hat": (n, nb, abi.NPARAM), "cov_diag": (n, nb, abi.NPARAM), "sse": (n,), "status": (n, nb)}
        res = {w: out[w] if out.get(w) is not None else
               torch.empty(shapes[w], dtype=torch.int32 if w == "status" else torch.float32, device=self.device) for w in want}
        for t, sh in [(info_mat, (n, p, p)), (info_vec, (n, p)), (stat, (n, 2)), (prior, shapes["pi_hat"]), (prior_weight, shapes["pi_hat"])] + \
                     [(res[w], shapes[w]) for w in want if w != "status"]:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == sh, tuple(t.shape)
        if "status" in res:
            t = res["status"]
            assert t.device == self.arena.device and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shapes["status"]
        ptr = lambda x: x.data_ptr() if x is not None else None
        check(self.L.wbc_sim_identification_solve(self.h, nb, info_mat.data_ptr(), info_vec.data_ptr(), ptr(stat), ptr(prior), ptr(prior_weight),
                                                  float(pivot_tol), *[ptr(res.get(w)) for w in self.IDENT_OUTPUTS], self._stream()),
              "wbc_sim_identification_solve")
        return res

    CDD_OUTPUTS = ("dnudot_dq", "dnudot_dnu", "dnudot_dtau", "dlambda_dq", "dlambda_dnu", "dlambda_dtau")

    def constrained_dynamics_derivatives(self, rigid_bodies, tau: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                                         acc_des: Optional[torch.Tensor] = None, damping: float = 0.0, armature: bool = False,
                                         transposed: bool = False, want=CDD_OUTPUTS, out=None):
        """wbc_sim_constrained_dynamics_derivatives on the current stream: constrained_dynamics' (nudot [N, 26], lam [N, K, 3]) for the
        same arguments and the partial derivatives of both with respect to q, nu and tau, in the tangent convention of
        inverse_dynamics_derivatives. Returns a dict with "nudot", "lambda" and the names in `want` (a subset of CDD_OUTPUTS; an
        output that is not wanted costs neither its walks nor its solves): dnudot_* f32 [N, 26, 26] with [e, i, j] = d nudot_i / d x_j,
        dlambda_* f32 [N, 3 K, 26] with [e, i, j] = d lambda_i / d x_j; with transposed [e, j, i], i.e. [N, 26, 26] and [N, 26, 3 K].
        out: an optional dict of caller-owned tensors under the same names (the rest are allocated). The workspace is cached per
        number of bodies."""
        n, ncol = self.num_envs, 6 + abi.NDOF
        rbs = [int(r) for r in (rigid_bodies.tolist() if isinstance(rigid_bodies, torch.Tensor) else rigid_bodies)]
        k = len(rbs)
        assert 1 <= k <= 5, k
        want = tuple(want)
        assert want and all(w in self.CDD_OUTPUTS for w in want), want
        out = dict(out) if out is not None else {}
        assert all(key in ("nudot", "lambda") + want for key in out), tuple(out)
        shapes = {"nudot": (n, ncol), "lambda": (n, k, 3)}
        for w in want:
            rows = ncol if w.startswith("dnudot") else 3 * k
            shapes[w] = (n, ncol, rows) if transposed else (n, rows, ncol)
        res = {key: out[key] if out.get(key) is not None else torch.empty(sh, dtype=torch.float32, device=self.device)
               for key, sh in shapes.items()}
        for t, shape in [(tau, (n, ncol)), (acc_des, (n, k, 3))] + [(res[key], sh) for key, sh in shapes.items()]:
            if t is not None:
                assert t.device == self.arena.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, tuple(t.shape)
        if active is not None:
            assert active.device == self.arena.device and active.dtype in (torch.bool, torch.uint8) and tuple(active.shape) == (n, k)
            active = active.contiguous()
            if active.dtype == torch.bool:
                active = active.view(torch.uint8)
        cache = self.__dict__.setdefault("_cdd_ws", {})
        if k not in cache:
            cache[k] = torch.empty(int(self.L.wbc_sim_constrained_dynamics_derivatives_workspace_floats(n, k)), dtype=torch.float32,
                                   device=self.device)
        ptr = lambda x: x.data_ptr() if x is not None else None
        check(self.L.wbc_sim_constrained_dynamics_derivatives(self.h, (C.c_int32 * k)(*rbs), k, ptr(active), ptr(tau), ptr(acc_des),
                                                              float(damping), (1 if armature else 0) | (2 if transposed else 0),
                                                              res["nudot"].data_ptr(), res["lambda"].data_ptr(),
                                                              *[ptr(res.get(w)) for w in self.CDD_OUTPUTS], cache[k].data_ptr(),
                                                              self._stream()), "wbc_sim_constrained_dynamics_derivatives")
        return res

    def episode_stats(self, scale: float, track_state: torch.Tensor = None, track_cap: int = 0) -> torch.Tensor:
        """Means over the envs that reset in the last step of their finished episode's reward sums [NREW] and metric
        sums [NMETRIC], times `scale`, as one fresh device tensor (WG:743-754 without a host sync). With `track_state`
        (wbc_runner_track_state_floats(n, cap) floats) the launch also advances the runner's episode deques (OPR:140-154)."""
        out = torch.empty(abi.NREW + abi.NMETRIC, dtype=torch.float32, device=self.device)
        prev = self.__dict__.get("_last_episode_stats")         # a step without resets re-publishes the previous values (WG:705-706)
        check(self.L.wbc_sim_episode_stats_track(self.h, float(scale), prev.data_ptr() if prev is not None else None, out.data_ptr(),
                                                 track_state.data_ptr() if track_state is not None else None, int(track_cap),
                                                 self._stream()), "wbc_sim_episode_stats")
        self._last_episode_stats = out
        return out

    def episode_stats_job(self, scale: float, track_state: torch.Tensor = None, track_cap: int = 0):
        """episode_stats without the launch: (out tensor, SideJob). Whoever takes the job executes it -- as extra workgroups of the
        policy inference that follows (ActorCritic.fused_act(side_job=...)) or stand-alone (SideJob.run) -- before the next step."""
        out = torch.empty(abi.NREW + abi.NMETRIC, dtype=torch.float32, device=self.device)
        prev = self.__dict__.get("_last_episode_stats")
        job = SideJob(self.L, (out, prev, track_state))
        check(self.L.wbc_sim_episode_stats_job(self.h, float(scale), prev.data_ptr() if prev is not None else None, out.data_ptr(),
                                               track_state.data_ptr() if track_state is not None else None, int(track_cap),
                                               C.byref(job.c)), "wbc_sim_episode_stats_job")
        self._last_episode_stats = out
        return out, job

    def set_dof_forces(self, torques: torch.Tensor) -> None:
        assert torques.is_cuda and torques.dtype == torch.float32 and torques.is_contiguous()
        check(self.L.wbc_sim_set_dof_forces(self.h, torques.data_ptr(), self._stream()), "wbc_sim_set_dof_forces")

    def simulate(self) -> None:
        check(self.L.wbc_sim_simulate(self.h, self._stream()), "wbc_sim_simulate")

    def set_root_state(self, root: torch.Tensor) -> None:
        check(self.L.wbc_sim_set_root_state(self.h, root.data_ptr(), self._stream()), "wbc_sim_set_root_state")

    def set_dof_state(self, dof: torch.Tensor) -> None:
        check(self.L.wbc_sim_set_dof_state(self.h, dof.data_ptr(), self._stream()), "wbc_sim_set_dof_state")

    def set_root_state_indexed(self, root: torch.Tensor, env_ids: torch.Tensor) -> None:
        ids = env_ids.to(torch.int32).contiguous()
        check(self.L.wbc_sim_set_root_state_indexed(self.h, root.data_ptr(), ids.data_ptr(), ids.numel(), self._stream()))

    def set_dof_state_indexed(self, dof: torch.Tensor, env_ids: torch.Tensor) -> None:
        ids = env_ids.to(torch.int32).contiguous()
        check(self.L.wbc_sim_set_dof_state_indexed(self.h, dof.data_ptr(), ids.data_ptr(), ids.numel(), self._stream()))

    def refresh_rigid_body_state(self) -> None:
        check(self.L.wbc_sim_refresh_rigid_body_state(self.h, self._stream()), "wbc_sim_refresh_rigid_body_state")
