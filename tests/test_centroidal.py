"""Centre of mass, centroidal momentum h_G, its rate, the centroidal momentum matrix A_G and the locked centroidal inertia I_G
(wbc_sim_centroidal, wbc_centroidal_kernel in csrc/wbc_arm_kernel.hip; definitions in include/wbc_sim.h). The CPU tests pin the fp64
direct sum of tests/centroidal_reference.py to independent routes -- the mass matrix, inverse dynamics and a central difference along
the flow -- and measure the fp32 yardstick; the GPU tests hold the kernel to the reference entry by entry, to the sibling kernels and
to its own invariances.

Bound: every entry of every output satisfies |kernel - ref| <= C 2^-24 mag, mag the reference's magnitude (the sizes of the terms
added; no term of an angular row grows with |v_root| or |nudot[0:3]|). K_ref is the fp32 yardstick's largest ratio over the two state
families below, 64 states each, with nudot given and NULL (asserted <= C / 16 on the CPU), C the smallest power of two >= 16 K_ref, and
the last column the kernel's largest ratio on an MI355X over n = 1, 13, 64, both families, nudot given and NULL:

    output                         K_ref     C       kernel's largest ratio
    com   (c - p_root, v, a)       3.20      64      2.51  (n = 64, nudot NULL)
    h_G                            3.24      64      2.22  (n = 64, fast)
    hdot_G                         2.75      64      2.80  (n = 64, nudot NULL)
    A_G                            15.1      256     27.8  (n = 13 and 64)
    inertia (m, I_G)               2.86      64      3.60  (n = 64)

A_G's largest entries are the linear rows of the arm's roll joints, whose axis nearly passes through the centres of mass they move. The
kernel's text compiled for the host (one thread per lane, a barrier for __syncthreads(), a stand-alone program under AddressSanitizer)
had predicted 1.97, 2.19, 2.70, 29.4 and 2.71 at n = 13. Against the sibling kernels the largest difference is 0.010 of the summed
allowances for A_G (mm_whole) and 0.0029 for hdot_G (inverse dynamics).

State families (seed s of _state): "slow" is tests/test_mass_solve.py's _random_state with random body params; "fast" is the same with
|v_root| in 2..10 m/s, |nudot[0:3]| in 10..50 m/s^2 and the root near (3, 110, 0). A yardstick that formed the angular rows from
absolute velocities would leave C / 16 on the fast family; the relative form does not see it.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import centroidal_reference as cr
import inverse_dynamics_reference as idr
import arm_codegen
import whole_body_reference as wb
from wbc_amd import abi

EPS, FAMILIES = cr.EPS, cr.FAMILIES
FINGERS = [6 + 18, 6 + 19]
SENTINEL = 12345.0
FAR = np.array([3.0, 110.0, 0.0])
SIZES = {"com": 9, "mom": 12, "cmm": 6 * 26, "inertia": 7}       # floats per env of the four output tensors
# The sibling kernels' allowances, restated: |tau - ref|_k <= C_ID 2^-24 mag_k (tests/test_inverse_dynamics.py) and
# |mm - ref| <= 1e-5 max |M_ref| per entry (tests/test_whole_body_dynamics.py).
C_ID = 4096.0
MM_REL = 1e-5


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _state(seed, fast):
    """(pos, quat, q, nu, body_params, nudot) of member `seed` of a family."""
    import test_mass_solve as tms
    rng = np.random.default_rng(700 + seed)
    pos, quat, q, nu = tms._random_state(rng)
    bp = tms._random_body_params(_model(), rng)
    nudot = np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]
    if fast:
        d = rng.normal(size=(2, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        nu[0:3] = d[0] * rng.uniform(2, 10)
        nudot[0:3] = d[1] * rng.uniform(10, 50)
        pos = pos + FAR
    return pos, quat, q, nu, bp, nudot


def _rotated(quat, w):
    import test_inverse_dynamics as tid
    th = np.linalg.norm(w)
    dq = np.r_[np.sin(th / 2) * w / th, np.cos(th / 2)] if th > 0 else np.array([0.0, 0.0, 0.0, 1.0])
    return tid._quat_mul(dq, quat)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.wbc_sim_centroidal(None, None, p, p, p, p, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_centroidal(None, None, None, None, None, None, None) == -1
    assert b"NULL" in L.wbc_last_error()


def test_centroidal_kernel_codegen():
    """The code object's metadata alone: no scratch, the launch's workgroup size, static LDS small enough for 16 workgroups per CU."""
    assert arm_codegen.meta("wbc_centroidal_kernel", "private_segment_fixed_size") == 0
    assert arm_codegen.meta("wbc_centroidal_kernel", "max_flat_workgroup_size") == 64
    assert arm_codegen.meta("wbc_centroidal_kernel", "group_segment_fixed_size") <= 160 * 1024 // 16


def test_reference_matrix_is_the_mass_matrix_moved_to_the_centre_of_mass():
    """A_G == [M[0:3] ; M[3:6] - (c - p_root) x M[0:3]], A_G nu == h_G, M[0, 0] == m, A_G[3:6, 3:6] == I_G; the exact blocks."""
    m = _model()
    for seed in range(20):
        pos, quat, q, nu, bp, _ = _state(seed, fast=seed % 2 == 1)
        out, mag = cr.centroidal(m, pos, quat, q, nu, None, bp)
        M = wb.mass_matrix(m, pos, quat, q, bp)
        c, A, mass = out["com"][0:3], out["cmm"], out["inertia"][0]
        assert np.abs(A - cr.shift_to_com(M[0:6], c)).max() <= 1e-13 * np.abs(M).max(), seed
        assert np.abs(A @ nu - out["mom"]).max() <= 1e-13 * np.abs(mag["mom"]).max(), seed
        assert abs(M[0, 0] - mass) <= 1e-14 * mass
        assert np.abs(A[3:6, 3:6] - wb._sym(out["inertia"][1:])).max() <= 1e-14 * np.abs(out["inertia"][1:]).max()
        assert np.all(A[0:3, 0:3] == mass * np.eye(3)) and np.all(A[3:6, 0:3] == 0) and np.all(A[:, FINGERS] == 0)
        assert np.all(mag["cmm"][3:6, 0:3] == 0) and np.all(mag["cmm"][:, FINGERS] == 0) and np.all(np.delete(mag["cmm"], FINGERS, 1)[0:3] > 0)
        # the centre of mass itself, by its definition, at the far position too
        R, p = cr.cdr._fk(m, pos, quat, q, np.float64)
        inert = wb.body_inertias(m, bp)
        cw = sum(mb * (p[b] + R[b] @ com) for b, (mb, com, _) in enumerate(inert)) / sum(mb for mb, _, _ in inert)
        assert np.abs(pos + c - cw).max() <= 1e-12


def test_reference_momentum_rate_is_the_derivative_of_the_momentum_along_the_flow():
    """hdot_G against the central difference of h_G along (q, nu, nudot): q +- eps qd, the root rotated by exp(+-eps omega^) and
    translated by +-eps v, nu +- eps nudot. fp64, error O(eps^2); a_com against the same difference of v_com."""
    m = _model()
    eps = 1e-5
    for seed in range(20):
        pos, quat, q, nu, bp, nudot = _state(seed, fast=seed % 2 == 1)
        nudot[FINGERS] = 0.0
        side = []
        for sgn in (1.0, -1.0):
            o, _ = cr.centroidal(m, pos + sgn * eps * nu[0:3], _rotated(quat, sgn * eps * nu[3:6]), q + sgn * eps * nu[6:],
                                 nu + sgn * eps * nudot, None, bp, cmm=False)
            side.append(np.r_[o["mom"], o["com"][3:6]])
        want = (side[0] - side[1]) / (2 * eps)
        out, mag = cr.centroidal(m, pos, quat, q, nu, nudot, bp, cmm=False)
        got = np.r_[out["momdot"], out["com"][6:9]]
        assert np.abs(got - want).max() <= 1e-8 * np.abs(mag["momdot"]).max(), (seed, np.abs(got - want).max())


def test_reference_momentum_rate_is_the_net_external_wrench_of_inverse_dynamics():
    """hdot_G == ((tau - g)[0:3] ; (tau - g)[3:6] - (c - p_root) x (tau - g)[0:3]) of inverse_dynamics_reference, with nudot and
    without."""
    m = _model()
    for seed in range(20):
        pos, quat, q, nu, bp, nudot = _state(seed, fast=seed % 2 == 1)
        g, _ = idr.gravity_forces(m, pos, quat, q, bp)
        for nd in (nudot, None):
            out, mag = cr.centroidal(m, pos, quat, q, nu, nd, bp, cmm=False)
            tau, _ = idr.inverse_dynamics(m, pos, quat, q, nu, nd, bp)
            want = cr.shift_to_com((tau - g)[0:6], out["com"][0:3])
            assert np.abs(out["momdot"] - want).max() <= 1e-12 * np.abs(mag["momdot"]).max(), seed


@functools.lru_cache(maxsize=None)
def _reference(seed, fast):
    """((out, mag) with nudot, (out, mag) without) of one family member in fp64; computed once and left unchanged."""
    pos, quat, q, nu, bp, nudot = _state(seed, fast)
    return cr.centroidal(_model(), pos, quat, q, nu, nudot, bp), cr.centroidal(_model(), pos, quat, q, nu, None, bp, cmm=False)


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output family: the fp32 yardstick's largest ratio over 64 members of each state family, nudot given and NULL."""
    m = _model()
    k = {f: 0.0 for f in FAMILIES}
    for fast in (False, True):
        for seed in range(64):
            pos, quat, q, nu, bp, nudot = _state(seed, fast)
            (out, mag), (out0, mag0) = _reference(seed, fast)
            y, _ = cr.centroidal(m, pos, quat, q, nu, nudot, bp, dtype=np.float32)
            y0, _ = cr.centroidal(m, pos, quat, q, nu, None, bp, dtype=np.float32, cmm=False)
            for f in FAMILIES:
                k[f] = max(k[f], cr.largest_ratio(y[f], out[f], mag[f]))
                if f != "cmm":
                    k[f] = max(k[f], cr.largest_ratio(y0[f], out0[f], mag0[f]))
    return k


def test_fp32_yardsticks_sit_well_inside_the_bounds():
    k = _yardsticks()
    print("centroidal yardsticks: " + ", ".join(f"{f} K_ref = {k[f]:.3g} (C = {cr.C[f]:g})" for f in FAMILIES))
    for f in FAMILIES:
        assert k[f] <= cr.C[f] / 16, (f, k[f])
        assert cr.C[f] == 2.0 ** np.ceil(np.log2(16 * k[f])), (f, k[f])


def test_magnitudes_do_not_grow_with_the_root_motion():
    """The angular rows' magnitudes are those of the same state with v_root = 0 and nudot[0:3] = 0, to the last bit."""
    m = _model()
    for seed in range(6):
        pos, quat, q, nu, bp, nudot = _state(seed, fast=True)
        _, mag = cr.centroidal(m, pos, quat, q, nu, nudot, bp, cmm=False)
        nu[0:3], nudot[0:3] = 0.0, 0.0
        _, still = cr.centroidal(m, pos, quat, q, nu, nudot, bp, cmm=False)
        assert np.all(mag["mom"][3:6] == still["mom"][3:6]) and np.all(mag["momdot"][3:6] == still["momdot"][3:6])
        assert np.all(mag["mom"][0:3] > still["mom"][0:3])


# ------------------------------------------------------------------------------------------------------------ GPU
def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(n, fast):
    """An env whose n robots hold members 0..n-1 of a family (state, body params), the nudot tensor, and the fp64 reference of every
    env at the sim's DOWNLOADED fp32 state, with nudot and without. Computed once and left unchanged."""
    import test_inverse_dynamics as tid
    env = tid._env(n, seed=5, steps=0)
    states = [_state(seed, fast) for seed in range(n)]
    root, dof = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    for e, (pos, quat, q, nu, _bp, _nd) in enumerate(states):
        root[e, 0] = torch.tensor(np.concatenate([pos, quat, nu[0:6]]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q, nu[6:]], -1), dtype=torch.float32)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    env.sim.tensor("BODY_PARAMS").copy_(torch.tensor(np.array([s[4] for s in states]), dtype=torch.float32))
    nudot = torch.tensor(np.array([s[5] for s in states]), dtype=torch.float32, device="cuda").contiguous()
    torch.cuda.synchronize()
    m = env.robot_model
    r64 = env.sim.tensor("ROOT_STATES")[:, 0].cpu().numpy().astype(np.float64)
    d64 = env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64)
    b64 = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    n64 = nudot.cpu().numpy().astype(np.float64)
    args = lambda e: (m, r64[e, :3], r64[e, 3:7], d64[e, :, 0], np.r_[r64[e, 7:13], d64[e, :, 1]])
    with_nd = [cr.centroidal(*args(e), n64[e], b64[e]) for e in range(n)]
    without = [cr.centroidal(*args(e), None, b64[e], cmm=False) for e in range(n)]
    return env, nudot, with_nd, without, (r64, d64, b64, n64)


def _launch(env, nudot, which=("com", "mom", "cmm", "inertia")):
    """A direct C-ABI call into sentinel-framed buffers; returns {name: [n, ...] tensor} of the outputs asked for."""
    n = env.num_envs
    bufs = {k: _sentinel_buffer(n * SIZES[k]) for k in which}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None
    rc = env.sim.L.wbc_sim_centroidal(env.sim.h, nudot.data_ptr() if nudot is not None else None, ptr("com"), ptr("mom"), ptr("cmm"),
                                      ptr("inertia"), None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[n * SIZES[k]:] == SENTINEL).all()), k
    return {k: b[:n * SIZES[k]].view(n, -1).clone() for k, b in bufs.items()}


def _ratios(got, refs):
    """Largest ratio per output family over every env and entry; got: {name: [n, ...]} of the kernel, refs: [(out, mag)] per env."""
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    worst = {}
    for e, (out, mag) in enumerate(refs):
        mine = {"com": g["com"][e], "mom": g["mom"][e, 0:6], "momdot": g["mom"][e, 6:12], "inertia": g["inertia"][e]}
        if out["cmm"] is not None:
            mine["cmm"] = g["cmm"][e].reshape(6, 26)
        for f, x in mine.items():
            worst[f] = max(worst.get(f, 0.0), cr.largest_ratio(x, out[f], mag[f]))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["slow", "fast"])
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_and_entry_of_every_output(n, fast):
    env, nudot, with_nd, without, _ = _case(n, fast)
    got, got0 = _launch(env, nudot), _launch(env, None)
    for tag, g, refs in (("nudot", got, with_nd), ("NULL", got0, without)):
        worst = _ratios(g, refs)
        print(f"centroidal n={n} {'fast' if fast else 'slow'} {tag}: largest |kernel - ref| / (2^-24 mag): {worst}")
        for f, w in worst.items():
            assert w <= cr.C[f], (tag, f, w)
    # what does not depend on nudot does not move with it
    assert torch.equal(got["cmm"], got0["cmm"]) and torch.equal(got["inertia"], got0["inertia"])
    assert torch.equal(got["com"][:, 0:6], got0["com"][:, 0:6]) and torch.equal(got["mom"][:, 0:6], got0["mom"][:, 0:6])
    # the exact blocks of A_G, as equalities
    A, mass = got["cmm"].view(n, 6, 26), got["inertia"][:, 0]
    assert torch.equal(A[:, 0:3, 0:3], mass[:, None, None] * torch.eye(3, device="cuda")) and bool((mass > 0).all())
    assert bool((A[:, 3:6, 0:3] == 0).all()) and bool((A[:, :, FINGERS] == 0).all())
    # the fingers' entries of nudot are ignored
    nd2 = nudot.clone(); nd2[:, FINGERS] = 7.0
    again = _launch(env, nd2)
    assert all(torch.equal(again[k], got[k]) for k in got)
    # the Python entry points are the same call
    com, mom, cmm, inr = env.sim.centroidal(nudot)
    assert com.shape == (n, 9) and mom.shape == (n, 12) and cmm.shape == (n, 6, 26) and inr.shape == (n, 7)
    assert torch.equal(com, got["com"]) and torch.equal(mom, got["mom"]) and torch.equal(cmm.view(n, -1), got["cmm"]) and torch.equal(inr, got["inertia"])
    pos, vel = env.centre_of_mass()
    assert torch.equal(pos, env.root_states[:, 0:3] + got["com"][:, 0:3]) and torch.equal(vel, got["com"][:, 3:6])
    h, hd = env.centroidal_momentum(nudot)
    assert torch.equal(h, got["mom"][:, 0:6]) and torch.equal(hd, got["mom"][:, 6:12])
    assert torch.equal(env.centroidal_momentum()[1], got0["mom"][:, 6:12])
    assert torch.equal(env.centroidal_momentum_matrix(), cmm)
    mass2, IG = env.centroidal_inertia()
    assert torch.equal(mass2, mass) and IG.shape == (n, 3, 3) and torch.equal(IG, IG.transpose(1, 2))
    assert torch.equal(IG[:, [0, 1, 2, 0, 0, 1], [0, 1, 2, 1, 2, 2]], got["inertia"][:, 1:7]) and torch.equal(IG, A[:, 3:6, 3:6])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_single_output_calls_give_the_bits_of_the_all_outputs_call(n):
    env, nudot, _, _, _ = _case(n, True)
    for nd in (nudot, None):
        full = _launch(env, nd)
        for k in SIZES:
            one = _launch(env, nd, which=(k,))
            assert torch.equal(one[k], full[k]), k
        pair = _launch(env, nd, which=("mom", "inertia"))
        assert torch.equal(pair["mom"], full["mom"]) and torch.equal(pair["inertia"], full["inertia"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_agrees_with_the_sibling_kernels(n):
    """A_G against the base rows of mm_whole moved to the centre of mass, hdot_G against inverse_dynamics(nudot) - gravity_forces()
    moved likewise (the fp64 reference's c moves both), each at the sum of both sides' bounds."""
    env, nudot, with_nd, _, (r64, d64, b64, n64) = _case(n, False)
    m = env.robot_model
    got = _launch(env, nudot)
    env.refresh_mass_matrix_tensors()
    tau, grav = env.inverse_dynamics(nudot), env.gravity_forces()
    torch.cuda.synchronize()
    A = got["cmm"].view(n, 6, 26).double().cpu().numpy()
    hd = got["mom"][:, 6:12].double().cpu().numpy()
    M = env.mm_whole.double().cpu().numpy()
    wrench = (tau.double() - grav.double()).cpu().numpy()
    g = [float(x) for x in env.tcfg.gravity]
    worst = [0.0, 0.0]
    for e in range(n):
        out, mag = with_nd[e]
        c = out["com"][0:3]
        lever = np.abs(c).sum()
        args = (m, r64[e, :3], r64[e, 3:7], d64[e, :, 0])
        bM = MM_REL * np.abs(wb.mass_matrix(*args, b64[e])).max()
        allow = cr.C["cmm"] * EPS * mag["cmm"] + bM * np.r_[np.ones(3), np.full(3, 1.0 + lever)][:, None]
        diff = np.abs(A[e] - cr.shift_to_com(M[e, 0:6], c))
        diff[:, FINGERS] = 0.0
        assert np.all(diff <= allow), ("cmm", e, float((diff / allow).max()))
        worst[0] = max(worst[0], float((diff / allow).max()))
        _, mt = idr.inverse_dynamics(*args, np.r_[r64[e, 7:13], d64[e, :, 1]], n64[e], b64[e], g)
        _, mg = idr.gravity_forces(*args, b64[e], g)
        bW = C_ID * EPS * (mt + mg)[0:6]
        allow = cr.C["momdot"] * EPS * mag["momdot"] + np.r_[bW[0:3], bW[3:6] + lever * bW[0:3].max()]
        diff = np.abs(hd[e] - cr.shift_to_com(wrench[e, 0:6], c))
        assert np.all(diff <= allow), ("momdot", e, float((diff / allow).max()))
        worst[1] = max(worst[1], float((diff / allow).max()))
    print(f"centroidal n={n} vs siblings: largest difference / allowance: A_G vs mm_whole {worst[0]:.3g}, hdot_G vs inverse dynamics {worst[1]:.3g}")


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    nudot = tid._random_nudot(n, 89)
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        outs.append([t.clone() for t in env.sim.centroidal(nudot)])
        torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert bool(x.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env, nudot, _, _, _ = _case(n, True)
    want = env.sim.centroidal(nudot)
    want0 = env.sim.centroidal()[1]
    outs = [torch.zeros_like(t) for t in want]
    mom0 = torch.zeros_like(want0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream
        env.sim.centroidal(nudot, *outs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in outs:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.centroidal(nudot, *outs)
        assert env.sim.L.wbc_sim_centroidal(env.sim.h, None, None, mom0.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want)) and torch.equal(mom0, want0)


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env, nudot, _, _, _ = _case(n, False)
    L, h = env.sim.L, env.sim.h
    bufs = {k: _sentinel_buffer(n * SIZES[k]) for k in SIZES}
    names = ("sim", "nudot", "com", "mom", "cmm", "inertia", "stream")
    base = dict(sim=h, nudot=nudot.data_ptr(), stream=None, **{k: b.data_ptr() for k, b in bufs.items()})
    call = lambda **kw: L.wbc_sim_centroidal(*[kw.get(k, base[k]) for k in names])
    refusals = [(dict(sim=None), b"NULL"), (dict(com=None, mom=None, cmm=None, inertia=None), b"NULL"),
                (dict(nudot=nudot.data_ptr() + 1), b"aligned"), (dict(nudot=nudot.data_ptr() + 2), b"aligned")]
    refusals += [({k: bufs[k].data_ptr() + off}, b"aligned") for k in SIZES for off in (1, 2, 3)]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for b in bufs.values():
        assert bool((b == SENTINEL).all())
    # 4-byte alignment is all that is needed: every output one float into its buffer
    want = _launch(env, nudot)
    assert call(**{k: b.data_ptr() + 4 for k, b in bufs.items()}) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert torch.equal(b[1:1 + n * SIZES[k]].view(n, -1), want[k]) and float(b[0]) == SENTINEL and bool((b[1 + n * SIZES[k]:] == SENTINEL).all()), k


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_calls():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        b = torch.ones(n, 26, device="cuda")
        for _ in range(5):
            if use:
                env.sim.centroidal(b); env.centre_of_mass()
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.centroidal_momentum(); env.centroidal_momentum_matrix(); env.centroidal_inertia()
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
