"""Self-collision proximity (wbc_sim_proximity: wbc_proximity_kernel in csrc/wbc_proximity_kernel.hip; definitions in include/wbc_sim.h): the
signed gaps of the robot's 44 limb pairs and 3 arm spheres against the trunk box, the unit normals, the witness points and the rows
d gap / d q. The CPU tests pin the fp64 restatement of tests/proximity_reference.py to what exists -- its own gap's Richardson differences
through the joint angles, the brute-force geometry of tests/self_collision_geometry.py -- and measure the fp32 yardstick; the GPU tests hold
the kernel to the reference entry by entry and to a certificate that needs no reference feature choice.

Families: "random" is seed 4000 + e of ik_reference.random_configuration(spread=0.9); "near" holds, for every pair that has one, the first
seed of 4000 .. 6999 whose gap for that pair lies in [-5 mm, 20 mm] (41 of the 47 pairs: 39 limb pairs, the gripper and the wrist against
the trunk). Env e of a GPU case holds member e of its family (the near family repeats). The reference is evaluated at the sim's
downloaded fp32 state.

Judged: an (env, pair) case with tie >= 1 mm and core >= 5 mm; jac and witness additionally need sin2 >= 1e-2 or a clamped parameter
(proximity_reference's conditioning numbers). Every test asserts that this leaves out at most 5 % of its cases (random family on the CPU:
47 of 3008). The cases left out are still held to the certificate.

Bound: every judged entry satisfies |kernel - ref| <= C 2^-24 mag, mag the reference's rotation-invariant magnitude (proximity_reference),
structural zeros as equalities. C is 4 x K_ref rounded up to a power of two, K_ref the fp32 yardstick's largest ratio over both families,
measured on the CPU and asserted there; it never comes from the kernel. The kernel's largest ratio on an MI355X (n = 1, 13, 64):

    output     K_ref     kernel's largest ratio          C
    gap        1.95      2.31  (n = 64)                  8
    normal     1.65      2.26  (n = 64)                  8
    witness    0.61      0.90  (n = 64)                  4
    jac        122       113   (n = 64)                  512

jac's K_ref is large because its magnitude |c - p_joint| + L |axis x (c - p_joint)| / core vanishes with the lever, while WHERE on its
shaft the core point lies depends on the other limb's position, which carries the rounding of a position (2^-24 of its distance from the
root, over the sine of the shafts' angle): a core point 2 mm from its own joint is the worst case. The kernel builds every lever from
the joint's own origin outwards; with the lever as the difference of two root-relative points its largest ratio was 509.

Certificate (every case, those left out included), largest fraction of the allowance on the MI355X: a witness off its primitive's surface
0.21, the witnesses' separation along n against the gap 0.44, the gap against the fp64 gap 0.29; | |n| - 1 | at most 0.51 of 4 x 2^-24.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import proximity_reference as px
from wbc_amd import abi

EPS, FAMILIES = px.EPS, px.FAMILIES
NCOL = 26
SENTINEL = 12345.0
ISENTINEL = -7777
# K_ref, the kernel's largest ratio on the MI355X (the docstring's table; for the record, no bound comes from it) and the constant
K_REF = {"gap": 1.95, "normal": 1.65, "witness": 0.61, "jac": 122.0}
K_GPU = {"gap": 2.31, "normal": 2.26, "witness": 0.90, "jac": 113.0}
CONST = {"gap": 8.0, "normal": 8.0, "witness": 4.0, "jac": 512.0}
assert all(CONST[f] == 2.0 ** np.ceil(np.log2(4 * K_REF[f])) for f in FAMILIES)
# |analytic row - Richardson difference of the reference's own gap| / sum of the row's levers |c - p_joint|: 4 x what fp64 was measured to give
# (central differences at 1e-5 and 5e-6 rad: rounding 2^-53 x 1 m / 5e-6 and the second derivative's jump where a parameter meets its clamp)
TOL_GRADIENT = 4e-10
TOL_OLD_GEOMETRY = 1e-12
LEFT_OUT_MAX = 0.05
NEAR_MIN_LIMB_PAIRS = 36
# static LDS bytes (19 frames of 16 floats, 19 x 6 joint-to-body vectors, the [64][26] tile, 64 gaps) and VGPRs of wbc_proximity_kernel,
# as DESIGN.md records them
LDS_BYTES, VGPRS = 9504, 77


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _members(family):
    m = _model()
    if family == "random":
        return [px.random_member(m, 4000 + e) for e in range(64)]
    return [px.random_member(m, seed) for _, seed in px.near_family(m)]


@functools.lru_cache(maxsize=None)
def _cpu_refs(family):
    """[(out, mag, cond, aux)] of the family's members at their fp64 states. Computed once and left unchanged."""
    return [px.proximity(_model(), quat, q) for quat, q in _members(family)]


def _rows(cond):
    a, b = px.judged(cond)
    return {"gap": a, "normal": a, "witness": b, "jac": b}


def _left_out(refs):
    out = sum(int((~px.judged(r[2])[1]).sum()) for r in refs)
    return out, sum(len(r[2]["tie"]) for r in refs)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_pair_list_is_the_models():
    m = _model()
    pairs, names = px.pair_list(m), px.pair_names(m)
    assert len(pairs) == 47 and [k for k, _, _ in pairs] == [abi.PR_LIMBS] * 44 + [abi.PR_STATIC] * 3
    assert names[44:] == [("gripper", "trunk"), ("wrist", "trunk"), ("elbow", "trunk")]
    _, limbs, _ = abi.collision_set(m)
    assert tuple(l["name"] for l in limbs) == abi.LIMB_NAMES and len(abi.SPHERE_NAMES) == abi.NSPH
    # the wbc_model carries the same list: the limb lanes in lane order, then the static pairs on the root body
    wm = abi.fill_model(m)
    lanes = [(wm.pr_a[k], wm.pr_b[k]) for k in range(abi.NCP) if wm.pr_kind[k] == abi.PR_LIMBS]
    static = [(wm.cp_sph[k], wm.cp_rb2[k]) for k in range(wm.ncp) if wm.cp_kind[k] == abi.CP_BOX and wm.cp_body2[k] != abi.BOX_BODY]
    assert lanes + static == [(a, b) for _, a, b in pairs]
    bare = abi.fill_model(m, self_collisions=False)
    assert not any(bare.pr_kind[k] == abi.PR_LIMBS or bare.cp_kind[k] == abi.CP_BOX for k in range(abi.NCP))


def test_prototypes_and_refusals_without_a_device():
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    for fn in ("wbc_sim_proximity_pair_count", "wbc_sim_proximity_pairs", "wbc_sim_proximity"):
        assert fn in EXPORTED_SYMBOLS and hasattr(L, fn)
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.wbc_sim_proximity(None, p, p, p, p, p, 3, None) == -1
    assert L.wbc_last_error().startswith(b"wbc_sim_proximity: ") and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_proximity_pair_count(None) == -1
    assert L.wbc_last_error().startswith(b"wbc_sim_proximity_pair_count: ") and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_proximity_pairs(None, p) == -1
    assert L.wbc_last_error().startswith(b"wbc_sim_proximity_pairs: ") and b"NULL" in L.wbc_last_error()
    assert all(x == 0.0 for x in buf)


@functools.lru_cache(maxsize=None)
def _kernel_assembly():
    """csrc/wbc_proximity_kernel.hip compiled to gfx950 assembly with the build's own flags, as arm_codegen does for wbc_arm_kernel.hip (the
    kernel has a translation unit of its own, because tests/test_identification.py pins the number of kernels in that one)."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    if not os.path.exists(arm_codegen.HIPCC):
        pytest.skip("hipcc not installed")
    source = "wbc_proximity_kernel.hip"
    assert source in g.SOURCES and "wbc_proximity.h" in g.HEADERS
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "proximity.s")
        subprocess.check_call([arm_codegen.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        return open(out).read()


def test_proximity_kernel_codegen():
    """The code object's metadata alone: one kernel, no scratch, a single wavefront per workgroup and therefore no s_barrier, the static
    LDS and the VGPR count DESIGN.md states."""
    import re
    text = _kernel_assembly()
    assert text.count(".amdhsa_kernel ") == 1
    entry = text[text.index("amdhsa.kernels:"):]
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))
    assert re.search(r"\.name:\s+wbc_proximity_kernel\n", entry)
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64
    assert meta("group_segment_fixed_size") == LDS_BYTES and meta("vgpr_count") == VGPRS
    body = text[text.index("\nwbc_proximity_kernel:"):]
    body = body[:body.index(".Lfunc_end")]
    print(f"wbc_proximity_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert "s_endpgm" in body and "scratch_" not in body and "s_barrier" not in body


def test_reference_row_is_the_gradient_of_its_own_gap():
    """Richardson differences (central, steps 1e-5 and 5e-6 rad) of the reference's fp64 gap through every live joint angle against its
    analytic row, on the judged cases of six members of each family."""
    m = _model()
    worst, cases = 0.0, 0
    for family in ("random", "near"):
        for (quat, q), (out, mag, cond, _) in list(zip(_members(family), _cpu_refs(family)))[:6]:
            rows = px.judged(cond)[1]
            grad = np.zeros((len(rows), NCOL))
            for d in range(abi.NJ):
                def diff(h):
                    side = []
                    for s in (1.0, -1.0):
                        qq = np.array(q, dtype=np.float64); qq[d] += s * h
                        side.append(px.proximity(m, quat, qq, rows=False)[0]["gap"])
                    return (side[0] - side[1]) / (2 * h)
                grad[:, 6 + d] = (4 * diff(5e-6) - diff(1e-5)) / 3
            err = np.abs(grad - out["jac"]).max(1) / np.maximum(cond["lever"].sum(1), 1e-300)
            assert np.all(out["jac"][:, :6] == 0) and np.all(out["jac"][:, 24:] == 0)
            worst, cases = max(worst, float(err[rows].max())), cases + int(rows.sum())
    print(f"proximity reference: largest |row - Richardson difference| / sum |lever| {worst:.3g} over {cases} (env, pair) cases")
    assert worst <= TOL_GRADIENT


def test_reference_gap_is_the_old_geometry():
    """self_collision_geometry.all_pairs at the same poses: the 44 limb pairs and the three spheres against the trunk."""
    m = _model()
    worst = 0.0
    for family in ("random", "near"):
        table = px.old_geometry_gaps(m, _members(family))
        gap = np.array([r[0]["gap"] for r in _cpu_refs(family)])
        for i, nm in enumerate(px.pair_names(m)):
            worst = max(worst, float(np.abs(px.old_gap(table, nm) - gap[:, i]).max()))
    print(f"proximity reference: largest |gap - self_collision_geometry's| {worst:.3g}")
    assert worst <= TOL_OLD_GEOMETRY


def test_families_are_the_ones_the_bounds_were_stated_for():
    m = _model()
    refs = _cpu_refs("random")
    gap = np.array([r[0]["gap"][:44] for r in refs])
    out, total = _left_out(refs)
    print(f"random family: {out} of {total} left out; gaps {gap.min():.4f} .. {gap.max():.4f} m, {(gap < 0.02).mean():.4f} below 20 mm")
    assert total == 64 * 47 and out <= LEFT_OUT_MAX * total
    assert gap.min() < -0.03 and gap.max() > 0.9 and 0.005 < (gap < 0.02).mean() < 0.02
    near = px.near_family(m)
    refs = _cpu_refs("near")
    out, total = _left_out(refs)
    assert sum(1 for i, _ in near if i < 44) >= NEAR_MIN_LIMB_PAIRS and {44, 45} <= {i for i, _ in near}
    for (i, _), r in zip(near, refs):
        assert px.NEAR_LO - 1e-9 <= r[0]["gap"][i] <= px.NEAR_HI + 1e-9, (i, r[0]["gap"][i])
    print(f"near family: {len(near)} members, {out} of {total} left out")
    assert out <= LEFT_OUT_MAX * total


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output: the fp32 yardstick's largest ratio over the judged entries of both families."""
    m = _model()
    k = {f: 0.0 for f in FAMILIES}
    for family in ("random", "near"):
        for (quat, q), (out, mag, cond, _) in zip(_members(family), _cpu_refs(family)):
            y = px.proximity(m, quat, q, dtype=np.float32)[0]
            rows = _rows(cond)
            for f in FAMILIES:
                k[f] = max(k[f], px.largest_ratio(y[f], out[f], mag[f], rows[f]))
    return k


def test_fp32_yardstick_is_where_the_constants_came_from():
    k = _yardsticks()
    print("proximity yardsticks: " + ", ".join(f"{f} K_ref = {k[f]:.3g} (C = {CONST[f]:g})" for f in FAMILIES))
    for f in FAMILIES:
        assert abs(k[f] - K_REF[f]) <= 0.25 * K_REF[f], (f, k[f])          # a largest ratio moves with the summation order of the BLAS at hand
        assert 4 * k[f] <= CONST[f]


def test_damper_rows_against_a_hand_written_case():
    """One env, three pairs, two columns in use: a pair inside the influence distance and closing, one at the safety distance, one outside."""
    from wbc_amd.sim import WbcSim
    gap = torch.tensor([[0.06, 0.02, 0.30]])
    jac = torch.zeros(1, 3, NCOL)
    jac[0, 0, 6], jac[0, 0, 7] = 0.5, -0.25
    jac[0, 1, 8] = 1.0
    jac[0, 2, 9] = 2.0
    nu = torch.zeros(1, NCOL)
    nu[0, 6], nu[0, 7], nu[0, 8], nu[0, 9] = 1.0, 2.0, -3.0, 4.0
    A, b = WbcSim.proximity_damper_rows(None, gap, jac, d_safe=0.02, d_influence=0.10, xi=2.0, dt=0.01, nu=nu)
    assert A.shape == (1, 3, NCOL) and b.shape == (1, 3)
    # pair 0: jac . nu = 0.5 - 0.5 = 0, b = -2 (0.06 - 0.02) / 0.08 = -1; pair 1: at d_safe, b = 0 - (-3) = 3; pair 2: outside
    assert torch.allclose(A[0, 0], 0.01 * jac[0, 0]) and torch.allclose(A[0, 1], 0.01 * jac[0, 1]) and bool((A[0, 2] == 0).all())
    assert torch.allclose(b[0, :2], torch.tensor([-1.0, 3.0])) and float(b[0, 2]) == float("-inf")
    # the rows say what they mean: the acceleration that just satisfies row 1 leaves the gap rate at its bound after dt
    nudot = torch.zeros(NCOL); nudot[8] = float(b[0, 1]) / float(A[0, 1, 8])
    assert abs(float(jac[0, 1] @ (nu[0] + 0.01 * nudot)) - 0.0) < 1e-5


# ------------------------------------------------------------------------------------------------------------ GPU
def _sizes(p, k=0):
    return {"gap": p, "normal": 3 * p, "witness": 6 * p, "jac": NCOL * p, "nearest": k}


def _set_states(env, members, velocities=None):
    root, dof = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    for e, (quat, q) in enumerate(members):
        rng = np.random.default_rng(900 + e)
        nu = np.zeros(26) if velocities is None else velocities[e]
        root[e, 0] = torch.tensor(np.concatenate([rng.uniform(-2, 2, 3), quat, nu[0:6]]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q, nu[6:]], -1), dtype=torch.float32)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(family, n):
    """An env whose robot e holds member e of the family (repeating), the fp64 reference of every env at the sim's DOWNLOADED fp32 state
    and the full launch's outputs. Computed once and left unchanged."""
    import test_inverse_dynamics as tid
    env = tid._env(n, seed=5, steps=0)
    members = _members(family)
    _set_states(env, [members[e % len(members)] for e in range(n)])
    r64, d64 = env.sim.tensor("ROOT_STATES")[:, 0].cpu().numpy().astype(np.float64), env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64)
    refs = [px.proximity(env.robot_model, r64[e, 3:7], d64[e, :, 0]) for e in range(n)]
    return env, refs, _launch(env, k=8)


def _launch(env, which=("gap", "normal", "witness", "jac", "nearest"), k=8):
    """A direct C-ABI call into sentinel-framed buffers; returns {name: [n, ...] tensor} of the outputs asked for."""
    n, p = env.num_envs, len(env.sim.proximity_pair_ids)
    size = _sizes(p, k)
    bufs = {}
    for name in which:
        if name == "nearest":
            bufs[name] = torch.full((n * k + 8,), ISENTINEL, dtype=torch.int32, device="cuda")
        else:
            bufs[name] = torch.full((n * size[name] + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    ptr = lambda name: bufs[name].data_ptr() if name in bufs else None
    rc = env.sim.L.wbc_sim_proximity(env.sim.h, ptr("gap"), ptr("normal"), ptr("witness"), ptr("jac"), ptr("nearest"), k, None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    shape = {"gap": (n, p), "normal": (n, p, 3), "witness": (n, p, 2, 3), "jac": (n, p, NCOL), "nearest": (n, k)}
    for name, b in bufs.items():
        assert bool((b[n * size[name]:] == (ISENTINEL if name == "nearest" else SENTINEL)).all()), name
    return {name: b[:n * size[name]].view(shape[name]).clone() for name, b in bufs.items()}


CASES = [(family, n) for family in ("random", "near") for n in (1, 13, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,n", CASES)
def test_every_judged_entry_of_every_output(family, n):
    env, refs, got = _case(family, n)
    assert env.sim.proximity_pair_ids[:, :3].tolist() == [list(t) for t in px.pair_list(env.robot_model)]
    assert env.sim.proximity_pairs == px.pair_names(env.robot_model)
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items() if k != "nearest"}
    worst = {f: 0.0 for f in FAMILIES}
    for e, (out, mag, cond, _) in enumerate(refs):
        rows = _rows(cond)
        for f in FAMILIES:
            worst[f] = max(worst[f], px.largest_ratio(g[f][e], out[f], mag[f], rows[f]))
    out_, total = _left_out(refs)
    print(f"proximity {family} n={n}: largest |kernel - ref| / (2^-24 mag): {worst}; {out_} of {total} cases left out")
    assert out_ <= LEFT_OUT_MAX * total
    for f, w in worst.items():
        assert w <= CONST[f], (f, w)
    # structure, as equalities, on every case: the root's and the fingers' columns, the joints that move neither side or both
    jac = got["jac"]
    zero = torch.tensor(np.array([r[1]["jac"] == 0 for r in refs]), device="cuda")
    assert bool((jac[:, :, :6] == 0).all()) and bool((jac[:, :, 24:] == 0).all()) and bool((jac[zero] == 0).all()) and bool((jac[~zero] != 0).any())
    # the Python entry point is the same call
    for a, name in zip(env.sim.proximity(k_nearest=8), ("gap", "normal", "witness", "jac", "nearest")):
        assert torch.equal(a, got[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("family,n", CASES)
def test_certificate_on_every_case(family, n):
    """Needs no agreement on the winning feature: each witness lies on its own primitive's surface, their separation along n is the reported
    gap, the gap is the fp64 gap, n is a unit vector -- on every (env, pair) case, those left out of the entry-wise test included."""
    env, refs, got = _case(family, n)
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    worst = np.zeros(4)
    for e, (out, mag, cond, aux) in enumerate(refs):
        for i, (kind, pa, pb) in enumerate(aux):
            allow_w, allow_g = CONST["witness"] * EPS * mag["witness"][i, 0, 0], CONST["gap"] * EPS * mag["gap"][i]
            wa, wb_, nrm, gp = g["witness"][e, i, 0], g["witness"][e, i, 1], g["normal"][e, i], g["gap"][e, i]
            if kind == "limbs":
                sd = (px.surface_distance("limb", pa, wa), px.surface_distance("limb", pb, wb_))
            else:
                sd = (px.surface_distance("sphere", pa, wa), px.surface_distance("box", pb, wb_))
            r = [max(abs(sd[0]), abs(sd[1])) / allow_w, abs((wa - wb_) @ nrm - gp) / allow_g, abs(gp - out["gap"][i]) / allow_g,
                 abs(np.linalg.norm(nrm) - 1.0) / (4 * EPS)]
            assert max(r) <= 1.0, (e, i, r)
            worst = np.maximum(worst, r)
    print(f"proximity {family} n={n} certificate: witness on its surface {worst[0]:.3g}, separation along n vs gap {worst[1]:.3g}, "
          f"gap vs fp64 {worst[2]:.3g} (of the allowances), | |n| - 1 | {worst[3]:.3g} of 4 x 2^-24")


@pytest.mark.gpu
def test_nearest_is_the_stable_argsort_of_the_kernels_own_gaps():
    env, _, got = _case("near", 64)
    order = torch.sort(got["gap"], dim=1, stable=True).indices.to(torch.int32)
    assert torch.equal(got["nearest"], order[:, :8])
    for k in (1, 3, 8):
        assert torch.equal(_launch(env, ("gap", "nearest"), k)["nearest"], order[:, :k])
        assert torch.equal(_launch(env, ("nearest",), k)["nearest"], order[:, :k])
        assert torch.equal(env.sim.proximity(k_nearest=k)[-1], order[:, :k])


@pytest.mark.gpu
def test_translation_and_velocities_leave_every_bit():
    n = 64
    env, _, want = _case("random", n)
    root0, dof0 = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    try:
        root = root0.clone(); root[:, 0, 0:3] += torch.tensor([64.0, -64.0, 32.0], device="cuda")
        env.sim.set_root_state(root.contiguous())
        moved = _launch(env)
        gen = torch.Generator(device="cuda"); gen.manual_seed(3)
        root[:, 0, 7:13] = torch.randn(n, 6, device="cuda", generator=gen) * 3
        dof = dof0.clone(); dof[:, :, 1] = torch.randn(n, 20, device="cuda", generator=gen) * 5
        env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
        moving = _launch(env)
    finally:
        env.sim.set_root_state(root0.contiguous()); env.sim.set_dof_state(dof0.contiguous())
        torch.cuda.synchronize()
    for k in want:
        assert bool(want[k].abs().sum() > 0) and torch.equal(moved[k], want[k]) and torch.equal(moving[k], want[k]), k
    assert all(torch.equal(v, want[k]) for k, v in _launch(env).items())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_partial_outputs_have_the_bits_of_the_full_launch(n):
    env, _, want = _case("near", n)
    before = [env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")]
    for which in (("gap",), ("normal",), ("witness",), ("jac",), ("gap", "nearest"), ("gap", "jac"), ("normal", "witness"), ("witness", "jac", "nearest")):
        part = _launch(env, which)
        for k in which:
            assert torch.equal(part[k], want[k]), (which, k)
    only = env.sim.proximity(jac=torch.empty_like(want["jac"]))
    assert len(only) == 1 and torch.equal(only[0], want["jac"])
    torch.cuda.synchronize()
    for k, t in zip(("ROOT_STATES", "DOF_STATE", "BODY_PARAMS"), before):
        assert torch.equal(env.sim.tensor(k), t), k                   # the sim's state is read, never written


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    env, _, want = _case("near", 13)
    names = ("gap", "normal", "witness", "jac", "nearest")
    outs = [torch.zeros_like(want[k]) for k in names]
    call = lambda: env.sim.proximity(*outs[:4], nearest=outs[4])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in outs:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, want[k]) for a, k in zip(outs, names))


@pytest.mark.gpu
def test_every_refusal_leaves_the_buffers_untouched():
    n = 13
    env, _, want = _case("near", n)
    L, h = env.sim.L, env.sim.h
    p = len(env.sim.proximity_pair_ids)
    size = _sizes(p, 8)
    bufs = {k: torch.full((n * size[k] + 8,), SENTINEL, dtype=torch.float32, device="cuda") for k in ("gap", "normal", "witness", "jac")}
    bufs["nearest"] = torch.full((n * 8 + 8,), ISENTINEL, dtype=torch.int32, device="cuda")
    names = ("sim", "gap", "normal", "witness", "jac", "nearest", "k", "stream")
    base = dict(sim=h, k=3, stream=None, **{k: b.data_ptr() for k, b in bufs.items()})
    call = lambda **kw: L.wbc_sim_proximity(*[kw.get(k, base[k]) for k in names])
    refusals = [(dict(sim=None), b"NULL"), (dict(gap=None, normal=None, witness=None, jac=None, nearest=None), b"NULL")]
    refusals += [({k: bufs[k].data_ptr() + off}, b"aligned") for k in bufs for off in (1, 2, 3)]
    refusals += [(dict(k=k), b"k_nearest") for k in (0, -1, 9, 64)]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_proximity: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert L.wbc_sim_proximity_pairs(h, None) == -1 and b"NULL" in L.wbc_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == (ISENTINEL if k == "nearest" else SENTINEL)).all()), k
    # 4-byte alignment is enough; k_nearest is ignored where nearest is NULL
    assert call(gap=bufs["gap"].data_ptr() + 4, normal=None, witness=None, jac=bufs["jac"].data_ptr() + 4, nearest=None, k=99) == 0
    torch.cuda.synchronize()
    for k in ("gap", "jac"):
        b = bufs[k]
        assert torch.equal(b[1:1 + n * size[k]].view(want[k].shape), want[k]) and float(b[0]) == SENTINEL and bool((b[1 + n * size[k]:] == SENTINEL).all())
    assert all(bool((bufs[k] == SENTINEL).all()) for k in ("normal", "witness")) and bool((bufs["nearest"] == ISENTINEL).all())


@pytest.mark.gpu
def test_a_model_without_self_collisions_has_no_pairs():
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = 1; cfg.terrain.mesh_type = "plane"
    cfg.asset.self_collisions = 1                                                 # Isaac Gym's filter bit: 1 = no self-collision
    env = WidowGo1(cfg, sim_device="cuda:0", seed=5)
    assert env.sim.L.wbc_sim_proximity_pair_count(env.sim.h) == 0 and env.sim.proximity_pairs == []
    buf = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    assert env.sim.L.wbc_sim_proximity(env.sim.h, buf.data_ptr(), None, None, None, None, 0, None) == -1
    assert env.sim.L.wbc_last_error().startswith(b"wbc_sim_proximity: ") and b"no self-collision pairs" in env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_call():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        for _ in range(5):
            if use:
                env.sim.proximity(k_nearest=3)
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                gap, _, _, jac = env.sim.proximity()
                env.sim.proximity_damper_rows(gap, jac, 0.02, 0.10, 1.0, env.dt)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
