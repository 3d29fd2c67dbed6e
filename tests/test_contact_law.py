"""The contact stage of one physics substep against the fp64 contact law, on the CPU: pins the checker of
tests/contact_law_reference.py to the C oracle, measures the constants that tests/test_gpu_contact_law.py holds the HIP kernels to and
shows that the checker can fail. Every case of the GPU test runs here through OracleSim(precision="f64") and OracleSim(precision="f32"),
same seeds, same n.

  * fp64 build: every ratio <= 1, no exact requirement violated (measured: see the table in tests/test_gpu_contact_law.py).
  * fp32 build: its largest ratio per tier is that tier's K_ref, asserted against contact_law_reference.K_REF.
  * the draws: at least 85 % of a case's envs are checked, the decision bands and the cell borders leave out at most 2 % each, no gap
    sits at the margin, and separating / stick / slide, mu = 0, the three branches of vn_tgt, both triangles and the clipped indices
    each occur at least 10 times -- on both builds.
  * nine seeded faults (a different spec or a different output handed to the checker) are each flagged in at least half of the envs
    they affect.
  * the checker's geometry (active, n, xc) is the oracle's contact_dump to 1e-12."""
import numpy as np
import pytest

import contact_law_reference as clr
import forward_dynamics_reference as fdr
import helpers

SINGLE = [k for k, c in clr.CASES.items() if c["kind"] == "single"]
ALL = list(clr.CASES) + list(clr.STEP_CASES)


def _params(name):
    case = clr.CASES.get(name) or clr.STEP_CASES[name]
    return helpers.random_env_params(case["n"], seed=case["seed"])


def _oracle(robot, name, prec):
    if name in clr.CASES:
        tc, ter = clr.case_states(robot, name)[:2]
    else:
        tc, ter = clr.step_states(robot, name)[:2]
    params = _params(name)
    o = helpers.make_oracle(robot, len(params["friction"]), params, prec, tcfg=tc)
    if ter is not None:
        o.set_heightfield(*clr.heightfield_args(ter))
    return o, params


@pytest.fixture(scope="module")
def runs(robot):
    """(precision, case name) -> (results per substep, states per substep, summary), each computed once."""
    cache = {}

    def get(prec, name):
        if (prec, name) not in cache:
            o, params = _oracle(robot, name, prec)
            run = clr.run_case if name in clr.CASES else clr.run_step
            outs, states = run(fdr.OracleAdapter(o), robot, name, params["friction"])
            cache[prec, name] = (outs, states, clr.summarise(outs))
        return cache[prec, name]
    return get


@pytest.mark.parametrize("name", ALL)
def test_f64_oracle_obeys_the_contact_law(robot, runs, name):
    _, _, s = runs("f64", name)
    print(clr.report(name + " fp64 oracle", s))
    assert s["exact"] == []
    for t in clr.TIERS:
        assert s["worst"][t][0] <= 1.0, (name, t, s["worst"][t])


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ALL)
def test_the_draws_cover_the_law(robot, runs, name, prec):
    """Eligibility, the caps on what is left out and the coverage counts, on the oracle's own output in both precisions."""
    _, _, s = runs(prec, name)
    print(clr.report(f"{name} {prec} oracle", s))
    params = _params(name)
    if s["n"] > 1:
        assert (params["friction"] < 0).any() and (params["friction"] > 1).any()
    assert s["exact"] == []
    assert s["checked"] >= clr.MIN_ELIGIBLE * s["n"], (name, s["checked"], s["n"], s["left_out"])
    assert s["left_out"].get("border", 0) <= clr.MAX_LEFT_OUT * s["n"] and s["near"] <= clr.MAX_LEFT_OUT * max(s["n"], 50)
    if name in SINGLE:
        assert s["left_out"].get("margin", 0) == 0 and s["left_out"].get("self", 0) == 0
        assert s["single"] == s["checked"]                                      # every checked env has exactly one active sphere
    if name in clr.COVERED:
        assert min(s["classes"][c] for c in ("separating", "stick", "slide")) >= clr.MIN_COUNT, s["classes"]
        assert s["mu0"] >= clr.MIN_COUNT and min(s["branches"]) >= clr.MIN_COUNT, (s["mu0"], s["branches"])
    if name == "C-256":
        assert min(s["tri"]) >= clr.MIN_COUNT and s["clipped"] >= clr.MIN_COUNT, (s["tri"], s["clipped"])
    if name in clr.STEP_CASES:
        assert s["left_out"].get("reset", 0) <= 0.05 * s["n"]
        assert s["single"] >= 0.8 * s["n"]


def test_every_sphere_is_the_active_one_somewhere(robot, runs):
    """Feet in A, the 20 other spheres that can touch a plane alone in B; a mid-shank (r = 0.008, on the segment between the knee and
    foot spheres of r = 0.02) cannot, its states are on the grid's ridges in C."""
    assert runs("f64", "A-256")[2]["spheres"] == set(clr.FEET)
    assert runs("f64", "B-192")[2]["spheres"] == set(clr.OTHERS) and len(clr.OTHERS) == 20
    assert runs("f64", "C-256")[2]["spheres"] == set(clr.GRID_TARGETS)
    assert set(clr.FEET) | set(clr.OTHERS) | set(clr.GRID_TARGETS) == set(range(clr.NSPH))


def test_the_cap_takes_over_where_the_cfg_says(robot):
    """The depth from which vn_tgt is max_depenetration_vel follows from the cfg (0.025 m), inside the drawn range of gaps."""
    cfg = clr.law_cfg(clr.case_cfg(robot["tcfg"]))
    d = clr.cap_depth(cfg)
    assert 0.0 < d < 0.04 and abs(d - cfg["vmax"] * cfg["dt"] / cfg["erp"]) == 0
    assert clr.vn_target(cfg, -0.999 * d, 1.0)[2] == 1 and clr.vn_target(cfg, -1.001 * d, 1.0)[2] == 2
    assert clr.vn_target(cfg, 1e-4, 1.0)[2] == 0 and clr.vn_target(cfg, -1.001 * d, 1.0)[0] == cfg["vmax"]


def test_k_ref_of_every_tier(robot, runs):
    """The fp32 oracle's largest ratios: printed, and asserted against the committed K_REF (not above it; not below 80 % of it, so that
    a committed constant cannot be looser than what was measured). The fp64 oracle's are printed next to them."""
    k = {t: (0.0, "") for t in clr.TIERS}
    k64 = {t: 0.0 for t in clr.TIERS}
    for name in ALL:
        s = runs("f32", name)[2]
        assert s["exact"] == []
        for t in clr.TIERS:
            if s["worst"][t][0] > k[t][0]:
                k[t] = (s["worst"][t][0], f"{name} substep {s['worst'][t][1]} env {s['worst'][t][2]}")
            k64[t] = max(k64[t], runs("f64", name)[2]["worst"][t][0])
    print("K_ref (fp32 oracle):", {t: (round(v, 3), w) for t, (v, w) in k.items()}, "C:", {t: clr.bound(t) for t in k},
          "fp64 oracle:", {t: float(f"{v:.3g}") for t, v in k64.items()})
    for t, (v, _) in k.items():
        assert 0.8 * clr.K_REF[t] <= v <= clr.K_REF[t], (t, v, clr.K_REF[t])
        assert clr.bound(t) <= clr.C_CAP


@pytest.mark.parametrize("name", SINGLE)
def test_geometry_is_the_oracles_contact_dump(robot, name):
    """active, n and xc (frame F) of the 28 terrain spheres against the fp64 oracle's contact list, 1e-12."""
    tc, ter, root, dof, tau = clr.case_states(robot, name)
    o, _ = _oracle(robot, name, "f64")
    fdr.OracleAdapter(o).load(root, dof, tau)
    tm, sph, cfg = clr.table_model(robot["model"], robot["wmodel"]), clr.spheres(robot["wmodel"]), clr.law_cfg(tc)
    slots = [s["slot"] for s in sph]
    for e in range(len(root)):
        d = o.debug_contacts(e)
        g = clr.geometry(tm, sph, ter, cfg, root[e, 0].astype(np.float64), dof[e, :, 0].astype(np.float64))
        assert np.array_equal(g["active"], d["active"][slots]) and g["active"].sum() == 1
        k = int(np.flatnonzero(g["active"])[0])
        np.testing.assert_allclose(g["n"][k], d["n"][slots[k]], rtol=0, atol=1e-12)
        np.testing.assert_allclose(g["xc"][k], d["xc"][slots[k]], rtol=0, atol=1e-12)
        assert d["nshare"][slots[k]] == 1


# ------------------------------------------------------------------------------------------------------- the checker can fail
def _flagged(robot, name, st, spec=None, **changed):
    """Per env: is any exact requirement violated or any ratio beyond its tier's C? (the fp64 oracle's state, possibly changed)"""
    tc, ter = clr.case_states(robot, name)[:2]
    outs = clr.evaluate(robot, tc, ter, **dict(st, **changed), spec=dict(clr.DEFAULT_SPEC, **(spec or {})))
    bad = np.array([r["left_out"] is None and (bool(r["exact"]) or any(r["ratio"][t] > clr.bound(t) for t in clr.TIERS)) for r in outs])
    return bad, outs


def _share(robot, runs, name, affected, spec=None, **changed):
    outs0, states, _ = runs("f64", name)
    bad0, _ = _flagged(robot, name, states[0])
    assert not bad0.any()
    bad, _ = _flagged(robot, name, states[0], spec, **changed)
    aff = np.array([r["left_out"] is None and affected(r) for r in outs0[0]])
    assert aff.sum() >= clr.MIN_COUNT
    return bad[aff].mean(), int(aff.sum())


def _forced(st, e):
    return bool(np.any(st["ncf"][e, :27] != 0))


FAULTS = [
    ("contact_erp 0.2 -> 0.21", "A-256", dict(erp=0.21), lambda r, f: f and r["branch"] == 1),
    ("terrain_friction off by 1 %", "A-256", dict(terrain_friction=1.01 * clr.TERRAIN_FRICTION), lambda r, f: f and r["cls"] == "slide" and r["mu"] > 0 and not r["near"]),
    ("one sphere radius off by 0.1 mm", "A-256", dict(radius_delta=(1, 1e-4)), lambda r, f: f and r["sphere"] == 1),
    ("gap without the n_z factor", "C-256", dict(gap_without_nz=True), lambda r, f: f),
    ("the other diagonal of the cell split", "C-256", dict(other_diagonal=True), lambda r, f: f),
    ("a normal left unnormalised", "C-256", dict(unit_normal=False), lambda r, f: f),
    ("friction direction from the stick impulse", "A-256", dict(direction_from_stick=True), lambda r, f: f and r["cls"] == "slide" and r["mu"] > 0 and not r["near"]),
    ("sensor lever arm with the wrong sign", "A-256", dict(lever_sign=-1.0), lambda r, f: f),
]


@pytest.mark.parametrize("what,name,spec,affected", FAULTS, ids=[f[0] for f in FAULTS])
def test_a_different_spec_is_flagged(robot, runs, what, name, spec, affected):
    states = runs("f64", name)[1]
    forced = [_forced(states[0], e) for e in range(len(states[0]["ncf"]))]
    outs0 = runs("f64", name)[0][0]
    idx = {id(r): e for e, r in enumerate(outs0)}
    share, count = _share(robot, runs, name, lambda r: affected(r, forced[idx[id(r)]]), spec)
    print(f"{what}: flagged in {100 * share:.0f} % of the {count} envs it affects ({name})")
    assert share >= 0.5


def test_forces_scaled_by_1_001_are_flagged(robot, runs):
    states = runs("f64", "A-256")[1]
    forced = [_forced(states[0], e) for e in range(len(states[0]["ncf"]))]
    outs0 = runs("f64", "A-256")[0][0]
    idx = {id(r): e for e, r in enumerate(outs0)}
    share, count = _share(robot, runs, "A-256", lambda r: forced[idx[id(r)]], ncf=1.001 * states[0]["ncf"], fs=1.001 * states[0]["fs"])
    print(f"forces scaled by 1.001 (NET_CONTACT_FORCE and FORCE_SENSOR alike): flagged in {100 * share:.0f} % of the {count} envs with a force")
    assert share >= 0.5
