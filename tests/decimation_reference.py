"""TEST INFRASTRUCTURE ONLY -- the driver that holds the DECIMATION LOOP of wbc_step_kernel (csrc/wbc_step_kernel.hip:
`for (t = 0; t < dec; ++t) { torque_pass; WSYNC; physics_substep(..., t == dec - 1); }`) to the one-substep fp64 tier. It adds no
physics reference: the kernel keeps no state between substeps other than what its prologue reloads from HBM, and the prologue loads
floats verbatim (no normalisation; BOX_SLEEP_TIMER an exact integer-valued float), so

  R1  one step at decimation D leaves the same BITS as D steps at decimation 1 under the same action, on everything the physics
      writes: ROOT_STATES (both rows), DOF_STATE, TORQUES, NET_CONTACT_FORCE, FORCE_SENSOR, RIGID_BODY_STATE, BASE_LIN_VEL,
      BASE_ANG_VEL, BOX_SLEEP_TIMER and the increment of DROPPED_HITS. (Sim X: one step at D. Sim Y: D steps at 1.)
  R2  the same chain through wbc_simulate_kernel: from the same start, D times (the TORQUES Y's k-th step stored written as the dof
      forces, simulate()); after each link ROOT_STATES, DOF_STATE, NET_CONTACT_FORCE, FORCE_SENSOR and BOX_SLEEP_TIMER are Y's, bit
      for bit.
  R3  every link of Y obeys the fp64 checkers of the decimation-1 tiers with their constants unchanged: the residual and integrator
      of forward_dynamics_reference and contact_law_reference.check_env (the airborne and the foot cases),
      pair_contact_reference.check_env (the limb, box and sleep cases), the PD torques of step_state_reference.check_action_path
      (every case).

Bit identity then transfers the whole fp64 tier to the shipped decimation, and fails on any carried-state or stale-LDS dependence
of substeps 2 .. D: the dyn_dirty restore of the per-body contact masks, the LDS aliases (IA / K / clam, U / out_contact /
out_sensor, pA / pD / g, c / aD), torque_pass reading q / qd from LDS (the wrap of column WBC_NACT - 8 included), the substeps
without outputs, and bxtimer / dropped carried in LDS.

Preconditions, so that nothing but the substeps touches the physics state: push_interval = 0; action_delay = -1 (one case at the
shipped delay, ACTION_HISTORY pre-filled with the step's action in every FIFO row: the delayed action is the newest in all D
steps); the attitude and height terminations out of reach; the same n, helpers.random_env_params, seed, staged ROOT_STATES,
DOF_STATE, BOX_SLEEP_TIMER and step counter in X and Y. An env that reset in any of the D + 1 steps is left out (the mask is
needed: see tests/test_step_decimation.py); at least MIN_SHARE of a case's envs must remain. A NaN anywhere is a failure.

The staged states are those of the one-substep tiers (no new geometry): see CASES. The transitions a case has to exercise between
consecutive links are counted from the fp64 restatement of Y's states (the active sets pair_contact_reference.check_env and
contact_law_reference.check_env derive, the sleep rule of pair_contact_reference), never from kernel internals.
Nothing under wbc_amd imports this file."""
import numpy as np

import contact_law_reference as clr
import forward_dynamics_reference as fdr
import pair_contact_reference as pcr
import step_state_reference as ssr
import task_logic_reference as tl

PHYSICS = ["ROOT_STATES", "DOF_STATE", "TORQUES", "NET_CONTACT_FORCE", "FORCE_SENSOR", "RIGID_BODY_STATE", "BASE_LIN_VEL", "BASE_ANG_VEL",
           "BOX_SLEEP_TIMER"]                                                                   # R1 (plus the DROPPED_HITS increment)
CHAIN = ["ROOT_STATES", "DOF_STATE", "NET_CONTACT_FORCE", "FORCE_SENSOR", "BOX_SLEEP_TIMER"]    # R2
DROPPED = "DROPPED_HITS increment"
MIN_SHARE = 0.8
MIN_TRANSITIONS = 8
STEP_COUNTER = 1
TRANSITIONS = ("dyn on->off", "dyn off->on", "foot opening", "foot closing", "box asleep->awake", "box awake->asleep")

# name -> dict(family, n, seed, D (tuple), source, sigma, need (the transitions with at least MIN_TRANSITIONS envs), delay)
#   air     reset_all, the actions of fdr.step_actions; every eighth env with q[WBC_NACT - 8] outside (-pi, pi] (ssr.torque_state)
#   feet    contact_law_reference.step_states from A-256 (plane) / C-256 (rough grid); stand: from D-256 (four feet down)
#   pair    pair_contact_reference.step_states from L-264 (limb pairs), M-256 (tangled), B-255 (free box), K-128(-grid) (box corners)
#           L-264 keeps its one limb pair in contact through all four substeps at any action scale (a pair leaves the 10 mm margin at
#           0.16 m/s x 5 ms = 0.8 mm a substep at most): the dynamic-slot transitions are M-256's (both directions) and B-255's (a
#           promoted sphere leaving the box); L-264 holds the slot that STAYS active across the substeps
#   sleep   S-64 as sleep_staging() presets its timers and moves its robots back. "box awake->asleep" is NOT in `need`: S-64 cannot
#           produce it inside one launch (an awake box resting on four corners leaves every substep at 0.011 .. 0.015 m/s, above
#           box_sleep_speed = 0.01 m/s, so it is not at rest at the next one); what the case does exercise upwards is bxtimer reaching
#           the threshold in substep 1 and being cleared in substep 2 (asserted through BOX_SLEEP_TIMER on every link)
CASES = {
    "air-13": dict(family="air", n=13, seed=107, D=(2, 4)),
    "air-13-delay": dict(family="air", n=13, seed=107, D=(4,), delay=None),                     # None: the shipped action_delay
    "air-2560": dict(family="air", n=2560, seed=108, D=(4,)),
    "feet-13": dict(family="feet", n=13, seed=407, source="A-256", D=(2, 4)),
    "feet-256": dict(family="feet", n=256, seed=721, source="A-256", D=(4,), need=("foot opening", "foot closing")),
    "grid-13": dict(family="feet", n=13, seed=412, source="C-256", D=(4,)),
    "grid-256": dict(family="feet", n=256, seed=722, source="C-256", D=(4,), need=("foot opening", "foot closing")),
    "stand-256": dict(family="feet", n=256, seed=723, source="D-256", D=(4,), sigma=0.3),
    "limbs-13": dict(family="pair", n=13, seed=615, source="L-264", D=(2, 4)),
    "limbs-256": dict(family="pair", n=256, seed=724, source="L-264", D=(4,)),
    "limbs-2560": dict(family="pair", n=2560, seed=616, source="L-264", D=(4,)),
    "tangle-256": dict(family="pair", n=256, seed=725, source="M-256", D=(4,), need=("dyn on->off", "dyn off->on")),
    "box-256": dict(family="pair", n=256, seed=726, source="B-255", D=(4,), need=("dyn on->off",)),
    "corner-128": dict(family="pair", n=128, seed=727, source="K-128", D=(4,)),
    "corner-128-grid": dict(family="pair", n=128, seed=728, source="K-128-grid", D=(4,)),
    "sleep-64": dict(family="sleep", n=64, seed=729, source="S-64", D=(4,), need=("box asleep->awake",)),
}
RUNS = [(name, D) for name, c in CASES.items() for D in c["D"]]


def build_case(robot, name):
    """dict(robot (the fixture or the pair cases' copy), cfg(D) -> task cfg, ter, root, dof (None: the reset state), act, timer, params,
    q2 (mask of the envs whose wrapped column is staged beyond the seam), q2_val, tangled)."""
    import helpers
    case = CASES[name]
    n, fam = case["n"], case["family"]
    delay = case.get("delay", -1)
    c = dict(name=name, n=n, family=fam, ter=None, root=None, dof=None, timer=np.zeros(n), q2=np.zeros(n, bool), tangled=False,
             need=case.get("need", ()))
    src = dict(n=n, seed=case["seed"], source=case.get("source"))
    if "sigma" in case:
        src["sigma"] = case["sigma"]
    if fam == "air":
        c["robot"] = robot
        delay = int(robot["tcfg"].action_delay) if delay is None else delay
        c["cfg"] = lambda D: tl.with_cfg(robot["tcfg"], decimation=D, action_delay=delay, push_interval=0, term_rp_threshold=100.0,
                                         term_z_threshold=-100.0)
        c["act"] = fdr.step_actions(n, case["seed"])[0]
        c["params"] = helpers.random_env_params(n, seed=case["seed"])
        rng = np.random.default_rng(case["seed"] + 1)
        c["q2"] = np.arange(n) % 8 == 5
        m = int(c["q2"].sum())
        c["q2_val"] = ((np.pi + rng.uniform(0.5, 1.5, m)) * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    elif fam == "feet":
        c["robot"] = robot
        c["cfg"] = lambda D: clr.step_states(robot, None, case=src, decimation=D, action_delay=delay, push_interval=0)[0]
        _, c["ter"], c["root"], c["dof"], c["act"] = clr.step_states(robot, None, case=src)
        c["params"] = helpers.random_env_params(n, seed=case["seed"])
    else:
        rb = c["robot"] = pcr.case_robot(robot)
        c["cfg"] = lambda D: pcr.step_states(rb, None, case=src, decimation=D, action_delay=delay, push_interval=0)[0]
        _, c["ter"], c["root"], c["dof"], c["act"] = pcr.step_states(rb, None, case=src)
        c["params"] = helpers.random_env_params(n, seed=case["seed"])
        c["params"]["box_dmass"] = np.random.default_rng(case["seed"] + 5000).uniform(-0.5, 1.5, n).astype(np.float32)
        c["tangled"] = pcr.CASES[case["source"]]["kind"] == "tangled"
        if fam == "sleep":
            c["root"], c["timer"] = sleep_staging(rb, c["cfg"](1), c["root"], c["dof"], case["seed"])
    c["delay"] = delay
    return c


WAKE_SPEED = 0.4              # m/s towards the box: 2 mm a substep
WAKE_CLEAR = (0.2e-3, 3.5e-3) # the staged foot's distance beyond the contact margin: it enters at substep 2 or 3


def sleep_staging(robot, tcfg, root, dof, seed):
    """S-64 for a launch of several substeps: (root, timer). First half (the robot 5 m up, the box at rest on its four lower corners):
    envs 0, 1 mod 4 asleep (timer at the threshold: asleep through every substep), 2 mod 4 one substep short of it (bxtimer reaches the
    threshold in substep 1 and falls back to 0 in substep 2: an awake box on four corners keeps (3/4)^4 g dt = 0.015 m/s after the
    four sweeps, above box_sleep_speed), 3 mod 4 two short. Second half (S-64 stages one foot inside the contact offset beside a
    vertical face): the box asleep, the robot moved back along that pair's normal until the foot clears the margin by WAKE_CLEAR and
    given WAKE_SPEED towards the box: the foot enters the margin, and wakes the box, between two substeps of the launch. Pose,
    attitude, joint state and the face are S-64's."""
    n = len(root)
    rng = np.random.default_rng(seed + 1)
    nsleep = pcr.sleep_threshold(robot["wmodel"], tcfg)
    timer = np.full(n, nsleep)
    first = np.arange(n) < n // 2
    timer[first & (np.arange(n) % 4 == 2)] -= 1
    timer[first & (np.arange(n) % 4 == 3)] -= 2
    tm, sph, bt, cfg = clr.table_model(robot["model"], robot["wmodel"]), clr.spheres(robot["wmodel"]), pcr.box_tables(robot["wmodel"]), clr.law_cfg(tcfg)
    root = root.copy()
    for e in np.flatnonzero(~first):
        G = pcr.box_geometry(tm, sph, bt, None, cfg, root[e], np.asarray(dof[e, :, 0], dtype=np.float64))
        act = [p for p in G["pairs"] if p["active"]]
        assert len(act) == 1 and act[0]["sphere"] < 4, (e, [p["sphere"] for p in act])
        nw = G["R0"] @ act[0]["n"]
        nw[2] = 0.0                                                       # (a vertical face: the robot keeps its height)
        nw /= np.linalg.norm(nw)
        root[e, 0, 0:3] += ((cfg["margin"] - act[0]["gap"] + rng.uniform(*WAKE_CLEAR)) * nw).astype(np.float32)
        root[e, 0, 7:10] -= (WAKE_SPEED * nw).astype(np.float32)
    return root, timer


class OracleAdapter(pcr.OracleAdapter):
    """The C oracle behind the interface of run(): get / set / step / simulate / reset_all / set_step_counter / set_torques."""

    def set_torques(self, tau):
        self.o.set("TORQUES", tau)


def oracle_sim(precision):
    def make(robot, tcfg, n, params, ter):
        import helpers
        o = helpers.make_oracle(robot, n, params, precision, tcfg=tcfg)
        if ter is not None:
            o.set_heightfield(*clr.heightfield_args(ter))
        return OracleAdapter(o)
    return make


def stage(sim, c):
    """The start of a chain: reset_all, the step counter, the staged state over the reset one, the sleep timer, the action FIFO."""
    sim.reset_all()
    sim.set_step_counter(STEP_COUNTER)
    if c["root"] is not None:
        sim.set("ROOT_STATES", c["root"])
        sim.set("DOF_STATE", c["dof"])
    elif c["q2"].any():
        dof = sim.get("DOF_STATE")
        dof[c["q2"], ssr.Q2_DOF, 0] = c["q2_val"]
        sim.set("DOF_STATE", dof)
    sim.set_torques(np.zeros((c["n"], 20)))
    sim.set("BOX_SLEEP_TIMER", c["timer"])
    if c["delay"] != -1:
        a = np.clip(np.asarray(c["act"], dtype=np.float64)[:, ssr.PERM18], -float(c["cfg"](1).clip_actions), float(c["cfg"](1).clip_actions))
        sim.set("ACTION_HISTORY", np.repeat(a[:, None], ssr.ADELAY, axis=1))


PRE = ["ROOT_STATES", "DOF_STATE", "BOX_SLEEP_TIMER", "DROPPED_HITS", "ACTION_HISTORY"]
POST = PHYSICS + ["DROPPED_HITS", "RESET_BUF", "ACTIONS", "LAST_ACTIONS", "ACTION_HISTORY", "MOTOR_STRENGTH"]


def _step(sim, act):
    pre = {k: sim.get(k) for k in PRE}
    sim.step(act)
    post = {k: sim.get(k) for k in POST}
    post[DROPPED] = post["DROPPED_HITS"] - pre["DROPPED_HITS"]
    return pre, post


def run(make_sim, robot, name, D, links=None, stale_torque=False, prepare=None):
    """make_sim(robot, tcfg, n, params, terrain) -> adapter. Returns dict(case, D, x (X's tensors after its one step), y [links] of
    (pre, post) of Y's steps, z [links] of the simulate chain's tensors, reset [n], bp, box_mass). links: the number of Y's steps
    (default D); stale_torque: the simulate chain's link k is fed link k - 1's TORQUES; prepare(sim): further staging of X and Y (the
    seeded faults of the CPU test)."""
    c = build_case(robot, name)
    X = make_sim(c["robot"], c["cfg"](D), c["n"], c["params"], c["ter"])
    Y = make_sim(c["robot"], c["cfg"](1), c["n"], c["params"], c["ter"])
    for sim in (X, Y):
        stage(sim, c)
        if prepare is not None:
            prepare(sim)
    _, x = _step(X, c["act"])
    y = [_step(Y, c["act"]) for _ in range(D if links is None else links)]
    # R2: the simulate chain, from Y's own start (read back from the sim: the reset state of the air cases)
    Y.set("ROOT_STATES", y[0][0]["ROOT_STATES"])
    Y.set("DOF_STATE", y[0][0]["DOF_STATE"])
    Y.set("BOX_SLEEP_TIMER", y[0][0]["BOX_SLEEP_TIMER"])
    z = []
    for k in range(len(y)):
        drop0 = Y.get("DROPPED_HITS")
        Y.set_torques(y[max(k - 1, 0) if stale_torque else k][1]["TORQUES"])
        Y.simulate()
        z.append({t: Y.get(t) for t in CHAIN})
        z[-1][DROPPED] = Y.get("DROPPED_HITS") - drop0
    reset = x["RESET_BUF"] != 0
    for _, post in y:
        reset |= post["RESET_BUF"] != 0
    return dict(case=c, D=D, x=x, y=y, z=z, reset=reset, bp=Y.get("BODY_PARAMS"), box_mass=Y.get("BOX_MASS"))


# ------------------------------------------------------------------------------------------------------------------ R1 and R2
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def differences(what, name, got, want, keep):
    """The entries of `got` whose bits are not those of `want`, in the envs of the mask `keep`: one line per entry (tensor, env,
    entry, both values); a non-finite value on either side in ANY env is reported too."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    out = []
    if got.shape != want.shape:
        return [f"{what}: {name}: shape {got.shape} against {want.shape}"]
    for label, a in (("the first", got), ("the second", want)):
        bad = np.argwhere(~np.isfinite(a))
        if len(bad):
            out.append(f"{what}: {name}: {len(bad)} non-finite entries in {label}, first at env {int(bad[0][0])} entry {tuple(int(i) for i in bad[0][1:])}")
    ne = (bits(got) != bits(want)) & np.asarray(keep, dtype=bool).reshape((-1,) + (1,) * (got.ndim - 1))
    for ix in np.argwhere(ne):
        ix = tuple(int(i) for i in ix)
        out.append(f"{what}: {name} env {ix[0]} entry {ix[1:]}: {got[ix]!r} against {want[ix]!r}")
    return out


def check_r1(r, keep=None):
    """X against the last link of Y. keep: the envs compared (default: those that never reset)."""
    keep = ~r["reset"] if keep is None else keep
    last = r["y"][-1][1]
    bad = []
    for t in PHYSICS + [DROPPED]:
        got = r["x"][t]
        want = last[t] if t != DROPPED else sum(post[DROPPED] for _, post in r["y"])
        bad += differences("R1", t, got, want, keep)
    return bad


def check_r2(r, keep=None):
    """Every link of the simulate chain against Y's."""
    keep = ~r["reset"] if keep is None else keep
    bad = []
    for k, zk in enumerate(r["z"]):
        for t in CHAIN + [DROPPED]:
            bad += differences(f"R2 link {k + 1}", t, zk[t], r["y"][k][1][t], keep)
    return bad


def share(r):
    return float((~r["reset"]).mean())


# ------------------------------------------------------------------------------------------------------------------------- R3
def bound(tier):
    mod, t = tier.split(".")
    if mod == "fdr":
        return fdr.bound(t)
    return dict(clr=clr, pcr=pcr, ssr=ssr)[mod].bound(t)


def check_r3(r, envs=None):
    """The decimation-1 checkers on every link of Y. Returns dict(worst {tier: [per link (ratio, env)]}, exact [...], states [links]
    of per-env dict(dyn, feet, asleep) (None: not evaluated), checked [links]). Tiers: "fdr.<family>" and "fdr.integrator", "clr.<tier>"
    (families air and feet), "pcr.<tier>" (families pair and sleep), "ssr.torque"."""
    c = r["case"]
    robot, tc, n, fam = c["robot"], c["cfg"](1), c["n"], c["family"]
    envs = fdr.step_envs(n) if envs is None else envs
    friction = np.asarray(c["params"]["friction"], dtype=np.float64)
    tt = ssr.torque_tables(tc)
    fdr_family = "step" if fam == "air" else "contact"
    worst, exact, states, checked, left_out = {}, [], [], [], []

    def put(tier, k, ratio, env):
        w = worst.setdefault(tier, [(0.0, -1)] * len(r["y"]))
        if ratio > w[k][0]:
            w[k] = (float(ratio), int(env))

    for k, (pre, post) in enumerate(r["y"]):
        skip = post["RESET_BUF"] != 0
        st = dict(root0=pre["ROOT_STATES"], dof0=pre["DOF_STATE"], root1=post["ROOT_STATES"], dof1=post["DOF_STATE"], ncf=post["NET_CONTACT_FORCE"],
                  fs=post["FORCE_SENSOR"], bp=r["bp"], friction=friction)
        # the PD torques
        w = ssr.Worst()
        bad, _ = ssr.check_action_path(tt, pre, post, c["act"], f"link {k + 1}", w)
        exact += bad
        put("ssr.torque", k, w.get("torque")[0], -1)
        # the contact law / the pair contacts
        if fam in ("air", "feet"):
            out = clr.evaluate(robot, tc, c["ter"], envs=envs, skip=skip, law=True, **st)
            tiers, mod = clr.TIERS, "clr"
        else:
            out = pcr.evaluate(robot, tc, c["ter"], envs=envs, skip=skip, tangled=c["tangled"], box_mass=r["box_mass"], dropped=post[DROPPED],
                               tau=post["TORQUES"], timer0=pre["BOX_SLEEP_TIMER"], timer1=post["BOX_SLEEP_TIMER"], **st)
            tiers, mod = pcr.TIERS, "pcr"
        # the equations of motion (families air and feet: the envs the contact law keeps -- no limb pair within the margin, inside the
        # joint limits, the velocity clamp idle -- with no sphere but the four feet within the margin: the residual reads a foot's wrench
        # off FORCE_SENSOR, which a knee or mid-shank on the same rigid body does not enter) and the robot's integrator (the same two
        # families, every env that did not reset: the quaternion row's scale |quat0| + dt |qdot| takes qdot after its products have
        # cancelled, which the tumbling robots of M-256 do not bear -- the fp32 oracle sits at 320 there; the pair families hold the
        # box's integrator through pair_contact_reference.box_integrator, whose scale sums the products' sizes)
        o = fdr.evaluate(robot["model"], robot["wmodel"], tc, "contact", st["root0"], st["dof0"], post["TORQUES"], r["bp"], st["root1"], st["dof1"],
                         st["fs"], st["ncf"], envs=envs, skip=skip | np.array([x is None or x["left_out"] is not None or mod != "clr" or bool(x["active"][4:].any()) for x in out]))
        for e in envs:
            if o["elig"][e]:
                put("fdr." + fdr_family, k, np.max(o["ratio"][e][fdr.LIVE]), e)
            if not skip[e] and mod == "clr":
                put("fdr.integrator", k, np.max(o["integ"][e]), e)
        nchecked, link_states, why = 0, [None] * n, {}
        for e in envs:
            res = out[e]
            why[res["left_out"]] = why.get(res["left_out"], 0) + 1
            if mod == "clr":
                link_states[e] = dict(dyn=frozenset(), feet=frozenset(int(i) for i in np.flatnonzero(res["active"][:4])), asleep=None)
            else:
                link_states[e] = dict(dyn=res["dyn"], feet=res["feet"], asleep=res["asleep"] if res["left_out"] is None else None)
            if res["left_out"] is not None:
                continue
            nchecked += 1
            exact += [f"link {k + 1} env {e}: {x}" for x in res["exact"]]
            for t in tiers:
                put(f"{mod}.{t}", k, res["ratio"][t], e)
        states.append(link_states)
        checked.append(nchecked)
        left_out.append({k_: v for k_, v in why.items() if k_ is not None})
    return dict(worst=worst, exact=exact, states=states, checked=checked, left_out=left_out, envs=list(envs))


def transitions(r3, reset):
    """Counts of the envs (never reset) in which a transition occurs between two consecutive links of Y: TRANSITIONS -> count."""
    cnt = {t: set() for t in TRANSITIONS}
    st = r3["states"]
    for k in range(len(st) - 1):
        for e in r3["envs"]:
            a, b = st[k][e], st[k + 1][e]
            if reset[e] or a is None or b is None:
                continue
            if a["dyn"] and not b["dyn"]:
                cnt["dyn on->off"].add(e)
            if b["dyn"] and not a["dyn"]:
                cnt["dyn off->on"].add(e)
            if a["feet"] - b["feet"]:
                cnt["foot opening"].add(e)
            if b["feet"] - a["feet"]:
                cnt["foot closing"].add(e)
            if a["asleep"] is not None and b["asleep"] is not None:
                if a["asleep"] and not b["asleep"]:
                    cnt["box asleep->awake"].add(e)
                if b["asleep"] and not a["asleep"]:
                    cnt["box awake->asleep"].add(e)
    return {t: len(v) for t, v in cnt.items()}


def report(name, D, who, r, r3, tr):
    lines = [f"{name} D={D} {who}: {int((~r['reset']).sum())} of {r['case']['n']} envs compared ({share(r):.3f}), checked per link {r3['checked']} of "
             f"{len(r3['envs'])} (left out {r3['left_out']}), with a dynamic slot {[sum(1 for x in st if x is not None and x['dyn']) for st in r3['states']]}, dropped hits {int(sum(p[DROPPED].sum() for _, p in r['y']))}, transitions {tr}"]
    for t in sorted(r3["worst"]):
        lines.append(f"    {t:<16} C = {bound(t):<6g} " + "  ".join(f"link {k + 1}: {w[0]:.3f} (env {w[1]})" for k, w in enumerate(r3["worst"][t])))
    return "\n".join(lines)


def assert_case(name, D, who, r, r3, c_factor=1.0):
    """Every figure first; then R1, R2, the compared share, R3 within c_factor x C (1 for the fp32 oracle and the kernel; the fp64
    oracle is held to ratio <= 1 by the caller), and the transition counts of the case."""
    tr = transitions(r3, r["reset"])
    print(report(name, D, who, r, r3, tr))
    bad = check_r1(r) + check_r2(r)
    assert not bad, f"{len(bad)} differences, the first: " + " | ".join(bad[:6])
    assert share(r) >= MIN_SHARE, (name, share(r))
    assert r3["exact"] == [], r3["exact"][:8]
    for t, w in r3["worst"].items():
        for k, (ratio, env) in enumerate(w):
            assert ratio <= c_factor * bound(t), (name, t, f"link {k + 1}", ratio, env, bound(t))
    for t in r["case"]["need"]:
        assert tr[t] >= MIN_TRANSITIONS, (name, t, tr[t])
    return tr
