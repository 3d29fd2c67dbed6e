"""bench.py's host-side pieces that need no GPU: the CPU-baseline leg on a small stand-in rollout (always this package's eager
path, which tests/test_ppo_parity.py pins to the reference: the same classes on every box, nothing outside the repository
executed inside the bench), the usable-core count, and the launcher's argument handling."""
import os
import subprocess

import pytest
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from wbc_amd.config import WidowGo1RoughCfgPPO, class_to_dict  # noqa: E402
from wbc_amd.rsl_rl.algorithms import PPO  # noqa: E402
from wbc_amd.rsl_rl.modules import ActorCritic  # noqa: E402


def _stand_in_runner(n=32, t=8):
    tr = class_to_dict(WidowGo1RoughCfgPPO())
    torch.manual_seed(0)
    ac = ActorCritic(76, 76, 18, **tr["policy"], num_priv=24, num_hist=10, num_prop=76)
    alg = PPO(ac, device="cpu", **tr["algorithm"])
    alg.init_storage(n, t, [860], [None], [18])
    st = alg.storage
    for x in (st.observations, st.actions, st.values, st.actions_log_prob, st.mu):
        x.normal_()
    st.rewards.normal_().mul_(0.01)
    st.sigma.fill_(1.0)
    return types.SimpleNamespace(alg=alg)


def test_cpu_baseline_leg_reports_the_contract_fields():
    out = bench.cpu_baseline(_stand_in_runner(), sim_sample_envs=16)
    assert set(out) >= {"value", "unit", "cores", "kind", "sample", "update_s", "compute_returns_s", "update_dagger_s"}
    assert out["kind"] == "port" and "learner only" in out["scope"]
    assert out["unit"] == "env-steps/s" and out["value"] > 0 and 1 <= out["cores"] <= 16
    assert out["sim_port"].get("value", 0) > 0


def test_cpu_baseline_never_imports_the_reference_tree():
    before = set(sys.modules)
    bench.cpu_baseline(_stand_in_runner(16, 4), sim_sample_envs=8)
    new = [m for m in set(sys.modules) - before if m == "rsl_rl" or m.startswith("rsl_rl.")]     # the reference's package (the port is wbc_amd.rsl_rl)
    assert not new and not (bench.REFERENCE_RSL_RL and bench.REFERENCE_RSL_RL in sys.path)


def _rsl_rl_checkout(root):
    """A stand-in for a checkout of the reference's rsl_rl: a package `rsl_rl` with the two entry points the reference leg imports
    (rsl_rl.algorithms.PPO, rsl_rl.modules.ActorCritic), here re-exporting this package's port so that the test needs nothing
    outside the repository."""
    for sub, name in (("algorithms", "PPO"), ("modules", "ActorCritic")):
        d = root / "rsl_rl" / sub
        d.mkdir(parents=True)
        (d / "__init__.py").write_text(f"from wbc_amd.rsl_rl.{sub} import {name}  # noqa: F401\n")
    (root / "rsl_rl" / "__init__.py").write_text("")
    return str(root)


def test_cpu_baseline_can_time_the_reference_classes_in_the_build_container(tmp_path, monkeypatch):
    """`bench.py --cpu-baseline-only`: kind 'reference' = the rsl_rl PPO / ActorCritic of the checkout $WBC_REFERENCE_RSL_RL names, on
    the same storage contents as the port (profiles/r05_cpu_baseline_reference_vs_port.json holds both lines from one box). The
    checkout is a stand-in built under tmp_path: what is checked is that the leg imports its classes from that location and times them."""
    ref = _rsl_rl_checkout(tmp_path)
    monkeypatch.setattr(bench, "REFERENCE_RSL_RL", ref)
    monkeypatch.setattr(sys, "dont_write_bytecode", sys.dont_write_bytecode)
    stale = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "rsl_rl" or m.startswith("rsl_rl.")}
    r = bench._synthetic_runner(32, 4)
    try:
        out = bench.cpu_baseline(r, sim_sample_envs=8, learner="reference")
        origin = sys.modules["rsl_rl"].__file__
    finally:
        while ref in sys.path:
            sys.path.remove(ref)
        for m in [m for m in sys.modules if m == "rsl_rl" or m.startswith("rsl_rl.")]:
            del sys.modules[m]
        sys.modules.update(stale)
    assert os.path.dirname(os.path.dirname(origin)) == ref
    assert out["kind"] == "reference" and ref in out["sample"] and out["value"] > 0
    port = bench.cpu_baseline(r, sim_sample_envs=8, learner="port")
    assert port["kind"] == "port" and port["value"] > 0


def test_world_size_mismatch_is_an_error_message_not_an_assert():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE=2" in (p.stderr + p.stdout)


def test_steps_below_one_is_refused_before_any_gpu_work():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps must be at least 1" in (p.stderr + p.stdout)
