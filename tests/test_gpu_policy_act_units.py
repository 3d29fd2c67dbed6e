"""wbc_policy_act on its unit mapping (csrc/wbc_policy_kernel.hip): a unit is a 16-row tile with one of the four head chains
(actor-leg, actor-arm, critic-leg, critic-arm), run by one wavefront; a workgroup is four consecutive tiles of one kind, so the
mapping has edges every 64 rows on top of the 16-row tile edges, and the side-job workgroups follow 4 x ceil(tiles / 4) unit
workgroups. The cases, their float64 reference (lr.policy_act) and the K_ACT bounds are those of test_gpu_policy_ppo_fp64.py:
nothing is restated here."""
import ctypes as C

import pytest
import torch

import learner_reference as lr
from test_gpu_policy_ppo_fp64 import DEV, K_ACT, _act_case, _guard_intact, _guarded, _ratio, _stream, pol  # noqa: F401  (pol: fixture)
from wbc_amd import abi
from wbc_amd.native import check, lib

pytestmark = pytest.mark.gpu
WIDTHS = dict(actions=18, mean=18, logp=2, values=2)
# 47 | 48 | 49: the third tile's last row, the fourth tile's first, one row into it; 63 | 64 | 65: the last row of a workgroup's four
# tiles, a full workgroup, the first row of the next; 127 | 129: two workgroups per kind less a row, and one row into a third
EDGE_ROWS = [47, 48, 49, 63, 64, 65, 127, 129]


@pytest.mark.parametrize("mode", ["priv_eps", "priv_mean", "latent_eps", "latent_mean"])
@pytest.mark.parametrize("rows", EDGE_ROWS)
def test_policy_act_matches_fp64_at_workgroup_edges(pol, rows, mode):
    """_act_case of test_gpu_policy_ppo_fp64.py at the edges of four-tiles-per-workgroup: every element within K_ACT x its own E
    of float64, NaN in every input row past `rows`, sentinels behind every output, actions == mean bit for bit without eps.
    Measured on the MI355X over the 32 cases, the kernel's largest ratio (fraction of its bound): mean 1.7e-3 (0.11), actions
    1.7e-3 (0.11), sampled log-probabilities 1.0e-3 (0.07), values 1.7e-3 (0.11), log-probabilities on the mean 0.55 (0.14)."""
    _act_case(pol, rows, mode)


def _act(pol, obs, eps, latent, rows, job=None):
    """One call into NaN-filled guarded outputs; returns the four [rows, width] outputs (guards checked)."""
    L = lib()
    out = {k: _guarded(rows * n) for k, n in WIDTHS.items()}
    args = (pol["ac"].fused_param_table(), pol["wpack"].data_ptr(), obs.data_ptr(), latent.data_ptr() if latent is not None else None,
            eps.data_ptr() if eps is not None else None, out["actions"].data_ptr(), out["mean"].data_ptr(), out["logp"].data_ptr(),
            out["values"].data_ptr(), rows)
    if job is None:
        check(L.wbc_policy_act(*args, _stream()), "wbc_policy_act")
    else:
        check(L.wbc_policy_act_job(*args, C.byref(job), _stream()), "wbc_policy_act_job")
    torch.cuda.synchronize()
    for k, n in WIDTHS.items():
        assert _guard_intact(out[k], rows * n), f"{k}: a write past rows x {n}"
    return {k: out[k][:rows * n].view(rows, n) for k, n in WIDTHS.items()}


@pytest.mark.parametrize("rows", [80, 16])
def test_side_job_behind_a_tile_count_that_is_no_multiple_of_four(pol, rows):
    """5 tiles (80 rows) and 1 tile (16 rows): the unit workgroups are 4 kinds x ceil(tiles / 4), the job's workgroups come after
    them. The job's 47 statistics columns equal those of wbc_side_job_run stand-alone bit for bit, and the inference outputs equal
    those of the same call without a job bit for bit. The stand-alone launch sums with 1024 threads, the carried one with 256: the
    episode sums here are small integers and the scale a power of two, so every partial sum is exact in float32 whatever its
    order, and equality to the bit is the mapping's doing, not the rounding's. Columns 0..36 see resets, the job's envs that reset
    are a random half; `prev` is what a column without a reset would publish (none here)."""
    L = lib()
    g = torch.Generator(device=DEV).manual_seed(rows)
    obs = torch.randn(rows, 860, generator=g, device=DEV)
    eps = torch.randn(rows, 18, generator=g, device=DEV)
    n = 1500
    ep = torch.randint(-8, 9, (n, abi.NREW), generator=g, device=DEV).float()
    met = torch.randint(-8, 9, (n, abi.NMETRIC), generator=g, device=DEV).float()
    reset = (torch.rand(n, generator=g, device=DEV) < 0.5).to(torch.int64)
    prev = torch.randn(abi.NREW + abi.NMETRIC, generator=g, device=DEV)
    assert 0 < int(reset.sum()) < n
    outs = []
    for carried in (False, True):
        stats = _guarded(abi.NREW + abi.NMETRIC)
        job = abi.WbcSideJob()
        job.ep_done, job.met_done, job.reset_buf, job.prev = ep.data_ptr(), met.data_ptr(), reset.data_ptr(), prev.data_ptr()
        job.rew = job.arm_rew = job.track_state = None
        job.out, job.n, job.track_cap, job.nblocks, job.scale = stats.data_ptr(), n, 0, abi.NREW + abi.NMETRIC, 0.25
        if carried:
            got = _act(pol, obs, eps, None, rows, job=job)
        else:
            check(L.wbc_side_job_run(C.byref(job), _stream()), "wbc_side_job_run")
            got = _act(pol, obs, eps, None, rows)
        torch.cuda.synchronize()
        assert _guard_intact(stats, abi.NREW + abi.NMETRIC)
        outs.append((stats[:abi.NREW + abi.NMETRIC].clone(), got))
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0])
    for k in WIDTHS:
        assert torch.isfinite(outs[0][1][k]).all()
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize("rows", [65, 4096])
def test_two_calls_agree_bit_for_bit(pol, rows):
    """No atomics, no order that depends on the dispatch: the same inputs give the same bits."""
    g = torch.Generator(device=DEV).manual_seed(rows)
    obs = torch.randn(rows, 860, generator=g, device=DEV)
    eps = torch.randn(rows, 18, generator=g, device=DEV)
    a, b = _act(pol, obs, eps, None, rows), _act(pol, obs, eps, None, rows)
    for k in WIDTHS:
        assert torch.isfinite(a[k]).all()
        assert torch.equal(a[k], b[k]), k


def test_student_path_never_reads_the_privileged_columns_across_a_workgroup_edge(pol):
    """49 rows (three tiles and one row), latent given, NaN in obs[:, 76:100]: the actor units start at the backbone and take the
    latent blocks from `latent`, so mean, actions and both log-probabilities stay finite and within the K_ACT bounds of float64.
    The CRITIC's input is obs[:, :100] by the network's definition (Critic.forward, lr._policy_net: layer 9 reads x), with or
    without a latent: its two values are NaN in the float64 reference and in the kernel alike, which is asserted instead of
    finiteness -- no implementation of this network can return finite values here."""
    rows = 49
    g = torch.Generator(device=DEV).manual_seed(4949)
    pad = 24
    obs = torch.full((rows + pad, 860), float("nan"), device=DEV)
    obs[:rows] = torch.randn(rows, 860, generator=g, device=DEV)
    obs[:, 76:100] = float("nan")
    eps = torch.full((rows + pad, 18), float("nan"), device=DEV)
    eps[:rows] = torch.randn(rows, 18, generator=g, device=DEV)
    latent = torch.full((rows + pad, 20), float("nan"), device=DEV)
    latent[:rows] = torch.randn(rows, 20, generator=g, device=DEV)
    got = _act(pol, obs, eps, latent, rows)
    ref, E = lr.policy_act(pol["w"], pol["std"], obs[:rows], eps[:rows], latent=latent[:rows])
    for name, r64, scale_e in zip(("mean", "actions", "logp"), ref, E):
        assert torch.isfinite(r64).all() and torch.isfinite(got[name]).all(), name
        k, _ = _ratio(got[name], r64, scale_e)
        print(f"\nACT student, NaN privileged columns, rows={rows} {name}: kernel={k:.3e}", flush=True)
        assert k <= K_ACT[name], (name, k, K_ACT[name])
    assert torch.isnan(ref[3]).all() and torch.isnan(got["values"]).all()
