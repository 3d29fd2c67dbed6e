"""The three fused MFMA kernels that carry the learner's arithmetic, each through its C-ABI, against the float64
restatements of tests/learner_reference.py (pinned on the CPU by tests/test_learner_reference.py), with element-wise bounds:

  wbc_policy_act            |err| <= K_ACT[output] * E     E: the running forward error scale of lr.policy_act
  wbc_ppo_minibatch_grad    |err| <= K_GRAD * u * S        S = sum_rows |dZ| |A|: each element's own round-off scale
  wbc_hist_train_grad       |err| <= K_HIST * u * S        (u = 2^-24)

instead of one tolerance per tensor relative to its largest entry, at the dispatch edges the kernels have (16-row tiles, two
tiles per chain workgroup, 24 <-> 48 weight-gradient row ranges at 12288 | 12289 rows, empty ranges, main loop / left-over
batch / 4-row tail; 24-row groups and 512 looping workgroups of the history-encoder kernel).

Every case: outputs and workspaces start as NaN, a sentinel region behind every buffer the kernels write must stay untouched,
the rollout tensors hold more rows than the minibatch and EVERY row idx does not name is NaN in every input, so a read
outside the gather poisons the result; no row and no element is left out of any comparison. The PPO inputs come from
lr.kink_free_batch: no row is within 1e-2 of a kink of the piecewise losses, so float32 and float64 take the same branches.

The constants are not derived and not read off the kernels: each is 4 x the largest K_ref of its family, rounded up to a power
of two, where K_ref = max over elements of |eager float32 PyTorch - float64| / E (resp. / (u S)) on the same inputs on the
MI355X -- lr.eager_act / eager_ppo_grad / eager_hist_grad, the module path with rocBLAS GEMMs that the reference implementation
itself runs. Every test prints its case's K_ref and the kernel's own maximum before it asserts (pytest -s). The margin of 4 is
two bits: the kernels sum in other orders (16 x 16 x 4 MFMA chains, 24 / 48 / up-to-512-way fixed-order splits) and use the fast
intrinsics; a bf16-split product that loses its low terms costs eight."""
import copy
import ctypes as C

import pytest
import torch

import golden_procedure as gp
import learner_reference as lr
from wbc_amd.native import check, lib
from wbc_amd.rsl_rl.modules import ActorCritic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
GUARD, SENTINEL = 256, 1.2345e30
# 4 x the largest K_ref (eager float32 vs float64, MI355X) of each group of cases, rounded up to a power of two; the K_ref
# themselves are in the tests' docstrings. One constant per kernel, as first intended, would be set by the smallest minibatch
# alone and leave the large ones unchecked -- K_ref falls from 2275 at one row to 1.3 at 40960, because S grows with the number
# of rows while round-off grows with its root, and the float32 error dZ and A already carry (which S does not model) is all
# there is at one row -- so the gradient constants are kept per minibatch size: each is at most the single constant.
# Likewise per output for the inference kernel, and the log-probabilities of actions ON the mean (eps = NULL: d = 0, E is
# u x the density's constant terms and nothing else) have their own.
K_ACT = dict(mean=2.0 ** -6, actions=2.0 ** -6, values=2.0 ** -6, logp=2.0 ** -6, logp_on_mean=4.0)
K_GRAD = {1: 16384.0, 15: 512.0, 16: 256.0, 17: 256.0, 33: 256.0, 1000: 64.0, 12288: 8.0, 12289: 64.0, 40960: 8.0}
K_HIST = {1: 2048.0, 23: 32.0, 24: 32.0, 25: 32.0, 333: 16.0, 12288: 8.0, 12289: 128.0, 24577: 256.0, 40960: 4.0}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, fill=float("nan"), dtype=torch.float32):
    """n elements of `fill` followed by GUARD sentinels."""
    t = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    t[n:] = SENTINEL
    return t


def _guard_intact(t, n):
    return bool((t[n:] == SENTINEL).all())


def _poisoned(rows_of, TN, idx):
    """Each [B, ...] tensor scattered to the rows idx of a [TN, ...] tensor that is NaN everywhere else."""
    out = {}
    for k, v in rows_of.items():
        full = torch.full((TN,) + tuple(v.shape[1:]), float("nan"), dtype=v.dtype, device=DEV)
        full[idx] = v
        out[k] = full
    return out


def _pick_rows(TN, B, g):
    """B of the rows 1 .. TN - 2 in random order: the first and the last row of the rollout tensors -- where an index clamped to
    the tensor instead of to the minibatch lands -- are never named, so they are always poison."""
    return (1 + torch.randperm(TN - 2, generator=g, device=DEV)[:B]).contiguous()


def _ratio(got, ref, scale):
    """max over elements of |got - ref| / scale (an element whose scale is 0 must be exact), and where it is."""
    err = (got.double() - ref).abs().reshape(-1)
    scale = scale.reshape(-1)
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    return r[i].item(), i


@pytest.fixture(scope="module")
def pol():
    """The policy of test_fused_act_matches_torch_modules: initialisation + 0.05 N(0, 1), std in [0.3, 1.3] -- no zero bias."""
    torch.manual_seed(3)
    ac = ActorCritic(76, 76, 18, **gp.POLICY_KW).to(DEV)
    with torch.no_grad():
        for p in ac.parameters():
            p.add_(0.05 * torch.randn_like(p))
        ac.std.copy_(0.3 + torch.rand_like(ac.std))
    w, std = lr.policy_weights(ac)
    L = lib()
    wpack = torch.empty(L.wbc_policy_pack_floats(), device=DEV)
    check(L.wbc_policy_pack(ac.fused_param_table(), wpack.data_ptr(), _stream()), "wbc_policy_pack")
    torch.cuda.synchronize()
    return dict(ac=ac, w=w, std=std, wpack=wpack, hw=lr.hist_weights(ac))


# ---------------------------------------------------------------------------------------------------------------------
# wbc_policy_act
ACT_ROWS = [1, 15, 16, 17, 31, 32, 33, 4096, 8224, 40960]
ACT_MODES = {"priv_eps": (True, False, 1.0), "priv_mean": (False, False, 1.0), "latent_eps": (True, True, 1.0), "latent_mean": (False, True, 1.0),
             "priv_eps_3x": (True, False, 3.0)}


@pytest.mark.parametrize("mode", ["priv_eps", "priv_mean", "latent_eps", "latent_mean"])
@pytest.mark.parametrize("rows", ACT_ROWS)
def test_policy_act_matches_fp64(pol, rows, mode):
    """wbc_policy_act vs lr.policy_act: mean, actions, log-probabilities, values, each element within K_ACT x its own E. With
    eps and without (actions == mean bit for bit), with the privileged encoder and with a given latent. The inputs hold 24
    more rows than `rows`, all NaN: the last 16-row tile must not let them reach a live row, and nothing is written behind
    rows x width.
    Measured on the MI355X over the 40 cases, largest K_ref of the eager float32 modules -> constant, and the kernel's largest
    ratio (as a fraction of the bound): mean 2.2e-3 -> 2^-6, kernel 2.3e-3 (0.14); actions 2.4e-3 -> 2^-6, 2.3e-3 (0.14); values
    2.3e-3 -> 2^-6, 2.5e-3 (0.16); sampled log-probabilities 2.5e-3 -> 2^-6, 2.5e-3 (0.16); log-probabilities on the mean
    0.55 -> 4, 0.55 (0.14) in all 20 cases: 18 x (log std + a constant), which both sides round alike. (E is a worst-case
    scale, about 1e-3 at the outputs: 2^-6 E is about 1e-5 ... 2e-5 absolute on means and values; 4 E about 3e-6 on a
    log-probability on the mean.)"""
    _act_case(pol, rows, mode)


def test_policy_act_matches_fp64_on_saturating_observations(pol):
    """Observations 3 N(0, 1): the tanh heads come near saturation (|mean| > 0.98 occurs) and ELU runs deep in its negative branch.
    Measured: K_ref 3.4e-4 (mean), 3.4e-4 (actions), 1.9e-4 (log-probabilities), 1.3e-3 (values), the kernel 3.7e-4, 3.8e-4, 1.1e-4,
    1.4e-3: at most 0.09 of the bounds of test_policy_act_matches_fp64, which it shares."""
    _act_case(pol, 4096, "priv_eps_3x")


def _act_case(pol, rows, mode):
    with_eps, with_latent, scale = ACT_MODES[mode]
    ac, L = pol["ac"], lib()
    g = torch.Generator(device=DEV).manual_seed(rows * 8 + list(ACT_MODES).index(mode))
    pad = 24
    obs = torch.full((rows + pad, 860), float("nan"), device=DEV)
    obs[:rows] = scale * torch.randn(rows, 860, generator=g, device=DEV)
    eps = latent = None
    if with_eps:
        eps = torch.full((rows + pad, 18), float("nan"), device=DEV)
        eps[:rows] = torch.randn(rows, 18, generator=g, device=DEV)
    if with_latent:
        latent = torch.full((rows + pad, 20), float("nan"), device=DEV)
        latent[:rows] = torch.randn(rows, 20, generator=g, device=DEV)
    widths = dict(mean=18, actions=18, logp=2, values=2)
    out = {k: _guarded(rows * n) for k, n in widths.items()}
    check(L.wbc_policy_act(ac.fused_param_table(), pol["wpack"].data_ptr(), obs.data_ptr(), latent.data_ptr() if with_latent else None,
                           eps.data_ptr() if with_eps else None, out["actions"].data_ptr(), out["mean"].data_ptr(), out["logp"].data_ptr(),
                           out["values"].data_ptr(), rows, _stream()), "wbc_policy_act")
    torch.cuda.synchronize()
    for k, n in widths.items():
        assert _guard_intact(out[k], rows * n), f"{k}: a write past rows x {n}"
    got = {k: out[k][:rows * n].view(rows, n) for k, n in widths.items()}
    assert all(torch.isfinite(v).all() for v in got.values())
    if not with_eps:
        assert torch.equal(got["actions"], got["mean"])
    o, e, lt = obs[:rows], eps[:rows] if with_eps else None, latent[:rows] if with_latent else None
    ref, E = lr.policy_act(pol["w"], pol["std"], o, e, latent=lt)
    assert scale == 1.0 or ref[0].abs().max().item() > 0.98
    with torch.no_grad():
        eager = lr.eager_act(ac, o, e, latent=lt)
    ks, kr = {}, {}
    for name, r64, scale_e, e32 in zip(("mean", "actions", "logp", "values"), ref, E, eager):
        ks[name], _ = _ratio(got[name], r64, scale_e)
        kr[name], _ = _ratio(e32, r64, scale_e)
    print(f"\nACT rows={rows} mode={mode} " + " ".join(f"{k}: K_ref={kr[k]:.3e} kernel={ks[k]:.3e}" for k in ks), flush=True)
    for name in ks:
        kname = "logp_on_mean" if name == "logp" and not with_eps else name
        assert ks[name] <= K_ACT[kname], (name, rows, mode, ks[name], K_ACT[kname])


# ---------------------------------------------------------------------------------------------------------------------
# wbc_ppo_minibatch_grad
PPO_DEFAULT = dict(clip=0.2, value_coef=1.0, mixing=0.5, roa_coef=0.1, use_clipped_value_loss=True)
# 1: one live row; 15 | 16 | 17: the 16-row tile; 33: three tiles (two chain waves idle), most row ranges empty; 1000: ranges of 48
# rows (main loop only); 12288 | 12289: 24 ranges of 512 rows <-> 48 of 264 with a 145-row last one (main loop + left-over batch +
# tail); 40960: the bench's minibatch
PPO_B = [1, 15, 16, 17, 33, 1000, 12288, 12289, 40960]
PPO_VARIANTS = {"unclipped_value": dict(use_clipped_value_loss=False), "mixing0": dict(mixing=0.0), "mixing1": dict(mixing=1.0),
                "roa0": dict(roa_coef=0.0), "value_coef_half": dict(value_coef=0.5)}
LOSS_ACCUM0 = (1.5, -2.25, 3.125)


def _ppo_inputs(pol, B, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = torch.randn(B, 860, generator=g, device=DEV)
    fields, margins = lr.kink_free_batch(pol["w"], pol["std"], obs, seed=seed + 1)
    TN = B + B // 4 + 19
    idx = _pick_rows(TN, B, g)
    return _poisoned(dict(fields, obs=obs), TN, idx), idx


def _ppo_call(fn, ac, batch, idx, opts, ws, grad, loss_accum):
    b = batch
    return fn(ac.fused_param_table(), b["obs"].data_ptr(), b["actions"].data_ptr(), b["old_values"].data_ptr(), b["advantages"].data_ptr(),
              b["returns"].data_ptr(), b["old_logp"].data_ptr(), b["hist_latent"].data_ptr(), idx.data_ptr(), idx.numel(), opts["clip"],
              opts["value_coef"], opts["mixing"], opts["roa_coef"], int(opts["use_clipped_value_loss"]), ws.data_ptr(), grad.data_ptr(),
              loss_accum.data_ptr() if loss_accum is not None else None, _stream())


def _grad_names(w):
    names = []
    for l, name in enumerate(lr.POLICY_LAYERS):
        names += [(name + ".weight", w[2 * l].numel()), (name + ".bias", w[2 * l + 1].numel())]
    return names + [("std", 18), ("loss sums", 3)]


def _where(names, i):
    for name, n in names:
        if i < n:
            return f"{name}[{i}]"
        i -= n


def _ppo_case(pol, B, opts, seed, compare=True):
    """One wbc_ppo_minibatch_grad call on poisoned inputs into guarded NaN buffers, checked against lr.ppo_minibatch.
    Returns what the follow-up checks need."""
    ac, L = pol["ac"], lib()
    batch, idx = _ppo_inputs(pol, B, seed)
    ng, nws = L.wbc_ppo_grad_floats(), L.wbc_ppo_workspace_floats(B)
    assert ng == lr.policy_grad_floats(pol["w"])
    ws, grad = _guarded(nws), _guarded(ng)
    accum = _guarded(3)
    accum[:3] = torch.tensor(LOSS_ACCUM0, device=DEV)
    check(_ppo_call(L.wbc_ppo_minibatch_grad, ac, batch, idx, opts, ws, grad, accum), "wbc_ppo_minibatch_grad")
    torch.cuda.synchronize()
    assert _guard_intact(ws, nws), "workspace written past wbc_ppo_workspace_floats(B)"
    assert _guard_intact(grad, ng), "gradient written past wbc_ppo_grad_floats()"
    assert _guard_intact(accum, 3)
    got = grad[:ng]
    assert torch.isfinite(got).all(), "a NaN reached the gradient: a read outside the rows idx names, or of memory nobody wrote"
    # loss_accum += the three sums: one float32 addition each
    assert torch.equal(accum[:3], torch.tensor(LOSS_ACCUM0, device=DEV) + got[ng - 3:])
    if not compare:
        return dict(batch=batch, idx=idx, ws=ws, grad=got.clone(), ng=ng)
    ref, S = lr.ppo_minibatch(pol["w"], pol["std"], batch, idx, **opts)
    eager = lr.eager_ppo_grad(ac, batch, idx, **opts)
    names = _grad_names(pol["w"])
    k, i = _ratio(got, ref, U * S)
    k_ref, j = _ratio(eager, ref, U * S)
    print(f"\nPPO B={B} {opts} K_ref={k_ref:.2f} at {_where(names, j)}  kernel={k:.2f} at {_where(names, i)}", flush=True)
    assert k <= K_GRAD[B], (B, opts, k, _where(names, i), got[i].item(), ref[i].item(), S[i].item())
    return dict(batch=batch, idx=idx, ws=ws, grad=got.clone(), ng=ng)


@pytest.mark.parametrize("B", PPO_B)
def test_ppo_minibatch_grad_matches_fp64(pol, B):
    """Default options (clip 0.2, value_coef 1, mixing 0.5, roa_coef 0.1, clipped value loss): every element of the 16 weight and
    bias gradients, of std's gradient and of the three loss sums within K_GRAD u S of float64; loss_accum receives += of the
    sums. Then the partial sums of squares the call left at wbc_ppo_sq_partials_offset(B): their float64 sum is the squared
    norm of the kernel's OWN gradient (weights, biases, std; not the loss slots) to 32 u relative -- each partial is a 256-leaf
    tree of non-negative terms, one squaring and 8 additions deep -- and wbc_ppo_clip_adam given them takes, bit for bit, the
    step it takes when it recomputes the norm itself (sq_partials = NULL), with the clip active.
    Measured on the MI355X, B: K_ref of eager float32 autograd -> K_GRAD[B], the kernel's largest ratio (fraction of the bound):
        1: 2275 -> 16384, 2054 (0.13)    15: 76.2 -> 512, 68.9 (0.13)     16: 46.7 -> 256, 60.1 (0.23)
       17: 48.7 -> 256, 63.1 (0.25)      33: 35.5 -> 256, 25.1 (0.10)   1000: 8.67 -> 64, 7.87 (0.12)
    12288: 1.80 -> 8, 1.54 (0.19)     12289: 8.53 -> 64, 1.93 (0.03)   40960: 1.30 -> 8, 1.47 (0.18)
    (1000 and 12289: the largest K_ref of the default case and the five of test_ppo_minibatch_grad_options_match_fp64. At 12289
    rows the eager path sums each weight gradient in one rocBLAS GEMM, at 12288 and 40960 in 32 partial ones: hence its K_ref.)
    The sums of squares: at most 0.17 u relative."""
    L = lib()
    c = _ppo_case(pol, B, PPO_DEFAULT, seed=B)
    nparam = c["ng"] - 3
    sq_off, nparts = int(L.wbc_ppo_sq_partials_offset(B)), int(L.wbc_ppo_clip_adam_workspace_floats())
    left = c["ws"][sq_off:sq_off + nparts].double()
    own = c["grad"][:nparam].double().pow(2).sum().item()
    assert torch.isfinite(left).all() and (left >= 0).all()
    print(f"\nSQ B={B} partials vs own squared norm: {abs(left.sum().item() - own) / (U * own):.2f} u", flush=True)
    assert abs(left.sum().item() - own) <= 32 * U * own, (left.sum().item(), own)
    max_norm = 0.5 * own ** 0.5
    gen = torch.Generator(device=DEV).manual_seed(B)
    m0 = 1e-3 * torch.randn(nparam, generator=gen, device=DEV)
    v0 = 1e-5 * torch.rand(nparam, generator=gen, device=DEV) + 1e-9
    steps = []
    for given in (True, False):
        ac = copy.deepcopy(pol["ac"])
        g, m, v = c["grad"].clone(), m0.clone(), v0.clone()
        aws = torch.full((nparts,), float("nan"), device=DEV)
        check(L.wbc_ppo_clip_adam(ac.fused_param_table(), g.data_ptr(), m.data_ptr(), v.data_ptr(), max_norm, 0.9, 0.999, 1e-8, 1e-3 / (1 - 0.9 ** 7),
                                  (1 - 0.999 ** 7) ** 0.5, 1.0, c["ws"].data_ptr() + 4 * sq_off if given else None, aws.data_ptr(), _stream()),
              "wbc_ppo_clip_adam")
        torch.cuda.synchronize()
        steps.append([g, m, v] + [p.detach().clone() for p in ac.fused_params()])
    clipped = steps[0][0][:nparam].double().norm().item()
    assert abs(clipped - max_norm) <= 1e-4 * max_norm                         # the clip was active
    assert not torch.equal(steps[0][3], pol["ac"].fused_params()[0])            # and a step was taken
    for a, b in zip(*steps):
        assert torch.equal(a, b)


@pytest.mark.parametrize("variant", list(PPO_VARIANTS))
@pytest.mark.parametrize("B", [1000, 12289])
def test_ppo_minibatch_grad_options_match_fp64(pol, B, variant):
    """The plain value loss, Advantage Mixing off and at 1, no latent regulariser, value_coef 0.5: the same element-wise bound.
    Measured: B = 1000: K_ref 6.84 ... 8.67, kernel 5.08 ... 7.58 (at most 0.12 of the bound); B = 12289: K_ref 5.68 ... 8.53, kernel
    1.52 ... 1.93 (0.03)."""
    _ppo_case(pol, B, dict(PPO_DEFAULT, **PPO_VARIANTS[variant]), seed=B + 100 * (1 + list(PPO_VARIANTS).index(variant)))


@pytest.mark.parametrize("B", [1000, 12289])
def test_ppo_packed_call_repeats_the_plain_one(pol, B):
    """wbc_ppo_minibatch_grad_packed on the workspace the plain call has just packed, with loss_accum = NULL (accepted): the same
    gradient bit for bit, into a buffer that started as NaN, nothing written behind it."""
    L = lib()
    c = _ppo_case(pol, B, PPO_DEFAULT, seed=B, compare=False)       # (compared in test_ppo_minibatch_grad_matches_fp64)
    grad = _guarded(c["ng"])
    check(_ppo_call(L.wbc_ppo_minibatch_grad_packed, pol["ac"], c["batch"], c["idx"], PPO_DEFAULT, c["ws"], grad, None), "wbc_ppo_minibatch_grad_packed")
    torch.cuda.synchronize()
    assert _guard_intact(grad, c["ng"]) and _guard_intact(c["ws"], L.wbc_ppo_workspace_floats(B))
    assert torch.equal(grad[:c["ng"]], c["grad"])


# ---------------------------------------------------------------------------------------------------------------------
# wbc_hist_train_grad
# 23 | 24 | 25: the 24-row group; 12288 | 12289: 512 groups = the last one-group-per-workgroup launch, then workgroup 0 loops;
# 24577: the first row of a third pass of workgroup 0
HIST_TRAIN_ROWS = [1, 23, 24, 25, 333, 12288, 12289, 24577, 40960]


@pytest.mark.parametrize("rows", HIST_TRAIN_ROWS)
def test_hist_train_grad_matches_fp64(pol, rows):
    """wbc_hist_train_grad vs lr.hist_train on rows gathered in random order out of a larger, otherwise-NaN batch: the eight
    gradient tensors and the loss sum in grad[-1], each element within K_HIST u S. Targets N(0, 1): no row is within 0.1 of the
    norm's kink at 0 (asserted).
    This test found a read outside the gather: the padding rows of a minibatch's last 24-row group took their x operand of the
    projection's weight gradient from row 0 of obs (times a gradient of 0: harmless only while that row is finite); they now re-read
    the minibatch's last row, as the forward pass does.
    Measured on the MI355X, rows: K_ref of eager float32 autograd -> K_HIST[rows], the kernel's largest ratio (fraction of the bound):
        1: 264 -> 2048, 263 (0.13)       23: 4.58 -> 32, 4.86 (0.15)      24: 6.61 -> 32, 7.28 (0.23)
       25: 5.30 -> 32, 6.41 (0.20)      333: 3.17 -> 16, 1.60 (0.10)   12288: 1.16 -> 8, 1.16 (0.15)
    12289: 17.8 -> 128, 1.13 (0.009)  24577: 32.2 -> 256, 1.48 (0.006)  40960: 0.67 -> 4, 0.67 (0.17)
    (12289 and 24577 rows x 10 steps do not split 32 ways: the eager path sums those weight gradients in one rocBLAS GEMM.)"""
    ac, L = pol["ac"], lib()
    g = torch.Generator(device=DEV).manual_seed(rows)
    TN = rows + rows // 4 + 19
    rows_of = dict(obs=torch.randn(rows, 860, generator=g, device=DEV), target=torch.randn(rows, 20, generator=g, device=DEV))
    idx = _pick_rows(TN, rows, g)
    full = _poisoned(rows_of, TN, idx)
    ng, nws = L.wbc_hist_train_grad_floats(), L.wbc_hist_train_workspace_floats()
    ws, grad = _guarded(nws), _guarded(ng)
    he = ac.actor.history_encoder
    hp = [he.encoder[0].weight, he.encoder[0].bias, he.conv_layers[0].weight, he.conv_layers[0].bias,
          he.conv_layers[2].weight, he.conv_layers[2].bias, he.linear_output[0].weight, he.linear_output[0].bias]
    table = (C.c_void_p * 8)(*[p.data_ptr() for p in hp])
    check(L.wbc_hist_train_grad(table, full["obs"].data_ptr(), full["target"].data_ptr(), idx.data_ptr(), rows, ws.data_ptr(), grad.data_ptr(),
                                _stream()), "wbc_hist_train_grad")
    torch.cuda.synchronize()
    assert _guard_intact(ws, nws), "workspace written past wbc_hist_train_workspace_floats()"
    assert _guard_intact(grad, ng), "gradient written past wbc_hist_train_grad_floats()"
    got = grad[:ng]
    assert torch.isfinite(got).all(), "a NaN reached the gradient: a read outside the rows idx names, or of memory nobody wrote"
    with torch.no_grad():
        dist = (full["target"][idx].double() - lr.hist_latent(pol["hw"], full["obs"][idx])).norm(p=2, dim=1)
    assert dist.min().item() >= 0.1
    ref, S = lr.hist_train(pol["hw"], full["obs"], full["target"], idx)
    assert ref.numel() == ng
    eager = lr.eager_hist_grad(ac, full["obs"], full["target"], idx)
    names = [(n, p.numel()) for n, p in zip(("encoder.weight", "encoder.bias", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
                                             "linear.weight", "linear.bias"), hp)] + [("loss sum", 1)]
    k, i = _ratio(got, ref, U * S)
    k_ref, j = _ratio(eager, ref, U * S)
    print(f"\nHIST rows={rows} K_ref={k_ref:.2f} at {_where(names, j)}  kernel={k:.2f} at {_where(names, i)}", flush=True)
    assert k <= K_HIST[rows], (rows, k, _where(names, i), got[i].item(), ref[i].item(), S[i].item())
