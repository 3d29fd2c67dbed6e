"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the recursive inertial-parameter identification that csrc/wbc_arm_kernel.hip
computes (wbc_sim_identification_accumulate, wbc_sim_identification_solve; the definitions are those of include/wbc_sim.h):

    A <- forget A + Phi^T W Phi,   b <- forget b + Phi^T W z,   stat <- forget stat + (sum_c w_c z_c^2, rows with w_c > 0),
    z = tau_gen - sum over the bodies that are not listed of Y_b pi_b,     (A + Lambda) pi_hat = b + Lambda pi_0.

Written on regressor_reference.py (world-frame recursion), not from the kernel. Next to every accumulated entry stands its magnitude: the
sum of the absolute values of the terms that make it up, propagated from regressor_reference's `mag` (products of magnitudes, sums of
magnitudes; the inertia about the body origin of a body that is not listed: |I_c| + m |(|c|^2 1 - c c^T)|), the scale an fp32
evaluation's rounding error is proportional to.

dtype=np.float32 runs the same chain in numpy float32: the yardstick the fp32 kernels are measured against."""
import numpy as np

import regressor_reference as rr

NCOL, NP = rr.NCOL, rr.NP


def live_rows(model):
    """[26] bool: the rows that count (every row but the locked fingers')."""
    return rr.subtree_mask(model).any(axis=1)


def linear_parameters(model, bp, dtype=np.float64):
    """(pi, pimag) [nb, 10] of every moving body at body_params bp [20], evaluated in `dtype`."""
    th = rr.theta_of(model, bp).astype(dtype)
    m, c, I = th[:, 0:1], th[:, 1:4], th[:, 4:10]
    shift = rr._shift(c)
    return (np.concatenate([m, m * c, I + m * shift], axis=1).astype(dtype),
            np.concatenate([np.abs(m), np.abs(m * c), np.abs(I) + np.abs(m) * np.abs(shift)], axis=1).astype(dtype))


def regress(model, quat, q, nu, nudot, bp, bodies, tau_gen, gravity=rr.GRAVITY, dtype=np.float64):
    """(Phi [26, P], Phimag, z [26], zmag) of one env: the listed bodies' columns and the target."""
    Y, mag = rr.regressor(model, quat, q, nu, nudot, gravity, dtype)
    return split(model, Y, mag, bp, bodies, tau_gen)


def split(model, Y, mag, bp, bodies, tau_gen):
    """regress() from the regressor (Y, mag) [26, nb, 10] of the state, in Y's dtype."""
    dtype = Y.dtype.type
    pi, pimag = linear_parameters(model, bp, dtype)
    others = [b for b in range(model.nb) if b not in bodies]
    tau_gen = np.asarray(tau_gen, dtype=dtype)
    z = tau_gen - np.einsum("cbk,bk->c", Y[:, others], pi[others]).astype(dtype)
    zmag = np.abs(tau_gen) + np.einsum("cbk,bk->c", mag[:, others], pimag[others]).astype(dtype)
    P = len(bodies) * NP
    return Y[:, list(bodies)].reshape(NCOL, P), mag[:, list(bodies)].reshape(NCOL, P), z, zmag


def accumulate(model, prev, Phi, Phimag, z, zmag, row_weight=None, forget=1.0):
    """One update of one env. prev: None (reset) or the dict a previous call returned. Returns a dict with A, b, stat and their
    magnitudes Amag, bmag, statmag (the count's magnitude is the count). An update without a row of positive weight returns prev as it
    is (zeros after a reset)."""
    dtype = Phi.dtype
    w = np.ones(NCOL, dtype) if row_weight is None else np.asarray(row_weight, dtype=dtype)
    w = np.where(live_rows(model), w, 0).astype(dtype)
    rows = int((w > 0).sum())
    if rows == 0 and prev is not None:
        return prev
    new = {"A": Phi.T @ (w[:, None] * Phi), "Amag": Phimag.T @ (w[:, None] * Phimag), "b": Phi.T @ (w * z), "bmag": Phimag.T @ (w * zmag),
           "stat": np.array([(w * z * z).sum(), rows], dtype), "statmag": np.array([(w * zmag * zmag).sum(), rows], dtype)}
    if prev is not None:
        f = dtype.type(forget)
        new = {k: (f * prev[k] + v).astype(dtype) for k, v in new.items()}
    return {k: v.astype(dtype) for k, v in new.items()}


def theta_map(pi):
    """(m, c = h / m, I_c = Ibar - m (|c|^2 1 - c c^T)) [..., 10] of linear parameters [..., 10]."""
    return rr.theta_from_pi(pi)


def flags(theta):
    """Bits 1..3 of the status word of one body's theta [10] (float64): m <= 0, I_c not positive definite, triangle inequality."""
    I6 = theta[4:10]
    lam = np.linalg.eigvalsh(np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]]))
    return (2 if not theta[0] > 0 else 0) | (4 if not lam[0] > 0 else 0) | (8 if not lam[0] + lam[1] >= lam[2] else 0)


def flags_are_clear(theta, margin=1e-3):
    """True where none of the three decisions of flags() is within `margin` (relative to the largest principal moment; the mass: to
    itself) of its boundary: the cases an fp32 evaluation must decide alike."""
    I6 = theta[4:10]
    lam = np.linalg.eigvalsh(np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]]))
    size = np.abs(lam).max()
    return bool(theta[0] != 0 and abs(lam[0]) > margin * size and abs(lam[0] + lam[1] - lam[2]) > margin * size)


def solve(A, b, stat=None, prior=None, prior_weight=None, pivot_tol=1e-5, dtype=np.float64):
    """One env: dict with pi_hat [P], theta_hat [P], cov_diag [P], sse, status [P / 10], pivot2 (the squared pivots of the equilibrated
    factor) of (A + Lambda) pi = b + Lambda pi_0, equilibrated to a unit diagonal and solved by Cholesky, in `dtype`."""
    A, b = np.asarray(A, dtype=dtype), np.asarray(b, dtype=dtype)
    P = len(b)
    lam = np.zeros(P, dtype) if prior_weight is None else np.asarray(prior_weight, dtype=dtype).reshape(P)
    p0 = np.zeros(P, dtype) if prior is None else np.asarray(prior, dtype=dtype).reshape(P)
    M = A + np.diag(lam)
    d = np.diag(M)
    bad = not np.all((d > 0) & np.isfinite(d))
    out = {"pivot2": None}
    if not bad:
        s = (1 / np.sqrt(d)).astype(dtype)
        Ms = (s[:, None] * M * s[None, :]).astype(dtype)
        try:
            L = np.linalg.cholesky(Ms)
            out["pivot2"] = np.diag(L) ** 2
            bad = not np.all(out["pivot2"] > pivot_tol)
        except np.linalg.LinAlgError:
            bad = True
    if bad:
        pi = p0.copy()
        out.update(pi_hat=pi, cov_diag=np.full(P, np.inf, dtype), status=np.ones(P // NP, np.int32),
                   theta_hat=theta_map(pi.reshape(-1, NP)).reshape(P) if prior is not None else np.zeros(P, dtype))
    else:
        rhs = (s * (b + lam * p0)).astype(dtype)
        y = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).astype(dtype)
        pi = (s * y).astype(dtype)
        Li = np.linalg.solve(L, np.eye(P, dtype=dtype))
        theta = theta_map(pi.reshape(-1, NP))
        out.update(pi_hat=pi, cov_diag=(s * (Li * Li).sum(axis=0) * s).astype(dtype), theta_hat=theta.reshape(P),
                   status=np.array([flags(t.astype(np.float64)) for t in theta], np.int32))
    if stat is not None:
        out["sse"] = max(dtype(stat[0]) - 2 * (pi @ b) + pi @ (A @ pi), dtype(0))
    return out
