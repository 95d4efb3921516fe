"""Reference-based regression used by the initialisers and by ``--nbunknown 0``, and the SVD initialiser's host route.

Host-side only (runs once, milliseconds).  The reference calls
scikit-learn's ``LinearRegression(fit_intercept=True, positive=True)`` with sample weights
(demethify/init_func.py:8-14); that estimator centres by the weighted means, rescales by
sqrt(weight) and solves scipy's NNLS, which is what is done here directly.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import nnls

__all__ = ["wls_intercept", "DEVICE_WLS_MIN_ELEMENTS", "device_wls", "nndsvd_initialize", "constrained_nndsvd",
           "nndsvd_from_eig", "project_simplex_columns", "DEVICE_SVD_MIN_ELEMENTS", "device_svd"]

# From this many elements N * S of meth_frequency on, the callers that solve one regression per sample (the reference-based
# run, its bootstrap, the "uniform" initialiser of the restart loop) take device.Problem.wls_intercept instead of S host
# solves; below it they run the host code unchanged.  The smallest power of two at which the device path, upload included,
# beats the host path by at least 2x, as measured by tools/wls_bench.py on one MI355X (profiles/r10_wls_bench.txt; 12+0
# types, 16 samples, target d v, medians of five):
#     N * S     host        device with upload   device, problem resident
#     2^12      2.31 ms     0.59 ms  (3.9x)      0.151 ms
#     2^14      4.17 ms     0.59 ms  (7.0x)      0.152 ms
#     2^16     10.51 ms     0.67 ms  (15.6x)     0.164 ms
#     2^20    262.7  ms     1.37 ms  (191x)      0.219 ms
#     2^22   1475.7  ms     4.39 ms  (336x)      0.425 ms
# 2^12 is the smallest size the sweep measured, and the smallest power of two above the 350 x 10 fixture that the
# test-suite's command-line runs must keep on the host path; below it nothing was measured.  Not measured either: one
# sample per call, where the ~0.6 ms of a problem upload and three launches is not shared between samples.
DEVICE_WLS_MIN_ELEMENTS = 1 << 12


def device_wls(n_rows, n_samples, n_types):
    """Whether a caller with an N x S problem and K = n_types profile columns takes the device regression."""
    from ._lib import MAX_K

    return n_rows * n_samples >= DEVICE_WLS_MIN_ELEMENTS and 1 <= n_types <= MAX_K


# From this many elements N * S on, the SVD initialiser takes device.Problem.nndsvd (the S x S Gram of the residual on the
# FP64 matrix cores, a host eigendecomposition, one projection pass) instead of S host regressions and a LAPACK SVD of the
# N x S residual; below it, for shapes the kernels do not take (device_svd) and for bi-cross-validation folds it runs the
# host code below.  NOT MEASURED: tools/svd_init_bench.py is the sweep that is to set this constant (the smallest power of
# two at which the device route, upload included, beats the host route by 2x); until its output is recorded under
# profiles/ the gate stays at the regression's value, whose S host solves are part of the host route here too.
DEVICE_SVD_MIN_ELEMENTS = DEVICE_WLS_MIN_ELEMENTS


def device_svd(n_rows, n_samples, n_c, rank):
    """Whether a caller with an N x S problem, n_c known profile columns and ``rank`` unknown ones takes the device
    route of the SVD initialiser."""
    from ._lib import SVD_MAX_LDS, SVD_MAX_NC, SVD_MAX_RANK, SVD_MAX_S, svd_project_lds_bytes

    return (n_rows * n_samples >= DEVICE_SVD_MIN_ELEMENTS and n_samples <= SVD_MAX_S and 0 <= n_c <= SVD_MAX_NC
            and 1 <= rank <= SVD_MAX_RANK and svd_project_lds_bytes(n_samples, rank) <= SVD_MAX_LDS)


def _pos_neg(x):
    return np.maximum(x, 0), np.maximum(-x, 0)


def nndsvd_initialize(V, rank, flag=0):
    """init_func.py:40-82 -> (W, H): NNDSVD of a non-negative N x S matrix from its leading ``rank`` singular triples.
    flag 1 fills the zeros with mean(V), flag 2 with mean(V) * uniform(0, 1) / 100 from numpy's global generator."""
    from scipy.linalg import svd

    V = np.asarray(V)
    if np.any(V < 0):
        raise ValueError("The input matrix contains negative elements.")
    U, S, E = svd(V, full_matrices=False)
    E = E.T
    W = np.zeros((V.shape[0], rank))
    H = np.zeros((rank, V.shape[1]))
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(E[:, 0].T)
    for i in range(1, rank):
        uup, uun = _pos_neg(U[:, i])
        vvp, vvn = _pos_neg(E[:, i])
        n_uup, n_vvp = np.linalg.norm(uup, 2), np.linalg.norm(vvp, 2)
        n_uun, n_vvn = np.linalg.norm(uun, 2), np.linalg.norm(vvn, 2)
        termp = n_uup * n_vvp
        termn = n_uun * n_vvn
        if termp >= termn:
            W[:, i] = np.sqrt(S[i] * termp) / n_uup * uup
            H[i, :] = np.sqrt(S[i] * termp) / n_vvp * vvp.T
        else:
            W[:, i] = np.sqrt(S[i] * termn) / n_uun * uun
            H[i, :] = np.sqrt(S[i] * termn) / n_vvn * vvn.T
    W[W < 1e-11] = 0
    H[H < 1e-11] = 0
    if flag == 1:
        avg = np.mean(V)
        W[W == 0] = avg
        H[H == 0] = avg
    elif flag == 2:
        avg = np.mean(V)
        W[W == 0] = avg * np.random.uniform(0, 1, size=W[W == 0].shape) / 100
        H[H == 0] = avg * np.random.uniform(0, 1, size=H[H == 0].shape) / 100
    return W, H


def constrained_nndsvd(Y, W1, counts, rank, flag=0):
    """init_func.py:17-37 -> (W, H) = ([W1 | W2], [H1; H2]): the per-sample regression on the known profiles W1, then
    NNDSVD of the residual max(Y - W1 H1, 1e-8), W2 clipped to [0, 1]."""
    n_samples = Y.shape[1]
    H1 = np.zeros((W1.shape[1], n_samples))
    for i in range(n_samples):
        H1[:, i] = wls_intercept(Y[:, i], counts[:, i], W1)
    Y_residual = np.maximum(Y - W1 @ H1, 1e-8)
    W2, H2 = nndsvd_initialize(Y_residual, rank=rank, flag=flag)
    W2 = np.clip(W2, 0, 1)
    return np.hstack([W1, W2]), np.vstack([H1, H2])


def project_simplex_columns(v, z=1):
    """deconvolution.py:21-37 on the host: the sort-based projection of every column onto the simplex of mass z (rho = the
    last index whose sorted entry exceeds the running threshold).  The SVD initialiser projects its K x S factor with this
    rather than with the device kernel: it also runs on worker threads, and a context is not thread-safe."""
    v = np.asarray(v, dtype=np.float64)
    p, n = v.shape
    srt = -np.sort(-v, axis=0)
    shifted = np.cumsum(srt, axis=0) - z
    ok = (srt - shifted / np.arange(1, p + 1, dtype=np.float64)[:, None]) > 0
    rho = np.where(ok.any(axis=0), p - 1 - np.argmax(ok[::-1], axis=0), -1)  # (-1 wraps around, as upstream's pi[rho])
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = shifted[rho, np.arange(n)] / (rho + 1)
    return np.maximum(v - theta[None, :], 0)


def nndsvd_from_eig(sigma, E, norms_sq):
    """The host half of the device route: from the leading singular values ``sigma`` (rank,), the right singular vectors
    ``E`` (S x rank) and the squared norms of the positive and negative parts of the left ones (``norms_sq``, 2 x rank),
    what init_func.py:50-71 decides -> (sign, scale, H): column j of W is scale_j |u_j| (sign 0) or scale_j
    max(sign_j u_j, 0) before the 1e-11 cut, and H is the cut rank x S factor."""
    rank = len(sigma)
    sign, scale = np.zeros(rank), np.zeros(rank)
    H = np.zeros((rank, E.shape[0]))
    scale[0] = np.sqrt(sigma[0])
    H[0, :] = np.sqrt(sigma[0]) * np.abs(E[:, 0])
    for i in range(1, rank):
        vvp, vvn = _pos_neg(E[:, i])
        n_uup, n_uun = np.sqrt(norms_sq[0, i]), np.sqrt(norms_sq[1, i])
        n_vvp, n_vvn = np.linalg.norm(vvp, 2), np.linalg.norm(vvn, 2)
        termp = n_uup * n_vvp
        termn = n_uun * n_vvn
        with np.errstate(divide="ignore", invalid="ignore"):
            if termp >= termn:
                sign[i], scale[i] = 1.0, np.sqrt(sigma[i] * termp) / n_uup
                H[i, :] = np.sqrt(sigma[i] * termp) / n_vvp * vvp
            else:
                sign[i], scale[i] = -1.0, np.sqrt(sigma[i] * termn) / n_uun
                H[i, :] = np.sqrt(sigma[i] * termn) / n_vvn * vvn
    H[H < 1e-11] = 0
    return sign, scale, H


def wls_intercept(x, d_x, R_full):
    """Weighted non-negative least squares with intercept, renormalised to proportions.

    Same arguments and return value as the reference's ``wls_intercept``: x (N,) or (N, 1)
    targets, d_x weights, R_full (N, K) profiles -> (K, 1) proportions summing to 1.
    """
    weights = np.asarray(d_x, dtype=np.float64).ravel()
    profiles = np.asarray(R_full, dtype=np.float64)
    target = np.asarray(x, dtype=np.float64)
    one_dim = target.ndim == 1
    target = target.reshape(profiles.shape[0], -1)
    root_w = np.sqrt(weights)[:, None]
    centred_profiles = (profiles - np.average(profiles, axis=0, weights=weights)) * root_w
    centred_target = (target - np.average(target, axis=0, weights=weights)) * root_w
    coef = np.stack([nnls(centred_profiles, centred_target[:, j])[0]
                     for j in range(centred_target.shape[1])])
    if one_dim:
        coef = coef[0]
    temp = coef.T
    return temp / max(temp.sum(), 1e-10)
