"""Reference-based regression used by the initialisers and by ``--nbunknown 0``.

Host-side only (runs once, milliseconds).  The reference calls
scikit-learn's ``LinearRegression(fit_intercept=True, positive=True)`` with sample weights
(demethify/init_func.py:8-14); that estimator centres by the weighted means, rescales by
sqrt(weight) and solves scipy's NNLS, which is what is done here directly.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import nnls

__all__ = ["wls_intercept", "DEVICE_WLS_MIN_ELEMENTS", "device_wls"]

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
