"""The numpy model of the profile intervals by CpG, shared by tests/test_ci_by_cpg_host.py and
tests/test_gpu_ci_by_cpg.py.

Replicate i has row indices idx_i (M indices into n_rows CpGs) and profiles u_i (M x n_u):
    first_i[c] = min { j : idx_i[j] == c }
    E_i[c, b]  = u_i[first_i[c], order[b]] if c was drawn in replicate i, else NaN
and the bounds are np.nanpercentile(stack(E_i), [lo, hi], axis=0)."""
import numpy as np
import pandas as pd


def first_occurrence(idx, n_rows):
    """first[c] for c < n_rows, -1 where c was not drawn: the definition, by a loop from the last position down."""
    first = np.full(n_rows, -1, dtype=np.int64)
    for j in range(len(idx) - 1, -1, -1):
        first[idx[j]] = j
    return first


def rows_by_cpg(u, idx, n_rows, order=None):
    """E_i: (n_rows, n_u), NaN rows where the CpG was not drawn; ``order`` renames the columns (None: as they are)."""
    u = np.asarray(u, dtype=np.float64)
    u = u.reshape(len(idx), -1)
    if order is not None:
        u = u[:, np.asarray(order)]
    first = first_occurrence(np.asarray(idx), n_rows)
    out = np.full((n_rows, u.shape[1]), np.nan)
    drawn = first >= 0
    out[drawn] = u[first[drawn]]
    return out


def bounds(stack, q):
    """(len(q), ...) percentiles over axis 0 with the NaNs left out; all-NaN columns give NaN (numpy warns: silenced)."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanpercentile(np.asarray(stack), q, axis=0)


def column_percentile(column, q):
    """np.percentile of one column with its NaNs removed; NaN for a column without a number."""
    kept = column[~np.isnan(column)]
    if kept.size == 0:
        return np.full(len(q), np.nan)
    return np.percentile(kept, q)


def plan(n, percentile):
    """numpy's "linear" plan for n values, in Python floats: (k_prev, k_next, gamma)."""
    quantile = percentile / 100.0
    vi = float(n - 1) * quantile
    if vi >= n - 1:
        return n - 1, n - 1, 0.0
    if vi < 0:
        return 0, 0, 0.0
    fl = np.floor(vi)
    return int(fl), int(fl) + 1, vi - fl


def interval_csv_bytes(columns, lower, upper):
    """The interval table as upstream writes it: a DataFrame of (lower, upper) tuples through DataFrame.to_csv."""
    n_rows, n_u = lower.shape
    df = pd.DataFrame({columns[k]: [(lower[j, k], upper[j, k]) for j in range(n_rows)] for k in range(n_u)})
    return df.to_csv(index=False).encode()
