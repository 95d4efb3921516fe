"""Profile intervals by CpG, the parts that need no GPU: the numpy model of the definition, what
np.nanpercentile is held to, the tail-depth bound the register-tails kernel relies on, the re-partition with NaNs in the
stack, the two entry points' declarations, and the refusals of bt_ci and of the command line."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import ci_by_cpg_model as model

from conftest import ROOT, UPSTREAM

Q_PAIRS = [[2.5, 97.5], [50.0, 50.0], [0.0, 100.0], [10.0, 90.0]]
# the percentiles at which the issue had the tail depths checked, n <= 3000
DEPTH_PERCENTILES = [0.0, 0.5, 2.5, 5.0, 50.0, 95.0, 97.5, 99.5, 100.0]


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("M,n_rows", [(1, 1), (257, 257), (100, 4099), (5000, 300)])
def test_first_occurrence_is_np_unique(M, n_rows):
    rs = np.random.RandomState(M + n_rows)
    idx = rs.randint(0, n_rows, size=M)
    first = model.first_occurrence(idx, n_rows)
    cpgs, where = np.unique(idx, return_index=True)
    want = np.full(n_rows, -1, dtype=np.int64)
    want[cpgs] = where
    assert np.array_equal(first, want)
    u = rs.rand(M, 3)
    E = model.rows_by_cpg(u, idx, n_rows, order=[2, 0, 1])
    assert np.array_equal(np.isnan(E).all(axis=1), first < 0) and not np.isnan(E[first >= 0]).any()
    assert np.array_equal(E[cpgs], u[where][:, [2, 0, 1]])
    # the product's host twin (bt_ci without torch) is the same gather
    from demethify_amd.bootstrap import _rows_by_cpg

    assert np.array_equal(_rows_by_cpg(u[:, [2, 0, 1]], idx, n_rows), E, equal_nan=True)


def nan_stack(n, m, fraction, seed):
    rs = np.random.RandomState(seed)
    x = rs.rand(n, m)
    x[rs.rand(n, m) < fraction] = np.nan
    if m >= 3:
        x[:, 0] = np.nan  # no number at all
        x[:, 1] = np.nan
        x[n // 2, 1] = 0.625  # one number
        x[:, 2] = np.round(x[:, 2], 1)  # ties
    return x


@pytest.mark.parametrize("n,m", [(1, 5), (2, 7), (7, 13), (40, 33), (200, 40), (1300, 40)])
@pytest.mark.parametrize("q", Q_PAIRS)
def test_nanpercentile_is_percentile_of_each_column_without_its_nans(n, m, q):
    x = nan_stack(n, m, 0.37, 17 * n + m)
    got = model.bounds(x, q)
    want = np.stack([model.column_percentile(x[:, c], q) for c in range(m)], axis=1)
    assert got.shape == (2, m) and np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[:, 0]).all()
    if n > 1:
        assert (got[:, 1] == 0.625).all()  # one value: that value for both bounds
    # ... and each column's value is lerp(sorted[k_prev], sorted[k_next], gamma) of the plan for its own count
    for c in range(m):
        kept = np.sort(x[~np.isnan(x[:, c]), c])
        if kept.size == 0:
            continue
        for qi, value in zip(q, got[:, c]):
            k_prev, k_next, gamma = model.plan(kept.size, qi)
            a, b = kept[k_prev], kept[k_next]
            lerp = b - (b - a) * (1 - gamma) if gamma >= 0.5 else a + (b - a) * gamma
            assert lerp == value, (c, qi, kept.size)


def test_tail_depths_do_not_shrink_as_the_count_grows():
    """The register-tails kernel is built for the depth of the full n and plans each column for its own n_c <= n on the
    same tail: k_next + 1 values from the bottom, n_c - k_prev from the top, must both be non-decreasing in n_c."""
    for q in DEPTH_PERCENTILES:
        bottom = top = 0
        for n in range(1, 3001):
            k_prev, k_next, _ = model.plan(n, q)
            assert 0 <= k_prev <= k_next <= n - 1
            assert k_next + 1 >= bottom and n - k_prev >= top, (q, n)
            bottom, top = k_next + 1, n - k_prev


# ------------------------------------------------------------------------------------------------ the re-partition
def _nanpercentile(x, q):
    return model.bounds(np.asarray(x), q)


def _repartition_stack():
    return nan_stack(7, 37, 0.37, 5)  # 7 replicates over 2 ranks: 4 + 3; 37 positions: 19 + 18


def test_percentile_over_replicates_takes_nanpercentile():
    from demethify_amd import shard

    full = _repartition_stack()
    got = shard.percentile_over_replicates(full, 7, [2.5, 97.5], _nanpercentile)
    assert np.array_equal(got, model.bounds(full, [2.5, 97.5]), equal_nan=True)
    assert np.isnan(got[:, 0]).all() and not np.isnan(got[:, 3:]).all()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist

    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    from demethify_amd import shard

    full = _repartition_stack()
    got = shard.percentile_over_replicates(full[shard.my_items(7)], 7, [2.5, 97.5], _nanpercentile)
    assert (got is not None) == (rank == 0)
    if rank == 0:
        np.save(os.path.join(out_dir, "bounds.npy"), got)
    dist.destroy_process_group()


def test_two_ranks_give_the_single_process_bounds(tmp_path):
    import torch.multiprocessing as mp

    from demethify_amd import shard

    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    single = shard.percentile_over_replicates(_repartition_stack(), 7, [2.5, 97.5], _nanpercentile)
    assert np.array_equal(np.load(tmp_path / "bounds.npy"), single, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the interface
def test_entry_points_are_declared_bound_and_exported():
    from demethify_amd import _build, _lib

    _build.build()
    header = (ROOT / "include" / "demethify_hip.h").read_text()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in ("dmf_solver_get_u_by_row", "dmf_nanpercentile_axis0"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dmf_solver_get_u_by_row"][1]) == 5
    assert _lib.SIGNATURES["dmf_nanpercentile_axis0"] == _lib.SIGNATURES["dmf_percentile_axis0"]
    assert "np.nanpercentile" in header and "np.unique" in header  # the numpy functions they restate
    assert _lib.load().dmf_abi_version() == 1  # additive: no signature changed
    # null handles are refused without a device
    assert _lib.load().dmf_solver_get_u_by_row(None, None, 1, None, None) == _lib.DMF_ERR_BAD_ARG


def test_interval_csv_writer_spells_nan_bounds_as_pandas_does(tmp_path):
    """A CpG that no replicate drew has (nan, nan): the library's writer gives the bytes DataFrame.to_csv gives."""
    from demethify_amd.bootstrap import _write_interval_csv

    rs = np.random.RandomState(2)
    lower = rs.rand(40, 2)
    upper = lower + 0.25
    for j in (0, 7, 39):
        lower[j] = upper[j] = np.nan
    lower[3, 1] = upper[3, 1] = np.nan
    cols = ["unknown_cell_1", "unknown_cell_2"]
    path = tmp_path / "native.csv"
    assert _write_interval_csv(str(path), cols, lower, upper)
    assert path.read_bytes() == model.interval_csv_bytes(cols, lower, upper)
    assert b"nan" in path.read_bytes()


def test_bt_ci_refuses_an_unknown_row_convention(tmp_path, toy):
    from demethify_amd.bootstrap import bt_ci

    V, D, ref, header = toy
    samples = [f"s{k}" for k in range(V.shape[1])]
    with pytest.raises(ValueError, match="profile_rows"):
        bt_ci(90, 2, 1, V, D, ref, "uniform_", 5, 5, 0.0, header, str(tmp_path), samples, None, 1, profile_rows="rows")
    assert not list(tmp_path.iterdir())


def test_command_line_refuses_an_unknown_row_convention(tmp_path):
    samples = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    proc = subprocess.run([sys.executable, "-m", "demethify_amd", "--ref", str(UPSTREAM / "output_gen" / "ref_matrix.bed"),
                           "--methfreq", *samples, "--bedmethyl", "--nbunknown", "1", "--confidence", "90", "4", "--outdir",
                           str(tmp_path / "out"), "--noprint"],
                          cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, DEMETHIFY_CI_ROWS="bogus"))
    assert proc.returncode == 1, proc.stderr[-2000:]
    assert "DEMETHIFY_CI_ROWS" in proc.stderr and "bogus" in proc.stderr
    assert not (tmp_path / "out").exists()  # before any output, and before any GPU work
