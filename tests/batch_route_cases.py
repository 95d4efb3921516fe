"""What the batch routes do, as plain records: which sink a command line reaches under every combination of the
DEMETHIFY_BATCH* switches (``route_matrix``), and the argument list every ``dmf_solve_{small,mid}{,_purity,_masked}`` entry
point is called with through its public ``Problem`` method (``entry_point_calls``).  No GPU and no pytest: the same functions
run in tools/record_batch_routes.py, which wrote tests/golden/batch_routes.json and batch_calls.json, and in
tests/test_batch_routes_host.py, which holds the code to those recordings.

The seams are the ones the host tests of the batch families use: Problem.__init__ / close / solve_many*,
device.get_context, staging.reserve, shard.sharded_restarts, bootstrap.bt_ci, ic.evaluate_best_ic and a stand-in for
Problem._lib."""
import contextlib
import ctypes
import io
import itertools
import os
import types
from pathlib import Path

import numpy as np

UPSTREAM = Path(__file__).resolve().parent / "golden" / "upstream"
SIZE = 350 * 10  # the toy's N x S
P = [60.0, 80.0, 90.0, 20.0, 50.0, 90.0, 100.0, 30.0, 50.0, 10.0]  # --purity, one percentage per sample of the toy
RUN_SWITCHES = ("DEMETHIFY_BATCH", "DEMETHIFY_BATCH_MID", "DEMETHIFY_BATCH_MID_PURITY")
IC_SWITCHES = ("DEMETHIFY_BATCH", "DEMETHIFY_BATCH_MID", "DEMETHIFY_BATCH_MID_IC")
# (module, MIN or None, MAX) of every size gate
GATES = (("bootstrap", None, "SMALL_BATCH_MAX_ELEMENTS"), ("bootstrap", None, "SMALL_BATCH_PURITY_MAX_ELEMENTS"),
         ("bootstrap", "MID_BATCH_MIN_ELEMENTS", "MID_BATCH_MAX_ELEMENTS"),
         ("bootstrap", "MID_BATCH_PURITY_MIN_ELEMENTS", "MID_BATCH_PURITY_MAX_ELEMENTS"),
         ("ic", None, "SMALL_BATCH_IC_MAX_ELEMENTS"), ("ic", "MID_BATCH_IC_MIN_ELEMENTS", "MID_BATCH_IC_MAX_ELEMENTS"))
BT_CI_KEYWORDS = {"batched": False, "batched_purity": False, "batch_kernel": "small", "batched_mid_purity": False}
IC_KEYWORDS = {"batched": False, "batch_kernel": "small"}


class _Stop(Exception):
    pass


def _subsets(names):
    return [tuple(n for n, on in zip(names, bits) if on) for bits in itertools.product((False, True), repeat=len(names))]


def route_cases():
    """The grid: (id, arguments after the inputs, switches set to "1", gates) with gates "open" (every gate around the toy's
    size), "shut" (every gate away from it) or ("closed", MAX name) (that range gate with MIN > MAX, the others open)."""
    purity = ["--purity", *[str(int(p)) for p in P]]
    out = []
    for what, flags in (("restart", ["--restart", "4"]), ("confidence", ["--confidence", "90", "4"])):
        for on in _subsets(RUN_SWITCHES):
            for with_purity in (False, True):
                for gates in ("open", "shut"):
                    name = f"{what}|{'+'.join(s[10:] for s in on) or '-'}|{'purity' if with_purity else 'plain'}|{gates}"
                    out.append((name, ["--ref", "--nbunknown", "1", *flags, *(purity if with_purity else [])], on, gates))
    for criterion in ("CCC", "AIC"):
        for on in _subsets(IC_SWITCHES):
            for gates in ("open", "shut"):
                name = f"ic {criterion}|{'+'.join(s[10:] for s in on) or '-'}|{gates}"
                out.append((name, ["--ref", "--ic", criterion, "3", "1", "2"], on, gates))
    out.append(("closed|BATCH_MID", ["--ref", "--nbunknown", "1", "--restart", "4"], ("DEMETHIFY_BATCH_MID",),
                ("closed", "MID_BATCH_MAX_ELEMENTS")))
    out.append(("closed|BATCH_MID_PURITY", ["--ref", "--nbunknown", "1", "--restart", "4", *purity],
                ("DEMETHIFY_BATCH_MID_PURITY",), ("closed", "MID_BATCH_PURITY_MAX_ELEMENTS")))
    out.append(("closed|BATCH_MID_IC", ["--ref", "--ic", "CCC", "3", "1", "2"], ("DEMETHIFY_BATCH_MID_IC",),
                ("closed", "MID_BATCH_IC_MAX_ELEMENTS")))
    out.append(("init uniform", ["--ref", "--nbunknown", "1", "--restart", "4", "--init", "uniform"],
                ("DEMETHIFY_BATCH", "DEMETHIFY_BATCH_MID"), "open"))
    # no reference and two unknown types: the point estimate runs first (its sink answers instead of stopping), then the
    # replicates would have to be aligned
    out.append(("aligning", ["--nbunknown", "2", "--confidence", "90", "4"], ("DEMETHIFY_BATCH", "DEMETHIFY_BATCH_MID"),
                "open"))
    return out


@contextlib.contextmanager
def _replaced(pairs):
    """setattr for the duration: pairs of (object, name, value)."""
    saved = [(obj, name, obj.__dict__[name] if name in vars(obj) else None, name in vars(obj)) for obj, name, _ in pairs]
    try:
        for obj, name, value in pairs:
            setattr(obj, name, value)
        yield
    finally:
        for obj, name, old, had in reversed(saved):
            if had:
                setattr(obj, name, old)
            else:
                delattr(obj, name)


def _purity_kind(value):
    if value is None:
        return "none"
    return "1 - P/100" if np.array_equal(np.asarray(value, dtype=np.float64), 1 - np.array(P) / 100) else "other"


def run_route_case(case, outdir):
    """One command line on the toy up to the first sink -> the record of what arrived there."""
    from demethify_amd import bootstrap, demethify, device, ic, shard, staging

    name, flags, switches, gates = case
    modules = {"bootstrap": bootstrap, "ic": ic}
    seen = {}

    def sink(kind, batch, purity, keywords=None):
        seen.update(sink=kind, batch=batch, purity=_purity_kind(purity), keywords=keywords)
        raise _Stop

    def sharded_restarts(n_restarts, *a, **k):
        if name == "aligning":
            return np.zeros((350, 2)), np.zeros((2, 10)), 0, [0.0]  # (the point estimate; the case is about what follows)
        sink("sharded_restarts", n_restarts, None)

    def solve_many(self, u0s, alpha0s, *a, **k):
        sink("solve_many", len(u0s), k.get("purity"))

    def solve_many_mid(self, u0s, alpha0s, *a, **k):
        sink("solve_many_mid", len(u0s), k.get("purity"))

    def bt_ci(*a, **k):
        sink("bt_ci", a[1], a[13], {key: k.get(key, default) for key, default in BT_CI_KEYWORDS.items()})

    def evaluate_best_ic(*a, **k):
        sink("evaluate_best_ic", k.get("n_restarts"), None, {key: k.get(key, default) for key, default in IC_KEYWORDS.items()})

    pairs = [(device.Problem, "__init__", lambda self, *a, **k: None), (device.Problem, "close", lambda self: None),
             (device.Problem, "solve_many", solve_many), (device.Problem, "solve_many_mid", solve_many_mid),
             (device, "get_context", lambda *a: None), (staging, "reserve", lambda *a, **k: None),
             (shard, "sharded_restarts", sharded_restarts), (bootstrap, "bt_ci", bt_ci), (ic, "evaluate_best_ic", evaluate_best_ic)]
    for module, lo, hi in GATES:
        if gates == "shut":  # (above the toy for a range, below it for a one-sided gate)
            values = (SIZE + 1, 10 * SIZE) if lo else (None, SIZE - 1)
        elif gates != "open" and gates[1] == hi:
            values = (SIZE, SIZE - 1)
        else:
            values = (SIZE, SIZE)
        pairs.append((modules[module], hi, values[1]))
        if lo:
            pairs.append((modules[module], lo, values[0]))

    files = [str(UPSTREAM / "output_gen" / f"sample{i}.bed") for i in range(1, 11)]
    argv = ["--methfreq", *files, "--bedmethyl", "--noprint", "--outdir", str(outdir)]
    for flag in flags:
        argv.append(flag)
        if flag == "--ref":
            argv.append(str(UPSTREAM / "output_gen" / "ref_matrix.bed"))
    every_switch = set(RUN_SWITCHES + IC_SWITCHES)
    saved_env = {s: os.environ.pop(s, None) for s in every_switch}
    text = io.StringIO()
    try:
        os.environ.update({s: "1" for s in switches})
        with _replaced(pairs), contextlib.redirect_stdout(text):
            try:
                demethify.main(argv)
            except _Stop:
                pass
    finally:
        for s, value in saved_env.items():
            os.environ.pop(s, None)
            if value is not None:
                os.environ[s] = value
    seen["notes"] = [line for line in text.getvalue().splitlines() if line.startswith("Note:")]
    return seen


def route_matrix(outdir):
    return {case[0]: run_route_case(case, outdir) for case in route_cases()}


# ---- the argument lists of the six entry points

N, S, N_C, N_U, B = 6, 5, 2, 2, 3
PARTIAL, UNSUPERVISED = 0, 1
STEPS = dict(n_iter1=11, n_iter2=7, tol=0.125)
TUNING = {"small": dict(iters_per_launch=13), "mid": dict(rows_per_workgroup=512, check_every=9)}


class _RecordingLib:
    """Stands in for Problem._lib: every function records its arguments and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def _problem(lib):
    from demethify_amd import device

    p = device.Problem.__new__(device.Problem)
    p.N, p.S, p.n_c, p._lib, p._h, p.ctx = N, S, N_C, lib, 5678, types.SimpleNamespace(_h=1234)
    return p


def _describe(args, inputs, outputs, packed):
    """The argument list as data.  A pointer is named after the array it points into: an input of the call (the methods
    pass C-contiguous arrays of the right type through as they are), an array the method returned, or -- the one buffer the
    method makes itself -- the packed form of bool train masks, recognised by its bytes."""
    known = {a.ctypes.data: (name, a) for name, a in list(inputs.items()) + list(outputs.items())}
    out = []
    for pos, arg in enumerate(args):
        if arg is None:
            out.append({"pos": pos, "pointer": "null"})
        elif isinstance(arg, ctypes.c_void_p):
            name, a = known.get(arg.value, (None, None))
            if name is None and packed is not None and ctypes.string_at(arg.value, packed.nbytes) == packed.tobytes():
                name, a = "packed train_masks", packed
            out.append({"pos": pos, "pointer": "non-null", "array": name, "dtype": None if a is None else str(a.dtype),
                        "shape": None if a is None else list(a.shape)})
        else:
            out.append({"pos": pos, "scalar": type(arg).__name__, "value": arg})
    return out


def entry_point_calls():
    """{case: {"function", "arguments"}} for each of the six entry points through its public method: the plain and purity
    entries once with ``idx`` and once without, the masked entries once with bool masks and once with packed ones."""
    rng = np.random.RandomState(0)
    u0s, alpha0s = rng.rand(B, N, N_U), rng.rand(B, N_C + N_U, S)
    idx = rng.randint(0, N, size=(B, N)).astype(np.int64)
    purity = rng.rand(S)
    masks = rng.rand(B, N, S) < 0.7
    packed = np.packbits(masks, axis=2, bitorder="little")
    out = {}
    for family, method, masked_method in (("small", "solve_many", "solve_many_masked"),
                                          ("mid", "solve_many_mid", "solve_many_mid_masked")):
        runs = []
        for with_purity in (False, True):
            for with_idx in (False, True):
                label = f"{method}({'purity, ' if with_purity else ''}{'idx' if with_idx else 'no idx'})"
                inputs = {"u0s": u0s, "alpha0s": alpha0s}
                kw = dict(TUNING[family])
                if with_idx:
                    inputs["idx"] = kw["idx"] = idx
                if with_purity:
                    inputs["purity"] = kw["purity"] = purity
                mode = PARTIAL if with_purity else UNSUPERVISED
                runs.append((label, method, (u0s, alpha0s, mode, *STEPS.values()), kw, inputs, None))
        for form, given in (("bool", masks), ("packed", packed)):
            inputs = {"u0s": u0s, "alpha0s": alpha0s}
            if form == "packed":
                inputs["train_masks"] = packed
            runs.append((f"{masked_method}({form} masks)", masked_method, (u0s, alpha0s, given, PARTIAL, *STEPS.values()),
                         dict(TUNING[family]), inputs, packed if form == "bool" else None))
        for label, name, args, kw, inputs, expect_packed in runs:
            lib = _RecordingLib()
            problem = _problem(lib)
            results = getattr(problem, name)(*args, **kw)
            names = ("u", "alpha", "cost", "iters", "holdout_sum_sq", "n_test")
            (function, call_args), = lib.calls  # (one library call per solve_many*)
            problem._h = None  # (there is nothing to destroy)
            out[label] = {"function": function,
                          "arguments": _describe(call_args, inputs, dict(zip((f"out {n}" for n in names), results)),
                                                 expect_packed)}
    return out
