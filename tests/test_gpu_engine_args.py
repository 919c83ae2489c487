"""What nn_fac_amd.engine.Engine refuses: every public method that takes a tensor, one operand spoilt at a time.

ROWS is one table: method -> rows, each a valid call at the smallest shapes that exercise every operand (m = 5, n = 7, r = 3, a
3 x 4 x 5 tensor, 2 groups; matrices are views of wider buffers wherever the method takes a leading dimension).  EVERY tensor
operand of a row is spoilt in EVERY way below, one at a time:
    +k  extent k one larger        -k  extent k one smaller        (each extent on its own)
    d   the other float width (int32 for the segment table)        c  the same tensor on the CPU
    n   the same shape, not contiguous (inner stride 2; not tried on a single element, which is contiguous whatever its stride)
and the method must raise EngineError (ArgumentException where EXC says so), reach no compute entry of the library -- a proxy in
`eng.lib` records every nnf_* entry that is not a host-side query -- and leave every tensor argument as it was, bit for bit.
The table does not list what is refused; it lists, per row, the few ways that are NOT, each for a reason the row states: an
operand that may be larger than needed (a Gram of at least r x r, float64 words, more snapshot blocks), an extent that sets the
problem's size when nothing else in the call fixes it, an operand the method copies before use.
Every row runs twice: as written, and with the caller's optional outputs (OUTPUTS) left out, so that a check cannot hide behind
the comparison with `out`; the fourth element of a row names what that frees.  The valid call of every row and variant runs on
the real library first: a row must not refuse for the wrong reason.  tests/test_abi_and_host.py checks on the CPU that every
public method of Engine has rows here or is listed in NO_TENSOR.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, R = 5, 7, 3
TS = (3, 4, 5)          # the 3-way tensor
NG, TOTAL = 2, 7        # groups, and the columns they share: [0, 3), [3, 7)
OUTPUTS = ("out", "G", "status")        # optional outputs a variant of each row leaves to the method

# public methods of Engine without a tensor argument
NO_TENSOR = {"hals_resid_floats", "hals_resident_columns", "hals_group_max_columns", "set_probe", "set_probe_ring",
             "probe_ring_count", "probe_pairs", "time_kernel"}
# entries a refusal may still reach: they launch nothing
HOST_QUERIES = {"nnf_status_string", "nnf_hals_resid_floats", "nnf_hals_resident_columns", "nnf_hals_group_max_columns"}


def mat(rows, cols, pad=3):
    """rows x cols float32 in (0.1, 1.1), a view of a buffer with `pad` more columns."""
    return (torch.rand(rows, cols + pad, device="cuda") + 0.1)[:, :cols]


def dense(*shape):
    return torch.rand(*shape, device="cuda") + 0.1


def f64(n, value=0.0):
    return torch.full((n,), float(value), dtype=torch.float64, device="cuda")


def gram(r, pad=3):
    """A well-conditioned r x r Gram as a padded view."""
    a = torch.rand(r, r + 2, device="cuda")
    buf = torch.zeros(r, r + pad, device="cuda")
    buf[:, :r] = a @ a.t() + torch.eye(r, device="cuda")
    return buf[:, :r]


def stack(groups, rows, cols, grams=False):
    buf = torch.rand(groups, rows, cols + 2, device="cuda") + 0.1
    if grams:
        for g in range(groups):
            buf[g, :, :cols] = gram(rows)
    return buf[:, :, :cols]


def off():
    return torch.tensor([0, 3, TOTAL], dtype=torch.int64, device="cuda")


def _xuv():
    return dict(X=mat(M, N), Ut=mat(R, M), V=mat(R, N))


def _solve():
    return dict(UtM=mat(R, N), UtU=gram(R), V=mat(R, N))


def _cp3():
    return dict(T=dense(*TS), Ft=[mat(R, d) for d in TS])


def _core(shape):
    return dict(core=dense(*shape), MtX=dense(*shape), grams=[gram(d).contiguous() for d in shape], status=f64(6))


def _arg_exc():
    from nn_fac_amd.utils.errors import ArgumentException
    return ArgumentException


BOTH = ("+0", "-0", "+1", "-1")
LARGER = ("+0", "+1")                 # a Gram may be larger than r x r: only its leading dimension is used
MORE = ("+0",)                        # float64 words / snapshot blocks: at least the count
GRAM = {"UtU": LARGER}
COPIED = {"MtX": ("n",), ("grams", 0): ("n",), ("grams", 1): ("n",), ("grams", 2): ("n",), ("grams", 3): ("n",), "status": MORE}
# operands whose refusal is an ArgumentException (the reference's class for a bad argument of the Tucker entries)
EXC = {("ttm3", "T", w) for w in "dcn"} | {(m, op, w) for m in ("ntd_core_pg", "ntd_core_pgn") for op in ("core", "MtX", "grams")
                                           for w in ("d", "c", "n") + tuple(s + str(k) for s in "+-" for k in range(4))}

# method -> [(operands, call(engine, operands), {operand: ways NOT refused}, {the same, more, when OUTPUTS are left out})]
ROWS = {
    "gram": [(lambda: dict(A=mat(R, N), out=mat(R, R), out64=f64(R * R)),
              lambda e, o: e.gram(o["A"], out=o.get("out"), out64=o["out64"]),
              {"A": ("+1", "-1"), "out64": MORE},                 # A's columns are summed over: any K
              {"A": ("-0",)})],                                   # without out, A sets r (r + 1 would outgrow out64)
    "xht": [(lambda: dict(X=mat(M, N), V=mat(R, N), out=mat(R, M)), lambda e, o: e.xht(o["X"], o["V"], out=o.get("out")),
             {}, {"X": ("+0", "-0"), "V": ("+0", "-0")})],        # without out: m and r are the operands' own
    "xty": [(lambda: dict(X=mat(M, N), Ut=mat(R, M), out=mat(R, N)), lambda e, o: e.xty(o["X"], o["Ut"], out=o.get("out")),
             {}, {"X": ("+1", "-1"), "Ut": ("+0", "-0")})],
    "xty_gram": [(lambda: dict(X=mat(M, N), Ut=mat(R, M), out=mat(R, N), G=mat(R, R), G64=f64(R * R)),
                  lambda e, o: e.xty_gram(o["X"], o["Ut"], out=o.get("out"), G=o.get("G"), G64=o["G64"]),
                  {"G64": MORE}, {"X": ("+1", "-1"), "Ut": ("-0",)})],
    "xht_gram": [(lambda: dict(X=mat(M, N), V=mat(R, N), out=mat(R, M), G=mat(R, R)),
                  lambda e, o: e.xht_gram(o["X"], o["V"], out=o.get("out"), G=o.get("G")),
                  {}, {"X": ("+0", "-0"), "V": ("+0", "-0")})],
    "frob_resid": [(lambda: dict(_xuv(), out=f64(1)), lambda e, o: e.frob_resid(o["X"], o["Ut"], o["V"], out=o.get("out")),
                    {"out": MORE})],
    "gram_cost": [(lambda: dict(_solve(), normx2=f64(1, 100.0), words=f64(3), UtU64=f64(R * R, 1.0)),
                   lambda e, o: e.gram_cost(o["V"], o["UtM"], o["UtU"], o["normx2"], o["words"], UtU64=o["UtU64"]),
                   dict(GRAM, normx2=MORE, words=MORE)),
                  (lambda: dict(_solve(), normx2=f64(1, 100.0), words=f64(3), UtU_b=gram(R)),
                   lambda e, o: e.gram_cost(o["V"], o["UtM"], o["UtU"], o["normx2"], o["words"], UtU_b=o["UtU_b"],
                                            rounding=(6e-8, 1e-9)),
                   dict(normx2=MORE, words=MORE))],
    "cross_rounding": [(lambda: dict(X=mat(M, N), Ut=mat(R, M)), lambda e, o: e.cross_rounding(o["X"], o["Ut"]),
                        {"X": ("+1", "-1"), "Ut": ("+0", "-0")})],                  # n and r are the operands' own
    "gram_rounding": [(lambda: dict(Ut=mat(R, M)), lambda e, o: e.gram_rounding(o["Ut"]), {"Ut": BOTH})],     # any r x m
    "dot": [(lambda: dict(A=mat(M, N), B=mat(M, N)), lambda e, o: e.dot(o["A"], o["B"]), {})],
    "hadamard": [(lambda: dict(A=mat(R, R), B=mat(R, R), out=dense(R, R)),
                  lambda e, o: e.hadamard(o["A"], o["B"], out=o.get("out")),
                  {"A": ("n",), "B": ("n",)})],                   # copied to contiguous buffers first (docstring)
    "hals_solve": [(lambda: dict(_solve(), status=f64(8)),
                    lambda e, o: e.hals_solve(o["UtM"], o["UtU"], o["V"], 3, status=o.get("status")), dict(GRAM, status=MORE))],
    "hals_solve_cross": [(lambda: dict(UtM=mat(R, N), Ga=gram(R), Gb=gram(R), V_in=mat(R, N), V_out=mat(R, N), status=f64(8)),
                          lambda e, o: e.hals_solve_cross(o["UtM"], o["Ga"], o["Gb"], o["V_in"], o["V_out"], 3,
                                                          status=o.get("status")), {"status": MORE}),
                         (lambda: dict(UtM=mat(R, N), Ga=gram(R), V_in=mat(R, N), V_out=mat(R, N)),
                          lambda e, o: e.hals_solve_cross(o["UtM"], o["Ga"], None, o["V_in"], o["V_out"], 3), {"Ga": LARGER})],
    "hals_sweeps": [(lambda: dict(_solve(), snapshots=dense(3, R, N), resid_in=dense(4), resid_out=dense(4)),
                     lambda e, o: e.hals_sweeps(o["UtM"], o["UtU"], o["V"], 3, snapshots=o["snapshots"], resid_in=o["resid_in"],
                                                resid_out=o["resid_out"]),
                     # (the kernel layout that runs at this shape keeps no residual state: hals_resid_floats() = 0 elements)
                     dict(GRAM, snapshots=MORE, resid_in=("+0", "-0"), resid_out=("+0", "-0")))],
    "hals_row_update": [(lambda: dict(_solve(), out=f64(2)),
                         lambda e, o: e.hals_row_update(o["UtM"], o["UtU"], o["V"], 1, out=o.get("out")), dict(GRAM, out=MORE))],
    "hals_row_scale": [(lambda: dict(V=mat(R, N), normsq=f64(1, 2.0)), lambda e, o: e.hals_row_scale(o["V"], 1, o["normsq"], N),
                        {"V": BOTH, "normsq": MORE})],            # V is the only matrix: any r x ncols
    "hals_solve_group": [(lambda: dict(UtM=mat(R, TOTAL), UtU=stack(NG, R, R, grams=True), V=mat(R, TOTAL), off=off(),
                                       status=torch.zeros((NG, 8), dtype=torch.float64, device="cuda")),
                          lambda e, o: e.hals_solve_group(o["UtM"], o["UtU"], o["V"], o["off"], 4, 3, status=o.get("status")),
                          {"UtU": ("+1", "+2"), "status": LARGER})],
    "group_gram": [(lambda: dict(A=mat(R, TOTAL), off=off(), B=mat(R, TOTAL), T=mat(R, TOTAL), out64=f64(NG * R * R)),
                    lambda e, o: e.group_gram(o["A"], o["off"], B=o["B"], T=o["T"], out64=o["out64"]),
                    {"off": ("-0",), "out64": MORE})],            # the table's length IS the number of groups; fewer fit out64
    "group_gemm": [(lambda: dict(M=stack(NG, 2, R), A=mat(R, TOTAL), off=off(), out=mat(2, TOTAL)),
                    lambda e, o: e.group_gemm(o["M"], o["A"], o["off"], 4, out=o.get("out")),
                    {}, {"M": ("+1", "-1"), "A": ("+1", "-1")})],                   # without out: p and total are the operands' own
    "frob_resid_rows": [(lambda: dict(_xuv(), out=f64(M)),
                         lambda e, o: e.frob_resid_rows(o["X"], o["Ut"], o["V"], out=o.get("out")), {"out": MORE})],
    "hals_stop_restore": [(lambda: dict(sums=torch.tensor([4.0, 1.0, 1e-3], dtype=torch.float64, device="cuda"),
                                        V=mat(R, N), snapshots=dense(3, R, N), st=f64(4)),
                           lambda e, o: e.hals_stop_restore(o["sums"], 0, 10, 0.01, o["V"], o["snapshots"], o["st"]),
                           {"sums": ("-0",), "snapshots": MORE, "st": MORE})],     # sums sets the number of sweeps (docstring)
    "mu_left": [(lambda: dict(_xuv(), out=mat(R, M), cost_out=f64(1)),
                 lambda e, o: e.mu_left(o["X"], o["Ut"], o["V"], 1, out=o.get("out"), cost_out=o["cost_out"]), {"cost_out": MORE}),
                (lambda: dict(_xuv(), out=mat(R, M)), lambda e, o: e.mu_left(o["X"], o["Ut"], o["V"], 0.5, out=o.get("out")), {})],
    "mu_mode": [(lambda: dict(T3=dense(*TS), Ft=mat(R, TS[1]), V=mat(R, TS[0] * TS[2]), out=mat(R, TS[1])),
                 lambda e, o: e.mu_mode(o["T3"], o["Ft"], o["V"], 1, out=o.get("out")), {})],
    "mu_right": [(lambda: dict(_xuv(), out=mat(R, N)), lambda e, o: e.mu_right(o["X"], o["Ut"], o["V"], 1, out=o.get("out")), {})],
    "mu_right_accum": [(_xuv, lambda e, o: e.mu_right_accum(o["X"], o["Ut"], o["V"], 1), {}),
                       (_xuv, lambda e, o: e.mu_right_accum(o["X"], o["Ut"], o["V"], 0.5), {})],
    "mu_apply": [(lambda: dict(F=mat(R, N), num=mat(R, N), den=mat(R, N), out=mat(R, N)),
                  lambda e, o: e.mu_apply(o["F"], o["num"], o["den"], None, 0.5, out=o.get("out")), {}),
                 (lambda: dict(F=mat(R, N), num=mat(R, N), den_vec=f64(R, 2.0)),
                  lambda e, o: e.mu_apply(o["F"], o["num"], None, o["den_vec"], 1), {"den_vec": MORE})],
    "simplex_proj": [(lambda: dict(H=mat(R, N), num=mat(R, N), den_vec=f64(R, 2.0), lambda0=f64(N), out=mat(R, N), lambda_out=f64(N),
                                   status=f64(2)),
                      lambda e, o: e.simplex_proj(o["H"], o["num"], None, o["den_vec"], lambda0=o["lambda0"], out=o.get("out"),
                                                  lambda_out=o["lambda_out"], status=o.get("status")),
                      {"den_vec": MORE, "lambda0": MORE, "lambda_out": MORE, "status": MORE}),
                     (lambda: dict(H=mat(R, N), num=mat(R, N), den=mat(R, N) + 1),
                      lambda e, o: e.simplex_proj(o["H"], o["num"], o["den"], None), {})],
    "mu_left_num": [(lambda: dict(_xuv(), out=mat(R, M)), lambda e, o: e.mu_left_num(o["X"], o["Ut"], o["V"], out=o.get("out")), {})],
    "small_gemm": [(lambda: dict(A=mat(2, R), B=mat(R, N), out=mat(2, N)), lambda e, o: e.small_gemm(o["A"], o["B"], out=o.get("out")),
                    {}, {"A": ("+0", "-0"), "B": ("+1", "-1")})],                   # without out: p and cols are the operands' own
    "deep_kl_apply": [(lambda: dict(Ft=mat(R, M), num=mat(R, M), hsum=f64(R, 2.0), WHnext_t=mat(R, M), out=mat(R, M)),
                       lambda e, o: e.deep_kl_apply(o["Ft"], o["num"], o["hsum"], o["WHnext_t"], 0.5, out=o.get("out")), {})],
    "mttkrp3_from_partial": [(lambda: dict(Y=dense(R, 4, 5), Ft=mat(R, 5), out=mat(R, 4)),
                              lambda e, o: e.mttkrp3_from_partial(o["Y"], o["Ft"], 2, out=o.get("out")),
                              {}, {"Y": ("+1", "-1")})],          # without out: the extent that is not contracted is Y's own
    "ttm3": [(lambda: dict(T=dense(*TS), Ft=mat(R, TS[2]), out=dense(R, TS[0], TS[1])),
              lambda e, o: e.ttm3(o["T"], o["Ft"], 2, out=o.get("out")),
              {}, {"T": ("+0", "-0", "+1", "-1"), "Ft": ("+0", "-0")})],            # without out: only the contracted extent is tied
    "ntd_core_pg": [(lambda: _core((2, 3, 2)),
                     lambda e, o: e.ntd_core_pg(o["core"], o["MtX"], o["grams"], 0.0, 0.01, 5, 100.0, status=o.get("status")), COPIED)],
    "ntd_core_pgn": [(lambda: _core((2, 3, 2, 2)),
                      lambda e, o: e.ntd_core_pgn(o["core"], o["MtX"], o["grams"], 0.0, 0.01, 5, 100.0, status=o.get("status")),
                      COPIED)],
    "betadiv": [(lambda: dict(_xuv(), out=f64(1)), lambda e, o: e.betadiv(o["X"], o["Ut"], o["V"], 1, out=o.get("out")),
                 {"out": MORE})],
    "mttkrp3": [(lambda: dict(_cp3(), out=mat(R, TS[1])), lambda e, o: e.mttkrp3(o["T"], o["Ft"], 1, out=o.get("out")), {})],
    "cp3_partial_cost": [(lambda: dict(_cp3(), Y=dense(R, TS[0], TS[1]), cost=f64(1)),
                          lambda e, o: e.cp3_partial_cost(o["T"], o["Ft"], o["Y"], o["cost"]), {"cost": MORE})],
    "cp3_betadiv": [(lambda: dict(_cp3(), out=f64(1)), lambda e, o: e.cp3_betadiv(o["T"], o["Ft"], 2, out=o.get("out")),
                     {"out": MORE})],
}
CASES = [(m, i, v) for m, rows in ROWS.items() for i in range(len(rows)) for v in ("as written", "outputs left out")]
IDS = [f"{m}-{i}-{'out' if v == 'as written' else 'noout'}" for m, i, v in CASES]
SAID_BY = {"cross_rounding": "xty", "gram_rounding": "gram"}     # (the two are compositions: the message names the product they call)


def ways(t):
    """Every way of spoiling `t` (module docstring)."""
    return [s + str(k) for k in range(t.dim()) for s in "+-"] + ["d", "c"] + (["n"] if t.numel() > 1 else [])


def spoil(t, how):
    """`t` with one property wrong; the values do not matter, the call must not get as far as reading them."""
    if how == "c":
        return t.cpu()
    if how == "d":
        return t.to({torch.float32: torch.float64, torch.float64: torch.float32, torch.int64: torch.int32}[t.dtype])
    shape = list(t.shape)
    if how == "n":
        shape[-1] *= 2
        return torch.ones(shape, dtype=t.dtype, device=t.device)[..., ::2]
    shape[int(how[1:])] += 1 if how[0] == "+" else -1
    return torch.ones(shape, dtype=t.dtype, device=t.device)


def _leaves(ops):
    """(key, tensor) of every tensor operand; the members of a list are keyed (name, index)."""
    for k, v in ops.items():
        if isinstance(v, list):
            yield from (((k, j), t) for j, t in enumerate(v))
        elif torch.is_tensor(v):
            yield k, v


def _bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _with(ops, key, t):
    new = {k: (list(v) if isinstance(v, list) else v) for k, v in ops.items()}
    if isinstance(key, tuple):
        new[key[0]][key[1]] = t
    else:
        new[key] = t
    return new


def row_of(method, i, variant):
    """(operands, call, {operand: ways not refused}) of one row in one variant."""
    make, call, free, *more = ROWS[method][i]
    torch.manual_seed(7)
    ops = make()
    free = {k: tuple(v) for k, v in free.items()}
    if variant != "as written":
        ops = {k: v for k, v in ops.items() if k not in OUTPUTS}
        for k, v in (more[0] if more else {}).items():
            free[k] = free.get(k, ()) + tuple(v)
    return ops, call, free


class RefusingLib:
    """Stands in for eng.lib while a refusal is expected: a compute entry that is reached is recorded and not run."""

    def __init__(self, lib):
        self._lib, self.reached = lib, []

    def __getattr__(self, name):
        if not name.startswith("nnf_") or name in HOST_QUERIES:
            return getattr(self._lib, name)

        def refused(*args):
            self.reached.append(name)
            return 0
        return refused


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.mark.parametrize("method,i,variant", CASES, ids=IDS)
def test_the_valid_call_of_the_row_is_accepted(eng, method, i, variant):
    ops, call, _ = row_of(method, i, variant)
    call(eng, ops)
    torch.cuda.synchronize()


@pytest.mark.parametrize("method,i,variant", CASES, ids=IDS)
def test_a_spoilt_operand_is_refused_before_anything_is_launched(eng, method, i, variant):
    from nn_fac_amd.engine import EngineError
    ops, call, free = row_of(method, i, variant)
    leaves = dict(_leaves(ops))
    assert set(free) <= set(leaves) | set(OUTPUTS) | {k for k in free if isinstance(k, tuple)}, "the row frees an operand it lacks"
    real = eng.lib
    try:
        for key, t in leaves.items():
            for how in ways(t):
                if how in free.get(key, ()):
                    continue
                name = key[0] if isinstance(key, tuple) else key
                want = _arg_exc() if (method, name, how) in EXC else EngineError
                tried = _with(ops, key, spoil(t, how))
                before = {k: _bits(v) for k, v in _leaves(tried)}
                eng.lib = proxy = RefusingLib(real)
                with pytest.raises(want) as info:
                    call(eng, tried)
                assert type(info.value) is want, (method, key, how, info.value)
                assert not proxy.reached, (method, key, how, proxy.reached)
                assert SAID_BY.get(method, method) in str(info.value), (method, key, how, str(info.value))
                assert {k: _bits(v) for k, v in _leaves(tried)} == before, (method, key, how)
    finally:
        eng.lib = real
