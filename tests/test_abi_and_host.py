"""C-ABI surface and host-side logic that need no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "nnfac_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nnf_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(built_lib):
    lib = ctypes.CDLL(built_lib)
    names = _declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/nnfac_hip.h but not exported"


def _header():
    txt = open(os.path.join(ROOT, "include", "nnfac_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


C_KINDS = ("int64_t", "size_t", "unsigned", "double", "float", "int")


def _c_kind(decl):
    """A parameter or return type of the header as one of {pointer, int, int64_t, unsigned, float, double, size_t}."""
    if "*" in decl:
        return "pointer"
    words = [w for w in re.findall(r"\w+", decl) if w != "const"]
    kinds = [w for w in words if w in C_KINDS]
    assert len(kinds) == 1 and words.index(kinds[0]) == 0, f"unparsed type in include/nnfac_hip.h: {decl!r}"
    return kinds[0]


def _ctypes_kind(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return "pointer"
    return {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_uint: "unsigned", ctypes.c_float: "float",
            ctypes.c_double: "double", ctypes.c_size_t: "size_t"}[t]


def _header_prototypes():
    """name -> (kind of the return type, [kind of each parameter]) for every prototype of include/nnfac_hip.h."""
    protos = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\b(nnf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M):
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        assert name not in protos, name
        protos[name] = (_c_kind(ret), [_c_kind(p) for p in params])
    return protos


def _header_defines():
    return {k: int(v.rstrip("u")) for k, v in re.findall(r"^#define\s+(NNF_\w+)\s+\(?(-?\d+u?)\)?\s*$", _header(), flags=re.M)}


def test_binding_table_matches_header(built_lib):
    """_lib.SIGNATURES against include/nnfac_hip.h, entry by entry: the same names, and for each the same kind of return value
    and of every parameter (any `*` is a pointer; an `int` bound as int64_t, or the reverse, would pass every other CPU test
    and corrupt a call).  The constants engine.py copies from the header equal their #defines."""
    from nn_fac_amd import _lib, engine
    assert sorted(_lib.SIGNATURES) == _declared_symbols()
    protos = _header_prototypes()
    assert sorted(protos) == _declared_symbols(), "a prototype of include/nnfac_hip.h was not parsed"
    for name, (res, args) in _lib.SIGNATURES.items():
        assert (_ctypes_kind(res), [_ctypes_kind(a) for a in args]) == protos[name], name
    d = _header_defines()
    assert engine.MAX_RANK == d["NNF_MAX_RANK"]
    assert (engine.HALS_SPARSITY, engine.HALS_NORMALIZE, engine.HALS_NONZERO) == (
        d["NNF_HALS_SPARSITY"], d["NNF_HALS_NORMALIZE"], d["NNF_HALS_NONZERO"])
    assert (engine.ST_EPS, engine.ST_CNT, engine.ST_EPS0, engine.ST_ERR, engine.ST_WORDS) == (
        d["NNF_HALS_ST_EPS"], d["NNF_HALS_ST_CNT"], d["NNF_HALS_ST_EPS0"], d["NNF_HALS_ST_ERR"], d["NNF_HALS_ST_WORDS"])
    probes = {k[len("NNF_PROBE_"):].lower(): v for k, v in d.items() if k.startswith("NNF_PROBE_") and k != "NNF_PROBE_COUNT"}
    assert engine.Engine.PROBE_KERNELS == probes and d["NNF_PROBE_COUNT"] == len(probes)
    lib = _lib.load()
    assert lib.nnf_version() >= 100
    assert lib.nnf_status_string(0) == b"ok"
    assert b"not supported" in lib.nnf_status_string(-3)


def test_built_library_carries_the_default_build_switches(built_lib):
    """The timing-only ablation / A-B macros of the kernel sources (XHT_ABL, SEG_ABL, MTTKRP_ABL, HALS_LATE_ISSUE, ...): a stray
    -D in a build would silently ship a kernel that skips work.  Every translation unit records the values it was compiled
    with (nnf_build_flags); the library under test must carry the product defaults in every unit."""
    from nn_fac_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192)
    n = lib.nnf_build_flags(buf, 8192)
    assert 0 < n < 8192
    got = dict(u.split(": ", 1) for u in buf.value.decode().split("; "))
    hals = "HALS_LATE_ISSUE=1 HALS_MID_AT(R)=((R) - 1) HALS_DBG=0"
    quad = "QUAD_MID_SEL=1 HALS_LATE_ISSUE=1"
    mu = "MU_WG_PER_CU=2 MU_STEP_FENCE()=__builtin_amdgcn_sched_barrier(0)"
    parts = _tool("check_sweep_spills").parts            # the part lists of the Makefile: the one place that names them
    assert len(parts("FAST")) >= 4 and len(parts("QUAD")) >= 4
    want = {"k_xht": "XHT_ABL=0", "k_xty": "XTY_BIG_WG=2", "k_mttkrp": "SEG_ABL=0 MTTKRP_ABL=0", "k_hals_wave": "WAVE_DBG=0 WAVE_REFRESH_V=8",
            "k_hals_mfma": "MFMA_NREF_V=32 MFMA_EARLY=1 MFMA_DBG=0",
            **{f"k_hals_fast{i}": hals for i in parts("FAST")}, **{f"k_hals_quad{i}": quad for i in parts("QUAD")},
            **{f"k_mu{i}": mu for i in range(3)}}
    for unit, flags in want.items():
        assert got.get(unit) == flags, (unit, got.get(unit))


def test_tucker_rank_above_the_kernels_limit_is_refused_at_the_boundary():
    """The reference takes any rank up to min(shape) (nn_fac/nmf.py:175-178).  The matrix path and NTF follow it (rank chunks,
    generic sweep kernel: tests/test_gpu_bigrank.py); the TUCKER kernels (core contractions, core update) stop at 128 and every
    drop-in entry on that path says so before anything is uploaded or launched (also without a GPU), not as a bare status code."""
    from nn_fac_amd.utils.errors import EngineError
    from nn_fac_amd.update_rules.mu import mu_tensorial
    from nn_fac_amd.ntd import ntd
    rng = np.random.RandomState(0)
    r = 129
    calls = [lambda: ntd(rng.rand(130, 131, 132), [r, 4, 4], n_iter_max=1),
             lambda: mu_tensorial(rng.rand(r, 4, 4), [rng.rand(130, r), rng.rand(131, 4), rng.rand(132, 4)], rng.rand(130, 131, 132), 1)]
    for f in calls:
        with pytest.raises(EngineError, match="rank 129 is above the 128"):
            f()


def test_no_gpu_means_loud_failure(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nn_fac_amd.utils.errors import EngineError
    from nn_fac_amd.update_rules.nnls import hals_nnls_acc
    from nn_fac_amd.nmf import nmf
    r = np.random.RandomState(0)
    with pytest.raises(EngineError):
        hals_nnls_acc(r.rand(4, 6), r.rand(4, 4), r.rand(4, 6))
    with pytest.raises(EngineError):
        nmf(r.rand(20, 10), 3, n_iter_max=2, deterministic=True)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "nn_fac_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert "nnfac_oracle" not in src and "import oracle" not in src and "from oracle" not in src, f


def test_argument_exceptions_are_raised_before_touching_the_device():
    from nn_fac_amd.utils import errors as err
    from nn_fac_amd.update_rules.nnls import hals_nnls_acc
    from nn_fac_amd.update_rules.mu import mu_betadivmin, switch_alternate_mu
    from nn_fac_amd.nmf import nmf
    r = np.random.RandomState(0)
    # tests/nnls_tests.py:21-28,46-47 of the reference
    with pytest.raises(err.ArgumentException):
        hals_nnls_acc(r.rand(8, 8), r.rand(8, 8), np.array([]))
    with pytest.raises(err.ArgumentException):
        hals_nnls_acc(r.rand(8), r.rand(8, 8), r.rand(8, 8))
    with pytest.raises(err.ArgumentException):
        hals_nnls_acc(r.rand(8, 8), r.rand(8), r.rand(8, 8))
    with pytest.raises(err.ArgumentException):
        hals_nnls_acc(r.rand(8), r.rand(15, 15), r.rand(15, 1), nonzero=True)
    with pytest.raises(err.InvalidArgumentValue):
        mu_betadivmin(r.rand(5, 2), r.rand(2, 4), r.rand(5, 4), -0.5)
    with pytest.raises(err.InvalidArgumentValue):
        switch_alternate_mu(r.rand(5, 4), r.rand(5, 2), r.rand(2, 4), 1, "Z")
    # tests/NMF_tests.py:45-54
    with pytest.raises(err.InvalidInitializationType):
        nmf(r.rand(20, 10), 3, init="invalid_init", n_iter_max=2, deterministic=True)
    with pytest.raises(err.CustomNotValidFactors):
        nmf(r.rand(20, 10), 3, init="custom", U_0=None, V_0=r.rand(3, 10), n_iter_max=2)
    assert issubclass(err.ArgumentException, BaseException) and not issubclass(err.ArgumentException, Exception)
    assert issubclass(err.ZeroColumnWhenUnautorized, err.OptimException)


def test_host_helpers():
    from nn_fac_amd.update_rules.nnls import sweep_budget
    from nn_fac_amd.utils.beta_divergence import gamma_beta
    from nn_fac_amd.utils.initialize_factors import nmf_initialization
    assert sweep_budget(100, math.inf, 100000) == 100
    assert sweep_budget(100, 0.5, 6.0) == 4          # cnt <= 1 + 0.5*6
    assert sweep_budget(100, 0.5, 100000) == 100
    assert sweep_budget(500, 0.5, 0.0) == 1
    assert gamma_beta(0) == 0.5 and gamma_beta(1) == 1 and gamma_beta(2) == 1 and gamma_beta(3) == 0.5
    U, V = nmf_initialization(np.zeros((73, 25)), 9, "random", deterministic=True, seed=0)
    assert abs(U[0][0] - 0.5488135) < 1e-7 and abs(V[0][0] - 1.15834001e-01) < 1e-7   # NMF_tests.py:40-41


def test_sweep_kernels_never_touch_a_load_destination_before_its_wait(built_lib):
    """tools/check_sweep_spills.py on the ISA the build kept next to the sweep objects (k_hals_fast: hand-issued s_load into
    SGPRs; k_hals_quad: hand-issued ds_read_b128 into VGPRs): no instruction of a sweep block may name a register with such a
    load in flight before the wait that covers it -- the abort class of round 1 (a rank instantiation over the SGPR budget
    made the allocator move an in-flight buffer).  Runs in seconds after `make`; compiles to assembly otherwise."""
    bad, blocks = _tool("check_sweep_spills").check_all()   # (asserts that every CH 1 .. 32 and every padded rank was seen)
    assert blocks >= 60, blocks          # every rank instantiation of both kernels was seen
    assert not bad, bad[:3]


def test_streaming_kernels_keep_their_prefetch_ring_in_flight(built_lib):
    """tools/check_loop_drains.py on the ISA the build kept for k_xty / k_xht / k_mttkrp: the chunk loops of the streaming MFMA
    kernels of the BASELINE configurations hold no `s_waitcnt vmcnt(0)` -- a full drain of the X prefetch ring per trip is
    what hipcc emits when a load sits under a branch and its value is used at once (round 2: 30 of the mode-2 MTTKRP's
    125 us).  A regression shows up here, on the CPU, instead of as a slower bench line."""
    mod = _tool("check_loop_drains")
    build = os.path.join(ROOT, "nn_fac_amd", "csrc", "build")
    want = {"k_xty.s": ["nnf_xty_kernel<3, 2, true>", "nnf_xty_kernel<6, 4, true>", "nnf_xty_kernel<2, 0, true>"],
            "k_xht.s": ["nnf_xht_kernel<3, 2, true, 4>", "nnf_xht_kernel<6, 4, true, 4>"],
            "k_mttkrp.s": ["nnf_mttkrp_rows_kernel<2, true, true>", "nnf_mttkrp_seg_kernel<2, true>",
                           "nnf_mttkrp_rows_kernel<4, true, true>", "nnf_mttkrp_seg_kernel<4, true>"]}
    for fname, kernels in want.items():
        path = os.path.join(build, fname)
        if not os.path.exists(path):     # a library that came without its build directory: make recreates objects and ISA
            import __graft_entry__
            __graft_entry__.build()
        assert os.path.exists(path), f"{path}: the Makefile keeps the ISA of the streaming kernels next to the objects"
        found = mod.scan(path)
        for k in kernels:
            hits = [loops for name, loops in found.items() if k + "(" in name]
            assert hits, f"{k} not found in {fname}"
            for loops in hits:
                # (X H^T: the one-tile loops of the k-split tail -- 16 MFMAs per rank tile and trip, two trips per wave -- are
                #  not the streaming loop)
                mt = int(k.split("<")[1].split(",")[0])
                main = [l for l in loops if l["mfma"] >= max(90, 16 * mt + 1)]
                assert main, (k, loops)
                assert all(l["vmcnt0"] == 0 for l in main), (k, main)


def test_tile_count_dispatcher_and_rank_passes_on_the_cpu(tmp_path):
    """nn_fac_amd/csrc/k_dispatch.h under the host compiler's address and undefined-behaviour sanitizers, as a stand-alone
    program (tools/dispatch_check.cpp): each of 1 .. N reaches its own instantiation exactly once, every value outside 1 .. N
    (0, N + 1, INT_MAX, negatives) takes N, and the rank passes cover a rank above 128 in order, hand the workspace back after
    each pass and stop at the first error."""
    import subprocess
    exe = str(tmp_path / "dispatch_check")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "nn_fac_amd", "csrc"), os.path.join(ROOT, "tools", "dispatch_check.cpp"), "-o", exe],
                   check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-2000:] + p.stderr[-2000:]


# Parameters of Engine methods the double does not take, each with the reason it may lack them.
ENGINE_ONLY_PARAMS = {
    ("gram", "out64"): "the fp64 Gram sums feed the Gram-identity cost, which nmf.py only turns on for the HIP engine",
    ("mu_left", "cost_out"): "the KL cost fused into the left update (r <= 64) is an Engine-only shortcut; drivers fall back to betadiv",
}


def test_engine_double_keeps_the_engine_signatures():
    """tests/engine_double.OracleEngine stands in for nn_fac_amd.engine.Engine in the gloo world-size-2 suite and bench.py's
    multi-rank launch test: every public method it has must exist on Engine with the same parameters (names, order, kinds,
    defaults) up to ENGINE_ONLY_PARAMS, the class constants both carry must agree, and every method must have a case in the GPU
    contract table (tests/test_gpu_engine_contract.py) that compares the two on the device."""
    import inspect
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from engine_double import OracleEngine
    from nn_fac_amd.engine import Engine
    from test_gpu_engine_contract import CONTRACT
    public = [n for n in vars(OracleEngine) if not n.startswith("_")]
    methods = [n for n in public if callable(getattr(OracleEngine, n))]
    consts = [n for n in public if n not in methods]
    assert methods and consts
    for name in methods:
        assert callable(getattr(Engine, name, None)), f"Engine has no method {name}"
        want = [p for p in inspect.signature(getattr(Engine, name)).parameters.values()
                if (name, p.name) not in ENGINE_ONLY_PARAMS]
        got = list(inspect.signature(getattr(OracleEngine, name)).parameters.values())
        assert [(p.name, p.kind, p.default) for p in got] == [(p.name, p.kind, p.default) for p in want], name
    for (name, param) in ENGINE_ONLY_PARAMS:           # the allow-list names real, current differences only
        assert param in inspect.signature(getattr(Engine, name)).parameters
        assert param not in inspect.signature(getattr(OracleEngine, name)).parameters
    for name in consts:
        assert getattr(Engine, name, None) == getattr(OracleEngine, name), name
    missing = sorted(set(methods) - set(CONTRACT))
    assert not missing, f"OracleEngine methods without a GPU contract case: {missing}"
    assert all(CONTRACT[m] for m in methods)


def test_every_engine_method_has_its_refusals_tested():
    """tests/test_gpu_engine_args.py spoils one operand at a time of every public Engine method that takes a tensor: a method
    added to Engine gets rows there (or a place in NO_TENSOR), a row is (operands, call, ways not refused[, more of them
    without the optional outputs]), and no row is left behind for a method that is gone."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from nn_fac_amd.engine import Engine
    from test_gpu_engine_args import NO_TENSOR, ROWS
    public = {n for n, v in vars(Engine).items() if not n.startswith("_") and callable(getattr(Engine, n))}
    assert not set(ROWS) & NO_TENSOR
    assert set(ROWS) | NO_TENSOR == public, sorted(public ^ (set(ROWS) | NO_TENSOR))
    for name, rows in ROWS.items():
        assert rows and all(len(row) in (3, 4) and callable(row[0]) and callable(row[1]) for row in rows), name
        known = {"d", "c", "n"} | {s + str(k) for s in "+-" for k in range(8)}
        assert all(set(ways) <= known for row in rows for free in row[2:] for ways in free.values()), name
