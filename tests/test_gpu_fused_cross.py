"""nnf_xty_gram_f32 / nnf_xht_gram_f32: a cross product with the Gram of its factor riding in the same launch, and one reduction
for the slab sets of both.  Kernel bodies, split plans and slab order are those of the separate entry points, so every output
must be the same BITS as nnf_xty_f32 + nnf_gram_f32 (nnf_gram_f64_f32) and nnf_xht_f32 + nnf_gram_f32 -- compared as integers,
so that a NaN has to match too.  The Gram rides where it has slabs (K > 1024 here, or a pitched G) and, for X H^T, at ranks above
32; everywhere else the fused entry runs the two apart, which the same comparison covers.  The last section runs the one
reduction launch of both slab sets with a main set in the plain or the four-column form (n from 8200 up) and reads the sets of
that launch from the library's NNF_REDUCE_DEBUG report."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [1, 63, 65, 257, 4099]
NS = [1, 255, 257, 1030]
RS = [1, 16, 48, 50, 52, 64, 100, 128]


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.fixture(scope="module")
def data():
    """One random pool (left unchanged): X, Ut and V of every shape are leading blocks of it."""
    g = torch.Generator(device="cpu").manual_seed(1234)
    return {"X": torch.rand(max(MS), max(NS) + 3, generator=g).cuda(), "Ut": torch.rand(max(RS), max(MS), generator=g).cuda(),
            "V": torch.rand(max(RS), max(NS), generator=g).cuda()}


def operands(data, m, n, r, pitched=False):
    """Contiguous operands, or (pitched) views into the pool, whose row pitches (1033, 4099, 1030) are no multiple of 4: the
    four-dword load path."""
    X, Ut, V = data["X"][:m, :n], data["Ut"][:r, :m], data["V"][:r, :n]
    return (X, Ut, V) if pitched else (X.contiguous(), Ut.contiguous(), V.contiguous())


def pitched_g(r, ldg):
    return torch.full((r, ldg or r), -7.0, device="cuda")[:, :r]


def check_xty(eng, X, Ut, what, ldg=None, with64=True):
    r = Ut.shape[0]
    O_ref, G_ref, G = eng.xty(X, Ut), pitched_g(r, ldg), pitched_g(r, ldg)
    g64_ref = torch.full((r, r), -7.0, dtype=torch.float64, device="cuda") if with64 else None
    g64 = g64_ref.clone() if with64 else None
    eng.gram(Ut, out=G_ref, out64=g64_ref)
    O, _ = eng.xty_gram(X, Ut, G=G, G64=g64)
    same(O, O_ref, f"xty_gram out {what}")
    same(G, G_ref, f"xty_gram G {what}")
    if with64:
        same(g64, g64_ref, f"xty_gram G64 {what}")


def check_xht(eng, X, V, what, ldg=None):
    r = V.shape[0]
    O_ref = eng.xht(X, V)
    G_ref, G = pitched_g(r, ldg), pitched_g(r, ldg)
    eng.gram(V, out=G_ref)
    O, _ = eng.xht_gram(X, V, G=G)
    same(O, O_ref, f"xht_gram out {what}")
    same(G, G_ref, f"xht_gram G {what}")


@pytest.mark.parametrize("r", RS)
def test_fused_equals_separate_all_shapes(eng, data, r):
    for m in MS:
        for n in NS:
            X, Ut, V = operands(data, m, n, r)
            check_xty(eng, X, Ut, (m, n, r))
            check_xht(eng, X, V, (m, n, r))


@pytest.mark.parametrize("r", [16, 50, 100])
def test_pitch_not_a_multiple_of_four(eng, data, r):
    """Row pitches of X (1033) and of the factors (4099, 1030) that are no multiple of 4: the dword load path of both bodies."""
    for m, n in [(4099, 1030), (257, 255), (4099, 257)]:
        X, Ut, V = operands(data, m, n, r, pitched=True)
        assert X.stride(0) == 1033 and Ut.stride(0) == 4099 and V.stride(0) == 1030
        check_xty(eng, X, Ut, ("pitched", m, n, r))
        check_xht(eng, X, V, ("pitched", m, n, r))


@pytest.mark.parametrize("r", [48, 50, 128])
def test_one_split_rider(eng, data, r):
    """K <= 64 with a pitched G: the Gram keeps its slab form with ONE split, so a single rider workgroup follows a one-split
    cross product (m = 63: one split of W^T X)."""
    X, Ut, V = operands(data, 63, 255, r)
    check_xty(eng, X, Ut, ("one split", 63, 255, r), ldg=r + 3)
    X, Ut, V = operands(data, 257, 63, r)
    check_xht(eng, X, V, ("one split", 257, 63, r), ldg=r + 3)
    check_xty(eng, X, Ut, ("no G64", 257, 63, r), ldg=r + 3, with64=False)


@pytest.mark.parametrize("r", [50, 100])
def test_nan_poisons_the_same_entries(eng, data, r):
    m, n = 4099, 1030
    X, Ut, V = operands(data, m, n, r)
    Xn = X.clone()
    Xn[m // 2, n // 3] = float("nan")
    check_xty(eng, Xn, Ut, "NaN in X")
    check_xht(eng, Xn, V, "NaN in X")
    Un, Vn = Ut.clone(), V.clone()
    Un[r // 2, m - 5] = float("nan")
    Vn[r - 1, 7] = float("nan")
    check_xty(eng, X, Un, "NaN in Ut")
    check_xht(eng, X, Vn, "NaN in V")
    O, G = eng.xty_gram(X, Un)
    assert torch.isnan(G[r // 2]).all() and torch.isnan(G[:, r // 2]).all() and int(torch.isnan(G).sum()) == 2 * r - 1
    assert torch.isnan(O[r // 2]).all() and int(torch.isnan(O).sum()) == n


def test_back_to_back_on_one_context(eng, data):
    """Two fused calls in a row on one context, different operands: the second reuses the workspace of the first."""
    r = 50
    X, Ut, V = operands(data, 4099, 1030, r)
    X2, Ut2, V2 = (X * 0.5 + 0.25), Ut.flip(1).contiguous(), V.flip(0).contiguous()
    want = [(eng.xty(a, b), eng.gram(b)) for a, b in ((X, Ut), (X2, Ut2))]
    got = [eng.xty_gram(a, b) for a, b in ((X, Ut), (X2, Ut2))]
    want_h = [(eng.xht(a, b), eng.gram(b)) for a, b in ((X, V), (X2, V2))]
    got_h = [eng.xht_gram(a, b) for a, b in ((X, V), (X2, V2))]
    for k in range(2):
        same(got[k][0], want[k][0], f"xty call {k}"), same(got[k][1], want[k][1], f"xty Gram call {k}")
        same(got_h[k][0], want_h[k][0], f"xht call {k}"), same(got_h[k][1], want_h[k][1], f"xht Gram call {k}")


def test_nmf_equals_the_separate_path(eng, monkeypatch):
    """Three HALS iterations at 2000 x 300, rank 50: the driver on the fused entries against the driver on an engine without
    them (separate launches, the Gram of V on its side stream).  Factors and costs are equal."""
    import numpy as np
    import nnfac_oracle as orc
    from nn_fac_amd import engine as _engine
    from nn_fac_amd.nmf import nmf

    class Separate(_engine.Engine):
        xty_gram = None
        xht_gram = None

    X, U0, V0 = orc.synth_nmf(2000, 300, 50, seed=3, dtype=np.float32)
    kw = dict(init="custom", U_0=U0, V_0=V0, n_iter_max=3, tol=0, update_rule="hals", return_costs=True, deterministic=True)
    with torch.cuda.device(0):
        U, V, costs, _ = nmf(X, 50, **kw)
        apart = Separate(torch.device("cuda:0"), workspace_bytes=256 << 20)
        monkeypatch.setattr(_engine, "get_engine", lambda device=None: apart)
        Us, Vs, costs_s, _ = nmf(X, 50, **kw)
    assert np.array_equal(U, Us) and np.array_equal(V, Vs)
    assert list(costs) == list(costs_s)


# ---- the multi-set reduction with a main set that is not a parts form (tests/test_gpu_reduce.py has the single sets) ----
# Up to n = 1030 the cross product's own set has r * n < 2^19: a parts form, or one slab.  Here it is several slabs in the plain
# form or the four-column form (column remainders 0, 1, 3), or one slab, next to the Gram's set in a parts form in ONE launch.
# (m, n, r, form of the main set, form of the Gram's set): m <= 257 keeps W^T X at 1 .. 5 slabs on any device.
BIG_XTY = [(130, 8200, 64, "plain", "par2"), (257, 16384, 128, "vec4", "par4"), (257, 16385, 128, "vec4", "par4"),
           (65, 16387, 128, "vec4", "par2"), (64, 16385, 128, "vec4", "plain")]


def big_xht(C):
    """X H^T shapes above rank 32 whose k-split tail has slabs, so that the tail's set and the Gram's share the launch, for a
    device of C compute units (nnf_plan_xht, k_stream_plan.h): one round of (3, 2) row tiles per wave with a few tiles beyond
    two per wave.  Rank 50 (two workgroups per CU): 106 tiles beyond -- a tail set of 50 x 1696 in a parts form; rank 128 (one
    workgroup per CU): C tiles beyond -- a tail set of 128 x 16 C >= 2^19 elements in four slabs, the plain form."""
    return [(16 * (16 * C + 106), 256, 50, "par4", "par4"), (16 * 9 * C, 256, 128, "plain", "par4")]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def big_data():
    g = torch.Generator(device="cpu").manual_seed(4321)
    return {"X": torch.rand(257, 16387, generator=g).cuda(), "Ut": torch.rand(128, 257, generator=g).cuda()}


@pytest.mark.parametrize("m,n,r,main,gram", BIG_XTY, ids=["%dx%dx%d" % s[:3] for s in BIG_XTY])
def test_main_set_plain_or_vec4_next_to_the_gram(eng, big_data, m, n, r, main, gram):
    X, Ut = big_data["X"][:m, :n].contiguous(), big_data["Ut"][:r, :m].contiguous()
    check_xty(eng, X, Ut, ("big", m, n, r), ldg=r + 3)
    check_xty(eng, X, Ut, ("big, no G64", m, n, r), ldg=r + 3, with64=False)


@pytest.mark.parametrize("which", [0, 1])
def test_tail_set_next_to_the_gram(eng, which):
    m, n, r, _, _ = big_xht(_cus())[which]
    g = torch.Generator(device="cuda").manual_seed(99 + which)
    X, V = torch.rand(m, n, generator=g, device="cuda"), torch.rand(r, n, generator=g, device="cuda")
    check_xht(eng, X, V, ("big", m, n, r), ldg=r + 3)


_REDUCE_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_fused_cross as F
from nn_fac_amd.engine import get_engine
eng = get_engine("cuda:0")
for m, n, r, _, _ in F.BIG_XTY:
    for with64 in (True, False):
        sys.stderr.write("[case] xty %d %d %d %d\n" % (m, n, r, with64))
        sys.stderr.flush()
        g64 = torch.zeros(r, r, dtype=torch.float64, device="cuda") if with64 else None
        eng.xty_gram(torch.ones(m, n, device="cuda"), torch.ones(r, m, device="cuda"), G=F.pitched_g(r, r + 3), G64=g64)
for m, n, r, _, _ in F.big_xht(F._cus()):
    sys.stderr.write("[case] xht %d %d %d 0\n" % (m, n, r))
    sys.stderr.flush()
    eng.xht_gram(torch.ones(m, n, device="cuda"), torch.ones(r, n, device="cuda"), G=F.pitched_g(r, r + 3))
torch.cuda.synchronize()
print("done")
"""


def test_fused_launch_reports_both_sets(built_lib):
    """The library's own report (NNF_REDUCE_DEBUG, one child process): every fused call above is ONE reduction launch of two
    sets, the main set in the form the table names next to the Gram's, and each set starts at the workgroup where the sets
    before it end."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _REDUCE_CHILD], env=dict(os.environ, NNF_REDUCE_DEBUG="1"), capture_output=True,
                       text=True, timeout=600, cwd=root)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    seen, cur = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[case] "):
            cur = tuple(line[7:].split())
            seen[cur] = []
        elif line.startswith("[nnf reduce] ") and cur is not None:
            seen[cur].append(dict(kv.split("=", 1) for kv in line[13:].split()))
    want = {("xty", str(m), str(n), str(r), str(int(w))): (m, n, r, a, b) for m, n, r, a, b in BIG_XTY for w in (True, False)}
    want.update({("xht", str(m), str(n), str(r), "0"): (m, n, r, a, b) for m, n, r, a, b in big_xht(_cus())})
    assert sorted(seen) == sorted(want)
    for key, (m, n, r, main, gram) in want.items():
        sets = seen[key]
        assert len(sets) == 2 and [s["set"] for s in sets] == ["0/2", "1/2"], (key, sets)
        assert [s["form"] for s in sets] == [main, gram], (key, sets)
        assert [int(s["block0"]) for s in sets] == [0, int(sets[0]["blocks"])], (key, sets)
        assert (int(sets[1]["rows"]), int(sets[1]["cols"]), sets[1]["out64"]) == (r, r, key[4]), (key, sets)
        if key[0] == "xty":
            assert (int(sets[0]["rows"]), int(sets[0]["cols"])) == (r, n) and (int(sets[0]["nslab"]) > 1) == (m > 64), (key, sets)
