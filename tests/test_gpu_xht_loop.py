"""The chunk loop of the register-fragment X H^T kernel (k_xht.hip): whole chunks two per trip without a mask, one odd whole
chunk behind them, the ragged end of the row in a masked copy of the chunk -- in every body a launch runs (four, three, two row
tiles per wave and the one-tile k-split shares), for nnf_xht_f32 and nnf_xht_gram_f32, with 16-byte and with dword loads of X.

Column counts: 0 .. 4 whole chunks with and without a ragged one (1, 3, 4, 63 .. 193), and 208 and 272, which end like 2000
(n % 64 = 16).  Ranks: leftover rows 0, 2 and 4 next to 2 .. 7 rank tiles.  Rows: two counts per rank, from the CU count of the
device, so that the one-round plans of k_stream_plan.h run the (3, 2)- and the (4, 3)-tile mixes; from 193 columns on (four
chunks) the same row counts take the k-split tail instead, whose shares here are 0, 1 and 2 chunks long, the last one ragged.
test_the_table_reaches_every_body asks the library's own plan header (tools/nnf_plan.cpp) which bodies and shares each case runs.

Checks per case: (a) against the fp64 product, within the bound tests/test_gpu_kernels.py puts on X H^T (1e-5 of the norm and
1e-5 of the largest entry); (b) NaN and Inf in the row padding of X (and NaN in that of V) change no bit; (c) a second launch
gives the same bits; (d) small integers: every partial sum is exact in fp32, so the result IS the integer product -- a chunk
dropped, doubled or masked wrongly is an integer off."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKSPACE = 256 << 20   # the context's default

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 63, 64, 65, 127, 128, 129, 191, 192, 193, 208, 272]
RS = [33, 48, 50, 52, 64, 100]
EXTRA = 30          # row tiles beyond a whole round: 8 workgroups of the taller mix, or a tail of 30 tiles


def bits(t):
    return t.contiguous().view(torch.int32)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def staged_tiles(r, vec):
    """Rank tiles the kernel stages (k_stream_plan.h: nnf_xht_tiles): 16-row tiles, plus one for 1 .. 4 leftover rows where X
    is read in 16-byte pieces (ranks 51, 52: four padded tiles)."""
    q, rem = divmod(r, 16)
    if vec and 1 <= q <= 7 and 1 <= rem <= 4 and not (q == 3 and rem > 2):
        return q + 1
    return (r + 15) // 16


def row_counts(cus, r):
    """Two row counts with a ragged last tile: EXTRA tiles beyond two, and beyond three, tiles per wave of one round."""
    slots = (2 if staged_tiles(r, True) <= 4 else 1) * cus
    return [16 * (k * 4 * slots + EXTRA) - 5 for k in (2, 3)]


@pytest.fixture(scope="module")
def plan_tool():
    """tools/nnf_plan.cpp, a plain host program over the header the launcher takes its plan from (k_stream_plan.h)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="nnf_plan_xht_loop_"), "nnf_plan")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-I", os.path.join(ROOT, "nn_fac_amd", "csrc"),
                    os.path.join(ROOT, "tools", "nnf_plan.cpp"), "-o", exe], check=True)
    return exe


def planned(tool, cus, cases):
    """For each (m, n, r, ld): (row tiles per wave of the bodies that run, chunk counts of the tail's shares), from the library's
    own plan (nnf_plan_xht_direct at the context's default workspace) as tools/nnf_plan prints it."""
    lines = "".join(f"xht {cus} {m} {n} {r} {ld} 0 {WORKSPACE}\n" for m, n, r, ld in cases)
    out = subprocess.run([tool], input=lines, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases), out[:3]
    res = []
    for (m, n, r, ld), l in zip(cases, out):
        kv = dict(f.split("=", 1) for f in re.findall(r"\S+=\S+", l))
        assert "lds" not in kv["form"] and int(kv["vec"]) == (ld % 4 == 0), l
        nth, n_hi, grid, parts, cpp = (int(kv[k]) for k in ("nth", "n_hi", "grid", "tail_parts", "tail_cpp"))
        nts = ({nth} if n_hi > 0 else set()) | ({nth - 1} if n_hi < grid else set()) | ({1} if parts else set())
        nchunk = -(-n // 64)
        res.append((nts, [max(0, min(nchunk, (p + 1) * cpp) - min(nchunk, p * cpp)) for p in range(parts)]))
    return res


def pitches(n):
    """Row pitches above n: a multiple of four (16-byte loads of X and V) and an odd one (dword loads)."""
    return 4 * ((n + 3) // 4) + 8, 4 * ((n + 3) // 4) + 9


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.fixture(scope="module")
def pool():
    """Random and small-integer operands of the largest shape (left unchanged): every case takes leading blocks of them."""
    mmax = max(max(row_counts(_cus(), r)) for r in RS)
    g = torch.Generator(device="cuda").manual_seed(2000)
    X, V = torch.rand(mmax, max(NS), device="cuda", generator=g), torch.rand(max(RS), max(NS), device="cuda", generator=g)
    Xi = torch.randint(0, 4, (mmax, max(NS)), device="cuda", generator=g).float()
    Vi = torch.randint(0, 4, (max(RS), max(NS)), device="cuda", generator=g).float()
    return {"X": X, "V": V, "Xi": Xi, "Vi": Vi, "X64": X.double(), "V64": V.double(), "Xi64": Xi.double(), "Vi64": Vi.double()}


def padded(A, rows, n, ld, pad):
    """The leading rows x n block of A as a view of a rows x ld buffer whose other columns hold `pad`."""
    buf = torch.full((rows, ld), pad, dtype=torch.float32, device="cuda")
    buf[:, :n] = A[:rows, :n]
    return buf[:, :n]


def test_the_table_reaches_every_body(plan_tool):
    """What the library plans for every case of test_chunk_loop: all four body heights run, the tail runs from four chunks on,
    and its shares are 0, 1 and 2 chunks long."""
    cus = _cus()
    cases = [(m, n, r, ld) for r in RS for m in row_counts(cus, r) for n in NS for ld in pitches(n)]
    seen, shares = set(), set()
    for (m, n, r, ld), (nts, sh) in zip(cases, planned(plan_tool, cus, cases)):
        seen |= nts
        shares |= set(sh)
        assert bool(sh) == (n >= 193), (m, n, r, ld)
        assert nts == ({min(nts - {1}), 1} if sh else {max(nts) - 1, max(nts)}), (m, n, r, ld, nts)
    assert seen == {1, 2, 3, 4} and shares == {0, 1, 2}


@pytest.mark.parametrize("n", NS)
def test_chunk_loop(eng, pool, n):
    cus = _cus()
    nan, inf = float("nan"), float("inf")
    for r in RS:
        for m in row_counts(cus, r):
            want = pool["V64"][:r, :n] @ pool["X64"][:m, :n].t()
            want_i = pool["Vi64"][:r, :n] @ pool["Xi64"][:m, :n].t()          # (integers below 2^24: exact in fp64 and fp32)
            gram = pool["V64"][:r, :n] @ pool["V64"][:r, :n].t()
            for ld in pitches(n):
                what = (m, n, r, ld)
                V0, Vn = padded(pool["V"], r, n, ld, 0.0), padded(pool["V"], r, n, ld, nan)
                zero = eng.xht(padded(pool["X"], m, n, ld, 0.0), V0)
                # (a) the fp64 product
                err = zero.double() - want
                assert float(err.norm() / want.norm()) < 1e-5, what
                assert float(err.abs().max() / want.abs().max()) < 1e-5, what
                # (b) the padding, both entry points; (c) a second launch
                assert bool(torch.isfinite(zero).all()), what
                assert torch.equal(bits(eng.xht(padded(pool["X"], m, n, ld, nan), Vn)), bits(zero)), ("xht, NaN", what)
                assert torch.equal(bits(eng.xht(padded(pool["X"], m, n, ld, inf), Vn)), bits(zero)), ("xht, Inf", what)
                Xn = padded(pool["X"], m, n, ld, nan)
                first, G = eng.xht_gram(Xn, Vn)
                assert torch.equal(bits(first), bits(zero)), ("xht_gram, NaN", what)
                assert float((G.double() - gram).norm() / gram.norm()) < 1e-5, what
                again, G2 = eng.xht_gram(Xn, Vn)
                assert torch.equal(bits(again), bits(first)) and torch.equal(bits(G2), bits(G)), ("second launch", what)
                assert torch.equal(bits(eng.xht_gram(padded(pool["X"], m, n, ld, inf), V0)[0]), bits(zero)), ("xht_gram, Inf", what)
                assert torch.equal(bits(eng.xht(Xn, Vn)), bits(zero)), ("second launch", what)
                # (d) the ordered sum on integers, padding NaN
                Xi, Vi = padded(pool["Xi"], m, n, ld, nan), padded(pool["Vi"], r, n, ld, nan)
                assert torch.equal(eng.xht(Xi, Vi).double(), want_i), ("xht, integers", what)
                assert torch.equal(eng.xht_gram(Xi, Vi)[0].double(), want_i), ("xht_gram, integers", what)
