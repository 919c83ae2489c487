"""The 576-thread form of the resident lane solve (k_hals_comm.hip: 8 compute waves + 1 communication wave per workgroup, the
scaled right-hand side in LDS) against the 256-thread lane kernel it stands in for, bit for bit.

The new form changes WHERE the per-sweep sums are formed (a communication wave instead of the compute waves), not their order:
for the same call it must return the same V, the same sweep count and the same eps / eps0 words as NNF_HALS_FORCE=lane.  Every
case runs once under NNF_HALS_FORCE=comm and once under NNF_HALS_FORCE=lane from the same operands, which sit in buffers with
NaN sentinels in front, behind and in the padding of every row; the sentinels must still be there afterwards."""
import numpy as np
import pytest
import torch

from test_gpu_hals_plans import parse_report

pytestmark = pytest.mark.gpu

GUARD = 64        # sentinel floats in front of and behind every buffer
ST = 4            # status words compared: eps, count, eps0, error


def _guarded(dev, rows, cols, pad):
    """(flat, view): a rows x cols view with row pitch cols + pad inside a buffer that is NaN everywhere else."""
    ld = cols + pad
    flat = torch.full((2 * GUARD + rows * ld,), float("nan"), dtype=torch.float32, device=dev)
    return flat, flat[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols]


def _sentinels_intact(flat, rows, cols, pad):
    ld = cols + pad
    body = flat[GUARD:GUARD + rows * ld].view(rows, ld)
    return bool(torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all() and torch.isnan(body[:, cols:]).all())


class Problem:
    """Operands of one solve on the host (float32), drawn once per (r, n)."""

    def __init__(self, r, n, seed=0):
        g = np.random.RandomState(seed + 1000 * r + n)
        A = g.rand(300, r).astype(np.float32)
        self.r, self.n = r, n
        self.G = (A.T @ A).astype(np.float32)
        self.UtM = (self.G @ g.rand(r, n).astype(np.float32)).astype(np.float32)
        self.V0 = g.rand(r, n).astype(np.float32)


def _solve(eng, monkeypatch, capfd, force, p, budget, delta, sparsity=None, cross=False, pads=(0, 0, 0), chain=None):
    """One solve under NNF_HALS_FORCE=`force`; returns (V bits, status bits, last report line)."""
    dev = torch.device("cuda:0")
    monkeypatch.setenv("NNF_HALS_FORCE", force)
    monkeypatch.setenv("NNF_HALS_DEBUG", "1")
    r, n = p.r, p.n
    fm, UtM = _guarded(dev, r, n, pads[0])
    fv, V = _guarded(dev, r, n, pads[1])
    fg, G = _guarded(dev, r, r, 0)
    UtM.copy_(torch.from_numpy(p.UtM))
    G.copy_(torch.from_numpy(p.G))
    st = torch.zeros(8, dtype=torch.float64, device=dev)
    capfd.readouterr()
    if cross:
        fs, Vin = _guarded(dev, r, n, pads[2])
        Vin.copy_(torch.from_numpy(p.V0))
        eng.hals_solve_cross(UtM, G, None, Vin, V, budget, delta=delta, sparsity=sparsity, status=st)
    else:
        V.copy_(torch.from_numpy(p.V0))
        monkeypatch.setattr(eng, "HALS_MAX_SWEEPS_PER_LAUNCH", chain or type(eng).HALS_MAX_SWEEPS_PER_LAUNCH, raising=False)
        eng.hals_solve(UtM, G, V, budget, delta=delta, sparsity=sparsity, status=st)
    torch.cuda.synchronize()
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[nnf hals]")]
    assert lines, "no plan report"
    assert _sentinels_intact(fm, r, n, pads[0]) and _sentinels_intact(fv, r, n, pads[1]) and _sentinels_intact(fg, r, r, 0)
    assert np.array_equal(UtM.cpu().numpy().view(np.int32), p.UtM.view(np.int32))
    if cross:
        assert _sentinels_intact(fs, r, n, pads[2]) and np.array_equal(Vin.cpu().numpy().view(np.int32), p.V0.view(np.int32))
    return V.cpu().numpy().view(np.int32).copy(), st.cpu().numpy()[:ST].view(np.int64).copy(), [parse_report(ln) for ln in lines]


def _both(eng, monkeypatch, capfd, p, budget, delta, **kw):
    """The same call under both forms; asserts which kernel ran and that every bit agrees.  Returns the sweep count."""
    vc, sc, rc = _solve(eng, monkeypatch, capfd, "comm", p, budget, delta, **kw)
    vl, sl, rl = _solve(eng, monkeypatch, capfd, "lane", p, budget, delta, **kw)
    for rep in rc:
        assert (rep["layout"], rep["comm"], rep["grid"]) == ("lane-resident", "1", str(-(-p.n // 512))), rep
    for rep in rl:
        assert (rep["layout"], rep["comm"], rep["grid"]) == ("lane-resident", "0", str(-(-p.n // 256))), rep
    assert np.array_equal(sc, sl), (sc.view(np.float64), sl.view(np.float64))
    assert np.array_equal(vc, vl), f"{int((vc != vl).sum())} of {vc.size} words of V differ"
    st = sl.view(np.float64)
    assert st[3] == 0.0
    return int(st[1]) - 1


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(r, n):
        if (r, n) not in cache:
            cache[(r, n)] = Problem(r, n)
        return cache[(r, n)]
    return get


@pytest.mark.parametrize("n", [513, 700, 1025])
@pytest.mark.parametrize("r", [33, 50, 52])
def test_same_bits_at_every_stop(eng, problems, monkeypatch, capfd, r, n):
    """Ragged last wave (513, 700) and a ragged 256-column half whose granule still exists (513, 1025): a solve that stops after
    sweep 1 (the speculative sweep 2 dropped), one that stops mid-way, one that runs to its budget."""
    p = problems(r, n)
    assert _both(eng, monkeypatch, capfd, p, 6, 2.0) == 1              # eps >= 2 eps0 fails at once
    mid = _both(eng, monkeypatch, capfd, p, 40, 0.3)
    assert 1 < mid < 40, mid
    assert _both(eng, monkeypatch, capfd, p, 5, 0.0) == 5
    assert _both(eng, monkeypatch, capfd, p, 1, 0.0) == 1


def test_zero_gram_diagonal(eng, problems, monkeypatch, capfd):
    """A zero on the Gram diagonal: every wave runs the guarded row update, the rows stay as they were."""
    p = problems(50, 700)
    q = Problem.__new__(Problem)
    q.__dict__.update(p.__dict__)
    q.G = p.G.copy()
    q.G[0, 0] = q.G[49, 49] = 0.0
    done = _both(eng, monkeypatch, capfd, q, 12, 0.1)
    assert 1 <= done <= 12


@pytest.mark.parametrize("what,val", [("UtM", float("nan")), ("V0", float("inf"))])
def test_non_finite_operand(eng, problems, monkeypatch, capfd, what, val):
    """A NaN in the right-hand side / an Inf in the start values: that wave takes the guarded form, the others the plain one."""
    p = problems(50, 1025)
    q = Problem.__new__(Problem)
    q.__dict__.update(p.__dict__)
    arr = getattr(p, what).copy()
    arr[17, 600] = val
    setattr(q, what, arr)
    vc, sc, _ = _solve(eng, monkeypatch, capfd, "comm", q, 4, 0.0)
    vl, sl, _ = _solve(eng, monkeypatch, capfd, "lane", q, 4, 0.0)
    assert np.array_equal(sc, sl) and np.array_equal(vc, vl)
    assert not np.isfinite(vl.view(np.float32)[:, 600]).all() and np.isfinite(np.delete(vl.view(np.float32), 600, axis=1)).all()


def test_sparsity_constant(eng, problems, monkeypatch, capfd):
    done = _both(eng, monkeypatch, capfd, problems(33, 700), 10, 0.2, sparsity=0.25)
    assert 1 <= done <= 10


def test_cross_form_with_padded_pitches(eng, problems, monkeypatch, capfd):
    """V_in != V_out (the kernel reads its start values itself, no copy) and a different padding on each operand."""
    done = _both(eng, monkeypatch, capfd, problems(52, 1025), 8, 0.0, cross=True, pads=(3, 5, 7))
    assert done == 8


def test_chained_launch(eng, problems, monkeypatch, capfd):
    """sweep0 > 0: launches of 2 sweeps each; the second and third take eps0 and the count over from the status block."""
    p = problems(50, 513)
    assert _both(eng, monkeypatch, capfd, p, 5, 0.0, chain=2) == 5
    mid = _both(eng, monkeypatch, capfd, p, 40, 0.3, chain=2)
    assert 1 < mid < 40, mid
    assert mid == _both(eng, monkeypatch, capfd, p, 40, 0.3)


def test_unforced_just_past_the_threshold(eng, monkeypatch, capfd):
    """Rank 50, one column more than 256 per CU, 3 sweeps, nothing forced: the plan takes the new form, and the result is the
    forced lane kernel's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 256 * cus + 1
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(300, 50, device=dev, generator=g)
    G = (A.t() @ A).contiguous()
    UtM = (G @ torch.rand(50, n, device=dev, generator=g)).contiguous()
    V0 = torch.rand(50, n, device=dev, generator=g)
    monkeypatch.setenv("NNF_HALS_DEBUG", "1")
    out = {}
    for force in (None, "lane"):
        if force:
            monkeypatch.setenv("NNF_HALS_FORCE", force)
        else:
            monkeypatch.delenv("NNF_HALS_FORCE", raising=False)
        V = V0.clone()
        st = torch.zeros(8, dtype=torch.float64, device=dev)
        capfd.readouterr()
        eng.hals_solve(UtM, G, V, 3, delta=0.0, status=st)
        torch.cuda.synchronize()
        rep = [parse_report(ln) for ln in capfd.readouterr().err.splitlines() if ln.startswith("[nnf hals]")][-1]
        want = ("1", str(-(-n // 512)), "1") if force is None else ("0", str(cus + 1), "2")
        assert (rep["layout"], rep["comm"], rep["grid"], rep["per_cu"]) == ("lane-resident",) + want, rep
        out[force] = (V, st[:ST].clone())
    assert torch.equal(out[None][1].view(torch.int64), out["lane"][1].view(torch.int64)), (out[None][1], out["lane"][1])
    assert int(out["lane"][1][1]) == 4 and float(out["lane"][1][3]) == 0.0
    assert torch.equal(out[None][0].view(torch.int32), out["lane"][0].view(torch.int32))
