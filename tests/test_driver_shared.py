"""What the drivers share below the outer loop, on the CPU: the wall-clock sweep rule under a scripted clock, the MU update of
one tensor mode on a recording engine, the words of the status blocks.  No device, no library."""
import math

import pytest
import torch

from engine_double import OracleEngine
from nn_fac_amd import _outer_loop as loop
from nn_fac_amd import _status, _tensor_state, dist, ntd, ntf
from nn_fac_amd.update_rules import nnls

CPU = torch.device("cpu")
# a probe "lasting 0.1": 0.6 / 0.1 is 5.999999999999999 in binary floating point (budget 3), 0.6 / (0.6 / 6) is 6.0
PROBE = 0.6 / 6


def scripted(monkeypatch, readings):
    """nnls.clock answers `readings` in order; returns the list, so that a test sees how many were taken."""
    left = list(readings)
    monkeypatch.setattr(nnls, "clock", lambda: left.pop(0))
    return left


def counting_probe():
    calls = []
    return calls, lambda: calls.append(1)


# ---- the timed rule ----
def test_timed_rule_divides_the_products_time_by_the_probes(monkeypatch):
    left = scripted(monkeypatch, [0.0, PROBE])
    calls, probe = counting_probe()
    budget, rho = nnls.timed_budget(100, 0.5, 0.6, probe, CPU)
    assert (budget, rho, len(calls), left) == (4, 6, 1, [])      # cnt <= 1 + 0.5 * 6, two readings around one probe


def test_a_probe_of_no_duration_counts_as_a_microsecond(monkeypatch):
    left = scripted(monkeypatch, [3.0, 3.0])
    calls, probe = counting_probe()
    budget, rho = nnls.timed_budget(100, 0.5, 0.6, probe, CPU)
    assert rho == 0.6 / 10e-7 and budget == 100 and len(calls) == 1 and left == []


@pytest.mark.parametrize("alpha,atime", [(math.inf, 0.6), (0.5, None), (0.5, 0.0), (math.inf, None)])
def test_without_a_finite_alpha_and_a_time_nothing_is_probed(monkeypatch, alpha, atime):
    left = scripted(monkeypatch, [])                             # (a reading would raise)
    calls, probe = counting_probe()
    budget, rho = nnls.timed_budget(37, alpha, atime, probe, CPU)
    assert (budget, rho, calls, left) == (37, 100000, [], [])


def test_no_sweeps_allowed_is_a_budget_of_zero(monkeypatch):
    scripted(monkeypatch, [0.0, PROBE])
    assert nnls.timed_budget(0, 0.5, 0.6, lambda: None, CPU)[0] == 0
    assert nnls.timed_budget(0, math.inf, None, lambda: None, CPU)[0] == 0
    scripted(monkeypatch, [0.0, 1.0])                            # rho = 0.6: 1 + 0.3 -> one sweep
    assert nnls.timed_budget(100, 0.5, 0.6, lambda: None, CPU)[0] == 1


def test_the_bracket_reads_nothing_with_an_infinite_alpha(monkeypatch):
    left = scripted(monkeypatch, [1.0, 1.75])
    assert nnls.tic(CPU, math.inf) is None and nnls.toc(CPU, None) is None and left == [1.0, 1.75]
    t0 = nnls.tic(CPU, 0.5)
    assert nnls.toc(CPU, t0) == 0.75 and left == []


def test_ntf_step_runs_the_timed_rule_on_the_cpu_engine(monkeypatch):
    """alpha = 0.5 on a CPU tensor: every mode's products "take" 0.6, its probe 0.1 -- rho = 6, budget 4; with delta = 0 every
    solve runs to it, and the kernels count like the reference (sweeps + 1)."""
    left = scripted(monkeypatch, [0.0, 0.6, 0.0, PROBE] * 3)
    g = torch.Generator().manual_seed(3)
    T = torch.rand(5, 6, 7, dtype=torch.float64, generator=g)
    Ft = [torch.rand(3, d, dtype=torch.float64, generator=g) for d in T.shape]
    st = ntf._NtfState(OracleEngine(), T)
    new, nstat = ntf._one_ntf_step_dev(st, 3, Ft, "hals", 2, [None] * 3, [], [False] * 3, 0.5, 0.0)
    assert nstat == 3 and left == []
    assert [int(st.solve_words(i)[1]) for i in range(3)] == [5, 5, 5]
    assert all(torch.isfinite(f).all() and (f >= 0).all() and f.shape == f0.shape for f, f0 in zip(new, Ft))
    assert math.isfinite(float(st.block[st.cost_at])) and float(st.block[st.cost_at]) > 0


# ---- the MU update of one mode ----
class RecordingEngine:
    MU_MODE_MAX_RANK = 64

    def __init__(self):
        self.calls = []

    def dot(self, A, B):
        return torch.sum(A * B).reshape(1).double()

    def mu_right(self, X, V, F, beta):
        self.calls.append(("mu_right", X, V, F, beta))
        return "right"

    def mu_mode(self, T3, F, V, beta):
        self.calls.append(("mu_mode", T3, F, V, beta))
        return "mode"


SHAPE, R = (3, 4, 5, 6), 2


def mode_updates(state_cls, r=R, passes=1):
    eng = RecordingEngine()
    st = state_cls(eng, torch.rand(SHAPE))
    made = []
    unfolded = st.unfolded_t
    st.unfolded_t = lambda mode: made.append(mode) or unfolded(mode)       # (called as st.unfolded_t(mode): what the spies need)
    F = [torch.rand(r, d) for d in SHAPE]
    V = [torch.rand(r, math.prod(SHAPE) // d) for d in SHAPE]
    out = [_tensor_state.mu_mode_update(st, mode, F[mode], V[mode], 1.5) for _ in range(passes) for mode in range(4)]
    return st, eng, F, V, out, made


@pytest.mark.parametrize("state_cls", [ntf._NtfState, ntd._NtdState])
def test_mode_update_on_the_tensors_own_layout(monkeypatch, state_cls):
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    st, eng, F, V, out, made = mode_updates(state_cls)
    assert out == ["mode", "mode", "mode", "right"] and made == []
    for mode, (name, T3, Fm, Vm, beta) in enumerate(eng.calls[:3]):
        assert name == "mu_mode" and tuple(T3.shape) == [(1, 3, 120), (3, 4, 30), (12, 5, 6)][mode]
        assert T3.data_ptr() == st.T.data_ptr() and Fm is F[mode] and Vm is V[mode] and beta == 1.5
    name, X, Vm, Fm, beta = eng.calls[3]                         # the last mode: its transposed unfolding is a view of T
    assert name == "mu_right" and tuple(X.shape) == (60, 6) and X.data_ptr() == st.T.data_ptr() and X.is_contiguous()
    assert Vm is V[3] and Fm is F[3] and beta == 1.5


@pytest.mark.parametrize("state_cls", [ntf._NtfState, ntd._NtdState])
@pytest.mark.parametrize("route", ["NNF_MU_UNFOLD=1", "rank above MU_MODE_MAX_RANK"])
def test_mode_update_on_materialised_unfoldings(monkeypatch, state_cls, route):
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    r = R
    if route == "NNF_MU_UNFOLD=1":
        monkeypatch.setenv("NNF_MU_UNFOLD", "1")                 # (read at call time: the state exists already below)
    else:
        r = RecordingEngine.MU_MODE_MAX_RANK + 1
    st, eng, F, V, out, made = mode_updates(state_cls, r=r, passes=2)
    assert out == ["right"] * 8 and made == [0, 1, 2, 0, 1, 2]
    for i, (name, X, Vm, Fm, beta) in enumerate(eng.calls):
        mode = i % 4
        assert name == "mu_right" and tuple(X.shape) == (math.prod(SHAPE) // SHAPE[mode], SHAPE[mode]) and X.is_contiguous()
        assert torch.equal(X, torch.movedim(st.T, mode, -1).reshape(-1, SHAPE[mode]))
        assert Vm is V[mode] and Fm is F[mode]
        assert (X.data_ptr() == st.T.data_ptr()) == (mode == 3)
        assert X.data_ptr() == eng.calls[mode][1].data_ptr()     # materialised once per mode over the two passes


# ---- the status blocks ----
def test_solve_words_alias_the_selected_block():
    ring = loop.StatusRing()
    ring.init_ring(3, _status.NMF_WORDS, CPU)
    ring.select(2)
    for i in range(2):
        words = ring.solve_words(i)
        assert words.shape == (8,) and words.data_ptr() == ring.blocks[2, 8 * i:].data_ptr()
        _status.write_status(words, 0.25 + i, 7 + i, 1.5)
    assert ring.blocks[2].tolist() == [0.25, 7.0, 1.5, 0.0] + [0.0] * 4 + [1.25, 8.0, 1.5, 0.0] + [0.0] * 12
    assert not ring.blocks[:2].any()
    ring.solve_words(1)[3] = 9.0                                 # a stale error word is overwritten
    _status.write_status(ring.solve_words(1), 0.5, 3, 2.0)
    assert ring.block[8:12].tolist() == [0.5, 3.0, 2.0, 0.0] and loop.sweep_counts(ring.block, 2) == [6, 2]


def test_agreed_code_reads_the_summed_error_words():
    host = torch.zeros(_status.NMF_WORDS, dtype=torch.float64)
    assert [dist.agreed_code(host, i, 2) for i in range(2)] == [0, 0]
    host[_status.NMF_ERRS], host[_status.NMF_ERRS + 1] = 6.0, 1.0      # both ranks: code 3 / one of the two timed out
    assert [dist.agreed_code(host, i, 2) for i in range(2)] == [3, 1]
    host[_status.NMF_ERRS + 1] = 5.0                                   # codes 2 and 3: mixed
    assert dist.agreed_code(host, 1, 2) == 1
    with pytest.raises(loop._GuessMissed):
        loop.check_status(host, 1, nranks=2)


def test_an_unsharded_group_leaves_the_block_alone():
    block = torch.arange(float(_status.NMF_WORDS), dtype=torch.float64)
    before = block.clone()
    assert dist.allreduce_cost_(block, None) is block and dist.allreduce_errs_(block, None) is block
    assert torch.equal(block, before)


def test_the_stopping_decisions_state_starts_disengaged():
    st = loop.AsyncStop()
    assert (st.async_sharded, st.async_ready, st.sync_next, st.last_step_async, st.last_count) == (None, False, False, False, None)
    assert (st.async_hits, st.async_misses) == (0, 0)
    guess = dist.SweepGuess()
    st.note_sweep_count(guess, 30, False)
    st.note_sweep_count(guess, 33, True)
    assert (st.async_ready, st.async_hits, guess.value) == (True, 1, 37)
