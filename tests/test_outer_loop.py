"""nn_fac_amd._outer_loop on fake steps: no engine, no device -- the host logic the NMF, NTF and NTD drivers share."""
import types

import pytest
import torch

from nn_fac_amd import _outer_loop as loop
from nn_fac_amd.utils import errors as err


class _Stream:
    def __init__(self):
        self.syncs = 0

    def synchronize(self):
        self.syncs += 1


def _run(n_iter, retired, depth=1, unreliable_at=None, tol=None):
    """Iteration i "computes" the result ("it", i) at cost 1 / (i + 1); while `ident`, iteration `unreliable_at` comes back with
    the identity cost's not-reliable word set.  Returns (result, enqueued iterations, in flight at each retirement, stream)."""
    enqueued, in_flight, stream = [], [], _Stream()
    state = types.SimpleNamespace(ident=unreliable_at is not None)
    guard = loop.IdentityGuard(tol)

    def enqueue(iteration, previous):
        assert previous == ("it", iteration - 1)
        enqueued.append(iteration)
        return loop.Step(iteration, iteration % 3, ("it", iteration), 0, ident=state.ident)

    def settle(step):
        if step.ident:
            guard.check(1.0 if step.it == unreliable_at else 0.0, 1.0 / (step.it + 1), 1e-6)
        in_flight.append(len(pipe.pending) - 1)
        return 1.0 / (step.it + 1), []

    def leave_identity(result):
        state.ident = False
        guard.switch(retired, lambda: ("direct", result))

    pipe = loop.Pipeline(enqueue, settle, retired, [stream], depth=depth)
    pipe.redo = {loop._IdentityUnreliable: leave_identity}
    return pipe.run(n_iter, ("it", -1)), enqueued, in_flight, stream


@pytest.mark.parametrize("depth", [1, 2])
def test_every_iteration_is_retired_once_and_in_order(depth):
    seen = []
    result, enqueued, in_flight, stream = _run(6, lambda it, cost, sweeps: seen.append((it, cost)), depth=depth)
    assert seen == [(i, 1.0 / (i + 1)) for i in range(6)] and enqueued == list(range(6))
    assert result == ("it", 5) and stream.syncs == 0
    assert in_flight[:6 - depth] == [depth] * (6 - depth)        # the host looks `depth` iterations behind the device ...
    assert in_flight[6 - depth:] == list(range(depth - 1, -1, -1))   # ... until the last one has been enqueued


def test_an_unreliable_identity_cost_redoes_that_iteration_once():
    seen, revised = [], []

    def retired(it, cost, sweeps):
        seen.append(it)
    retired.revise_last = revised.append
    result, enqueued, _, stream = _run(6, retired, unreliable_at=3)
    assert seen == list(range(6)) and result == ("it", 5)
    assert enqueued == [0, 1, 2, 3, 4, 3, 4, 5]                 # iteration 4 was in flight behind 3: dropped, both run again
    assert revised == [("direct", ("it", 2))]                   # the last retired iterate, costed again, exactly once
    assert stream.syncs == 1                                    # what was dropped has been waited for


def test_a_near_stop_identity_cost_is_a_redo_too():
    seen = []
    _, enqueued, _, _ = _run(4, lambda it, cost, sweeps: seen.append(it), unreliable_at=-1, tol=0.2)
    assert seen == list(range(4))                               # |1/2 - 1/3| < tol + estimates at iteration 2 ...
    assert enqueued == [0, 1, 2, 3, 2, 3]                       # ... (a plain callable: nothing to revise, the loop goes on)


def test_a_stop_returns_that_iteration_and_drops_the_one_behind_it():
    seen = []

    def retired(it, cost, sweeps):
        seen.append(it)
        return it == 2
    result, enqueued, in_flight, stream = _run(10, retired)
    assert result == ("it", 2) and seen == [0, 1, 2]
    assert enqueued == [0, 1, 2, 3] and in_flight[-1] == 1 and stream.syncs == 1


def test_a_redo_without_a_handler_is_not_swallowed():
    def settle(step):
        raise loop._GuessMissed()
    pipe = loop.Pipeline(lambda it, prev: loop.Step(it, 0, it, 0), settle, lambda *a: False)
    with pytest.raises(loop._GuessMissed):
        pipe.run(3, None)


def test_status_words():
    host = torch.zeros(24, dtype=torch.float64)
    loop.check_status(host, 2)
    host[8 + 1], host[1] = 5.0, 3.0
    assert loop.sweep_counts(host, 2) == [2, 4]
    for code, fall_back, exc in [(1, True, loop._SolveTimedOut), (1, False, err.EngineError), (7, False, err.EngineError),
                                 (2, True, err.ZeroColumnWhenUnautorized), (3, False, loop._GuessMissed),
                                 (4, True, loop._GuessMissed)]:
        host[8 + 3] = code
        loop.check_status(host, 1)                              # (the second solve's word is not looked at)
        with pytest.raises(exc):
            loop.check_status(host, 2, can_fall_back=fall_back)
    host[8 + 3] = 0.0
    host[17], host[18] = 0.0, 1.0                               # row-sharded: one of two ranks timed out in the second solve
    with pytest.raises(loop._SolveTimedOut):
        loop.check_status(host, 2, nranks=2, can_fall_back=True)
    host[18] = 6.0                                              # both ranks: the guess missed
    with pytest.raises(loop._GuessMissed):
        loop.check_status(host, 2, nranks=2)


def test_retired_prints_and_stops_like_the_reference(capsys):
    log = []
    retired = loop.Retired(1e-3, verbose=True, sweep_log=log, switch_message='(switched; {} -> {})')
    assert [retired(0, 4.0, [3, 2]), retired(1, 5.0, [1]), retired(2, 3.0, [])] == [False, False, False]
    retired.revise_last(3.0005)
    assert retired(3, 3.0, []) is True
    assert retired.cost_fct_vals == [4.0, 5.0, 3.0005, 3.0] and log == [3, 2, 1] and len(retired.toc) == 4
    assert capsys.readouterr().out == (
        "Normalized cost function value=4.0\n"
        "\033[91mNormalized cost function value=5.0, variation=-1.0.\033[0m\n"
        "Normalized cost function value=3.0, variation=2.0.\n"
        "(switched; 3.0 -> 3.0005)\n"
        "Normalized cost function value=3.0, variation=" + str(3.0005 - 3.0) + ".\n"
        "Converged in 3 iterations.\n")
    quiet = loop.Retired(1e-3)
    quiet(0, 1.0, [])
    quiet.revise_last(2.0)
    assert quiet.cost_fct_vals == [2.0] and capsys.readouterr().out == ""


def test_sweep_count_bookkeeping():
    st = types.SimpleNamespace(async_ready=False, last_count=None, async_hits=0)
    guess = types.SimpleNamespace(value=16, max_chunk=40)
    for count, hit, ready, hits, value in [(33, False, False, 0, 16), (52, False, False, 0, 16), (50, False, True, 0, 16),
                                           (46, True, True, 1, 40), (3, True, False, 2, 8), (7, True, True, 3, 11)]:
        loop.note_sweep_count(st, guess, count, hit)
        assert (st.async_ready, st.async_hits, guess.value) == (ready, hits, value)
