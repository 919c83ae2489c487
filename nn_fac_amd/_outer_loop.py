"""The outer loop the NMF, NTF and NTD drivers share: the device runs ahead, the host looks at finished iterations in order.

Every driver enqueues one iteration after the other; each leaves a status block (the solves' status words, the cost) that
reaches the host through an asynchronous copy and an event.  What the host does with such a block -- when it looks, what a
"redo" word in it leads to, what it prints, when it stops -- is written here once:

    StatusRing          the ring of status blocks with their host mirrors (the words of a block: _status.py)
    check_status        status words -> nothing / a redo exception / the user-facing exception
    Retired             the host side of a finished iteration (costs, times, printing, stopping test: the reference's)
    Pipeline            pending queue, in-order retirement, flush, stop, rewind to a failed iteration
    IdentityGuard       when a cost taken from the Gram identity cannot be trusted
    AsyncStop           row-sharded runs: when the device-side stopping decision is engaged, where its next guess sits

The drivers supply what is theirs: how a step is enqueued, where cost and sweep counts sit in a block, and what each redo
exception changes in their own switches.  Nothing here asks which driver it serves.
"""
import dataclasses
import time

import torch

from .utils import errors as err
from . import engine as _engine
from . import dist as _dist


class StatusRing:
    """`nslots` status blocks of `width` float64 on the device and their host mirrors (pinned next to a GPU, so that the copy
    of a block is asynchronous): a step writes the block it `select`ed while the host still reads an earlier one."""

    def init_ring(self, nslots, width, device):
        self.blocks = torch.zeros((nslots, width), dtype=torch.float64, device=device)
        self.host = torch.zeros((nslots, width), dtype=torch.float64)
        if self.blocks.is_cuda:
            self.host = self.host.pin_memory()
        self.select(0)

    def select(self, slot):
        self.slot = slot
        self.block = self.blocks[slot]

    def solve_words(self, i):
        """The 8 status words of solve `i` of the selected block (a view)."""
        return self.block[_engine.ST_WORDS * i:_engine.ST_WORDS * (i + 1)]


class _SolveTimedOut(Exception):
    """A persistent HALS solve gave up waiting for its other workgroups (status word 1)."""


class _IdentityUnreliable(Exception):
    """HALS cost through the Gram identity (nnf_nmf_gram_cost_f32): the kernel's own error estimate is above 5e-4 of the
    cost -- the residual is too small next to ||X||^2 for fp32 cross terms (an almost exact fit).  The iteration is redone
    with the streaming cost kernel, and so is the rest of the run."""


class _IdentityNearStop(_IdentityUnreliable):
    """Two consecutive identity costs differ by the caller's `tol` give or take their error estimates: the stopping test
    needs better."""


class _GuessMissed(Exception):
    """Row-sharded run: the blind chunk of the device-side protocol did not contain the stopping sweep in its snapshot window
    (status words 3 / 4 of nnf_hals_stop_restore_f32): the iteration is redone with the host-synchronous protocol."""


def check_status(host, nstat, nranks=0, can_fall_back=False):
    """Decode the error words of the `nstat` solves of one iteration (`host`: its status block, 8 words per solve).
    Code 2 is only written by a solve run with nonzero=True, codes 3 / 4 only by nnf_hals_stop_restore_f32 (the device-side
    protocol of a row-sharded solve); any other non-zero word is a persistent solve that gave up waiting for its workgroups:
    a redo (`can_fall_back`: the caller has chunked launches to fall back to) or the end of the run.
    `nranks` > 0: a row-sharded run -- the error words are read from the copies that travelled with the cost's all-reduce
    (dist.allreduce_cost_), so every rank sees the same code for the same iteration and takes the same branch: a time-out
    is a rank-local event (the replicated V-side solve of ONE rank found the chip shared), and a rank that fell back to
    chunked solves alone would issue a different sequence of collectives than its peers (a hang over RCCL)."""
    for i in range(nstat):
        code = _dist.agreed_code(host, i, nranks) if nranks else int(host[_engine.ST_WORDS * i + _engine.ST_ERR])
        if code == 2:
            raise err.ZeroColumnWhenUnautorized("A column of U is zero with nonzero condition")
        if code in (_dist.ERR_BEFORE_WINDOW, _dist.ERR_NOT_STOPPED):
            raise _GuessMissed()
        if code != 0:
            if can_fall_back:
                raise _SolveTimedOut()
            raise err.EngineError("hals grid barrier timed out; result invalid")


def sweep_counts(host, nstat):
    """Inner sweeps of each of the `nstat` solves of a status block (the kernels count like the reference: sweeps + 1)."""
    return [int(host[_engine.ST_WORDS * i + _engine.ST_CNT]) - 1 for i in range(nstat)]


class Retired:
    """Host side of one finished iteration, the same lines in the three reference loops (nmf.py:315-324, ntf.py:325-340,
    ntd.py:410-428): called with (iteration, cost, sweeps) in order, True = the stopping test fired.  `switch_message`: what
    a verbose run prints when the loop re-evaluates the last cost another way (`revise_last`), formatted with the old and
    the new value."""

    def __init__(self, tol, verbose=False, sweep_log=None, switch_message=None):
        self.tol, self.verbose, self.sweep_log, self.switch_message = tol, verbose, sweep_log, switch_message
        self.cost_fct_vals, self.toc = [], []
        self.tic = time.time()

    def __call__(self, iteration, cost, sweeps):
        cost_fct_vals = self.cost_fct_vals
        if self.sweep_log is not None:
            self.sweep_log.extend(sweeps)
        self.toc.append(time.time() - self.tic)
        cost_fct_vals.append(cost)

        if self.verbose:
            if iteration == 0:
                print('Normalized cost function value={}'.format(cost))
            else:
                if cost_fct_vals[-2] - cost_fct_vals[-1] > 0:
                    print('Normalized cost function value={}, variation={}.'.format(
                        cost_fct_vals[-1], cost_fct_vals[-2] - cost_fct_vals[-1]))
                else:
                    print('\033[91m' + 'Normalized cost function value={}, variation={}.'.format(
                        cost_fct_vals[-1], cost_fct_vals[-2] - cost_fct_vals[-1]) + '\033[0m')

        if iteration > 0 and abs(cost_fct_vals[-2] - cost_fct_vals[-1]) < self.tol:
            if self.verbose:
                print('Converged in {} iterations.'.format(iteration))
            return True
        return False

    def revise_last(self, cost):
        # the loop switched from the Gram-identity cost to the streaming kernel: the last value is re-evaluated the same way,
        # so that the variation printed next -- and the stopping test -- compare two costs of one kind
        if self.verbose and self.switch_message is not None:
            print(self.switch_message.format(self.cost_fct_vals[-1], cost))
        self.cost_fct_vals[-1] = cost


@dataclasses.dataclass
class Step:
    """One enqueued iteration: its number, its slot of the status ring, what it computed (fresh tensors: a dropped step costs
    nothing), its number of solves, the event after the copy of its block (None: the block is already on the host -- or its
    cost has not been launched yet) and what the driver's `settle` wants to know about how it ran."""
    it: int
    slot: int
    result: object
    nstat: int
    event: object = None
    ident: bool = False          # its cost came from the Gram identity
    async_solve: bool = False    # its row-sharded solve took the device-side stopping decision


class Pipeline:
    """Steps are enqueued one after the other and retired in order once more than `depth` are in flight, all of them after
    the last one has been enqueued.

    enqueue(iteration, previous result) -> Step      launches the iteration and the copy of its block
    settle(step) -> (cost, sweeps)                   reads the step's block on the host; raises a redo exception (the step
                                                     stays at the head of the queue) or the user's
    retired(iteration, cost, sweeps) -> bool         any callable, called once per iteration, in order; True stops the loop:
                                                     the result of that iteration is returned, the speculative steps behind
                                                     it are dropped -- and waited for, they still use shared scratch
    streams                                          every stream the steps run on (what "waited for" synchronises)
    before_flush()                                   called after the last step has been enqueued, before the rest is retired
    redo[exception class] = handler(last retired result)
                                                     everything in flight is waited for and dropped, the handler flips the
                                                     driver's switches (it may change `depth`), and the loop goes on from the
                                                     failed iteration and the last retired result
    """

    def __init__(self, enqueue, settle, retired, streams=(), depth=1, before_flush=None):
        self.enqueue, self.settle, self.retired, self.streams = enqueue, settle, retired, streams
        self.depth, self.before_flush = depth, before_flush
        self.redo = {}
        self.pending = []

    def drain(self):
        for stream in self.streams:
            stream.synchronize()

    def _retire(self):
        step = self.pending[0]
        if step.event is not None:
            step.event.synchronize()
        cost, sweeps = self.settle(step)
        self.pending.pop(0)                 # (a step that has to be redone stays at the head: `run` resumes from it)
        self.result = step.result
        return bool(self.retired(step.it, cost, sweeps))

    def run(self, n_iter, start):
        self.result = current = start
        pending, stop, iteration = self.pending, False, 0
        while iteration < n_iter and not stop:
            current = self.enqueue(iteration, current)
            pending.append(current)
            current = current.result
            iteration += 1
            try:
                if len(pending) > self.depth:
                    stop = self._retire()
                if iteration == n_iter and not stop:
                    if self.before_flush is not None:
                        self.before_flush()
                    while pending and not stop:
                        stop = self._retire()
            except tuple(self.redo) as redo:
                failed = pending[0].it            # the step being retired is still at the head of the queue
                self.drain()
                pending.clear()
                next(h for c, h in self.redo.items() if isinstance(redo, c))(self.result)
                current = self.result             # what the last iteration that retired cleanly computed
                iteration = failed
        if pending:                               # dropped speculative iterations still use the shared scratch
            self.drain()
            pending.clear()
        return self.result


class IdentityGuard:
    """A cost taken from the Gram identity (Engine.gram_cost) is accepted while the kernel calls it reliable and -- `tol`
    given: the caller stops on |cost[i-1] - cost[i]| < tol -- while that difference is further from `tol` than the two error
    estimates together.  `check` takes costs and estimates as the stopping test sees them (normalised where the driver
    normalises)."""

    def __init__(self, tol):
        self.tol = tol
        self.last = None      # (cost, error estimate) of the last retired iterate while both came from the identity

    def check(self, unreliable, cost, estimate):
        if unreliable != 0.0:
            raise _IdentityUnreliable()
        last = self.last
        if self.tol is not None and self.tol > 0 and last is not None and abs(last[0] - cost) < self.tol + estimate + last[1]:
            raise _IdentityNearStop()
        self.last = (cost, estimate)

    def switch(self, retired, direct_cost_of_last):
        """The run leaves the identity.  Whichever test failed: the iterate before it was costed by the identity -- it is
        re-evaluated too (`direct_cost_of_last()`) and handed to `retired.revise_last`, so that the stopping test never
        compares a cost of one kind with a cost of the other."""
        if self.last is not None and hasattr(retired, "revise_last"):
            retired.revise_last(direct_cost_of_last())
        self.last = None


class AsyncStop:
    """Row-sharded runs: the state of the device-side stopping decision of the sharded solve (dist.sharded_hals_solve_async).
    `async_sharded`: the run may take it (dist.opt_in; None = not decided yet); `async_ready`: it is engaged (below);
    `sync_next`: the next step uses the host-synchronous protocol (after a redo); `last_step_async`: the last step took it."""

    def __init__(self, async_sharded=None):
        self.async_sharded = async_sharded
        self.async_ready = self.sync_next = self.last_step_async = False
        self.last_count = None
        self.async_hits = self.async_misses = 0

    def note_sweep_count(self, guess, count, hit):
        """After a retired iteration whose sharded solve took `count` sweeps.  A missed guess costs a pipeline drain + a redone
        iteration, and the sweep counts of the first outer iterations jump by tens (33, 52, 67, 38, ... at NMF config B), so the
        decision is engaged only once two consecutive solves differ by <= 4 sweeps (`async_ready`).  `hit`: this solve took it,
        and its guess held -- the next blind chunk is centred on this count."""
        self.async_ready = self.last_count is not None and abs(count - self.last_count) <= 4
        self.last_count = count
        if hit:
            self.async_hits += 1
            guess.value = max(8, min(count + 4, guess.max_chunk))


note_sweep_count = AsyncStop.note_sweep_count      # (state, guess, count, hit): on any object with those fields
