"""Where things sit in the float64 status blocks the drivers read back, named once.  (A leaf module: dist.py, engine.py and
_outer_loop.py all use it, and _outer_loop.py imports the other two.)

Every block opens with 8 words per HALS solve, {eps, cnt, eps0, error code, 4 spare} (engine.ST_*; StatusRing.solve_words).
The NMF step's block (two solves) goes on with the words below; NTF and NTD name theirs on their states (cost_at, pg_at).
"""
import torch

NMF_COST = 16                 # the iteration's cost from the pass over X (streaming kernel / beta-divergence)
# row-sharded: copies of the two solves' error words summed over the ranks, two words right behind the cost, so that one
# all-reduce carries the three (dist.allreduce_cost_)
NMF_ERRS = 17
NMF_IDENT_COST, NMF_IDENT_VERDICT, NMF_IDENT_ESTIMATE = 19, 20, 21     # Engine.gram_cost: {cost, 1 = not reliable, estimate}
NMF_WORDS = 24


def write_status(words, eps, cnt, eps0):
    """A solve whose (eps, cnt, eps0) the host already knows (the chunked protocols of dist.py) into its status words, error
    word 0: one host-to-device copy."""
    words[:4] = torch.tensor([eps, cnt, eps0, 0.0], dtype=torch.float64)
