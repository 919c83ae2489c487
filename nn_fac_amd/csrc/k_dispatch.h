// Host-side helpers that every launcher shares: a run-time count turned into a template argument, and the walk over a rank
// above NNF_MAX_RANK.  No HIP in here: tools/dispatch_check.cpp runs both on the CPU (tests/test_abi_and_host.py).
#pragma once
#include <type_traits>
#include "k_stream_plan.h"

template <int V>
using nnf_int = std::integral_constant<int, V>;

// f(nnf_int<v>) for v = 1 .. N.  Every other value -- 0, negatives, anything above N -- takes N, the widest instantiation (a
// rank-tile count is 1 .. 8 by the time it gets here: ranks above NNF_MAX_RANK are walked in passes, nnf_rank_passes).
// f is a generic lambda; it is instantiated once per value of 1 .. N.
template <int N, int I = 1, class F>
inline auto nnf_dispatch(int v, F&& f) {
    if constexpr (I == N) return f(nnf_int<N>{});
    else return v == I ? f(nnf_int<I>{}) : nnf_dispatch<N, I + 1>(v, f);
}

// A rank above NNF_MAX_RANK whose rank rows are independent of each other: fn(k0, rc) for the passes of rc <= NNF_MAX_RANK rows
// starting at row k0, in order.  Every pass takes the workspace of the one before it (same stream): the cursor is put back to
// where it stood.  Stops at the first pass that fails and returns its status.
template <class F>
inline int nnf_rank_passes(int r, nnf_ws_cursor& cur, F&& fn) {
    for (int k0 = 0; k0 < r; k0 += NNF_MAX_RANK) {
        const size_t mark = cur.off;
        const int rc = fn(k0, r - k0 < NNF_MAX_RANK ? r - k0 : NNF_MAX_RANK);
        cur.off = mark;
        if (rc != NNF_OK) return rc;
    }
    return NNF_OK;
}
