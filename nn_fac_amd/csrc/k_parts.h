// Range-split translation units.  A kernel family with too many instantiations for one compilation (k_hals_fast.hip: the padded
// ranks; k_hals_quad.hip: the quads per column) is compiled once per part, -D<FAMILY>_PART=p, and a part instantiates its own
// values only.  The family writes ONE table of X(part, value) entries,
//     #define QUAD_TABLE(X) X(0, 1) X(0, 2) ... X(9, 32)
// defines NNF_PART as the part being compiled, and takes everything that has to agree with the table from the table:
//   * NNF_PART_DISPATCHER(name, TABLE), in every part: `int name(int value, int miss, f)` calls f(nnf_int<value>) for this part's
//     values and returns `miss` for every other one;
//   * part 0 runs its own X macros over the same table for the declarations of the parts' functions and for the switches that
//     send a value to the part that holds it (NNF_PART_FN(base, p) is that part's function).
// The Makefile names the parts once more (<FAMILY>_PARTS): one it lacks fails to link, one the table lacks fails to compile.
#pragma once
#include "k_dispatch.h"

// f is a generic lambda: its body is instantiated for the values it is called with, so other parts' entries cost nothing here
template <bool MINE, int V, class F>
inline int nnf_part_call(F&& f, int miss) {
    if constexpr (MINE) return f(nnf_int<V>{});
    else return miss;
}

#define NNF_PART_FN(base, p) base##p
#define NNF_PART_CASE(p, v) case v: return nnf_part_call<(p) == (NNF_PART), v>(f, miss);
#define NNF_PART_MINE(p, v) +((p) == (NNF_PART) ? 1 : 0)
#define NNF_PART_DISPATCHER(name, TABLE)                                                       \
    template <class F>                                                                         \
    static int name(int value, int miss, F&& f) {                                              \
        static_assert((0 TABLE(NNF_PART_MINE)) > 0, "the table gives this part no value");     \
        switch (value) { TABLE(NNF_PART_CASE) default: return miss; }                          \
    }
