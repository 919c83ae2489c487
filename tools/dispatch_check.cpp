// Host check of nn_fac_amd/csrc/k_dispatch.h (tests/test_abi_and_host.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it): the tile-count dispatcher and the rank-pass walk, on the CPU.
//     c++ -std=c++17 -fsanitize=address,undefined -I nn_fac_amd/csrc tools/dispatch_check.cpp -o dispatch_check && ./dispatch_check
#include <limits.h>
#include <stdio.h>
#include <vector>
#include "k_dispatch.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            ++failures;                                                  \
        }                                                                \
    } while (0)

template <int N>
static void check_dispatch() {
    int hits[N + 1] = {};
    const auto f = [&](auto c) {
        constexpr int I = decltype(c)::value;     // a template argument, as a launcher uses it
        static_assert(I >= 1 && I <= N, "instantiated outside 1 .. N");
        ++hits[I];
        return I;
    };
    for (int v = 1; v <= N; ++v) CHECK(nnf_dispatch<N>(v, f) == v);
    for (int i = 1; i <= N; ++i) CHECK(hits[i] == 1);            // each value reached its own instantiation, once
    // the documented clamp: everything outside 1 .. N takes N
    const int outside[] = {0, N + 1, INT_MAX, -1, INT_MIN};
    for (int v : outside) CHECK(nnf_dispatch<N>(v, f) == N);
    for (int i = 1; i < N; ++i) CHECK(hits[i] == 1);
    CHECK(hits[N] == 1 + (int)(sizeof(outside) / sizeof(outside[0])));
}

struct pass { int k0, rc; };
static void check_rank_passes() {
    char ws[4096];
    for (int r : {1, NNF_MAX_RANK, NNF_MAX_RANK + 1, 2 * NNF_MAX_RANK, 300}) {
        nnf_ws_cursor cur(ws, sizeof ws);
        CHECK(cur.take(100) != nullptr);
        const size_t mark = cur.off;
        std::vector<pass> seen;
        const int rc = nnf_rank_passes(r, cur, [&](int k0, int n) {
            CHECK(cur.off == mark);                  // every pass starts where the one before it started
            CHECK(cur.take(512) != nullptr);
            seen.push_back({k0, n});
            return NNF_OK;
        });
        CHECK(rc == NNF_OK && cur.off == mark);
        int next = 0;
        for (const pass& p : seen) {
            CHECK(p.k0 == next && p.rc >= 1 && p.rc <= NNF_MAX_RANK);
            next += p.rc;
        }
        CHECK(next == r && (int)seen.size() == (r + NNF_MAX_RANK - 1) / NNF_MAX_RANK);
    }
    // the first failing pass ends the walk, its status comes back and the cursor is where it was
    nnf_ws_cursor cur(ws, sizeof ws);
    int calls = 0;
    const int rc = nnf_rank_passes(3 * NNF_MAX_RANK, cur, [&](int, int) {
        (void)cur.take(64);
        return ++calls == 2 ? NNF_ERR_WORKSPACE : NNF_OK;
    });
    CHECK(rc == NNF_ERR_WORKSPACE && calls == 2 && cur.off == 0);
}

int main() {
    check_dispatch<8>();    // rank tiles, k steps of the short Gram
    check_dispatch<4>();    // parts per element of the slab sum
    check_dispatch<1>();
    check_rank_passes();
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
