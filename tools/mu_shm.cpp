// Prints the dynamic LDS the launchers of the fused MU kernels ask for at ranks 65 .. 128, one line per (MT, form):
//   "<MT> <REM> <KL|GEN> <bytes>"   (r = 16 MT + REM, the largest rank of the split; both kernels use the same arithmetic).
// Build: c++ -std=c++17 -I nn_fac_amd/csrc tools/mu_shm.cpp -o mu_shm   (tools/mu_rank128_budget.py does it)
#include <stdio.h>
#include "k_mu_plan.h"

int main() {
    for (int MT = 5; MT <= 8; ++MT)
        for (int gen = 0; gen < 2; ++gen)
            printf("%d 0 %s %zu\n", MT, gen ? "GEN" : "KL", mu_shm(MT, 0, 16 * MT, mu_frags_in_regs(MT, gen != 0)));
    printf("6 4 KL %zu\n", mu_shm(6, 4, 100, mu_frags_in_regs(6, false)));   // ranks 97 .. 100: leftover ranks on the VALU pipe
    return 0;
}
