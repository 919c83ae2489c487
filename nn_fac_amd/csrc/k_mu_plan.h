// Residency arithmetic of the fused MU kernels that the kernels, their launchers (k_mu.hip) and tools/mu_shm.cpp share.
// No HIP in here: the tool is a plain host program.
#pragma once
#include <stddef.h>

// Where the loop-invariant ("resident") factor fragments of MFMA #1 live: in registers for the KL forms, and for every form
// above rank 64 (MT > 4 rank tiles, where the chunk images alone take 16 KiB of LDS per tile); otherwise (general beta,
// r <= 64) in LDS.
constexpr bool mu_frags_in_regs(int MT, bool general_beta) { return !general_beta || MT > 4; }

// dynamic LDS of one workgroup: two double-buffered chunk images (+ the resident fragments unless in registers)
constexpr size_t mu_shm(int MT, int REM, int r, bool regf) {
    return ((regf ? 0 : (size_t)4 * ((r + 3) / 4) * 64) + (size_t)2 * (2 * MT + (REM > 0 ? 1 : 0)) * 256) * 16;
}
