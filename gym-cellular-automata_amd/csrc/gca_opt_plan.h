// gca_opt_plan.h — what gca_adam_step and gca_permutation share between the device build (gca_opt.hip) and the host
// build (gca_cpu.cpp): the chunking of the optimizer's tensors (which fixes the summation order of the gradient norm
// and the workspace size), the layout of the state block, the learning-rate schedule, and the walk of the keyed
// permutation. Plain C++, no device code; GCA_OPT_HD marks what a kernel calls too.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GCA_OPT_HD __device__ __forceinline__
#else
#define GCA_OPT_HD inline
#endif

// ------------------------------------------------------------------ Adam: chunks and state
constexpr int ADAM_THREADS = 256;       // lanes of a chunk's sum
// whole chunks of the concatenated tensors at the most (+ one tail per tensor). At 4.09 M parameters 1024 and 512 were
// within 6 % of this (26.0 and 26.9 us against 27.7 us per step, profiles/helicopter_adam_chunks.json)
constexpr int ADAM_MAX_CHUNKS = 2048;

// state block words (include/gca.h "optimizer"): the live scalars, then the slot the next step's scalars wait in
enum { ADAM_COUNT = 0, ADAM_B1POW = 1, ADAM_B2POW = 2, ADAM_NORM = 3, ADAM_LR = 4, ADAM_PENDING = 8 };

// elements per chunk: a multiple of 1024 that depends on the total length only
static inline int64_t adam_chunk(int64_t total) {
    const int64_t per = (total + (int64_t)ADAM_MAX_CHUNKS * 1024 - 1) / ((int64_t)ADAM_MAX_CHUNKS * 1024);
    return 1024 * (per < 1 ? 1 : per);
}

static inline int64_t adam_workspace_bytes(int64_t total) {
    return 8 * (total / adam_chunk(total) + GCA_ADAM_MAX_TENSORS);
}

// the reference's linear_schedule (agents/jax_ppo.py:677-702) in double, rounded once; the clamp at zero is ours
GCA_OPT_HD float adam_lr(float lr0, int32_t count_before, int64_t steps_per_iteration, int64_t num_iterations) {
    if (steps_per_iteration <= 0) return lr0;
    const double frac = 1.0 - (double)((int64_t)count_before / steps_per_iteration) / (double)num_iterations;
    return (float)((double)lr0 * (frac > 0.0 ? frac : 0.0));
}

// ------------------------------------------------------------------ the keyed permutation
constexpr int PERM_ROUNDS = 4;
constexpr int PERM_WALK_CAP = 1024;

// half width h of the balanced Feistel network on [0, 2^(2h)): the smallest with 2^(2h) >= T, at least 1
static inline int perm_half_bits(int64_t T) {
    int h = 1;
    while (((int64_t)1 << (2 * h)) < T) ++h;
    return h;
}

// out[r][i] for one i: the network is applied until the value falls below T (a bijection of [0, 2^(2h)) walked
// cyclically is a bijection of [0, T)). f(right, round, row_key) is word 0 of the round's Philox block. A walk that
// reaches the cap yields i and sets *capped.
template <class F>
GCA_OPT_HD uint32_t perm_walk(uint32_t i, uint32_t T, int h, uint32_t row_key, const F& f, bool* capped) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = i;
    for (int it = 0; it < PERM_WALK_CAP; ++it) {
        uint32_t L = x >> h, R = x & mask;
        for (uint32_t round = 0; round < (uint32_t)PERM_ROUNDS; ++round) {
            const uint32_t n = L ^ (f(R, round, row_key) & mask);
            L = R;
            R = n;
        }
        x = (L << h) | R;
        if (x < T) return x;
    }
    *capped = true;
    return i;
}
