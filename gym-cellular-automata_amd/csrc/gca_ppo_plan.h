// gca_ppo_plan.h — the launch shape and the workspace layout of gca_helicopter_policy_grad and gca_bulldozer_policy_grad
// as a function of (S, C, Hd, N, NOUT) and of nothing else (NOUT: the network's outputs, 10 for the helicopter's nine
// logits and the value, 12 for the bulldozer's 9 + 2 logits and the value), shared by the device build (gca_ppo.hip)
// and the host build (gca_cpu.cpp), so both answer the workspace queries alike and refuse the same short workspace.
// Plain C++, no device code.
#pragma once
#include <stdint.h>

struct PpoPlan {
    int TS;          // samples per tile: 64, or 32 at Hd = 256 (the tile's hidden vectors stay under 64 KiB of LDS)
    int R;           // gradient rows per workgroup of the weight-gradient kernel: 1024 / Hd
    int nbL, nbC, nbO, nb;  // its row blocks: window cells, coarse rows + b1, the NOUT w_out columns
    int P;           // sample splits (grid.y of the weight-gradient kernel) = partial gradients to reduce
    int64_t ntiles, npad, tps;  // tiles, samples rounded up to whole tiles, tiles per split
    int64_t GF;      // floats of one partial: w_local | w_coarse | b1 | w_out
    int64_t off_wl, off_wc, off_b1, off_wo;  // float offsets inside a partial
    int64_t off_da, off_h, off_do, off_tp, off_part, bytes;  // byte offsets inside the workspace, and its size
};

// [0] the minibatch's advantage mean, [1] its standard deviation; the _vclip entries: [2] U f32, [3] n_U i32, [4] the
// samples outside the value clip i32
constexpr int PPO_HDR_FLOATS = 64;
constexpr int64_t PPO_PART_BYTES_MAX = 256ll << 20;

// floats per tile partial: 5 statistics sums, NOUT b2 gradient sums, rounded up to a multiple of four (16 at NOUT = 10
// with one unused, 20 at NOUT = 12 with three)
constexpr int ppo_tp(int NOUT) { return (5 + NOUT + 3) & ~3; }

static inline int64_t ppo_align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// S*S = SS window cells, C coarse values, Hd hidden units (a power of two in [32, 256]), N >= 1 samples, NOUT outputs
static inline PpoPlan ppo_plan(int SS, int C, int Hd, int64_t N, int NOUT) {
    PpoPlan p;
    p.TS = Hd == 256 ? 32 : 64;
    p.R = 1024 / Hd;
    p.nbL = (SS + p.R - 1) / p.R;
    p.nbC = (C + 1 + p.R - 1) / p.R;
    p.nbO = (NOUT + p.R - 1) / p.R;
    p.nb = p.nbL + p.nbC + p.nbO;
    p.ntiles = (N + p.TS - 1) / p.TS;
    p.npad = p.ntiles * p.TS;
    p.off_wl = 0;
    p.off_wc = (int64_t)SS * 4 * Hd;
    p.off_b1 = p.off_wc + (int64_t)C * Hd;
    p.off_wo = p.off_b1 + Hd;
    p.GF = p.off_wo + (int64_t)Hd * NOUT;
    int64_t P = 1024 / p.nb;
    const int64_t by_mem = PPO_PART_BYTES_MAX / (p.GF * 4);
    if (P > by_mem) P = by_mem;
    if (P > p.ntiles) P = p.ntiles;
    if (P < 1) P = 1;
    p.tps = (p.ntiles + P - 1) / P;
    p.P = (int)((p.ntiles + p.tps - 1) / p.tps);
    p.off_da = ppo_align256(PPO_HDR_FLOATS * 4);
    p.off_h = p.off_da + ppo_align256(p.npad * Hd * 4);
    p.off_do = p.off_h + ppo_align256(p.npad * Hd * 4);
    p.off_tp = p.off_do + ppo_align256(p.npad * NOUT * 4);
    p.off_part = p.off_tp + ppo_align256(p.ntiles * ppo_tp(NOUT) * 4);
    p.bytes = p.off_part + ppo_align256((int64_t)p.P * p.GF * 4);
    return p;
}
