// gca_policy_obs_dev.h — the rows form of the policy observation's coarse map (gca_policy_obs.hip) as a device function
// of one wave, shared by policy_obs_rows_kernel and the bulldozer policy rollout kernel (gca_windy.hip), which keeps the
// env's coarse map in LDS and recounts it with the same instructions: one copy of the SWAR equality and the DPP sums.
#pragma once
#include "gca_common.h"

constexpr int POBS_STRIP = 32;  // rows of one wave of the rows form: the largest block, so a strip is whole block-rows
constexpr int POBS_RD = 8;      // rows per group of loads (the smallest block: every block-row is whole groups)

template <int NW>
struct ObsRow {
    uint32_t w[NW];
};

// S: the env's wave-uniform base, lofs: the lane's column offset, R wave-uniform and inside the grid (the caller's loop
// bounds): one global_load_dword / dwordx2 with a scalar base
template <int NW>
__device__ __forceinline__ ObsRow<NW> load_obsrow(const uint8_t* __restrict__ S, uint32_t lofs, int R) {
    constexpr int W = 256 * NW;
    const uint8_t* p = S + (uint32_t)R * (uint32_t)W + lofs;
    ObsRow<NW> x;
    if (NW == 1) {
        x.w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        x.w[0] = v.x; x.w[1 % NW] = v.y;
    }
    return x;
}

template <int CTRL>
__device__ __forceinline__ uint32_t obs_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// A wave takes strip `strip` of POBS_STRIP rows of one env's plane S = 32 / B block-rows (H % B == 0, so every block-row
// is whole and inside the grid; all 64 lanes active). Per block-row: TREE and FIRE flags as 0x01 bytes by SWAR equality
// (bytes_eq01), added per byte over its B rows (<= 32 per byte); then the lane's bytes summed by v_sad_u8 against 0, TREE
// in the low half and FIRE in the high half of one dword (<= 1024 each), and the G = B / (4 NW) lanes of a tile added by
// DPP (quad_perm xor 1, xor 2, row_half_mirror: every lane of the group ends with the tile's sum; G = 1, W = 512 with
// B = 8, needs none). The group's first lane hands the tile's index bi * Wc + bj and its two counts to store(o, T, F).
template <int NW, class Store>
__device__ __forceinline__ void policy_obs_rows_strip(const uint8_t* __restrict__ S, uint32_t lofs, int lane, int strip,
                                                      int H, int lgB, uint32_t Tp, uint32_t Fp, Store store) {
    constexpr int W = 256 * NW;
    const int B = 1 << lgB;
    const int lgG = lgB - (NW == 1 ? 2 : 3);  // lanes per tile: G = B / (4 NW) = 1, 2, 4, 8
    const int Wc = W >> lgB;
    const int row_end = min(H, strip * POBS_STRIP + POBS_STRIP);
    uint32_t aT[NW], aF[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) aT[j] = aF[j] = 0u;
    // the strip's rows in groups of POBS_RD, unrolled over the strip's four groups with two register sets: the next
    // group's loads are issued before the current group is classified (two groups in flight, across block-row boundaries
    // too); a block-row ends where (r + POBS_RD) % B == 0
    ObsRow<NW> x[2][POBS_RD];
    const int base = strip * POBS_STRIP;
#pragma unroll
    for (int k = 0; k < POBS_RD; ++k) x[0][k] = load_obsrow<NW>(S, lofs, base + k);
#pragma unroll
    for (int g = 0; g < POBS_STRIP / POBS_RD; ++g) {
        const int r = base + g * POBS_RD;
        if (r >= row_end) break;  // wave-uniform: a strip cut short by the grid's last row
        if (g + 1 < POBS_STRIP / POBS_RD && r + POBS_RD < row_end) {
#pragma unroll
            for (int k = 0; k < POBS_RD; ++k) x[(g + 1) & 1][k] = load_obsrow<NW>(S, lofs, r + POBS_RD + k);
        }
#pragma unroll
        for (int k = 0; k < POBS_RD; ++k) {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                aT[j] += bytes_eq01(x[g & 1][k].w[j], Tp);
                aF[j] += bytes_eq01(x[g & 1][k].w[j], Fp);
            }
        }
        if (((r + POBS_RD) & (B - 1)) != 0) continue;
        uint32_t sT = 0u, sF = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            sT = __builtin_amdgcn_sad_u8(aT[j], 0u, sT);
            sF = __builtin_amdgcn_sad_u8(aF[j], 0u, sF);
            aT[j] = aF[j] = 0u;
        }
        uint32_t s = sT | (sF << 16);
        if (lgG >= 1) s += obs_dpp<0xB1>(s);   // quad_perm [1, 0, 3, 2]
        if (lgG >= 2) s += obs_dpp<0x4E>(s);   // quad_perm [2, 3, 0, 1]
        if (lgG >= 3) s += obs_dpp<0x141>(s);  // row_half_mirror: the other quad of the lane's eight
        if ((lane & ((1 << lgG) - 1)) == 0) store((r >> lgB) * Wc + (lane >> lgG), s & 0xFFFFu, s >> 16);
    }
}
