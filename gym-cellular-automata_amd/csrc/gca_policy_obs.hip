// gca_policy_obs.hip — the policy observation of the batched bulldozer / helicopter envs (gca_policy_observation).
//
// What a closed-loop agent looks at between two env steps, written by ONE launch that reads each env's current plane
// buf[parity[e]][e] once (1 B per cell; env.grids() gathers both planes into a third: 3 B per cell):
//   local   u8  [E][S][S], S = 2 radius + 1: the classes (0 other, 1 TREE, 2 FIRE, 3 outside the grid) of the cells
//           around the agent's position
//   coarse  f32 [E][2][Hc][Wc]: TREE and FIRE cells per block x block tile times 1 / block^2 (exact: counts <= 4096, the
//           scale a power of two)
// Classification is equality with the env's codes everywhere (no bit shortcut: a fourth code is class 0 / counts in
// neither channel). The definition is the project's own, pinned by tests/_policy_obs_ref.py.
//
// One grid, two kinds of workgroup: the first `window_wgs` workgroups write the windows (one wave per env), the
// workgroups after them build `coarse`. Two forms of the coarse part, bit-equal:
//   rows     W = 256 NW (NW = 1, 2), block = 8 / 16 / 32, H % block == 0: windy_rows_kernel's lane map (a wave holds whole
//            image rows, lane l owning columns [4 NW l, 4 NW l + 4 NW): one dword, or two, per row). The hot path.
//   generic  any H, W, block: a thread per tile with byte loads (the helicopter's 42 x 42).
// Device pointers only, no allocation, no memset, no atomics, no LDS, no host synchronisation: capturable.
#include "gca_common.h"
#include "gca_policy_obs_dev.h"  // the rows form's strip of one wave, shared with the bulldozer policy rollout

#define POBS_THREADS 256
#define POBS_WAVES (POBS_THREADS / GCA_WAVE)

// ------------------------------------------------------------------ the window part (both kernels)
// One wave per env, lane j the window's column j (S <= 63), its S rows in groups of POBS_WIN with the group's loads in
// flight together (a row at a time cost one load latency per row: 33 in a row at radius 16). Row and column are taken
// in wrapping unsigned arithmetic and tested by one unsigned compare each, so a position anywhere in int32 (the
// caller's own value; Move never leaves the grid) gives class 3, never an address: the only load of the window part
// reads the tested in-grid cell, or, for a cell outside the grid, the first byte of the env's own plane (its value is
// discarded), so no branch sits between the loads of a group.
constexpr int POBS_WIN = 8;

__device__ __forceinline__ void policy_window_wave(const uint8_t* __restrict__ buf0, const uint8_t* __restrict__ buf1,
                                                   const uint8_t* __restrict__ parity, const int32_t* __restrict__ pos,
                                                   int e, int lane, int H, int W, uint32_t tree, uint32_t fire,
                                                   int radius, uint8_t* __restrict__ local_out) {
    const int S = 2 * radius + 1;
    if (lane >= S) return;
    const uint8_t* __restrict__ g = ((parity && parity[e]) ? buf1 : buf0) + (int64_t)e * H * W;
    const uint32_t row0 = (uint32_t)pos[2 * e] - (uint32_t)radius;
    const uint32_t col = (uint32_t)pos[2 * e + 1] - (uint32_t)radius + (uint32_t)lane;
    const bool col_in = col < (uint32_t)W;
    uint8_t* __restrict__ out = local_out + (int64_t)e * S * S + lane;
    for (int i0 = 0; i0 < S; i0 += POBS_WIN) {
        uint32_t v[POBS_WIN];
        bool in[POBS_WIN];
#pragma unroll
        for (int k = 0; k < POBS_WIN; ++k) {
            const uint32_t row = row0 + (uint32_t)(i0 + k);
            in[k] = col_in && row < (uint32_t)H;
            v[k] = g[in[k] ? row * (uint32_t)W + col : 0u];  // < H * W < 2^30
        }
#pragma unroll
        for (int k = 0; k < POBS_WIN; ++k) {
            const uint32_t cls = !in[k] ? 3u : (v[k] == tree ? 1u : (v[k] == fire ? 2u : 0u));
            if (i0 + k < S) out[(i0 + k) * S] = (uint8_t)cls;
        }
    }
}

// The window workgroups of a launch (its first `window_wgs` workgroups, so their short serial chains start at once and
// run under the coarse part's stream): workgroup wb takes envs [POBS_WAVES wb, POBS_WAVES wb + POBS_WAVES).
__device__ __forceinline__ void policy_window_group(const uint8_t* __restrict__ buf0, const uint8_t* __restrict__ buf1,
                                                    const uint8_t* __restrict__ parity, const int32_t* __restrict__ pos,
                                                    int wb, int E, int H, int W, uint32_t tree, uint32_t fire,
                                                    int radius, uint8_t* __restrict__ local_out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int e = wb * POBS_WAVES + wave;
    if (e >= E) return;
    policy_window_wave(buf0, buf1, parity, pos, e, lane, H, W, tree, fire, radius, local_out);
}

// ------------------------------------------------------------------ rows form (W = 256 NW, NW = 1, 2)
// A wave takes a strip of POBS_STRIP rows of one env (policy_obs_rows_strip, gca_policy_obs_dev.h); the first lane of
// every tile stores the tile's two f32.
template <int NW>
__global__ __launch_bounds__(POBS_THREADS) void policy_obs_rows_kernel(
    const uint8_t* __restrict__ buf0, const uint8_t* __restrict__ buf1, const uint8_t* __restrict__ parity,
    const int32_t* __restrict__ pos, int E, int H, int lgB, int strips, int window_wgs, uint32_t tree, uint32_t fire,
    int radius, float inv, uint8_t* __restrict__ local_out, float* __restrict__ coarse_out) {
    constexpr int W = 256 * NW;
    if ((int)blockIdx.x < window_wgs) {
        policy_window_group(buf0, buf1, parity, pos, (int)blockIdx.x, E, H, W, tree, fire, radius, local_out);
        return;
    }
    // the wave index is wave-uniform: readfirstlane keeps the env, the strip and every row index in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int unit = ((int)blockIdx.x - window_wgs) * POBS_WAVES + wave;
    const int env = unit / strips;
    if (env >= E) return;
    const int strip = unit - env * strips;
    const int Hc = H >> lgB, Wc = W >> lgB;
    const uint8_t* __restrict__ S = ((parity && parity[env]) ? buf1 : buf0) + (int64_t)env * H * W;
    float* __restrict__ C = coarse_out + (int64_t)env * 2 * Hc * Wc;
    policy_obs_rows_strip<NW>(S, 4 * NW * (uint32_t)lane, lane, strip, H, lgB, rep4(tree), rep4(fire),
                              [&](int o, uint32_t nT, uint32_t nF) {
                                  C[o] = (float)nT * inv;
                                  C[Hc * Wc + o] = (float)nF * inv;
                              });
}

// ------------------------------------------------------------------ generic form (any H, W, block)
// A thread per tile (e, bi, bj), byte loads over the tile's in-grid cells. Simple indexing on purpose: it is the form
// the rows form is held against, and the one small grids (the helicopter's 42 x 42, cache-resident) take.
__global__ __launch_bounds__(POBS_THREADS) void policy_obs_generic_kernel(
    const uint8_t* __restrict__ buf0, const uint8_t* __restrict__ buf1, const uint8_t* __restrict__ parity,
    const int32_t* __restrict__ pos, int E, int H, int W, int B, int Hc, int Wc, int64_t tiles, int window_wgs,
    uint32_t tree, uint32_t fire, int radius, float inv, uint8_t* __restrict__ local_out,
    float* __restrict__ coarse_out) {
    if ((int)blockIdx.x < window_wgs) {
        policy_window_group(buf0, buf1, parity, pos, (int)blockIdx.x, E, H, W, tree, fire, radius, local_out);
        return;
    }
    const int64_t t = (int64_t)((int)blockIdx.x - window_wgs) * POBS_THREADS + threadIdx.x;
    if (t >= tiles) return;
    const int bj = (int)(t % Wc);
    const int64_t q = t / Wc;
    const int bi = (int)(q % Hc), e = (int)(q / Hc);
    const uint8_t* __restrict__ g = ((parity && parity[e]) ? buf1 : buf0) + (int64_t)e * H * W;
    const int r1 = min(H, bi * B + B), c1 = min(W, bj * B + B);
    int32_t cT = 0, cF = 0;
    for (int r = bi * B; r < r1; ++r)
        for (int c = bj * B; c < c1; ++c) {
            const uint32_t v = g[(uint32_t)r * (uint32_t)W + (uint32_t)c];
            cT += v == tree;
            cF += v == fire;
        }
    float* __restrict__ C = coarse_out + (int64_t)e * 2 * Hc * Wc;
    C[bi * Wc + bj] = (float)cT * inv;
    C[Hc * Wc + bi * Wc + bj] = (float)cF * inv;
}

extern "C" int gca_policy_observation(const uint8_t* buf0, const uint8_t* buf1, const uint8_t* parity,
                                      const int32_t* pos, int E, int H, int W, int empty, int tree, int fire, int radius,
                                      int block, int form, uint8_t* local_out, float* coarse_out, void* stream) {
    if (const int st = gca_check_policy_observation(buf0, buf1, parity, pos, E, H, W, empty, tree, fire, radius, block,
                                                    form, local_out, coarse_out))
        return st;
    // the rows kernel's 8-B loads: the host build has one form and takes any alignment
    const bool aligned = (((uintptr_t)buf0 | (parity ? (uintptr_t)buf1 : (uintptr_t)0)) & 7u) == 0;
    GCA_CHECK_ARG(form != 2 || aligned, "policy_observation: form 2 (rows) needs 8-B aligned planes");
    const bool rows = form != 1 && gca_policy_obs_rows_shape(H, W, block) && aligned;
    const int Hc = (H + block - 1) / block, Wc = (W + block - 1) / block;
    const int64_t tiles = (int64_t)E * Hc * Wc;
    const int strips = (H + POBS_STRIP - 1) / POBS_STRIP;
    int64_t coarse_wgs = 0;
    if (coarse_out)
        coarse_wgs = rows ? ((int64_t)E * strips + POBS_WAVES - 1) / POBS_WAVES : (tiles + POBS_THREADS - 1) / POBS_THREADS;
    const int64_t window_wgs = local_out ? ((int64_t)E + POBS_WAVES - 1) / POBS_WAVES : 0;
    // the kernels' 32-bit wave / workgroup indices: the host build launches nothing
    GCA_CHECK_ARG(coarse_wgs + window_wgs < (1ll << 29), "policy_observation: too many envs for one launch");
    const dim3 grid((unsigned)(coarse_wgs + window_wgs)), wg(POBS_THREADS);
    const float inv = 1.0f / (float)(block * block);
    const uint32_t T = (uint32_t)tree, F = (uint32_t)fire;
    hipStream_t st = (hipStream_t)stream;
    if (rows) {
        int lgB = 3;
        while ((1 << lgB) < block) ++lgB;
        if (W == 256)
            hipLaunchKernelGGL(policy_obs_rows_kernel<1>, grid, wg, 0, st, buf0, buf1, parity, pos, E, H, lgB, strips,
                               (int)window_wgs, T, F, radius, inv, local_out, coarse_out);
        else
            hipLaunchKernelGGL(policy_obs_rows_kernel<2>, grid, wg, 0, st, buf0, buf1, parity, pos, E, H, lgB, strips,
                               (int)window_wgs, T, F, radius, inv, local_out, coarse_out);
    } else {
        hipLaunchKernelGGL(policy_obs_generic_kernel, grid, wg, 0, st, buf0, buf1, parity, pos, E, H, W, block, Hc, Wc,
                           tiles, (int)window_wgs, T, F, radius, inv, local_out, coarse_out);
    }
    GCA_CHECK_LAUNCH("policy_observation");
    return GCA_OK;
}
