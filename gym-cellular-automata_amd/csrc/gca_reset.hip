// gca_reset.hip — per-env reset of the batched ForestFireBulldozer env on the device (gca_bulldozer_reset_where).
//
// The initial distribution of bulldozer.py:221-275 for the selected envs only, in one launch: the grid from Philox per
// cell (fill_categorical_kernel's draw, gca_util.hip, with counter word 2 = the env's episode index), one FIRE cell and
// the bulldozer's position from the per-env draws of _seeding.env_integers restated here, the cell counts of the grid
// just written, and the per-env state of a fresh episode (ca_env.py:64-81). Device pointers only, no memset, no atomics,
// no host synchronisation: the call can be captured in a graph right after an env step.
#include "gca_reset_dev.h"  // the draws, shared with the rollout kernel's in-launch reset (gca_windy.hip)

#define RESET_MAX_THREADS 1024

// One workgroup per env. Every thread reads the env's selection inputs (wave-uniform addresses) before any write of the
// launch to them: the only writer of done / steps_elapsed / episode is thread 0 after the barrier below.
__global__ __launch_bounds__(RESET_MAX_THREADS) void bulldozer_reset_where_kernel(
    int env_offset, uint32_t empty, uint32_t tree, uint32_t fire, uint64_t reset_seed, const uint8_t* mask,
    int64_t max_steps, int64_t set_episode, const float* __restrict__ cdf, const uint8_t* __restrict__ values,
    uint8_t* done, uint8_t* __restrict__ terminated_out, uint8_t* __restrict__ truncated_out,
    uint32_t* __restrict__ episode, int64_t* __restrict__ last_length_out, double* __restrict__ accu,
    uint8_t* __restrict__ parity, uint8_t* __restrict__ buf0, int H, int W, int32_t* __restrict__ pos,
    int32_t* __restrict__ counts, uint8_t* __restrict__ hit, int64_t* __restrict__ steps_elapsed) {
    __shared__ int32_t wave_cnt[RESET_MAX_THREADS / GCA_WAVE][3];
    const int e = blockIdx.x;
    const int tid = threadIdx.x;
    // ---- per-env inputs, issued together
    const bool was_done = done[e] != 0;
    const int64_t se = steps_elapsed[e];
    const uint32_t ep = episode[e];
    const bool by_mask = mask ? mask[e] != 0 : was_done;
    const ResetDist dist = reset_dist(cdf, values);
    const bool by_limit = max_steps > 0 && se >= max_steps;
    const bool selected = by_mask || by_limit;
    if (tid == 0) {
        if (terminated_out) terminated_out[e] = was_done ? 1 : 0;
        if (truncated_out) truncated_out[e] = (by_limit && !was_done) ? 1 : 0;
    }
    if (!selected) return;  // wave-uniform: nothing of this env is written

    const uint32_t k = set_episode >= 0 ? (uint32_t)set_episode : ep + 1u;
    const uint64_t env_id = (uint64_t)(int64_t)(env_offset + e);
    const int64_t HW = (int64_t)H * W;
    int32_t cE = 0, cT = 0, cF = 0;
    reset_fill_grid<false>(buf0 + e * HW, HW, tid, (int)blockDim.x, reset_seed, env_id, k, dist,
                           reset_fire_cell(reset_seed, env_id, k, H, W), empty, tree, fire, cE, cT, cF);
    wave_sum3(cE, cT, cF);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        wave_cnt[wave][0] = cE;
        wave_cnt[wave][1] = cT;
        wave_cnt[wave][2] = cF;
    }
    __syncthreads();
    if (tid != 0) return;
    const int nw = (int)((blockDim.x + 63) >> 6);
    int32_t sE = 0, sT = 0, sF = 0;
    for (int w = 0; w < nw; ++w) {
        sE += wave_cnt[w][0];
        sT += wave_cnt[w][1];
        sF += wave_cnt[w][2];
    }
    counts[3 * e + 0] = sE;
    counts[3 * e + 1] = sT;
    counts[3 * e + 2] = sF;
    int32_t row, col;
    reset_position(reset_seed, env_id, k, H, W, row, col);
    pos[2 * e] = row;
    pos[2 * e + 1] = col;
    if (last_length_out) last_length_out[e] = se;
    episode[e] = k;
    parity[e] = 0;
    accu[e] = 0.0;
    done[e] = 0;
    hit[e] = 0;
    steps_elapsed[e] = 0;
}

extern "C" int gca_bulldozer_reset_where(const gca_bulldozer_params* p, uint64_t reset_seed, const uint8_t* mask,
                                         int64_t max_steps, int64_t set_episode, const float* cdf,
                                         const uint8_t* values, uint8_t* done, uint8_t* terminated_out,
                                         uint8_t* truncated_out, uint32_t* episode, int64_t* last_length_out,
                                         double* accu, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W,
                                         int32_t* pos, int32_t* counts, uint8_t* hit, int64_t* steps_elapsed, int E,
                                         void* stream) {
    if (const int st = gca_check_bulldozer_reset_where(p, max_steps, set_episode, cdf, values, done, episode, accu,
                                                       parity, buf0, buf1, H, W, pos, counts, hit, steps_elapsed, E))
        return st;
    // a workgroup per env, a thread per quad of cells up to 1024 (whole waves); larger grids loop
    const int64_t quads = ((int64_t)H * W + 3) / 4;
    const int threads = (int)min((int64_t)RESET_MAX_THREADS, (quads + 63) / 64 * 64);
    hipLaunchKernelGGL(bulldozer_reset_where_kernel, dim3((unsigned)E), dim3((unsigned)threads), 0,
                       (hipStream_t)stream, (int)p->env_offset, (uint32_t)p->empty, (uint32_t)p->tree,
                       (uint32_t)p->fire, reset_seed, mask,
                       max_steps, set_episode, cdf, values, done, terminated_out, truncated_out, episode,
                       last_length_out, accu, parity, buf0, H, W, pos, counts, hit, steps_elapsed);
    GCA_CHECK_LAUNCH("bulldozer_reset_where");
    return GCA_OK;
}
