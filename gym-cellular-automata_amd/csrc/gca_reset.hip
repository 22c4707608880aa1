// gca_reset.hip — per-env reset of the batched ForestFireBulldozer env on the device (gca_bulldozer_reset_where).
//
// The initial distribution of bulldozer.py:221-275 for the selected envs only, in one launch: the grid from Philox per
// cell (fill_categorical_kernel's draw, gca_util.hip, with counter word 2 = the env's episode index), one FIRE cell and
// the bulldozer's position from the per-env draws of _seeding.env_integers restated here, the cell counts of the grid
// just written, and the per-env state of a fresh episode (ca_env.py:64-81). Device pointers only, no memset, no atomics,
// no host synchronisation: the call can be captured in a graph right after an env step.
#include "gca_common.h"

#define RESET_MAX_THREADS 1024

// _seeding._splitmix64 / env_draws / env_integers, bit for bit
__device__ __forceinline__ uint64_t splitmix64_dev(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// integer in [0, span) for (seed, global env id, tag): multiply-shift of the draw's top 32 bits
__device__ __forceinline__ int32_t env_integer_dev(uint64_t seed, uint64_t env_id, uint32_t tag, uint32_t span) {
    const uint64_t h = splitmix64_dev(seed ^ (uint64_t)tag);
    const uint64_t r = splitmix64_dev(h ^ splitmix64_dev(env_id));
    return (int32_t)(((r >> 32) * (uint64_t)span) >> 32);
}

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
    const uint32_t k0 = (uint32_t)reset_seed, k1 = (uint32_t)(reset_seed >> 32);
    // ---- per-env inputs, issued together
    const bool was_done = done[e] != 0;
    const int64_t se = steps_elapsed[e];
    const uint32_t ep = episode[e];
    const bool by_mask = mask ? mask[e] != 0 : was_done;
    const float cdf0 = cdf[0], cdf1 = cdf[1];
    const uint32_t v0 = values[0], v1 = values[1], v2 = values[2];
    const bool by_limit = max_steps > 0 && se >= max_steps;
    const bool selected = by_mask || by_limit;
    if (tid == 0) {
        if (terminated_out) terminated_out[e] = was_done ? 1 : 0;
        if (truncated_out) truncated_out[e] = (by_limit && !was_done) ? 1 : 0;
    }
    if (!selected) return;  // wave-uniform: nothing of this env is written

    const uint32_t k = set_episode >= 0 ? (uint32_t)set_episode : ep + 1u;
    const uint64_t env_id = (uint64_t)(int64_t)(env_offset + e);
    const uint32_t ktag = (k & 0xFFFFFFu) << 8;
    const uint32_t span_h = (uint32_t)max(1, H / 12), span_w = (uint32_t)max(1, W / 12);
    // one FIRE around the lower-left quadrant (bulldozer.py:221-253); the bulldozer around the upper-right (:255-275)
    const int fr = 3 * H / 4 + env_integer_dev(reset_seed, env_id, 1u | ktag, span_h);
    const int fc = W / 4 + env_integer_dev(reset_seed, env_id, 2u | ktag, span_w);
    const int64_t HW = (int64_t)H * W;
    const int64_t fire_cell = (int64_t)fr * W + fc;
    const int64_t fire_quad = fire_cell >> 2;
    const uint32_t fire_shift = 8u * (uint32_t)(fire_cell & 3);

    uint8_t* __restrict__ g = buf0 + e * HW;
    const bool aligned = (((uintptr_t)g) & 3u) == 0;  // wave-uniform
    const int64_t quads = (HW + 3) >> 2;
    const uint32_t pe = rep4(empty), pt = rep4(tree), pf = rep4(fire);
    int32_t cE = 0, cT = 0, cF = 0;
    for (int64_t q = tid; q < quads; q += blockDim.x) {
        const u32x4 x = philox4x32_10(u32x4{(uint32_t)q, (uint32_t)env_id, k, GCA_TAG_INIT}, k0, k1);
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = u01_f32(xs[j]);
            const uint32_t v = u < cdf0 ? v0 : (u < cdf1 ? v1 : v2);
            word |= v << (8 * j);
        }
        // the owner of the fire cell's quad plants it before the store: one store per byte, no ordering to reason about
        if (q == fire_quad) word = (word & ~(0xFFu << fire_shift)) | ((fire & 0xFFu) << fire_shift);
        const int64_t i = q << 2;
        const int nvalid = (int)min((int64_t)4, HW - i);
        const uint32_t valid = nvalid == 4 ? 0x01010101u : ((1u << (8 * nvalid)) - 1u) & 0x01010101u;
        cE += __popc(bytes_eq01(word, pe) & valid);
        cT += __popc(bytes_eq01(word, pt) & valid);
        cF += __popc(bytes_eq01(word, pf) & valid);
        if (aligned && nvalid == 4) {
            *reinterpret_cast<uint32_t*>(g + i) = word;
        } else {
            for (int j = 0; j < nvalid; ++j) g[i + j] = (uint8_t)(word >> (8 * j));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cE += __shfl_xor(cE, off);
        cT += __shfl_xor(cT, off);
        cF += __shfl_xor(cF, off);
    }
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
    pos[2 * e] = H / 4 + env_integer_dev(reset_seed, env_id, 3u | ktag, span_h);
    pos[2 * e + 1] = 3 * W / 4 + env_integer_dev(reset_seed, env_id, 4u | ktag, span_w);
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
    GCA_CHECK_ARG(p && cdf && values && done && episode && accu && parity && buf0 && buf1 && pos && counts && hit &&
                      steps_elapsed,
                  "bulldozer_reset_where: null argument");
    GCA_CHECK_ARG(E > 0 && H > 0 && W > 0, "bulldozer_reset_where: E, H, W must be positive");
    GCA_CHECK_ARG(H < 32768 && W < 32768, "bulldozer_reset_where: H, W < 32768");
    GCA_CHECK_ARG(buf0 != buf1, "bulldozer_reset_where: buf0 and buf1 must differ");
    GCA_CHECK_ARG(max_steps >= 0 && set_episode >= -1 && set_episode <= 0xFFFFFFFFll,
                  "bulldozer_reset_where: max_steps >= 0 and set_episode in [-1, 2^32)");
    GCA_CHECK_ARG(p->env_offset >= 0, "bulldozer_reset_where: env_offset >= 0");
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
