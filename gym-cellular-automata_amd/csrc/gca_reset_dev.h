// gca_reset_dev.h — the draws of a fresh ForestFireBulldozer episode (bulldozer.py:221-275), stated once for the two
// kernels that start one: bulldozer_reset_where_kernel (gca_reset.hip, one launch for the selected envs) and the
// reset instantiation of bulldozer_rollout_random_kernel (gca_windy.hip, an env's reset between two of its K steps).
#pragma once
#include "gca_common.h"

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

// Episode k of the env with global id env_id under reset_seed: one FIRE around the lower-left quadrant
// (bulldozer.py:221-253), the bulldozer around the upper-right (:255-275); the tag carries the episode index
__device__ __forceinline__ int64_t reset_fire_cell(uint64_t reset_seed, uint64_t env_id, uint32_t k, int H, int W) {
    const uint32_t ktag = (k & 0xFFFFFFu) << 8;
    const int fr = 3 * H / 4 + env_integer_dev(reset_seed, env_id, 1u | ktag, (uint32_t)max(1, H / 12));
    const int fc = W / 4 + env_integer_dev(reset_seed, env_id, 2u | ktag, (uint32_t)max(1, W / 12));
    return (int64_t)fr * W + fc;
}
__device__ __forceinline__ void reset_position(uint64_t reset_seed, uint64_t env_id, uint32_t k, int H, int W,
                                               int32_t& row, int32_t& col) {
    const uint32_t ktag = (k & 0xFFFFFFu) << 8;
    row = H / 4 + env_integer_dev(reset_seed, env_id, 3u | ktag, (uint32_t)max(1, H / 12));
    col = 3 * W / 4 + env_integer_dev(reset_seed, env_id, 4u | ktag, (uint32_t)max(1, W / 12));
}

// The three categories and their codes of the fill: cdf[0..1] (cdf[2] = 1 is implied) and values[0..2], device arrays
struct ResetDist {
    float cdf0, cdf1;
    uint32_t v0, v1, v2;
};
__device__ __forceinline__ ResetDist reset_dist(const float* __restrict__ cdf, const uint8_t* __restrict__ values) {
    return ResetDist{cdf[0], cdf[1], values[0], values[1], values[2]};
}

// The grid g (HW cells) of episode k from Philox per quad of cells (fill_categorical_kernel's draw, gca_util.hip, with
// counter word 2 = k), the FIRE cell planted, by the nthreads threads of one workgroup (thread tid takes quads tid,
// tid + nthreads, ...); the cells this thread wrote are added to (cE, cT, cF). WHOLE: g is 4-B aligned and HW a
// multiple of 4 (the row-stream grids), so every quad is one dword store; otherwise a partial last quad and an
// unaligned base take byte stores.
template <bool WHOLE>
__device__ __forceinline__ void reset_fill_grid(uint8_t* __restrict__ g, int64_t HW, int tid, int nthreads,
                                                uint64_t reset_seed, uint64_t env_id, uint32_t k, const ResetDist d,
                                                int64_t fire_cell, uint32_t empty, uint32_t tree, uint32_t fire,
                                                int32_t& cE, int32_t& cT, int32_t& cF) {
    const uint32_t k0 = (uint32_t)reset_seed, k1 = (uint32_t)(reset_seed >> 32);
    const int64_t fire_quad = fire_cell >> 2;
    const uint32_t fire_shift = 8u * (uint32_t)(fire_cell & 3);
    const bool aligned = WHOLE || (((uintptr_t)g) & 3u) == 0;  // wave-uniform
    const int64_t quads = (HW + 3) >> 2;
    const uint32_t pe = rep4(empty), pt = rep4(tree), pf = rep4(fire);
    for (int64_t q = tid; q < quads; q += nthreads) {
        const u32x4 x = philox4x32_10(u32x4{(uint32_t)q, (uint32_t)env_id, k, GCA_TAG_INIT}, k0, k1);
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = u01_f32(xs[j]);
            const uint32_t v = u < d.cdf0 ? d.v0 : (u < d.cdf1 ? d.v1 : d.v2);
            word |= v << (8 * j);
        }
        // the owner of the fire cell's quad plants it before the store: one store per byte, no ordering to reason about
        if (q == fire_quad) word = (word & ~(0xFFu << fire_shift)) | ((fire & 0xFFu) << fire_shift);
        const int64_t i = q << 2;
        const int nvalid = WHOLE ? 4 : (int)min((int64_t)4, HW - i);
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
}

// the three counts summed over the wave: every lane holds the wave's totals
__device__ __forceinline__ void wave_sum3(int32_t& a, int32_t& b, int32_t& c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        c += __shfl_xor(c, off);
    }
}
