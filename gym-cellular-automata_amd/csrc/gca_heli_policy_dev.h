// gca_heli_policy_dev.h — the helicopter policy network (include/gca.h "helicopter policy") as device functions of one
// 256-thread workgroup per env, shared by the stand-alone act kernel and the resident policy rollout (gca_heli.hip), so
// the two evaluate it with the same instructions in the same order: the rollout is bit for bit K x (observe, act, step).
//
// The summation order is the one written down in gca.h; here is how the workgroup realises it.
//   hidden  the layer is a gather of N = S*S + C weight rows of Hd floats from L2, so it is laid out for bytes in
//           flight: a thread owns FOUR consecutive units (one 16-B load per row) and Hd / 4 threads cover a row, which
//           leaves G = 1024 / Hd groups of threads. Group g adds the terms n = g, g + G, ... in that order onto 0.0f,
//           four rows in flight per thread; its partial goes to LDS (part[g][j]).
//   relu    thread j < Hd: h_j = relu(b1[j] + p_0[j] + .. + p_{G-1}[j]), left to right, to LDS.
//   heads   thread t < 160 is lane r = t % 16 of output o = t / 16: it adds w_out[j][o] * h_j for j = r, r + 16, ...
//           onto 0.0f in that order, and the 16 lanes of an output meet in the xor butterfly 8, 4, 2, 1 (f32 addition
//           commutes, so every lane holds the tree's value).
//   sample  every thread reads the ten outputs back and samples redundantly: the action is known to all 256 threads
//           without another barrier (the rollout carries the env's position in every thread).
// Four barriers, each outside every condition: A the caller's coarse map in LDS, B the partials, C the hidden vector, D
// the outputs. Every LDS word is written again one evaluation later at the earliest, with at least three barriers in
// between.
#pragma once
#include "gca_common.h"

constexpr int POL_THREADS = 256;
constexpr int POL_NOUT = 10;               // 9 action logits and the value
constexpr int POL_PART = 4 * POL_THREADS;  // floats of the partials: G * Hd = 1024 for every Hd

struct HeliPolicyW {
    const float* __restrict__ w_local;   // [S*S][4][Hd], 16-B aligned
    const float* __restrict__ w_coarse;  // [C][Hd], 16-B aligned
    const float* __restrict__ b1;        // [Hd]
    const float* __restrict__ w_out;     // [Hd][10]
    const float* __restrict__ b2;        // [10]
    int S, SS, C, Hd, lgHd, greedy;
    uint32_t k0, k1;  // the policy seed
};

// LDS words of one evaluation: the coarse map (rounded up to 4 words), the partials, the hidden vector, the outputs
__host__ __device__ constexpr int heli_policy_lds_words(int C) { return ((C + 3) & ~3) + POL_PART + POL_THREADS + 16; }

// The action from the nine logits l (gca.h "sampling"). Comparisons only, no fmax: NaN logits give an action in [0, 8].
// Every wave runs it whole (all 64 lanes active) and every lane gets the same action. The nine exponentials are one
// exp_f32 per wave: lane i takes p_i, and the running sum reads them back lane by lane (v_readlane), in the order i =
// 0..8 -- the same nine values and the same eight additions as the plain loop.
__device__ __forceinline__ int32_t heli_policy_sample(const float (&l)[9], float l_lane, const HeliPolicyW& w,
                                                      uint32_t env_id, uint32_t rs) {
    float m = l[0];
    int32_t first = 0;
#pragma unroll
    for (int i = 1; i < 9; ++i)
        if (l[i] > m) {
            m = l[i];
            first = i;
        }
    if (w.greedy) return first;
    const int pe = __float_as_int(exp_f32(l_lane - m));  // lane i < 9: p_i
    float c[9], s = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        s = s + __int_as_float(__builtin_amdgcn_readlane(pe, i));
        c[i] = s;
    }
    const u32x4 x = philox4x32_10(u32x4{0u, env_id, rs, GCA_TAG_POLICY}, w.k0, w.k1);
    const float t = u01_f32(x.x) * c[8];
    int32_t act = 8;
#pragma unroll
    for (int i = 7; i >= 0; --i)
        if (t < c[i]) act = i;
    return act;
}

// One evaluation by the whole workgroup. cs: the env's coarse map in LDS, written by the caller before the call (barrier
// A is the first thing here); part (16-B aligned) / hs / outs: LDS scratch of POL_PART / POL_THREADS / 16 floats.
// class_at(n, i, j): the class (0..3) of window cell n = i * S + j. logits_row / value_ptr (nullable): this env's record
// of the outputs. Returns the action, the same in every thread.
template <class ClassAt>
__device__ __forceinline__ int32_t heli_policy_eval(const HeliPolicyW& w, const float* cs, float* part, float* hs,
                                                    float* outs, int tid, uint32_t env_id, uint32_t rs,
                                                    float* logits_row, float* value_ptr, ClassAt class_at) {
    __syncthreads();  // A
    const int Hd = w.Hd, lgQ = w.lgHd - 2;  // 2^lgQ = Hd / 4 threads per weight row
    const int q = tid & ((1 << lgQ) - 1), g = tid >> lgQ, G = POL_PART >> w.lgHd;
    const int S = w.S, SS = w.SS, N = w.SS + w.C;
    const int dI = G / S, dJ = G - dI * S;  // the window cell G terms on, walked without a division per term
    const float4* __restrict__ wl = reinterpret_cast<const float4*>(w.w_local) + q;
    const float4* __restrict__ wc = reinterpret_cast<const float4*>(w.w_coarse) + q;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int n = g, wi = g / S, wj = g - wi * S;
#pragma unroll 4
    for (; n < SS; n += G) {
        const uint32_t cls = class_at(n, wi, wj);
        const float4 t = wl[(n * 4 + (int)cls) << lgQ];
        acc.x = acc.x + t.x;
        acc.y = acc.y + t.y;
        acc.z = acc.z + t.z;
        acc.w = acc.w + t.w;
        wi += dI;
        wj += dJ;
        if (wj >= S) {
            wj -= S;
            wi += 1;
        }
    }
#pragma unroll 4
    for (; n < N; n += G) {
        const int c = n - SS;
        const float4 t = wc[c << lgQ];
        const float s = cs[c];
        acc.x = acc.x + t.x * s;
        acc.y = acc.y + t.y * s;
        acc.z = acc.z + t.z * s;
        acc.w = acc.w + t.w * s;
    }
    reinterpret_cast<float4*>(part)[tid] = acc;  // part[g][4 q ..]: g * Hd + 4 q = 4 tid
    __syncthreads();  // B
    if (tid < Hd) {
        float h = w.b1[tid];
        for (int gg = 0; gg < G; ++gg) h = h + part[gg * Hd + tid];
        hs[tid] = h > 0.0f ? h : 0.0f;
    }
    __syncthreads();  // C
    if (tid < 192) {  // waves 0..2 (wave-uniform); lanes 160..191 duplicate output 9 and store nothing
        const int o = min(tid >> 4, POL_NOUT - 1), r = tid & 15;
        float qs = 0.0f;
        for (int jj = r; jj < Hd; jj += 16) qs = qs + w.w_out[jj * POL_NOUT + o] * hs[jj];
        qs = qs + __shfl_xor(qs, 8);
        qs = qs + __shfl_xor(qs, 4);
        qs = qs + __shfl_xor(qs, 2);
        qs = qs + __shfl_xor(qs, 1);
        if (r == 0 && tid < 16 * POL_NOUT) outs[o] = w.b2[o] + qs;
    }
    __syncthreads();  // D
    float l[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) l[i] = outs[i];
    if (tid < 9 && logits_row) logits_row[tid] = outs[tid];
    if (tid == 9 && value_ptr) *value_ptr = outs[9];
    return heli_policy_sample(l, outs[min(tid & 63, 8)], w, env_id, rs);  // lane i < 9 also holds l_i on its own
}
