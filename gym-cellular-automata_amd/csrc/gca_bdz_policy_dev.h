// gca_bdz_policy_dev.h — the bulldozer policy network (include/gca.h "bulldozer policy") as device functions of ONE
// workgroup per env of ANY whole number of waves, shared by the stand-alone act kernel (256 threads) and the policy
// rollout kernel (a wave per strip of the grid, 1 to 16 waves; both in gca_windy.hip), so the two evaluate it with the
// same instructions in the same order: the rollout is bit for bit K x (observe, act, step).
//
// The summation order is the helicopter policy's (gca.h); gca_heli_policy_dev.h realises it with exactly 256 threads.
// Here the 256 float4 "virtual threads" of that layout are looped over the nt real threads, so the order is a function
// of (S, C, Hd) alone:
//   hidden  virtual thread vt owns four consecutive units (one 16-B load per weight row): q = vt % (Hd / 4) the quad,
//           g = vt / (Hd / 4) the group of G = 1024 / Hd. It adds the terms n = g, g + G, ... in that order onto 0.0f
//           and writes part[g][4 q ..]. Real thread tid runs vt = tid, tid + nt, ... < 256.
//   relu    unit j = tid, tid + nt, ... < Hd: h_j = relu(b1[j] + p_0[j] + .. + p_{G-1}[j]), left to right.
//   heads   virtual lane t < 192 is lane r = t % 16 of output o = t / 16 (12 outputs): w_out[j][o] * h_j for j = r,
//           r + 16, ... onto 0.0f, then the xor butterfly 8, 4, 2, 1 inside its 16 lanes. nt is a multiple of 64 and
//           192 = 3 * 64, so a wave runs an iteration with all 64 lanes or not at all: every shuffle finds its partner.
//   sample  every thread reads the twelve outputs back and samples both heads redundantly: the action is known to all
//           threads without another barrier (the rollout carries the env's state in every thread).
// Four barriers, each outside every condition (the loops' trip counts differ between threads, the barriers sit between
// the loops): A the caller's coarse map in LDS (and, in the rollout, thread 0's Modify byte and its coarse adjustment of
// the step before), B the partials, C the hidden vector, D the outputs. LDS reuse across evaluations: part is written
// after A and read before C, hs written after B and read before D, outs written after C and read after D. The next
// write of each word comes after the NEXT evaluation's A, B or C, which every thread reaches only after its reads of this
// one: at least two barriers lie between any read and the next write of the same word. cs is read between A and B only;
// its writers (the rollout's recount, thread 0's adjustment) run after D and before the next A.
#pragma once
#include "gca_common.h"

constexpr int BPOL_VT = 256;             // virtual threads of the hidden layer
constexpr int BPOL_NOUT = 12;            // 9 move logits, 2 shoot logits, the value
constexpr int BPOL_PART = 4 * BPOL_VT;   // floats of the partials: G * Hd = 1024 for every Hd

struct BdzPolicyW {
    const float* __restrict__ w_local;   // [S*S][4][Hd], 16-B aligned
    const float* __restrict__ w_coarse;  // [C][Hd], 16-B aligned
    const float* __restrict__ b1;        // [Hd]
    const float* __restrict__ w_out;     // [Hd][12]
    const float* __restrict__ b2;        // [12]
    int S, SS, C, Hd, lgHd, greedy;
    uint32_t k0, k1;  // the policy seed
};

// LDS words of one evaluation: the coarse map (rounded up to 4 words), the partials, the hidden vector, the outputs
__host__ __device__ constexpr int bdz_policy_lds_words(int C) { return ((C + 3) & ~3) + BPOL_PART + BPOL_VT + 16; }

// (move, shoot) from the twelve outputs (gca.h "bulldozer policy"). Comparisons only, no fmax: NaN logits give a move in
// [0, 8] and a shoot in {0, 1}. Plain loops, the same in every thread.
__device__ __forceinline__ void bdz_policy_sample(const float (&o)[BPOL_NOUT], const BdzPolicyW& w, uint32_t step,
                                                  uint32_t env_id, uint32_t ep, int32_t& move, int32_t& shoot) {
    float m = o[0];
    int32_t first = 0;
#pragma unroll
    for (int i = 1; i < 9; ++i)
        if (o[i] > m) {
            m = o[i];
            first = i;
        }
    const float s0 = o[9], s1 = o[10];
    if (w.greedy) {
        move = first;
        shoot = s1 > s0 ? 1 : 0;
        return;
    }
    float c[9], s = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        s = s + exp_f32(o[i] - m);
        c[i] = s;
    }
    const u32x4 x = philox4x32_10(u32x4{step, env_id, ep, GCA_TAG_BPOLICY}, w.k0, w.k1);
    const float t = u01_f32(x.x) * c[8];
    int32_t mv = 8;
#pragma unroll
    for (int i = 7; i >= 0; --i)
        if (t < c[i]) mv = i;
    move = mv;
    const float ms = s1 > s0 ? s1 : s0;
    const float c0 = exp_f32(s0 - ms), c1 = c0 + exp_f32(s1 - ms);
    shoot = u01_f32(x.y) * c1 < c0 ? 0 : 1;
}

// One evaluation by the whole workgroup of nt threads (a multiple of 64). cs: the env's coarse map in LDS, complete
// before the call (barrier A is the first thing here); part (16-B aligned) / hs / outs: LDS scratch of BPOL_PART /
// BPOL_VT / 16 floats. class_at(n, i, j): the class (0..3) of window cell n = i * S + j. record(): the caller's stores
// of what this step observed, run between A and B, where the observation (cs, the plane behind class_at) is stable.
// logits_row / value_ptr (nullable): this env's record of the outputs. move / shoot: the same in every thread.
template <class ClassAt, class Record>
__device__ __forceinline__ void bdz_policy_eval(const BdzPolicyW& w, const float* cs, float* part, float* hs,
                                                float* outs, int tid, int nt, uint32_t step, uint32_t env_id,
                                                uint32_t ep, float* logits_row, float* value_ptr, ClassAt class_at,
                                                Record record, int32_t& move, int32_t& shoot) {
    __syncthreads();  // A
    const int Hd = w.Hd, lgQ = w.lgHd - 2;  // 2^lgQ = Hd / 4 virtual threads per weight row
    const int G = BPOL_PART >> w.lgHd;
    const int S = w.S, SS = w.SS, N = w.SS + w.C;
    const int dI = G / S, dJ = G - dI * S;  // the window cell G terms on, walked without a division per term
    for (int vt = tid; vt < BPOL_VT; vt += nt) {
        const int q = vt & ((1 << lgQ) - 1), g = vt >> lgQ;
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
        reinterpret_cast<float4*>(part)[vt] = acc;  // part[g][4 q ..]: g * Hd + 4 q = 4 vt
    }
    record();
    __syncthreads();  // B
    for (int j = tid; j < Hd; j += nt) {
        float h = w.b1[j];
        for (int gg = 0; gg < G; ++gg) h = h + part[gg * Hd + j];
        hs[j] = h > 0.0f ? h : 0.0f;
    }
    __syncthreads();  // C
    for (int t = tid; t < 16 * BPOL_NOUT; t += nt) {  // whole waves (see above)
        const int o = t >> 4, r = t & 15;
        float qs = 0.0f;
        for (int jj = r; jj < Hd; jj += 16) qs = qs + w.w_out[jj * BPOL_NOUT + o] * hs[jj];
        qs = qs + __shfl_xor(qs, 8);
        qs = qs + __shfl_xor(qs, 4);
        qs = qs + __shfl_xor(qs, 2);
        qs = qs + __shfl_xor(qs, 1);
        if (r == 0) outs[o] = w.b2[o] + qs;
    }
    __syncthreads();  // D
    float o[BPOL_NOUT];
#pragma unroll
    for (int i = 0; i < BPOL_NOUT; ++i) o[i] = outs[i];
    if (tid < 11 && logits_row) logits_row[tid] = outs[tid];
    if (tid == 11 && value_ptr) *value_ptr = outs[11];
    bdz_policy_sample(o, w, step, env_id, ep, move, shoot);
}
