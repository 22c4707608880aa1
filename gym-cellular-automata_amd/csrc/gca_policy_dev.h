// gca_policy_dev.h — the policy network of both agents (include/gca.h "helicopter policy", "bulldozer policy") as device
// functions of ONE workgroup per env, written once: the weights' view, the LDS layout, the network from the observation
// to its NOUT outputs (policy_outputs<NOUT, NT>: 10 for the helicopter, 12 for the bulldozer, 15 for the bulldozer with
// the extension head) and the agents' samplers. The stand-alone act kernels and the resident policy rollouts
// (gca_heli.hip, gca_windy.hip) all evaluate the network through policy_outputs, with the same instructions in the same
// order: a rollout is bit for bit K x (observe, act, step), and an output column is the same sum whichever agent owns
// it.
//
// The summation order is the one written down in gca.h; here is how the workgroup realises it. The layout is that of
// 256 float4 "virtual threads"; the workgroup is either exactly those 256 threads (NT = 256: the two act kernels and
// the helicopter's rollout, every loop below then is one guarded pass) or any whole number of waves, nt threads at run
// time (NT = 0: the bulldozer's rollout, a wave per strip of the grid, 1 to 16 waves), which loop over the virtual
// threads. Either way the order is a function of (S, C, Hd) alone:
//   hidden  the layer is a gather of N = S*S + C weight rows of Hd floats from L2, so it is laid out for bytes in
//           flight: virtual thread vt owns FOUR consecutive units (one 16-B load per row), q = vt % (Hd / 4) the quad
//           and g = vt / (Hd / 4) the group of G = 1024 / Hd. It adds the terms n = g, g + G, ... in that order onto
//           0.0f, four rows in flight, and writes part[g][4 q ..]. Real thread tid runs vt = tid, tid + nt, ... < 256.
//   relu    unit j = tid, tid + nt, ... < Hd: h_j = relu(b1[j] + p_0[j] + .. + p_{G-1}[j]), left to right, to LDS.
//   heads   virtual lane t < policy_head_lanes(NOUT) (16 NOUT rounded up to whole waves: 192 for 10 and 12 outputs,
//           256 for 15) is lane r = t % 16 of output o = t / 16: it adds w_out[j][o] * h_j for j = r, r + 16,
//           ... onto 0.0f in that order, and the 16 lanes of an output meet in the xor butterfly 8, 4, 2, 1 (f32
//           addition commutes, so every lane holds the tree's value). The lane count and nt are multiples of 64, so a
//           wave runs an iteration with all 64 lanes or not at all: every shuffle finds its partner. With NOUT = 10
//           lanes 160..191 compute a clamped duplicate of output 9 and store nothing; with 15, lanes 240..255 do.
//   sample  every thread reads the outputs back and samples redundantly: the action is known to all threads without
//           another barrier (the rollouts carry the env's state in every thread).
// Four barriers, each outside every condition (the loops' trip counts differ between threads, the barriers sit between
// the loops): A the caller's coarse map in LDS (and, in the bulldozer's rollout, thread 0's Modify byte and its coarse
// adjustment of the step before), B the partials, C the hidden vector, D the outputs. LDS reuse across evaluations:
// part is written after A and read before C, hs written after B and read before D, outs written after C and read after
// D. The next write of each word comes after the NEXT evaluation's A, B or C, which every thread reaches only after
// its reads of this one: at least two barriers lie between any read and the next write of the same word. cs is read
// between A and B only; its writers (the helicopter rollout's per-step count, the bulldozer rollout's recount and
// thread 0's adjustment) run after D and before the next A.
#pragma once
#include "gca_common.h"

constexpr int POL_VT = 256;            // virtual threads of the hidden layer; the act kernels' workgroup
constexpr int POL_PART = 4 * POL_VT;   // floats of the partials: G * Hd = 1024 for every Hd
constexpr int HELI_POL_NOUT = 10;      // 9 action logits and the value
constexpr int BDZ_POL_NOUT = 12;       // 9 move logits, 2 shoot logits and the value
constexpr int EXT_POL_NOUT = 15;       // 9 move logits, 2 shoot logits, 3 extension logits and the value
// virtual lanes of the heads: 16 per output, rounded up to whole waves (192 for 10 and 12 outputs, 256 for 15)
__host__ __device__ constexpr int policy_head_lanes(int NOUT) { return (16 * NOUT + 63) & ~63; }

struct PolicyW {
    const float* __restrict__ w_local;   // [S*S][4][Hd], 16-B aligned
    const float* __restrict__ w_coarse;  // [C][Hd], 16-B aligned
    const float* __restrict__ b1;        // [Hd]
    const float* __restrict__ w_out;     // [Hd][NOUT]
    const float* __restrict__ b2;        // [NOUT]
    int S, SS, C, Hd, lgHd, greedy;
    uint32_t k0, k1;  // the policy seed
};

// LDS words of one evaluation: the coarse map (rounded up to 4 words), the partials, the hidden vector, the outputs
__host__ __device__ constexpr int policy_lds_words(int C) { return ((C + 3) & ~3) + POL_PART + POL_VT + 16; }
// the largest coarse map the shared checks admit is the one whose network words fill a workgroup's 64 KiB of LDS
static_assert(policy_lds_words(GCA_POLICY_C_MAX) * 4 == 65536, "GCA_POLICY_C_MAX must follow policy_lds_words");

// The device's view of the weights of a checked policy. who: the bulldozer's entry point, which names the argument
// `policy`; NULL for the helicopter's entry points, which refuse in the struct's name.
static inline int policy_view(const char* who, const gca_policy* p, int C, uint64_t policy_seed, int greedy,
                              PolicyW* w) {
    // the kernels' 16-B loads of the weights: the host build's loops take any alignment
    if (!gca_policy_weights_aligned(p))
        return who ? gca_refuse(who, "policy.w_local and policy.w_coarse must be 16-B aligned")
                   : gca_refuse("helicopter_policy", "w_local and w_coarse must be 16-B aligned");
    w->w_local = p->w_local; w->w_coarse = p->w_coarse; w->b1 = p->b1; w->w_out = p->w_out; w->b2 = p->b2;
    w->S = 2 * p->radius + 1;
    w->SS = w->S * w->S;
    w->C = C;
    w->Hd = p->hidden;
    w->lgHd = 5;
    while ((1 << w->lgHd) < p->hidden) ++w->lgHd;
    w->greedy = greedy != 0;
    w->k0 = (uint32_t)policy_seed;
    w->k1 = (uint32_t)(policy_seed >> 32);
    return GCA_OK;
}

// body(v) for v = tid, tid + nt, ... < n (n <= 256) -- with the workgroup fixed at 256 threads (NT) at most one pass
template <int NT, class Body>
__device__ __forceinline__ void policy_each(int tid, int nt, int n, Body body) {
    if constexpr (NT == POL_VT) {
        if (tid < n) body(tid);
    } else {
        for (int v = tid; v < n; v += nt) body(v);
    }
}

// One evaluation by the whole workgroup, from barrier A to the outputs: NT = 256 threads, or NT = 0 and nt threads (a
// multiple of 64). cs: the env's coarse map in LDS, complete before the call (barrier A is the first thing here); part
// (16-B aligned) / hs / outs: LDS scratch of POL_PART / POL_VT / 16 floats. class_at(n, i, j): the class (0..3) of
// window cell n = i * S + j. record(): the caller's stores of what this step observed, run between A and B, where the
// observation (cs, the plane behind class_at) is stable. logits_row / value_ptr (nullable): this env's record of the
// outputs. o: the NOUT outputs, the same in every thread.
template <int NOUT, int NT, class ClassAt, class Record>
__device__ __forceinline__ void policy_outputs(const PolicyW& w, const float* cs, float* part, float* hs, float* outs,
                                               int tid, int nt, float* logits_row, float* value_ptr, ClassAt class_at,
                                               Record record, float (&o)[NOUT]) {
    constexpr int HEADS = policy_head_lanes(NOUT);
    static_assert(NOUT <= 16 && HEADS <= POL_VT && HEADS % 64 == 0 && (NT == 0 || NT == POL_VT), "whole waves");
    __syncthreads();  // A
    const int Hd = w.Hd, lgQ = w.lgHd - 2;  // 2^lgQ = Hd / 4 virtual threads per weight row
    const int G = POL_PART >> w.lgHd;
    const int S = w.S, SS = w.SS, N = w.SS + w.C;
    const int dI = G / S, dJ = G - dI * S;  // the window cell G terms on, walked without a division per term
    policy_each<NT>(tid, nt, POL_VT, [&](int vt) {
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
    });
    record();
    __syncthreads();  // B
    policy_each<NT>(tid, nt, Hd, [&](int j) {
        float h = w.b1[j];
        for (int gg = 0; gg < G; ++gg) h = h + part[gg * Hd + j];
        hs[j] = h > 0.0f ? h : 0.0f;
    });
    __syncthreads();  // C
    policy_each<NT>(tid, nt, HEADS, [&](int t) {  // whole waves (see above)
        const int oo = min(t >> 4, NOUT - 1), r = t & 15;
        float qs = 0.0f;
        for (int jj = r; jj < Hd; jj += 16) qs = qs + w.w_out[jj * NOUT + oo] * hs[jj];
        qs = qs + __shfl_xor(qs, 8);
        qs = qs + __shfl_xor(qs, 4);
        qs = qs + __shfl_xor(qs, 2);
        qs = qs + __shfl_xor(qs, 1);
        if (r == 0 && t < 16 * NOUT) outs[oo] = w.b2[oo] + qs;
    });
    __syncthreads();  // D
#pragma unroll
    for (int i = 0; i < NOUT; ++i) o[i] = outs[i];
    if (tid < NOUT - 1 && logits_row) logits_row[tid] = outs[tid];
    if (tid == NOUT - 1 && value_ptr) *value_ptr = outs[NOUT - 1];
}

// ---- the helicopter's sampler. The action from the nine logits o[0..9) (gca.h "sampling"). Comparisons only, no fmax:
// NaN logits give an action in [0, 8]. Every wave runs it whole (all 64 lanes active) and every lane gets the same
// action. The nine exponentials are one exp_f32 per wave: lane i takes p_i from l_lane, its own copy of logit
// min(lane, 8), and the running sum reads them back lane by lane (v_readlane), in the order i = 0..8 -- the same nine
// values and the same eight additions as the plain loop. The draw is keyed (0, env, rng_step, POLICY).
__device__ __forceinline__ int32_t heli_policy_sample(const float (&o)[HELI_POL_NOUT], float l_lane, const PolicyW& w,
                                                      uint32_t env_id, uint32_t rs) {
    float m = o[0];
    int32_t first = 0;
#pragma unroll
    for (int i = 1; i < 9; ++i)
        if (o[i] > m) {
            m = o[i];
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

// ---- the bulldozer's sampler. (move, shoot) from the twelve outputs (gca.h "bulldozer policy"). Comparisons only, no
// fmax: NaN logits give a move in [0, 8] and a shoot in {0, 1}. Plain loops, the same in every thread. The draw is
// keyed (steps_elapsed, env, episode, BPOLICY).
// With fifteen outputs (gca.h "extension policy") the same draw's word 2 picks the extension from o[11..13] by the move
// rule over three logits; move and shoot are computed by the very same statements, so equal logits and an equal seed
// give the two-head agent's move and shoot.
template <int NOUT>
__device__ __forceinline__ void bdz_policy_sample(const float (&o)[NOUT], const PolicyW& w, uint32_t step,
                                                  uint32_t env_id, uint32_t ep, int32_t& move, int32_t& shoot,
                                                  int32_t* ext = nullptr) {
    static_assert(NOUT == BDZ_POL_NOUT || NOUT == EXT_POL_NOUT, "the bulldozer's two or three heads");
    float em = 0.0f;
    int32_t efirst = 0;
    if constexpr (NOUT == EXT_POL_NOUT) {
        em = o[11];
#pragma unroll
        for (int i = 1; i < 3; ++i)
            if (o[11 + i] > em) {
                em = o[11 + i];
                efirst = i;
            }
    }
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
        if constexpr (NOUT == EXT_POL_NOUT) *ext = efirst;
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
    if constexpr (NOUT == EXT_POL_NOUT) {
        float ce[3], se = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            se = se + exp_f32(o[11 + i] - em);
            ce[i] = se;
        }
        const float te = u01_f32(x.z) * ce[2];
        int32_t ev = 2;
#pragma unroll
        for (int i = 1; i >= 0; --i)
            if (te < ce[i]) ev = i;
        *ext = ev;
    }
}
