// gca_ppo.hip — the learner's side of the two policies (include/gca.h "PPO update"): gca_gae, the reference's
// generalised advantage estimate in one launch, and gca_helicopter_policy_grad / gca_bulldozer_policy_grad, the PPO
// clipped-surrogate loss (per head), its statistics and its gradient with respect to the five policy tensors over a
// minibatch of rollout_policy's records. The kernels are written over a compile-time head layout PpoHeads<N0, N1>:
// (9) for the helicopter, NOUT = 10 outputs; (9, 2) for the bulldozer, NOUT = 12; (9, 2, 3) for the bulldozer with the
// extension head (gca_extension_policy_grad), NOUT = 15; the value is column NOUT - 1.
//
// A policy_grad call is four launches on the caller's stream, all sums in a fixed order (no atomics):
//   adv     one workgroup: mean and population standard deviation of the minibatch's advantages (two passes, a
//           sequential partial per thread, a tree over the threads) -> workspace header.
//   fwd     one workgroup per tile of TS samples (64; 32 at Hd = 256). The tile's hidden layer is a tiled matvec: a
//           thread owns four consecutive units of SPT samples; w_local goes through LDS in chunks of 1024 / Hd cells
//           (16 KiB) with the chunk's class bytes, w_coarse in chunks of 32 rows with the tile's coarse values, so a
//           weight row is loaded from L2 once per tile, not once per sample. Then relu -> LDS, the NOUT outputs (a
//           thread per (sample, output), sixteen running sums over j mod 16 and a tree), the loss of each sample in one
//           thread, d loss / d outputs, and d loss / d pre-activations. Writes da (N, Hd), h (N, Hd) and dout (N, NOUT) to the workspace
//           and the tile's statistics and b2 gradient sums (a pairwise tree over the tile's samples).
//   wgrad   G[r][j] = sum_s x[s][r] * D[s][j]: grid (row blocks, P sample splits). A thread owns one row r and four
//           units: for a window cell the four class vectors (x the one-hot class: a select per class, so a class no
//           sample selects stays exactly 0.0f), for a coarse row x = the coarse value, for b1 x = 1 (D = da), for a
//           w_out column x = dout (D = h). Tiles of TS samples go through LDS; a tile's sum is added to the split's
//           running sum per tile (the sums stay short: TS, then tiles per split, then P terms). Partials -> workspace.
//   reduce  a thread per gradient element adds the P partials in increasing p; the last workgroup adds the tile
//           partials (a sequential partial per thread over tiles t, t + 256, .., then a tree) into g_b2 and the stats.
// gca_*_policy_grad_vclip (the reference's clipped value loss, gca.h) is eight launches: every sample's d loss / d v
// depends on two minibatch-wide scalars (U and n_U): U exists only after every tile's forward, n_U only after every
// sample has been compared with U. So fwd (instantiated with VCLIP) leaves the value column out, and four launches
// follow it, the per-sample work in a workgroup per tile, the two scalars in one small workgroup each:
//   vsum    one workgroup: U from fwd's tile sums -> workspace header word 2.
//   vcount  one wave per tile: the samples with U >= q_s and those outside the clip, as integers -> tile partials.
//   vsum    one workgroup: the two integer sums -> header words 3, 4 and vstats.
//   vfix    one workgroup per tile: d loss / d v_s into dout's value column (which carried v_s), its term added to da
//           last, as the plain fwd adds it, and the tile partial's v_loss and b2[value] sums in fwd's tree.
// (One workgroup walking all N samples for U and the counts, the first shape of this, cost 560 us at N = 131072: two
// dependent gathers per sample and nothing to hide them behind.)
// The plain entries launch the VCLIP = false instantiation, which is the kernel they always had.
// fmaf is written out where a fused multiply-add is wanted (the build runs with -ffp-contract=off).
#include "gca_common.h"
#include "gca_ppo_plan.h"

#define PPO_THREADS 256

// ------------------------------------------------------------------ GAE
__global__ __launch_bounds__(PPO_THREADS) void gae_kernel(const double* __restrict__ reward,
                                                          const float* __restrict__ value,
                                                          const float* __restrict__ next_value,
                                                          const uint8_t* __restrict__ terminal, float gamma,
                                                          float gamma_lambda, int K, int E,
                                                          float* __restrict__ advantage, float* __restrict__ returns) {
    const int e = blockIdx.x * PPO_THREADS + threadIdx.x;
    if (e >= E) return;
    float A = 0.0f, nv = next_value[e];
    for (int k = K - 1; k >= 0; --k) {
        const size_t o = (size_t)k * E + e;
        const float r = (float)reward[o];
        const float nn = (terminal && terminal[o]) ? 0.0f : 1.0f;
        const float v = value[o];
        const float delta = (r + (gamma * nv) * nn) - v;
        A = delta + (gamma_lambda * nn) * A;
        advantage[o] = A;
        returns[o] = A + v;
        nv = v;
    }
}

extern "C" int gca_gae(const double* reward, const float* value, const float* next_value, const uint8_t* terminal,
                       float gamma, float gamma_lambda, int K, int E, float* advantage, float* returns, void* stream) {
    if (const int st = gca_check_gae(reward, value, next_value, K, E, advantage, returns)) return st;
    if (K == 0) return GCA_OK;
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((E + PPO_THREADS - 1) / PPO_THREADS)), dim3(PPO_THREADS), 0,
                       (hipStream_t)stream, reward, value, next_value, terminal, gamma, gamma_lambda, K, E, advantage,
                       returns);
    GCA_CHECK_LAUNCH("gae");
    return GCA_OK;
}

// ------------------------------------------------------------------ the minibatch
struct PpoBatch {
    const uint8_t* __restrict__ local;      // [T][SS]
    const float* __restrict__ coarse;       // [T][C]
    const int32_t* __restrict__ action;     // [T][NH]
    const float* __restrict__ old_logits;   // [T][NL]
    const float* __restrict__ advantage;    // [T]
    const float* __restrict__ returns;      // [T]
    const int32_t* __restrict__ idx;        // [N] or null
    int N, T, SS, C;
};

// The record row of minibatch sample t < N. An index outside [0, T) cannot be refused without a sync: it is clamped,
// so no address leaves the records.
__device__ __forceinline__ int ppo_row(const PpoBatch& b, int t) {
    return b.idx ? min(max(b.idx[t], 0), b.T - 1) : t;
}

// ------------------------------------------------------------------ adv: mean and standard deviation
constexpr int PPO_ADV_THREADS = 1024;

__device__ __forceinline__ float ppo_block_sum(float v, float* red, int tid) {
    __syncthreads();  // the previous use of red
    red[tid] = v;
    __syncthreads();
    for (int s = PPO_ADV_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(PPO_ADV_THREADS) void ppo_adv_kernel(PpoBatch b, float* __restrict__ hdr) {
    __shared__ float red[PPO_ADV_THREADS];
    const int tid = threadIdx.x;
    float s = 0.0f;
    for (int t = tid; t < b.N; t += PPO_ADV_THREADS) s = s + b.advantage[ppo_row(b, t)];
    const float mean = ppo_block_sum(s, red, tid) / (float)b.N;
    float q = 0.0f;
    for (int t = tid; t < b.N; t += PPO_ADV_THREADS) {
        const float d = b.advantage[ppo_row(b, t)] - mean;
        q = fmaf(d, d, q);
    }
    const float var = ppo_block_sum(q, red, tid) / (float)b.N;
    if (tid == 0) {
        hdr[0] = mean;
        hdr[1] = sqrtf(var);
    }
}

// ------------------------------------------------------------------ fwd: forward, loss, d loss / d pre-activations
template <int HD>
struct PpoCfg {
    static constexpr int TS = HD == 256 ? 32 : 64;  // samples per tile (ppo_plan's TS)
    static constexpr int Q = HD / 4;                // threads per hidden vector (four units each)
    static constexpr int R = PPO_THREADS / Q;       // sample groups of the workgroup = rows per wgrad workgroup
    static constexpr int SPT = TS / R;              // samples per thread
    static constexpr int CH = 1024 / HD;            // window cells per w_local chunk: CH * 4 * HD = 4096 floats
    static constexpr int CC = 32;                   // coarse rows per w_coarse chunk
    static constexpr int WBUF = (CC * HD > 4096) ? CC * HD : 4096;  // floats of the weight chunk
    static constexpr int XST = CC + 1;              // row stride of the tile's coarse chunk (odd: no bank conflicts)
    static constexpr int HST = HD + 1;              // row stride of the tile's hidden vectors
    static constexpr int UNI = (WBUF + TS * XST > TS * HST) ? WBUF + TS * XST : TS * HST;  // the two share LDS
};

struct PpoLossArgs {
    float clip_coef, ent_coef, vf_coef, inv_n;
    int norm_adv;
};

// The head layout: N0 logits of the first head, N1 of the second (0: one head), N2 of the third (0: two heads), then
// the value.
template <int N0_, int N1_, int N2_ = 0>
struct PpoHeads {
    static constexpr int N0 = N0_, N1 = N1_, N2 = N2_;
    static_assert(N1 > 0 || N2 == 0, "a third head follows a second");
    static constexpr int NH = N2 > 0 ? 3 : (N1 > 0 ? 2 : 1);  // heads
    static constexpr int NL = N0 + N1 + N2;    // logits = the width of a record's old_logits
    static constexpr int NOUT = NL + 1;        // outputs (ppo_plan's NOUT)
    static constexpr int OST = NOUT + 1;       // row stride of a tile's outputs in LDS
    static constexpr int TP = ppo_tp(NOUT);    // floats of a tile partial
    static constexpr int WO = (NOUT + 3) & ~3;  // floats after w_out in LDS: b2, rounded up to four
};

// The loss of ONE sample is a chain of scalar operations in one thread with two cancellations (logp_new - logp_old,
// and the mean of pg under normalised advantages, whose terms nearly cancel): it runs in double and is rounded to f32
// once per term. Every sum over samples, units or inputs is f32.
// logsumexp of a head's N logits: the maximum, the sum of exp(l_i - max) left to right, max + log(sum)
template <int N>
__device__ __forceinline__ double ppo_lse(const double (&l)[N]) {
    double m = l[0];
#pragma unroll
    for (int i = 1; i < N; ++i) m = fmax(m, l[i]);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) s = s + exp(l[i] - m);
    return m + log(s);
}

template <int N>
__device__ __forceinline__ double ppo_pick(const double (&l)[N], int a) {
    double v = l[0];
#pragma unroll
    for (int i = 1; i < N; ++i) v = (a == i) ? l[i] : v;
    return v;
}

// One head of one sample (include/gca.h) on record row `row`: outs its N logits of this call, old the recorded ones, a
// its action (clamped here); A^ is formed here, from the same values for every head. Writes d loss / d l to d[0..N)
// and returns the head's terms of the four statistics sums.
struct PpoHeadTerms {
    double pg, ent, kl;
    float clipped;
};

template <int N>
__device__ __forceinline__ PpoHeadTerms ppo_head(const PpoBatch& b, int row, const float* __restrict__ hdr,
                                                 const float* outs, const float* __restrict__ old, int a,
                                                 const PpoLossArgs& la, double inv_nh, float* d) {
    double l[N], lo[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        l[i] = (double)outs[i];
        lo[i] = (double)old[i];
    }
    a = min(max(a, 0), N - 1);
    const double lse = ppo_lse<N>(l), lse_old = ppo_lse<N>(lo);
    const double logratio = (ppo_pick<N>(l, a) - lse) - (ppo_pick<N>(lo, a) - lse_old);
    const double ratio = exp(logratio);
    double adv = (double)b.advantage[row];
    if (la.norm_adv) adv = (adv - (double)hdr[0]) / ((double)hdr[1] + 1e-8);
    const double lo_c = 1.0 - (double)la.clip_coef, hi_c = 1.0 + (double)la.clip_coef;
    const bool clipped = ratio < lo_c || ratio > hi_c;
    const double pg1 = -adv * ratio, pg2 = -adv * fmin(fmax(ratio, lo_c), hi_c);
    const double dpg_dr = (!clipped || pg1 > pg2) ? -adv : 0.0;
    double p[N], lp[N], ent = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        lp[i] = l[i] - lse;
        p[i] = exp(lp[i]);
        ent = ent - p[i] * lp[i];
    }
    const double g = dpg_dr * ratio;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double onehot = (a == i) ? 1.0 : 0.0;
        d[i] = (float)((g * (onehot - p[i]) + (double)la.ent_coef * (p[i] * (lp[i] + ent))) * inv_nh);
    }
    return PpoHeadTerms{fmax(pg1, pg2), ent, (ratio - 1.0) - logratio, clipped ? 1.0f : 0.0f};
}

// VCLIP (the _vclip entries): the value column waits for U and vfix. DO[s][NOUT - 1] carries the value v_s itself, da
// is formed from the logit columns only, the tile partial's v_loss slot holds the tile's term of U (the plain kernel's
// sum) and its b2[value] slot zero; vcount and vfix replace both. Everything else is the plain instantiation's, in its
// order.
template <int HD, class HL, bool VCLIP>
__global__ __launch_bounds__(PPO_THREADS) void ppo_fwd_kernel(
    PpoBatch b, const float* __restrict__ w_local, const float* __restrict__ w_coarse, const float* __restrict__ b1,
    const float* __restrict__ w_out, const float* __restrict__ b2, PpoLossArgs la, const float* __restrict__ hdr,
    float* __restrict__ DA, float* __restrict__ H, float* __restrict__ DO, float* __restrict__ TP) {
    using Cf = PpoCfg<HD>;
    constexpr int TS = Cf::TS, Q = Cf::Q, R = Cf::R, SPT = Cf::SPT, CH = Cf::CH, CC = Cf::CC;
    constexpr int NOUT = HL::NOUT, NL = HL::NL, NH = HL::NH, OST = HL::OST, PPO_TP = HL::TP;
    __shared__ __attribute__((aligned(16))) float uni[Cf::UNI];  // weight chunk + x chunk, later the hidden vectors
    __shared__ float wo[HD * NOUT + HL::WO];                     // w_out, then b2
    __shared__ float outs[TS * OST], douts[TS * OST], tsum[TS * PPO_TP];
    __shared__ int rows[TS];
    static_assert((Cf::UNI + HD * NOUT + HL::WO + 2 * TS * OST + TS * PPO_TP + TS) * 4 <= 64 * 1024,
                  "the forward kernel's static LDS (55344 B at NOUT = 12, 59200 B at NOUT = 15; HD = 256)");
    float* const wbuf = uni;
    float* const xs = uni + Cf::WBUF;
    uint8_t* const clsb = reinterpret_cast<uint8_t*>(xs);  // TS * CH <= 2048 bytes
    float* const hs = uni;

    const int tid = threadIdx.x, jq = tid % Q, sg = tid / Q;
    const int64_t t0 = (int64_t)blockIdx.x * TS;
    const int SS = b.SS, C = b.C;
    for (int i = tid; i < HD * NOUT; i += PPO_THREADS) wo[i] = w_out[i];
    if (tid < NOUT) wo[HD * NOUT + tid] = b2[tid];
    if (tid < TS) rows[tid] = t0 + tid < b.N ? ppo_row(b, (int)(t0 + tid)) : 0;
    __syncthreads();

    // a chunk's terms are summed on their own (acc) and the chunk's sum is added to the running sum (tot): no chain of
    // additions is longer than a chunk plus the number of chunks, which keeps the f32 rounding of the pre-activations at
    // the level of a blocked matmul
    float4 acc[SPT], tot[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) tot[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // the window: chunks of CH cells, their 4 x HD weights and the tile's class bytes through LDS
    for (int c0 = 0; c0 < SS; c0 += CH) {
        const int cnt = min(CH, SS - c0);
        const float4* __restrict__ src = reinterpret_cast<const float4*>(w_local + (size_t)c0 * 4 * HD);
        for (int i = tid; i < cnt * HD; i += PPO_THREADS) reinterpret_cast<float4*>(wbuf)[i] = src[i];
        for (int i = tid; i < TS * CH; i += PPO_THREADS) {
            const int s = i / CH, c = i % CH;
            clsb[i] = c < cnt ? (b.local[(size_t)rows[s] * SS + c0 + c] & 3) : 0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SPT; ++i) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int c = 0; c < cnt; ++c) {
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int cls = clsb[(sg + R * i) * CH + c];
                const float4 w = reinterpret_cast<const float4*>(wbuf)[(c * 4 + cls) * Q + jq];
                acc[i].x += w.x;
                acc[i].y += w.y;
                acc[i].z += w.z;
                acc[i].w += w.w;
            }
        }
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
            tot[i].x += acc[i].x;
            tot[i].y += acc[i].y;
            tot[i].z += acc[i].z;
            tot[i].w += acc[i].w;
        }
        __syncthreads();
    }
    // the coarse map: chunks of CC rows of w_coarse and the tile's CC coarse values per sample
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cnt = min(CC, C - c0);
        const float4* __restrict__ src = reinterpret_cast<const float4*>(w_coarse + (size_t)c0 * HD);
        for (int i = tid; i < cnt * Q; i += PPO_THREADS) reinterpret_cast<float4*>(wbuf)[i] = src[i];
        for (int i = tid; i < TS * CC; i += PPO_THREADS) {
            const int s = i / CC, c = i % CC;
            xs[s * Cf::XST + c] = c < cnt ? b.coarse[(size_t)rows[s] * C + c0 + c] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SPT; ++i) acc[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int c = 0; c < cnt; ++c) {
            const float4 w = reinterpret_cast<const float4*>(wbuf)[c * Q + jq];
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const float x = xs[(sg + R * i) * Cf::XST + c];
                acc[i].x = fmaf(w.x, x, acc[i].x);
                acc[i].y = fmaf(w.y, x, acc[i].y);
                acc[i].z = fmaf(w.z, x, acc[i].z);
                acc[i].w = fmaf(w.w, x, acc[i].w);
            }
        }
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
            tot[i].x += acc[i].x;
            tot[i].y += acc[i].y;
            tot[i].z += acc[i].z;
            tot[i].w += acc[i].w;
        }
        __syncthreads();
    }
    // relu; the hidden vectors to LDS (over the weight chunk: the barrier above ended its last read) and to the workspace
    const float4 bb = reinterpret_cast<const float4*>(b1)[jq];
    uint32_t posmask = 0;  // bit 4 i + k: unit 4 jq + k of sample i is active
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int s = sg + R * i;
        const bool valid = t0 + s < b.N;
        float a[4] = {tot[i].x + bb.x, tot[i].y + bb.y, tot[i].z + bb.z, tot[i].w + bb.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool on = valid && a[k] > 0.0f;
            posmask |= on ? (1u << (4 * i + k)) : 0u;
            a[k] = on ? a[k] : 0.0f;
            hs[s * Cf::HST + 4 * jq + k] = a[k];
        }
        reinterpret_cast<float4*>(H + (size_t)(t0 + s) * HD)[jq] = make_float4(a[0], a[1], a[2], a[3]);
    }
    __syncthreads();
    // the NOUT outputs: a thread per (sample, output)
    {
        const int s = tid % TS;
        for (int o = tid / TS; o < NOUT; o += PPO_THREADS / TS) {
            float q[16];  // sixteen running sums over j mod 16, then a pairwise tree: no chain longer than HD / 16 + 4
#pragma unroll
            for (int k = 0; k < 16; ++k) q[k] = 0.0f;
            const float* hrow = hs + s * Cf::HST;
#pragma unroll 1
            for (int j = 0; j < HD; j += 16) {
#pragma unroll
                for (int k = 0; k < 16; ++k) q[k] = fmaf(wo[(j + k) * NOUT + o], hrow[j + k], q[k]);
            }
#pragma unroll
            for (int half = 8; half >= 1; half >>= 1)
#pragma unroll
                for (int k = 0; k < half; ++k) q[k] = q[k] + q[k + half];
            outs[s * OST + o] = wo[HD * NOUT + o] + q[0];
        }
    }
    __syncthreads();
    // the loss of one sample per thread: its heads one after the other, their terms of a statistic added in double
    // and rounded once
    if (tid < TS) {
        const int s = tid;
        const bool valid = t0 + s < b.N;
        float d[NOUT], st[5];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) d[o] = 0.0f;
#pragma unroll
        for (int o = 0; o < 5; ++o) st[o] = 0.0f;
        if (valid) {
            const int row = rows[s];
            const double inv_n = 1.0 / (double)b.N, inv_nh = NH == 1 ? inv_n : 1.0 / ((double)b.N * (double)NH);
            const float* __restrict__ old = b.old_logits + (size_t)row * NL;
            PpoHeadTerms t = ppo_head<HL::N0>(b, row, hdr, outs + s * OST, old, b.action[(size_t)row * NH], la, inv_nh, d);
            if constexpr (NH >= 2) {
                const PpoHeadTerms u = ppo_head<HL::N1>(b, row, hdr, outs + s * OST + HL::N0, old + HL::N0,
                                                        b.action[(size_t)row * NH + 1], la, inv_nh, d + HL::N0);
                t.pg = t.pg + u.pg;
                t.ent = t.ent + u.ent;
                t.kl = t.kl + u.kl;
                t.clipped = t.clipped + u.clipped;
            }
            if constexpr (NH == 3) {
                constexpr int O2 = HL::N0 + HL::N1;
                const PpoHeadTerms u = ppo_head<HL::N2>(b, row, hdr, outs + s * OST + O2, old + O2,
                                                        b.action[(size_t)row * NH + 2], la, inv_nh, d + O2);
                t.pg = t.pg + u.pg;
                t.ent = t.ent + u.ent;
                t.kl = t.kl + u.kl;
                t.clipped = t.clipped + u.clipped;
            }
            const double dv = (double)outs[s * OST + NL] - (double)b.returns[row];
            if constexpr (!VCLIP) d[NL] = (float)(((double)la.vf_coef * dv) * inv_n);  // VCLIP: stays 0 for vfix
            st[0] = (float)t.pg;
            st[1] = (float)(0.5 * dv * dv);  // VCLIP: the tile's term of U, until vfix writes the tile's v_loss
            st[2] = (float)t.ent;
            st[3] = (float)t.kl;
            st[4] = t.clipped;
        }
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            douts[s * OST + o] = d[o];
            DO[(size_t)(t0 + s) * NOUT + o] = d[o];
        }
        if constexpr (VCLIP) DO[(size_t)(t0 + s) * NOUT + NL] = valid ? outs[s * OST + NL] : 0.0f;  // d[NL] is 0
#pragma unroll
        for (int o = 0; o < 5; ++o) tsum[s * PPO_TP + o] = st[o];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) tsum[s * PPO_TP + 5 + o] = d[o];
#pragma unroll
        for (int o = 5 + NOUT; o < PPO_TP; ++o) tsum[s * PPO_TP + o] = 0.0f;
    }
    __syncthreads();
    // the tile's partial sums: a pairwise tree over the samples (s += s + half), the same order on every call
    for (int half = TS / 2; half >= 1; half >>= 1) {
        for (int i = tid; i < half * PPO_TP; i += PPO_THREADS) tsum[i] = tsum[i] + tsum[i + half * PPO_TP];
        __syncthreads();
    }
    if (tid < PPO_TP) TP[(size_t)blockIdx.x * PPO_TP + tid] = tsum[tid];
    // d loss / d pre-activation = relu'(a) * sum_o w_out[j][o] * dout[o]
    float wr[4][NOUT];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 0; o < NOUT; ++o) wr[k][o] = wo[(4 * jq + k) * NOUT + o];
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int s = sg + R * i;
        float da[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < (VCLIP ? NL : NOUT); ++o) {  // VCLIP: vfix adds the value column's term, last as here
            const float dd = douts[s * OST + o];
#pragma unroll
            for (int k = 0; k < 4; ++k) da[k] = fmaf(wr[k][o], dd, da[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) da[k] = ((posmask >> (4 * i + k)) & 1u) ? da[k] : 0.0f;
        reinterpret_cast<float4*>(DA + (size_t)(t0 + s) * HD)[jq] = make_float4(da[0], da[1], da[2], da[3]);
    }
}

// ------------------------------------------------------------------ vsum, vcount, vfix: the clipped value loss (gca.h)
// One sample's terms of the clipped value loss, in double from the f32 value v, return R and recorded value vo; U is
// the minibatch's f32 scalar, compared as (double)U. vcount and vfix call this one function on the same words, so they
// take the same side of both kinks.
struct PpoVTerms {
    double dvr, dcr, q;  // v - R, vc - R, (vc - R)^2
    bool in, u;          // |v - vo| <= c; U >= q
};

__device__ __forceinline__ PpoVTerms ppo_vterms(float v, float R, float vo, float clip_coef, float U) {
    PpoVTerms t;
    const double c = (double)clip_coef, diff = (double)v - (double)vo;
    t.in = fabs(diff) <= c;
    const double vc = (double)vo + fmin(fmax(diff, -c), c);
    t.dvr = (double)v - (double)R;
    t.dcr = vc - (double)R;
    t.q = t.dcr * t.dcr;
    t.u = (double)U >= t.q;
    return t;
}

__device__ __forceinline__ int ppo_block_count(int v, int* red, int tid) {
    __syncthreads();  // the previous use of red
    red[tid] = v;
    __syncthreads();
    for (int s = PPO_ADV_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// header words of the _vclip calls: [2] U f32, [3] n_U i32, [4] the samples outside the clip i32
constexpr int PPO_HDR_U = 2, PPO_HDR_NU = 3, PPO_HDR_NCLIP = 4;
constexpr int PPO_VCOUNT_THREADS = 64;  // one wave: a tile has at most 64 samples

// vsum, one workgroup, over the tile partials (a sequential partial per thread over tiles t, t + 1024, .., then a tree,
// as adv sums). COUNTS = false: U = (the sum of slot sa, fwd's tile sums of f32(0.5 (v_s - R_s)^2)) * (1 / N) -> header.
// COUNTS = true: the integer sums of slots sa (n_U) and sb (the samples outside the clip), vcount's -> header, vstats.
template <bool COUNTS>
__global__ __launch_bounds__(PPO_ADV_THREADS) void ppo_vsum_kernel(const float* __restrict__ TP, int tp, int64_t ntiles,
                                                                   int sa, int sb, float inv_n, int N,
                                                                   float* __restrict__ hdr,
                                                                   float* __restrict__ vstats) {
    __shared__ float red[PPO_ADV_THREADS];
    const int tid = threadIdx.x;
    if constexpr (!COUNTS) {
        float s = 0.0f;
        for (int64_t t = tid; t < ntiles; t += PPO_ADV_THREADS) s = s + TP[(size_t)t * tp + sa];
        const float sum = ppo_block_sum(s, red, tid);
        if (tid == 0) hdr[PPO_HDR_U] = sum * inv_n;
    } else {
        const int* __restrict__ TPi = reinterpret_cast<const int*>(TP);
        int nu = 0, nc = 0;
        for (int64_t t = tid; t < ntiles; t += PPO_ADV_THREADS) {
            nu += TPi[(size_t)t * tp + sa];
            nc += TPi[(size_t)t * tp + sb];
        }
        nu = ppo_block_count(nu, reinterpret_cast<int*>(red), tid);
        nc = ppo_block_count(nc, reinterpret_cast<int*>(red), tid);
        if (tid == 0) {
            reinterpret_cast<int*>(hdr)[PPO_HDR_NU] = nu;
            reinterpret_cast<int*>(hdr)[PPO_HDR_NCLIP] = nc;
            if (vstats) {
                vstats[0] = hdr[PPO_HDR_U];
                vstats[1] = (float)((double)nu / (double)N);
                vstats[2] = (float)((double)nc / (double)N);
            }
        }
    }
}

// vcount, one wave per tile of fwd's: the tile's samples with U >= q_s and those outside the clip, counted as integers
// (a ballot) into the tile partial's v_loss and b2[value] slots, which vfix overwrites after vsum has read them.
template <int TS, int NOUT, int TPF>
__global__ __launch_bounds__(PPO_VCOUNT_THREADS) void ppo_vcount_kernel(PpoBatch b, const float* __restrict__ old_value,
                                                                        float clip_coef, const float* __restrict__ hdr,
                                                                        const float* __restrict__ DO,
                                                                        float* __restrict__ TP) {
    static_assert(TS <= PPO_VCOUNT_THREADS, "a thread per sample of the tile");
    const int s = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * TS + s;
    bool u = false, out = false;
    if (s < TS && t < b.N) {
        const int row = ppo_row(b, (int)t);
        const PpoVTerms vt = ppo_vterms(DO[(size_t)t * NOUT + NOUT - 1], b.returns[row], old_value[row], clip_coef,
                                        hdr[PPO_HDR_U]);
        u = vt.u;
        out = !vt.in;
    }
    const int nu = __popcll(__ballot(u)), nc = __popcll(__ballot(out));
    if (s == 0) {
        int* tp = reinterpret_cast<int*>(TP + (size_t)blockIdx.x * TPF);
        tp[1] = nu;
        tp[5 + NOUT - 1] = nc;
    }
}

// vfix, one workgroup per tile of fwd's: d loss / d v_s replaces v_s in DO, its term is added to da (last, as the plain
// fwd adds it), and the tile partial's v_loss and b2[value] sums are formed in fwd's pairwise tree over the samples.
template <int HD, class HL>
__global__ __launch_bounds__(PPO_THREADS) void ppo_vfix_kernel(PpoBatch b, const float* __restrict__ old_value,
                                                               const float* __restrict__ w_out, PpoLossArgs la,
                                                               const float* __restrict__ hdr, float* __restrict__ DA,
                                                               const float* __restrict__ H, float* __restrict__ DO,
                                                               float* __restrict__ TP) {
    using Cf = PpoCfg<HD>;
    constexpr int TS = Cf::TS, Q = Cf::Q, R = Cf::R, SPT = Cf::SPT;
    constexpr int NOUT = HL::NOUT, NL = HL::NL, PPO_TP = HL::TP;
    __shared__ float dvs[TS], tsum[TS * 2];
    const int tid = threadIdx.x, jq = tid % Q, sg = tid / Q;
    const int64_t t0 = (int64_t)blockIdx.x * TS;
    if (tid < TS) {
        const int s = tid;
        float d = 0.0f, vl = 0.0f;
        if (t0 + s < b.N) {
            const int row = ppo_row(b, (int)(t0 + s));
            const float U = hdr[PPO_HDR_U];
            const double n = (double)b.N, share = (double)reinterpret_cast<const int*>(hdr)[PPO_HDR_NU] / n;
            const PpoVTerms vt = ppo_vterms(DO[(size_t)(t0 + s) * NOUT + NL], b.returns[row], old_value[row],
                                            la.clip_coef, U);
            const double own = (!vt.u && vt.in) ? 2.0 * vt.dcr : 0.0;
            d = (float)(((double)la.vf_coef * (0.5 / n)) * (share * vt.dvr + own));
            vl = (float)(0.5 * (vt.u ? (double)U : vt.q));
        }
        dvs[s] = d;
        DO[(size_t)(t0 + s) * NOUT + NL] = d;
        tsum[2 * s] = vl;
        tsum[2 * s + 1] = d;
    }
    __syncthreads();
    for (int half = TS / 2; half >= 1; half >>= 1) {
        if (tid < half * 2) tsum[tid] = tsum[tid] + tsum[tid + half * 2];
        __syncthreads();
    }
    if (tid == 0) {
        TP[(size_t)blockIdx.x * PPO_TP + 1] = tsum[0];
        TP[(size_t)blockIdx.x * PPO_TP + 5 + NL] = tsum[1];
    }
    float wv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) wv[k] = w_out[(4 * jq + k) * NOUT + NL];
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int s = sg + R * i;
        const float dd = dvs[s];
        const float4 h = reinterpret_cast<const float4*>(H + (size_t)(t0 + s) * HD)[jq];
        float4* const dst = reinterpret_cast<float4*>(DA + (size_t)(t0 + s) * HD) + jq;
        float4 da = *dst;
        da.x = h.x > 0.0f ? fmaf(wv[0], dd, da.x) : da.x;
        da.y = h.y > 0.0f ? fmaf(wv[1], dd, da.y) : da.y;
        da.z = h.z > 0.0f ? fmaf(wv[2], dd, da.z) : da.z;
        da.w = h.w > 0.0f ? fmaf(wv[3], dd, da.w) : da.w;
        *dst = da;
    }
}

// ------------------------------------------------------------------ wgrad: partial weight gradients
template <int HD, int NOUT>
__global__ __launch_bounds__(PPO_THREADS) void ppo_wgrad_kernel(PpoBatch b, PpoPlan pl, const float* __restrict__ DA,
                                                                const float* __restrict__ H,
                                                                const float* __restrict__ DO,
                                                                float* __restrict__ part) {
    using Cf = PpoCfg<HD>;
    constexpr int TS = Cf::TS, Q = Cf::Q, R = Cf::R;
    __shared__ __attribute__((aligned(16))) float dt[TS * HD];
    __shared__ uint32_t xt[TS * R];
    const int tid = threadIdx.x, jq = tid % Q, rl = tid / Q;
    const int blk = blockIdx.x, SS = b.SS, C = b.C;
    // kind 0: window cells (x = class), 1: coarse rows and b1 (x = coarse value / 1), 2: w_out columns (x = dout, D = h)
    const int kind = blk < pl.nbL ? 0 : (blk < pl.nbL + pl.nbC ? 1 : 2);
    const int r0 = (kind == 0 ? blk : kind == 1 ? blk - pl.nbL : blk - pl.nbL - pl.nbC) * R;
    const int nrows = kind == 0 ? SS : kind == 1 ? C + 1 : NOUT;
    const float* __restrict__ D = kind == 2 ? H : DA;
    const int64_t tile0 = (int64_t)blockIdx.y * pl.tps;
    const int64_t tile1 = min(tile0 + pl.tps, pl.ntiles);
    float4 tot[4], acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t t0 = tile * TS;
        const float4* __restrict__ src = reinterpret_cast<const float4*>(D + (size_t)t0 * HD);
        for (int i = tid; i < TS * Q; i += PPO_THREADS) reinterpret_cast<float4*>(dt)[i] = src[i];
        for (int i = tid; i < TS * R; i += PPO_THREADS) {
            const int s = i / R, r = r0 + i % R;
            uint32_t x = 0u;  // a row past the block's last, or a sample past N (its D row is zero)
            if (r < nrows && t0 + s < b.N) {
                if (kind == 2) {
                    x = __float_as_uint(DO[(size_t)(t0 + s) * NOUT + r]);
                } else {
                    const int row = ppo_row(b, (int)(t0 + s));
                    if (kind == 0) x = b.local[(size_t)row * SS + r] & 3u;
                    else x = r < C ? __float_as_uint(b.coarse[(size_t)row * C + r]) : __float_as_uint(1.0f);
                }
            }
            xt[i] = x;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (kind == 0) {
#pragma unroll 4
            for (int s = 0; s < TS; ++s) {
                const float4 d = reinterpret_cast<const float4*>(dt)[s * Q + jq];
                const uint32_t c = xt[s * R + rl];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool on = c == (uint32_t)k;  // a select, not a 0 / 1 factor: 0 * Inf would be NaN
                    acc[k].x += on ? d.x : 0.0f;
                    acc[k].y += on ? d.y : 0.0f;
                    acc[k].z += on ? d.z : 0.0f;
                    acc[k].w += on ? d.w : 0.0f;
                }
            }
        } else {
#pragma unroll 4
            for (int s = 0; s < TS; ++s) {
                const float4 d = reinterpret_cast<const float4*>(dt)[s * Q + jq];
                const float x = __uint_as_float(xt[s * R + rl]);
                acc[0].x = fmaf(x, d.x, acc[0].x);
                acc[0].y = fmaf(x, d.y, acc[0].y);
                acc[0].z = fmaf(x, d.z, acc[0].z);
                acc[0].w = fmaf(x, d.w, acc[0].w);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tot[k].x += acc[k].x;
            tot[k].y += acc[k].y;
            tot[k].z += acc[k].z;
            tot[k].w += acc[k].w;
        }
        __syncthreads();
    }
    const int r = r0 + rl;
    if (r >= nrows) return;
    float* __restrict__ out = part + (size_t)blockIdx.y * pl.GF;
    if (kind == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<float4*>(out + pl.off_wl + ((size_t)r * 4 + k) * HD)[jq] = tot[k];
    } else if (kind == 1) {
        // row C of this kind is b1, which follows w_coarse in the partial
        reinterpret_cast<float4*>(out + pl.off_wc + (size_t)r * HD)[jq] = tot[0];
    } else {
        float* o = out + pl.off_wo + (size_t)(4 * jq) * NOUT + r;
        o[0] = tot[0].x;
        o[NOUT] = tot[0].y;
        o[2 * NOUT] = tot[0].z;
        o[3 * NOUT] = tot[0].w;
    }
}

// ------------------------------------------------------------------ reduce: the partials, g_b2 and the stats
struct PpoOut {
    float *g_w_local, *g_w_coarse, *g_b1, *g_w_out, *g_b2, *stats;
};

template <int NOUT, int NH>
__global__ __launch_bounds__(PPO_THREADS) void ppo_reduce_kernel(PpoPlan pl, PpoLossArgs la,
                                                                 const float* __restrict__ part,
                                                                 const float* __restrict__ TP,
                                                                 const float* __restrict__ hdr, PpoOut out,
                                                                 int elem_blocks) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < elem_blocks) {
        const int64_t e = (int64_t)blockIdx.x * PPO_THREADS + tid;
        if (e >= pl.GF) return;
        float s = 0.0f;
        for (int p = 0; p < pl.P; ++p) s = s + part[(size_t)p * pl.GF + e];
        if (e < pl.off_wc) out.g_w_local[e] = s;
        else if (e < pl.off_b1) out.g_w_coarse[e - pl.off_wc] = s;
        else if (e < pl.off_wo) out.g_b1[e - pl.off_b1] = s;
        else out.g_w_out[e - pl.off_wo] = s;
        return;
    }
    constexpr int PPO_TP = ppo_tp(NOUT), USED = 5 + NOUT;
    __shared__ float red[PPO_THREADS * PPO_TP];
    float s[PPO_TP];
#pragma unroll
    for (int q = 0; q < PPO_TP; ++q) s[q] = 0.0f;
    for (int64_t t = tid; t < pl.ntiles; t += PPO_THREADS) {
#pragma unroll
        for (int q = 0; q < USED; ++q) s[q] = s[q] + TP[(size_t)t * PPO_TP + q];
    }
#pragma unroll
    for (int q = 0; q < PPO_TP; ++q) red[tid * PPO_TP + q] = s[q];
    __syncthreads();
    for (int st = PPO_THREADS / 2; st >= 1; st >>= 1) {
        if (tid < st)
            for (int q = 0; q < USED; ++q) red[tid * PPO_TP + q] = red[tid * PPO_TP + q] + red[(tid + st) * PPO_TP + q];
        __syncthreads();
    }
    if (tid < NOUT) out.g_b2[tid] = red[5 + tid];
    if (tid == 0) {
        // pg, the entropy, approx_kl and the clip fraction are means over the N * NH (sample, head) pairs (1 / NH is
        // exact for one and two heads, one rounded division for three), the value loss over the N samples
        const float inv_nh = NH == 1 ? la.inv_n : la.inv_n / (float)NH;
        const float pg = red[0] * inv_nh, vl = red[1] * la.inv_n, ent = red[2] * inv_nh;
        out.stats[0] = (pg - la.ent_coef * ent) + la.vf_coef * vl;
        out.stats[1] = pg;
        out.stats[2] = vl;
        out.stats[3] = ent;
        out.stats[4] = red[3] * inv_nh;
        out.stats[5] = red[4] * inv_nh;
        out.stats[6] = hdr[0];
        out.stats[7] = hdr[1];
    }
}

// ------------------------------------------------------------------ host side
using PpoHeli = PpoHeads<9, 0>;
using PpoBdz = PpoHeads<9, 2>;
using PpoExt = PpoHeads<9, 2, 3>;

static int64_t ppo_workspace(const GcaGradAgent& ag, const gca_policy* p, int C, int N) {
    if (gca_check_policy_grad_workspace(ag, p, C, N)) return -1;
    const int S = 2 * p->radius + 1;
    return ppo_plan(S * S, C, p->hidden, N, ag.nout).bytes;
}

extern "C" int64_t gca_helicopter_policy_grad_workspace(const gca_heli_policy* p, int C, int N) {
    return ppo_workspace(GCA_GRAD_HELI, p, C, N);
}

extern "C" int64_t gca_bulldozer_policy_grad_workspace(const gca_bulldozer_policy* p, int C, int N) {
    return ppo_workspace(GCA_GRAD_BDZ, p, C, N);
}

extern "C" int64_t gca_extension_policy_grad_workspace(const gca_bulldozer_policy* p, int C, int N) {
    return ppo_workspace(GCA_GRAD_EXT, p, C, N);
}

template <int HD, class HL, bool VCLIP>
static void ppo_launch(const PpoBatch& b, const PpoPlan& pl, const gca_policy* p, const PpoLossArgs& la,
                       const PpoOut& out, const float* old_value, float* vstats, char* ws, hipStream_t st) {
    float* hdr = reinterpret_cast<float*>(ws);
    float* DA = reinterpret_cast<float*>(ws + pl.off_da);
    float* H = reinterpret_cast<float*>(ws + pl.off_h);
    float* DO = reinterpret_cast<float*>(ws + pl.off_do);
    float* TP = reinterpret_cast<float*>(ws + pl.off_tp);
    float* part = reinterpret_cast<float*>(ws + pl.off_part);
    hipLaunchKernelGGL(ppo_adv_kernel, dim3(1), dim3(PPO_ADV_THREADS), 0, st, b, hdr);
    hipLaunchKernelGGL((ppo_fwd_kernel<HD, HL, VCLIP>), dim3((unsigned)pl.ntiles), dim3(PPO_THREADS), 0, st, b,
                       p->w_local, p->w_coarse, p->b1, p->w_out, p->b2, la, hdr, DA, H, DO, TP);
    if constexpr (VCLIP) {
        using Cf = PpoCfg<HD>;
        hipLaunchKernelGGL(ppo_vsum_kernel<false>, dim3(1), dim3(PPO_ADV_THREADS), 0, st, TP, (int)HL::TP, pl.ntiles, 1,
                           5 + HL::NL, la.inv_n, b.N, hdr, vstats);
        hipLaunchKernelGGL((ppo_vcount_kernel<Cf::TS, HL::NOUT, HL::TP>), dim3((unsigned)pl.ntiles),
                           dim3(PPO_VCOUNT_THREADS), 0, st, b, old_value, la.clip_coef, hdr, DO, TP);
        hipLaunchKernelGGL(ppo_vsum_kernel<true>, dim3(1), dim3(PPO_ADV_THREADS), 0, st, TP, (int)HL::TP, pl.ntiles, 1,
                           5 + HL::NL, la.inv_n, b.N, hdr, vstats);
        hipLaunchKernelGGL((ppo_vfix_kernel<HD, HL>), dim3((unsigned)pl.ntiles), dim3(PPO_THREADS), 0, st, b, old_value,
                           p->w_out, la, hdr, DA, H, DO, TP);
    }
    hipLaunchKernelGGL((ppo_wgrad_kernel<HD, HL::NOUT>), dim3((unsigned)pl.nb, (unsigned)pl.P), dim3(PPO_THREADS), 0,
                       st, b, pl, DA, H, DO, part);
    const int elem_blocks = (int)((pl.GF + PPO_THREADS - 1) / PPO_THREADS);
    hipLaunchKernelGGL((ppo_reduce_kernel<HL::NOUT, HL::NH>), dim3((unsigned)elem_blocks + 1), dim3(PPO_THREADS), 0, st,
                       pl, la, part, TP, hdr, out, elem_blocks);
}

// the body of the four entry points: the shared checks, then the launches of the agent's head layout (four; eight with
// VCLIP, where old_value and vstats are the _vclip entries' two further arguments)
template <class HL, bool VCLIP>
static int ppo_policy_grad(const GcaGradAgent& ag, const gca_policy* p, int C, const uint8_t* local,
                           const float* coarse, const int32_t* action, const float* old_logits, const float* old_value,
                           const float* advantage, const float* returns, int64_t T, const int32_t* idx, int N,
                           float clip_coef, float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                           float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                           void* workspace, int64_t workspace_bytes, void* stream) {
    static_assert(HL::NOUT == 10 || HL::NOUT == 12 || HL::NOUT == 15, "the agents' outputs (GcaGradAgent::nout)");
    PpoPlan pl;
    if constexpr (VCLIP) {
        if (const int st = gca_check_policy_grad_vclip(ag, p, C, local, coarse, action, old_logits, old_value, advantage,
                                                       returns, T, idx, N, clip_coef, g_w_local, g_w_coarse, g_b1,
                                                       g_w_out, g_b2, stats, vstats, workspace, workspace_bytes, &pl))
            return st;
    } else {
        if (const int st = gca_check_policy_grad(ag, p, C, local, coarse, action, old_logits, advantage, returns, T, idx,
                                                 N, clip_coef, g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats,
                                                 workspace, workspace_bytes, &pl))
            return st;
    }
    const int S = 2 * p->radius + 1, SS = S * S, Hd = p->hidden;
    PpoBatch b{local, coarse, action, old_logits, advantage, returns, idx, N, (int)T, SS, C};
    const PpoLossArgs la{clip_coef, ent_coef, vf_coef, 1.0f / (float)N, norm_adv ? 1 : 0};
    const PpoOut out{g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats};
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    switch (Hd) {
        case 32: ppo_launch<32, HL, VCLIP>(b, pl, p, la, out, old_value, vstats, ws, st); break;
        case 64: ppo_launch<64, HL, VCLIP>(b, pl, p, la, out, old_value, vstats, ws, st); break;
        case 128: ppo_launch<128, HL, VCLIP>(b, pl, p, la, out, old_value, vstats, ws, st); break;
        default: ppo_launch<256, HL, VCLIP>(b, pl, p, la, out, old_value, vstats, ws, st); break;
    }
    GCA_CHECK_LAUNCH(ag.who);
    return GCA_OK;
}

extern "C" int gca_helicopter_policy_grad(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                                          const int32_t* action, const float* old_logits, const float* advantage,
                                          const float* returns, int64_t T, const int32_t* idx, int N, float clip_coef,
                                          float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                                          float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
    return ppo_policy_grad<PpoHeli, false>(GCA_GRAD_HELI, p, C, local, coarse, action, old_logits, nullptr, advantage,
                                           returns, T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local,
                                           g_w_coarse, g_b1, g_w_out, g_b2, stats, nullptr, workspace, workspace_bytes,
                                           stream);
}

extern "C" int gca_bulldozer_policy_grad(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                         const float* coarse, const int32_t* action, const float* old_logits,
                                         const float* advantage, const float* returns, int64_t T, const int32_t* idx,
                                         int N, float clip_coef, float ent_coef, float vf_coef, int norm_adv,
                                         float* g_w_local, float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2,
                                         float* stats, void* workspace, int64_t workspace_bytes, void* stream) {
    return ppo_policy_grad<PpoBdz, false>(GCA_GRAD_BDZ, p, C, local, coarse, action, old_logits, nullptr, advantage,
                                          returns, T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local,
                                          g_w_coarse, g_b1, g_w_out, g_b2, stats, nullptr, workspace, workspace_bytes,
                                          stream);
}

extern "C" int gca_helicopter_policy_grad_vclip(const gca_heli_policy* p, int C, const uint8_t* local,
                                                const float* coarse, const int32_t* action, const float* old_logits,
                                                const float* old_value, const float* advantage, const float* returns,
                                                int64_t T, const int32_t* idx, int N, float clip_coef, float ent_coef,
                                                float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                                                float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                                                void* workspace, int64_t workspace_bytes, void* stream) {
    return ppo_policy_grad<PpoHeli, true>(GCA_GRAD_HELI_VCLIP, p, C, local, coarse, action, old_logits, old_value,
                                          advantage, returns, T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv,
                                          g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats, vstats, workspace,
                                          workspace_bytes, stream);
}

extern "C" int gca_bulldozer_policy_grad_vclip(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                               const float* coarse, const int32_t* action, const float* old_logits,
                                               const float* old_value, const float* advantage, const float* returns,
                                               int64_t T, const int32_t* idx, int N, float clip_coef, float ent_coef,
                                               float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                                               float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
    return ppo_policy_grad<PpoBdz, true>(GCA_GRAD_BDZ_VCLIP, p, C, local, coarse, action, old_logits, old_value,
                                         advantage, returns, T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv,
                                         g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats, vstats, workspace,
                                         workspace_bytes, stream);
}

extern "C" int gca_extension_policy_grad(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                         const float* coarse, const int32_t* action, const float* old_logits,
                                         const float* advantage, const float* returns, int64_t T, const int32_t* idx,
                                         int N, float clip_coef, float ent_coef, float vf_coef, int norm_adv,
                                         float* g_w_local, float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2,
                                         float* stats, void* workspace, int64_t workspace_bytes, void* stream) {
    return ppo_policy_grad<PpoExt, false>(GCA_GRAD_EXT, p, C, local, coarse, action, old_logits, nullptr, advantage,
                                          returns, T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local,
                                          g_w_coarse, g_b1, g_w_out, g_b2, stats, nullptr, workspace, workspace_bytes,
                                          stream);
}

extern "C" int gca_extension_policy_grad_vclip(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                               const float* coarse, const int32_t* action, const float* old_logits,
                                               const float* old_value, const float* advantage, const float* returns,
                                               int64_t T, const int32_t* idx, int N, float clip_coef, float ent_coef,
                                               float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                                               float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
    return ppo_policy_grad<PpoExt, true>(GCA_GRAD_EXT_VCLIP, p, C, local, coarse, action, old_logits, old_value,
                                         advantage, returns, T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv,
                                         g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats, vstats, workspace,
                                         workspace_bytes, stream);
}
