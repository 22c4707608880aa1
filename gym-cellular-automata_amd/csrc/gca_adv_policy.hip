// gca_adv_policy.hip — the bulldozer agent on the Advanced (Alexandridis) bulldozer env: observe and act in ONE launch
// (gca_advanced_policy_act, gca.h "advanced policy").
//
// The Advanced env keeps one plane per env (no parity), its step counter as i32 time_step and no episode counter, so
// neither gca_policy_observation + gca_bulldozer_policy_act nor the Windy rollout's kernel fit it as they are. This
// kernel is the pair of them with the observation kept on chip: one 256-thread workgroup per env builds the env's
// coarse map straight into the network's LDS words (cs), reads the window from the plane in global memory and runs
// policy_outputs / bdz_policy_sample (gca_policy_dev.h), the very device functions of the act kernels. The coarse map
// never round-trips through HBM and the pair's second launch is gone; the results are the pair's bit for bit: the
// counts are integers, the scale 1 / block^2 a power of two, and the network's order is policy_outputs'.
//
// Three forms of the coarse part (the template parameter), all giving gca_policy_observation's values:
//   NW = 1, 2  the rows form (W = 256 NW, block 8 / 16 / 32, H % block == 0, an 8-B aligned plane): wave w takes the
//              strips w, w + 4, ... of 32 rows through policy_obs_rows_strip (gca_policy_obs_dev.h), the observation
//              kernel's own strip code, as bulldozer_policy_rollout_kernel's recount does.
//   NW = 0     the generic form for every other shape: thread t takes tiles t, t + 256, ... with
//              policy_obs_generic_kernel's byte loops.
//
// Barriers. The kernel has the four of policy_outputs and no other:
//   A  (the evaluation's first) every thread's stores of cs -- a strip's tiles by the first lane of each tile's lanes,
//      a generic tile by its thread; each word of cs[0 .. C) has exactly one writer -- before any thread's coarse terms
//      read them. The window needs no ordering: it is read from the plane, which nothing writes during the launch.
//   B  ends the reads of cs: the records (record(), between A and B) copy cs and the window's classes out while the
//      observation is stable. Nothing writes cs after A, so B matters only to part (gca_policy_dev.h).
//   C, D  the network's. One evaluation per launch: no LDS word is reused.
// No env state is written, no scratch, no atomics; a launch is a function of its inputs: capturable.
#include "gca_common.h"
#include "gca_policy_dev.h"      // the policy network and the bulldozer's sampler
#include "gca_policy_obs_dev.h"  // the coarse map's rows-form strip

struct AdvPolArgs {
    PolicyW w;
    int H, W, B, lgB, Hc, Wc, radius;
    float inv;  // 1 / block^2
    uint32_t tree, fire;
    int env_offset, action_stride;
};

template <int NW>
__global__ __launch_bounds__(POL_VT) void advanced_policy_act_kernel(
    AdvPolArgs q, const uint8_t* __restrict__ planes, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ time_step, int32_t* __restrict__ action, float* __restrict__ logits,
    float* __restrict__ value, uint8_t* __restrict__ local_out, float* __restrict__ coarse_out) {
    extern __shared__ __attribute__((aligned(16))) float apol_lds[];
    const int e = blockIdx.x, tid = threadIdx.x;
    float* cs = apol_lds;
    float* part = cs + ((q.w.C + 3) & ~3);
    float* hs = part + POL_PART;
    float* outs = hs + POL_VT;
    const int H = q.H, W = q.W, HcWc = q.Hc * q.Wc;
    const uint8_t* __restrict__ grid = planes + (size_t)e * (size_t)H * (size_t)W;
    // ---- the coarse map into cs
    if constexpr (NW != 0) {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int strips = (H + POBS_STRIP - 1) / POBS_STRIP;
        const uint32_t Tp = rep4(q.tree), Fp = rep4(q.fire);
        for (int s = wave; s < strips; s += POL_VT / GCA_WAVE)
            policy_obs_rows_strip<NW>(grid, 4 * NW * (uint32_t)lane, lane, s, H, q.lgB, Tp, Fp,
                                      [&](int o, uint32_t nT, uint32_t nF) {
                                          cs[o] = (float)nT * q.inv;
                                          cs[HcWc + o] = (float)nF * q.inv;
                                      });
    } else {
        const int B = q.B, Wc = q.Wc;
        for (int t = tid; t < HcWc; t += POL_VT) {
            const int bi = t / Wc, bj = t - bi * Wc;
            const int r1 = min(H, bi * B + B), c1 = min(W, bj * B + B);
            int32_t cT = 0, cF = 0;
            for (int r = bi * B; r < r1; ++r)
                for (int c = bj * B; c < c1; ++c) {
                    const uint32_t v = grid[(uint32_t)r * (uint32_t)W + (uint32_t)c];
                    cT += v == q.tree;
                    cF += v == q.fire;
                }
            cs[t] = (float)cT * q.inv;
            cs[HcWc + t] = (float)cF * q.inv;
        }
    }
    // ---- the window, the network, the draw
    const uint32_t wr0 = (uint32_t)pos[2 * e] - (uint32_t)q.radius, wc0 = (uint32_t)pos[2 * e + 1] - (uint32_t)q.radius;
    auto class_at = [&](int, int i, int j) -> uint32_t {
        const uint32_t r = wr0 + (uint32_t)i, c = wc0 + (uint32_t)j;
        const bool in = r < (uint32_t)H && c < (uint32_t)W;
        const uint32_t v = grid[in ? r * (uint32_t)W + c : 0u];  // < H * W < 2^30
        return !in ? 3u : (v == q.tree ? 1u : (v == q.fire ? 2u : 0u));
    };
    const size_t SS = (size_t)q.w.SS, C = (size_t)q.w.C;
    auto record = [&]() {
        if (local_out) {
            uint8_t* lo = local_out + (size_t)e * SS;
            const int S = q.w.S;
            for (int n = tid; n < (int)SS; n += POL_VT) {
                const int i = n / S;
                lo[n] = (uint8_t)class_at(n, i, n - i * S);
            }
        }
        if (coarse_out) {
            float* co = coarse_out + (size_t)e * C;
            for (int c = tid; c < (int)C; c += POL_VT) co[c] = cs[c];
        }
    };
    float o[BDZ_POL_NOUT];
    policy_outputs<BDZ_POL_NOUT, POL_VT>(q.w, cs, part, hs, outs, tid, POL_VT,
                                         logits ? logits + (size_t)e * 11 : nullptr, value ? value + e : nullptr,
                                         class_at, record, o);
    int32_t move, shoot;
    bdz_policy_sample(o, q.w, (uint32_t)time_step[e], (uint32_t)(q.env_offset + e), 0u, move, shoot);
    if (tid == 0) {
        int32_t* a = action + (size_t)e * (size_t)q.action_stride;
        a[0] = move;
        a[1] = shoot;
    }
}

extern "C" int gca_advanced_policy_act(const gca_bulldozer_policy* policy, const uint8_t* grid, const int32_t* pos,
                                       const int32_t* time_step, int E, int H, int W, int empty, int tree, int fire,
                                       int env_offset, uint64_t policy_seed, int greedy, int32_t* action,
                                       int action_stride, float* logits, float* value, uint8_t* local_out,
                                       float* coarse_out, void* stream) {
    if (const int st = gca_check_advanced_policy_act(policy, grid, pos, time_step, E, H, W, empty, tree, fire, action,
                                                     action_stride))
        return st;
    const char* who = "advanced_policy_act";
    AdvPolArgs q;
    const int B = policy->block;
    q.H = H; q.W = W; q.B = B;
    q.Hc = (H + B - 1) / B;
    q.Wc = (W + B - 1) / B;
    const int C = 2 * q.Hc * q.Wc;  // checked: at most GCA_POLICY_C_MAX, so the LDS below is at most 64 KiB
    if (const int st = policy_view(who, policy, C, policy_seed, greedy, &q.w)) return st;
    q.lgB = 0;
    while ((1 << q.lgB) < B) ++q.lgB;
    q.radius = policy->radius;
    q.inv = 1.0f / (float)(B * B);
    q.tree = (uint32_t)tree; q.fire = (uint32_t)fire;
    q.env_offset = env_offset; q.action_stride = action_stride;
    // the rows form's 8-B loads: every other plane takes the generic form's byte loads
    const bool rows = gca_policy_obs_rows_shape(H, W, B) && ((uintptr_t)grid & 7u) == 0;
    const dim3 wgs((unsigned)E), wg(POL_VT);
    const size_t lds_bytes = (size_t)policy_lds_words(C) * 4;
    hipStream_t st = (hipStream_t)stream;
#define GCA_APOL_LAUNCH(NWV)                                                                                       \
    hipLaunchKernelGGL(advanced_policy_act_kernel<NWV>, wgs, wg, lds_bytes, st, q, grid, pos, time_step, action, \
                       logits, value, local_out, coarse_out)
    if (rows && W == 256) GCA_APOL_LAUNCH(1);
    else if (rows) GCA_APOL_LAUNCH(2);
    else GCA_APOL_LAUNCH(0);
#undef GCA_APOL_LAUNCH
    GCA_CHECK_LAUNCH(who);
    return GCA_OK;
}
