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
//
// The second half of the file is the same launch for a policy that sees the env's retardant
// (gca_advanced_policy_observation, gca_advanced_policy_act_retardant); advanced_policy_act_kernel stays as it is.
#include "gca_common.h"
#include "gca_policy_dev.h"      // the policy network and the bulldozer's sampler
#include "gca_policy_obs_dev.h"  // the coarse map's rows-form strip
#include "gca_obs_dev.h"         // the observation's cell transforms and display selection (the extension policy)

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

// ------------------------------------------------------------------ the retardant observation (gca.h "advanced policy")
// gca_advanced_policy_observation and gca_advanced_policy_act_retardant: the same launch shape with the env's retardant
// in the vector the network reads. One device function, retardant_features, writes an env's C2 words -- the two grid
// channels as advanced_policy_act_kernel counts them, the retardant share of every block, the window's retardant flags
// and the pad word -- to `dst`: the network's LDS words cs in the act kernel, the caller's feat_out in the observation
// kernel (no LDS there, so no limit on C2). Every word has one writer; nothing is read back.
//
// The retardant channel, by q.dmode:
//   2  from dous_bits by dwords (block 8 / 16 / 32, W % 32 == 0, 4-B aligned bits): item (bi, j) is dword j of the bit
//      rows of block-row bi, 32 columns = four, two or one tile. Per row one 4-B load and a SWAR popcount per byte; the
//      four byte counts are added over the block's rows in 16-bit lanes (at most 32 rows x 8 bits), then joined per tile.
//   1  from dous_bits for any other shape: a thread per tile masks the tile's bit range out of each u16 word it touches.
//   0  from the u8 layer: a thread per tile, byte loops.
// Occupancy: the act kernel's LDS is policy_lds_words(C2), half as much coarse map again as advanced_policy_act_kernel:
// 17.5 KiB against 13.1 KiB at 256 x 256, block 8, where the CU's 32 waves (eight workgroups) bind before its 160 KiB
// of LDS does; 53.5 KiB against 37.1 KiB at 512 x 512, block 8, two workgroups per CU where the parent has four.
struct AdvRetArgs {
    PolicyW w;  // the act kernel's; the observation kernel reads S and SS only
    int H, W, B, lgB, Hc, Wc, radius, dmode;
    float inv;  // 1 / block^2
    uint32_t tree, fire;
    int env_offset, action_stride;
};

// the class of window cell (i, j) of the window whose corner is (wr0, wc0): gca_policy_observation's
__device__ __forceinline__ uint32_t window_class(const uint8_t* __restrict__ grid, int H, int W, uint32_t wr0,
                                                 uint32_t wc0, int i, int j, uint32_t tree, uint32_t fire) {
    const uint32_t r = wr0 + (uint32_t)i, c = wc0 + (uint32_t)j;
    const bool in = r < (uint32_t)H && c < (uint32_t)W;
    const uint32_t v = grid[in ? r * (uint32_t)W + c : 0u];  // < H * W < 2^30
    return !in ? 3u : (v == tree ? 1u : (v == fire ? 2u : 0u));
}

template <int NW>
__device__ __forceinline__ void retardant_features(const AdvRetArgs& q, const uint8_t* __restrict__ grid,
                                                   const uint8_t* __restrict__ dous, const uint16_t* __restrict__ bits,
                                                   uint32_t wr0, uint32_t wc0, float* dst, int tid) {
    const int H = q.H, W = q.W, B = q.B, Wc = q.Wc, HcWc = q.Hc * q.Wc;
    // ---- channels 0 and 1: the grid's TREE and FIRE shares, as advanced_policy_act_kernel counts them
    if constexpr (NW != 0) {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int strips = (H + POBS_STRIP - 1) / POBS_STRIP;
        const uint32_t Tp = rep4(q.tree), Fp = rep4(q.fire);
        for (int s = wave; s < strips; s += POL_VT / GCA_WAVE)
            policy_obs_rows_strip<NW>(grid, 4 * NW * (uint32_t)lane, lane, s, H, q.lgB, Tp, Fp,
                                      [&](int o, uint32_t nT, uint32_t nF) {
                                          dst[o] = (float)nT * q.inv;
                                          dst[HcWc + o] = (float)nF * q.inv;
                                      });
    } else {
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
            dst[t] = (float)cT * q.inv;
            dst[HcWc + t] = (float)cF * q.inv;
        }
    }
    // ---- channel 2: the retardant share of every block
    float* dd = dst + 2 * HcWc;
    if (q.dmode == 2) {
        const int wpr = W >> 5;  // dwords of a bit row; W % 32 == 0, so Wc = wpr << (5 - lgB)
        const uint32_t* __restrict__ b32 = reinterpret_cast<const uint32_t*>(bits);
        for (int it = tid; it < q.Hc * wpr; it += POL_VT) {
            const int bi = it / wpr, j = it - bi * wpr;
            const int r1 = min(H, bi * B + B);
            uint32_t lo = 0u, hi = 0u;  // bytes 0, 2 and bytes 1, 3 of the dword, a 16-bit count each
            for (int r = bi * B; r < r1; ++r) {
                uint32_t x = b32[(uint32_t)r * (uint32_t)wpr + (uint32_t)j];  // < H * W / 32
                x = x - ((x >> 1) & 0x55555555u);
                x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
                x = (x + (x >> 4)) & 0x0F0F0F0Fu;  // the popcount of every byte
                lo += x & 0x00FF00FFu;
                hi += (x >> 8) & 0x00FF00FFu;
            }
            const uint32_t n0 = lo & 0xFFFFu, n1 = hi & 0xFFFFu, n2 = lo >> 16, n3 = hi >> 16;  // columns 8 k .. 8 k + 7
            float* o = dd + bi * Wc + (j << (5 - q.lgB));
            if (q.lgB == 3) {
                o[0] = (float)n0 * q.inv;
                o[1] = (float)n1 * q.inv;
                o[2] = (float)n2 * q.inv;
                o[3] = (float)n3 * q.inv;
            } else if (q.lgB == 4) {
                o[0] = (float)(n0 + n1) * q.inv;
                o[1] = (float)(n2 + n3) * q.inv;
            } else {
                o[0] = (float)(n0 + n1 + n2 + n3) * q.inv;
            }
        }
    } else {
        const int wpr = W >> 4;  // u16 words of a bit row (dmode 1: W % 16 == 0)
        for (int t = tid; t < HcWc; t += POL_VT) {
            const int bi = t / Wc, bj = t - bi * Wc;
            const int r1 = min(H, bi * B + B), c0 = bj * B, c1 = min(W, c0 + B);
            int32_t cD = 0;
            if (q.dmode == 1) {
                for (int r = bi * B; r < r1; ++r)
                    for (int wd = c0 >> 4; wd <= (c1 - 1) >> 4; ++wd) {
                        const int b0 = max(c0 - 16 * wd, 0), b1 = min(c1 - 16 * wd, 16);  // the tile's bits [b0, b1)
                        const uint32_t mask = ((1u << b1) - 1u) & ~((1u << b0) - 1u);
                        cD += __popc((uint32_t)bits[(uint32_t)r * (uint32_t)wpr + (uint32_t)wd] & mask);
                    }
            } else {
                for (int r = bi * B; r < r1; ++r)
                    for (int c = c0; c < c1; ++c) cD += dous[(uint32_t)r * (uint32_t)W + (uint32_t)c] != 0;
            }
            dd[t] = (float)cD * q.inv;
        }
    }
    // ---- the window's retardant flags and the pad word
    const int S = q.w.S, SS = q.w.SS;
    float* dw = dst + 3 * HcWc;
    for (int n = tid; n < SS; n += POL_VT) {
        const int i = n / S;
        const uint32_t r = wr0 + (uint32_t)i, c = wc0 + (uint32_t)(n - i * S);
        const bool in = r < (uint32_t)H && c < (uint32_t)W;
        const uint32_t cell = in ? r * (uint32_t)W + c : 0u;
        const bool d = q.dmode ? ((bits[cell >> 4] >> (cell & 15u)) & 1u) != 0 : dous[cell] != 0;
        dw[n] = in && d ? 1.0f : 0.0f;
    }
    if (tid == 0 && ((3 * HcWc + SS) & 1)) dw[SS] = 0.0f;
}

template <int NW>
__global__ __launch_bounds__(POL_VT) void advanced_retardant_obs_kernel(
    AdvRetArgs q, const uint8_t* __restrict__ planes, const uint8_t* __restrict__ dousing,
    const uint16_t* __restrict__ dous_bits, const int32_t* __restrict__ pos, uint8_t* __restrict__ local_out,
    float* __restrict__ feat_out, int C2) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const size_t HW = (size_t)q.H * (size_t)q.W;
    const uint8_t* __restrict__ grid = planes + (size_t)e * HW;
    const uint32_t wr0 = (uint32_t)pos[2 * e] - (uint32_t)q.radius, wc0 = (uint32_t)pos[2 * e + 1] - (uint32_t)q.radius;
    if (feat_out)
        retardant_features<NW>(q, grid, dousing + (size_t)e * HW, dous_bits ? dous_bits + (size_t)e * (HW >> 4) : nullptr,
                               wr0, wc0, feat_out + (size_t)e * (size_t)C2, tid);
    if (local_out) {
        uint8_t* lo = local_out + (size_t)e * (size_t)q.w.SS;
        const int S = q.w.S;
        for (int n = tid; n < q.w.SS; n += POL_VT) {
            const int i = n / S;
            lo[n] = (uint8_t)window_class(grid, q.H, q.W, wr0, wc0, i, n - i * S, q.tree, q.fire);
        }
    }
}

// Barriers: the four of policy_outputs and no other, as in advanced_policy_act_kernel. A orders every thread's stores of
// cs[0 .. C2) -- retardant_features', one writer per word -- before the coarse terms read them; record() copies cs out
// between A and B.
template <int NW>
__global__ __launch_bounds__(POL_VT) void advanced_policy_act_retardant_kernel(
    AdvRetArgs q, const uint8_t* __restrict__ planes, const uint8_t* __restrict__ dousing,
    const uint16_t* __restrict__ dous_bits, const int32_t* __restrict__ pos, const int32_t* __restrict__ time_step,
    int32_t* __restrict__ action, float* __restrict__ logits, float* __restrict__ value,
    uint8_t* __restrict__ local_out, float* __restrict__ feat_out) {
    extern __shared__ __attribute__((aligned(16))) float aret_lds[];
    const int e = blockIdx.x, tid = threadIdx.x;
    float* cs = aret_lds;
    float* part = cs + ((q.w.C + 3) & ~3);
    float* hs = part + POL_PART;
    float* outs = hs + POL_VT;
    const int H = q.H, W = q.W;
    const size_t HW = (size_t)H * (size_t)W;
    const uint8_t* __restrict__ grid = planes + (size_t)e * HW;
    const uint32_t wr0 = (uint32_t)pos[2 * e] - (uint32_t)q.radius, wc0 = (uint32_t)pos[2 * e + 1] - (uint32_t)q.radius;
    retardant_features<NW>(q, grid, dousing + (size_t)e * HW, dous_bits ? dous_bits + (size_t)e * (HW >> 4) : nullptr,
                           wr0, wc0, cs, tid);
    auto class_at = [&](int, int i, int j) -> uint32_t {
        return window_class(grid, H, W, wr0, wc0, i, j, q.tree, q.fire);
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
        if (feat_out) {
            float* fo = feat_out + (size_t)e * C;
            for (int c = tid; c < (int)C; c += POL_VT) fo[c] = cs[c];
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

// the shape's part of the launch arguments; *rows: the grid's channels take the rows form
static void retardant_args(AdvRetArgs* q, const uint8_t* grid, const uint16_t* dous_bits, int H, int W, int B,
                           int radius, int tree, int fire, bool* rows) {
    q->H = H; q->W = W; q->B = B;
    q->Hc = (H + B - 1) / B;
    q->Wc = (W + B - 1) / B;
    q->lgB = 0;
    while ((1 << q->lgB) < B) ++q->lgB;
    q->radius = radius;
    q->inv = 1.0f / (float)(B * B);
    q->tree = (uint32_t)tree; q->fire = (uint32_t)fire;
    q->env_offset = 0; q->action_stride = 2;
    const bool dwords = (B == 8 || B == 16 || B == 32) && W % 32 == 0 && ((uintptr_t)dous_bits & 3u) == 0;
    q->dmode = !dous_bits ? 0 : (dwords ? 2 : 1);
    // the rows form's 8-B loads: every other plane takes the generic form's byte loads
    *rows = gca_policy_obs_rows_shape(H, W, B) && ((uintptr_t)grid & 7u) == 0;
}

extern "C" int gca_advanced_policy_observation(const uint8_t* grid, const uint8_t* dousing, const uint16_t* dous_bits,
                                               const int32_t* pos, int E, int H, int W, int empty, int tree, int fire,
                                               int radius, int block, uint8_t* local_out, float* feat_out,
                                               void* stream) {
    if (const int st = gca_check_advanced_policy_observation(grid, dousing, dous_bits, pos, E, H, W, empty, tree, fire,
                                                             radius, block, local_out, feat_out))
        return st;
    AdvRetArgs q{};
    bool rows;
    retardant_args(&q, grid, dous_bits, H, W, block, radius, tree, fire, &rows);
    q.w.S = 2 * radius + 1;
    q.w.SS = q.w.S * q.w.S;
    const int C2 = (int)gca_retardant_c2(H, W, block, radius);
    const dim3 wgs((unsigned)E), wg(POL_VT);
    hipStream_t st = (hipStream_t)stream;
#define GCA_AROBS_LAUNCH(NWV)                                                                                      \
    hipLaunchKernelGGL(advanced_retardant_obs_kernel<NWV>, wgs, wg, 0, st, q, grid, dousing, dous_bits, pos, local_out, \
                       feat_out, C2)
    if (rows && W == 256) GCA_AROBS_LAUNCH(1);
    else if (rows) GCA_AROBS_LAUNCH(2);
    else GCA_AROBS_LAUNCH(0);
#undef GCA_AROBS_LAUNCH
    GCA_CHECK_LAUNCH("advanced_policy_observation");
    return GCA_OK;
}

extern "C" int gca_advanced_policy_act_retardant(const gca_bulldozer_policy* policy, const uint8_t* grid,
                                                 const uint8_t* dousing, const uint16_t* dous_bits, const int32_t* pos,
                                                 const int32_t* time_step, int E, int H, int W, int empty, int tree,
                                                 int fire, int env_offset, uint64_t policy_seed, int greedy,
                                                 int32_t* action, int action_stride, float* logits, float* value,
                                                 uint8_t* local_out, float* feat_out, void* stream) {
    if (const int st = gca_check_advanced_policy_act_retardant(policy, grid, dousing, dous_bits, pos, time_step, E, H, W,
                                                               empty, tree, fire, action, action_stride))
        return st;
    const char* who = "advanced_policy_act_retardant";
    AdvRetArgs q{};
    // checked: at most GCA_POLICY_C_MAX, so the LDS below is at most 64 KiB
    const int C2 = (int)gca_retardant_c2(H, W, policy->block, policy->radius);
    if (const int st = policy_view(who, policy, C2, policy_seed, greedy, &q.w)) return st;
    bool rows;
    retardant_args(&q, grid, dous_bits, H, W, policy->block, policy->radius, tree, fire, &rows);
    q.env_offset = env_offset; q.action_stride = action_stride;
    const dim3 wgs((unsigned)E), wg(POL_VT);
    const size_t lds_bytes = (size_t)policy_lds_words(C2) * 4;
    hipStream_t st = (hipStream_t)stream;
#define GCA_ARET_LAUNCH(NWV)                                                                                         \
    hipLaunchKernelGGL(advanced_policy_act_retardant_kernel<NWV>, wgs, wg, lds_bytes, st, q, grid, dousing, dous_bits, \
                       pos, time_step, action, logits, value, local_out, feat_out)
    if (rows && W == 256) GCA_ARET_LAUNCH(1);
    else if (rows) GCA_ARET_LAUNCH(2);
    else GCA_ARET_LAUNCH(0);
#undef GCA_ARET_LAUNCH
    GCA_CHECK_LAUNCH(who);
    return GCA_OK;
}

// ------------------------------------------------------------------ the extension policy (gca.h "extension policy")
// The third half of the file: the agent the reference trains on this env. Its action has a third part, the extension
// choice, and it observes the DISPLAYED plane -- the blurred, visibility-filtered grid or the extension channel its
// previous choice switched on (gca_obs_dev.h, shared with the frame kernel of gca_obs.hip) -- not the true grid.
//   gca_extension_policy_act         the network with fifteen outputs on a given observation
//   gca_advanced_display             the u8 plane the frame colours, one value per cell
//   gca_advanced_policy_act_display  display + gca_policy_observation + gca_extension_policy_act in ONE launch; the
//                                    displayed plane never exists
__global__ __launch_bounds__(POL_VT) void extension_policy_act_kernel(
    PolicyW w, const uint8_t* __restrict__ local, const float* __restrict__ coarse,
    const int64_t* __restrict__ steps_elapsed, const uint32_t* __restrict__ episode, int env_offset,
    int32_t* __restrict__ action, float* __restrict__ logits, float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) float epol_lds[];
    const int e = blockIdx.x, tid = threadIdx.x;
    float* cs = epol_lds;
    float* part = cs + ((w.C + 3) & ~3);
    float* hs = part + POL_PART;
    float* outs = hs + POL_VT;
    for (int c = tid; c < w.C; c += POL_VT) cs[c] = coarse[(size_t)e * (size_t)w.C + c];
    const uint8_t* __restrict__ loc = local + (size_t)e * (size_t)w.SS;
    float o[EXT_POL_NOUT];
    policy_outputs<EXT_POL_NOUT, POL_VT>(
        w, cs, part, hs, outs, tid, POL_VT, logits ? logits + (size_t)e * 14 : nullptr, value ? value + e : nullptr,
        [&](int n, int, int) -> uint32_t { return (uint32_t)loc[n] & 3u; }, [] {}, o);
    int32_t move, shoot, ext;
    bdz_policy_sample(o, w, (uint32_t)steps_elapsed[e], (uint32_t)(env_offset + e), episode ? episode[e] : 0u, move,
                      shoot, &ext);
    if (tid == 0) {
        action[3 * (size_t)e] = move;
        action[3 * (size_t)e + 1] = shoot;
        action[3 * (size_t)e + 2] = ext;
    }
}

extern "C" int gca_extension_policy_act(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                                        const int64_t* steps_elapsed, const uint32_t* episode, int env_offset,
                                        uint64_t policy_seed, int greedy, int32_t* action, float* logits, float* value,
                                        int E, void* stream) {
    const char* who = "extension_policy_act";
    if (const int st = gca_check_bdz_policy_act_as(who, p, C, local, coarse, steps_elapsed, action, E)) return st;
    PolicyW w;
    if (const int st = policy_view(who, p, C, policy_seed, greedy, &w)) return st;
    hipLaunchKernelGGL(extension_policy_act_kernel, dim3((unsigned)E), dim3(POL_VT),
                       (size_t)policy_lds_words(C) * 4, (hipStream_t)stream, w, local, coarse, steps_elapsed,
                       episode, env_offset, action, logits, value);
    GCA_CHECK_LAUNCH(who);
    return GCA_OK;
}

// the day/night, the active channels and (by every wave on its own) the selection of env e: what its display shows
__device__ __forceinline__ ObsShow display_of_env(const gca_obs_params& p, const uint8_t* __restrict__ g, int H, int W,
                                                  const int32_t* __restrict__ is_night,
                                                  const int32_t* __restrict__ time_step, int choice, int e, int lane) {
    ObsCfg k;
    k.night = obs_night(p, is_night, time_step, e);
    k.on = (p.enable_extensions && p.n_choices > 0) ? obs_channels_on(p, choice) : 0u;
    k.need_blur = false;  // the frame kernel's staging hint, not read here
    const int sel = k.on ? obs_display_select(p, k, g, H, W, lane) : -1;
    return obs_display_show(p, k, sel);
}

// the displayed value of cell (r, c), from the plane
__device__ __forceinline__ int display_at(const ObsShow& s, const uint8_t* __restrict__ g, int H, int W, int r, int c) {
    if (s.kind == OBS_SHOW_ZERO) return 0;
    return obs_display_value(s, s.kind == OBS_SHOW_BLUR ? blur_at(g, H, W, r, c) : (int)g[(uint32_t)r * (uint32_t)W +
                                                                                          (uint32_t)c]);
}

constexpr int DISP_RB = 16;  // rows per workgroup of advanced_display_kernel

// Grid: (env, block of DISP_RB rows); 256 threads. Every block of the env repeats the selection scan (it normally ends
// at row 0), as the frame kernel does. W % 4 == 0 (4-B aligned planes): four cells and one 4-B store per thread.
__global__ __launch_bounds__(256) void advanced_display_kernel(gca_obs_params p, int H, int W, int blocks_per_env,
                                                               bool words, const uint8_t* __restrict__ grid,
                                                               const int32_t* __restrict__ is_night,
                                                               const int32_t* __restrict__ time_step,
                                                               const int32_t* __restrict__ choice, int choice_stride,
                                                               uint8_t* __restrict__ out) {
    const int e = blockIdx.x / blocks_per_env;
    const int r0 = (blockIdx.x - e * blocks_per_env) * DISP_RB;
    const int rows = min(DISP_RB, H - r0);
    const size_t HW = (size_t)H * (size_t)W;
    const uint8_t* __restrict__ g = grid + (size_t)e * HW;
    uint8_t* __restrict__ o = out + (size_t)e * HW;
    const ObsShow s = display_of_env(p, g, H, W, is_night, time_step,
                                     choice ? choice[(size_t)e * (size_t)choice_stride] : 0, e, (int)threadIdx.x & 63);
    if (words) {
        const int wq = W >> 2;
        for (int idx = threadIdx.x; idx < rows * wq; idx += 256) {
            const int lr = idx / wq, c0 = (idx - lr * wq) * 4, r = r0 + lr;
            uint32_t v = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)display_at(s, g, H, W, r, c0 + j) << (8 * j);
            *reinterpret_cast<uint32_t*>(o + (size_t)r * W + c0) = v;
        }
    } else {
        for (int idx = threadIdx.x; idx < rows * W; idx += 256) {
            const int lr = idx / W, c = idx - lr * W, r = r0 + lr;
            o[(size_t)r * W + c] = (uint8_t)display_at(s, g, H, W, r, c);
        }
    }
}

extern "C" int gca_advanced_display(const gca_obs_params* p, int E, int H, int W, const uint8_t* grid,
                                    const int32_t* is_night, const int32_t* time_step, const int32_t* choice,
                                    int choice_stride, uint8_t* display_out, void* stream) {
    if (const int st = gca_check_advanced_display(p, E, H, W, grid, is_night, choice, choice_stride, display_out))
        return st;
    const int bpe = (H + DISP_RB - 1) / DISP_RB;
    GCA_CHECK_ARG((int64_t)E * bpe < (1ll << 31), "advanced_display: too many envs for one launch");
    // the selection scan's 4-B loads of a row whose width is a multiple of four
    GCA_CHECK_ARG((W & 3) != 0 || ((uintptr_t)grid & 3u) == 0, "advanced_display: grid must be 4-B aligned");
    const bool words = (W & 3) == 0 && ((((uintptr_t)grid) | ((uintptr_t)display_out)) & 3u) == 0;
    hipLaunchKernelGGL(advanced_display_kernel, dim3((unsigned)((int64_t)E * bpe)), dim3(256), 0, (hipStream_t)stream,
                       *p, H, W, bpe, words, grid, is_night, time_step, choice, choice_stride, display_out);
    GCA_CHECK_LAUNCH("advanced_display");
    return GCA_OK;
}

// ---- observe the display and act in ONE launch. One 256-thread workgroup per env, as advanced_policy_act_kernel; the
// coarse TREE / FIRE shares of the DISPLAYED values are counted straight into the network's LDS words cs, the window's
// classes are computed from the plane (the blur on the fly), policy_outputs / bdz_policy_sample run on them.
// Every thread reads the env's choice first, every wave then runs the selection scan on its own (a ballot per row, no
// barrier; all waves agree). The three outcomes of the selection are exact shortcuts:
//   zero  a switched-off channel is displayed: every value is 0, the plane is not read for the coarse part (a tile's
//         TREE share is its in-grid cells / block^2 if the TREE code is 0, else 0; FIRE likewise);
//   raw   the grid itself is displayed: the strip code of advanced_policy_act_kernel runs on the plane unchanged
//         (where visibility would turn a 3 into 0 and a code is 0 or 3, the generic loops run instead);
//   blur  the blurred grid is displayed. Rows form (NW = 1, 2): a lane owns 4 NW consecutive bytes of a row; the row's
//         horizontal 3-sums come from the lane's bytes and one byte of each neighbouring lane (a lane shift; lanes 0
//         and 63 pad with their own edge byte), the vertical sum is a rolling window of three rows of those sums in
//         registers, S <= 9 * 255. No LDS beyond the network's. Generic form: byte loops through blur_at.
// Barriers: the four of policy_outputs and no other, outside every condition (the branches above are workgroup-uniform
// and hold no barrier). A orders every thread's stores of cs (one writer per word in every branch) before the coarse
// terms read them, and it is also what orders every thread's read of env e's `choice` before thread 0's store of env
// e's action after D: `choice` may be column 2 of the same action rows. No atomics, no scratch: capturable.
struct AdvDispArgs {
    AdvPolArgs a;
    gca_obs_params p;
    int choice_stride;
};

template <int NW>
__device__ __forceinline__ void display_blur_strip(const uint8_t* __restrict__ grid, const ObsShow& show, int lane,
                                                   int strip, int H, int lgB, uint32_t tree, uint32_t fire, float inv,
                                                   int HcWc, float* cs) {
    constexpr int W = 256 * NW, NB = 4 * NW;
    const int B = 1 << lgB;
    const int lgG = lgB - (NW == 1 ? 2 : 3);  // lanes per tile, as policy_obs_rows_strip
    const int Wc = W >> lgB;
    const int base = strip * POBS_STRIP;
    const int row_end = min(H, base + POBS_STRIP);
    const uint32_t lofs = 4 * NW * (uint32_t)lane;
    // the horizontal 3-sums of the lane's NB bytes of row R (clamped into the grid: the vertical edge padding)
    auto hsum = [&](int R, int (&h)[NB]) {
        const ObsRow<NW> x = load_obsrow<NW>(grid, lofs, min(max(R, 0), H - 1));
        int b[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) b[j] = (int)((x.w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        const int up = __shfl_up(b[NB - 1], 1), dn = __shfl_down(b[0], 1);
        const int left = lane == 0 ? b[0] : up, right = lane == 63 ? b[NB - 1] : dn;
#pragma unroll
        for (int j = 0; j < NB; ++j) h[j] = (j ? b[j - 1] : left) + b[j] + (j + 1 < NB ? b[j + 1] : right);
    };
    int hp[NB], hc[NB], hn[NB];
    hsum(base - 1, hp);
    hsum(base, hc);
    uint32_t cT = 0u, cF = 0u;
    for (int r = base; r < row_end; ++r) {  // wave-uniform bounds: all 64 lanes run every shuffle
        hsum(r + 1, hn);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const uint32_t v = (uint32_t)obs_display_value(show, (2 * (hp[j] + hc[j] + hn[j]) + 9) / 18);
            cT += v == tree;
            cF += v == fire;
            hp[j] = hc[j];
            hc[j] = hn[j];
        }
        if (((r + 1) & (B - 1)) != 0) continue;
        uint32_t s = cT | (cF << 16);  // at most 32 * 8 = 256 per lane, 1024 per tile
        cT = cF = 0u;
        if (lgG >= 1) s += obs_dpp<0xB1>(s);
        if (lgG >= 2) s += obs_dpp<0x4E>(s);
        if (lgG >= 3) s += obs_dpp<0x141>(s);
        if ((lane & ((1 << lgG) - 1)) == 0) {
            const int o = (r >> lgB) * Wc + (lane >> lgG);
            cs[o] = (float)(s & 0xFFFFu) * inv;
            cs[HcWc + o] = (float)(s >> 16) * inv;
        }
    }
}

template <int NW>
__global__ __launch_bounds__(POL_VT) void advanced_policy_act_display_kernel(
    AdvDispArgs qq, const uint8_t* __restrict__ planes, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ is_night, const int32_t* __restrict__ time_step, const int32_t* __restrict__ choice,
    int32_t* __restrict__ action, float* __restrict__ logits, float* __restrict__ value,
    uint8_t* __restrict__ local_out, float* __restrict__ coarse_out) {
    extern __shared__ __attribute__((aligned(16))) float adisp_lds[];
    const AdvPolArgs& q = qq.a;
    const int e = blockIdx.x, tid = threadIdx.x;
    float* cs = adisp_lds;
    float* part = cs + ((q.w.C + 3) & ~3);
    float* hs = part + POL_PART;
    float* outs = hs + POL_VT;
    const int H = q.H, W = q.W, HcWc = q.Hc * q.Wc;
    const uint8_t* __restrict__ grid = planes + (size_t)e * (size_t)H * (size_t)W;
    // env e's choice, read by every thread before anything else (see "Barriers" above)
    const int ch = choice ? choice[(size_t)e * (size_t)qq.choice_stride] : 0;
    const ObsShow show = display_of_env(qq.p, grid, H, W, is_night, time_step, ch, e, tid & 63);
    // ---- the coarse map of the displayed values into cs
    // visibility's 3 -> 0 leaves the TREE and FIRE counts of the raw plane alone unless one of the codes is 0 or 3
    const bool codes_plain = !show.vis3 || (q.tree != 0u && q.tree != 3u && q.fire != 0u && q.fire != 3u);
    if (show.kind == OBS_SHOW_ZERO) {
        const int B = q.B, Wc = q.Wc;
        for (int t = tid; t < HcWc; t += POL_VT) {
            const int bi = t / Wc, bj = t - bi * Wc;
            const int n = (min(H, bi * B + B) - bi * B) * (min(W, bj * B + B) - bj * B);
            cs[t] = q.tree == 0u ? (float)n * q.inv : 0.0f;
            cs[HcWc + t] = q.fire == 0u ? (float)n * q.inv : 0.0f;
        }
    } else if (NW != 0 && show.kind == OBS_SHOW_RAW && codes_plain) {
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
        }
    } else if (NW != 0 && show.kind == OBS_SHOW_BLUR) {
        if constexpr (NW != 0) {
            const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
            const int strips = (H + POBS_STRIP - 1) / POBS_STRIP;
            for (int s = wave; s < strips; s += POL_VT / GCA_WAVE)
                display_blur_strip<NW>(grid, show, lane, s, H, q.lgB, q.tree, q.fire, q.inv, HcWc, cs);
        }
    } else {
        const int B = q.B, Wc = q.Wc;
        for (int t = tid; t < HcWc; t += POL_VT) {
            const int bi = t / Wc, bj = t - bi * Wc;
            const int r1 = min(H, bi * B + B), c1 = min(W, bj * B + B);
            int32_t cT = 0, cF = 0;
            for (int r = bi * B; r < r1; ++r)
                for (int c = bj * B; c < c1; ++c) {
                    const uint32_t v = (uint32_t)display_at(show, grid, H, W, r, c);
                    cT += v == q.tree;
                    cF += v == q.fire;
                }
            cs[t] = (float)cT * q.inv;
            cs[HcWc + t] = (float)cF * q.inv;
        }
    }
    // ---- the window of the displayed values, the network, the draw
    const uint32_t wr0 = (uint32_t)pos[2 * e] - (uint32_t)q.radius, wc0 = (uint32_t)pos[2 * e + 1] - (uint32_t)q.radius;
    auto class_at = [&](int, int i, int j) -> uint32_t {
        const uint32_t r = wr0 + (uint32_t)i, c = wc0 + (uint32_t)j;
        const bool in = r < (uint32_t)H && c < (uint32_t)W;
        const uint32_t v = (uint32_t)display_at(show, grid, H, W, in ? (int)r : 0, in ? (int)c : 0);
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
    float o[EXT_POL_NOUT];
    policy_outputs<EXT_POL_NOUT, POL_VT>(q.w, cs, part, hs, outs, tid, POL_VT,
                                         logits ? logits + (size_t)e * 14 : nullptr, value ? value + e : nullptr,
                                         class_at, record, o);
    int32_t move, shoot, ext;
    bdz_policy_sample(o, q.w, (uint32_t)time_step[e], (uint32_t)(q.env_offset + e), 0u, move, shoot, &ext);
    if (tid == 0) {
        int32_t* a = action + (size_t)e * (size_t)q.action_stride;
        a[0] = move;
        a[1] = shoot;
        a[2] = ext;
    }
}

extern "C" int gca_advanced_policy_act_display(const gca_bulldozer_policy* policy, const gca_obs_params* p,
                                               const uint8_t* grid, const int32_t* pos, const int32_t* is_night,
                                               const int32_t* time_step, const int32_t* choice, int choice_stride,
                                               int E, int H, int W, int env_offset, uint64_t policy_seed, int greedy,
                                               int32_t* action, int action_stride, float* logits, float* value,
                                               uint8_t* local_out, float* coarse_out, void* stream) {
    if (const int st = gca_check_advanced_policy_act_display(policy, p, grid, pos, is_night, time_step, choice,
                                                             choice_stride, E, H, W, action, action_stride))
        return st;
    const char* who = "advanced_policy_act_display";
    // the selection scan's 4-B loads of a row whose width is a multiple of four
    if ((W & 3) == 0 && ((uintptr_t)grid & 3u) != 0) return gca_refuse(who, "grid must be 4-B aligned");
    AdvDispArgs qq;
    AdvPolArgs& q = qq.a;
    qq.p = *p;
    qq.choice_stride = choice_stride;
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
    q.tree = (uint32_t)p->tree; q.fire = (uint32_t)p->fire;
    q.env_offset = env_offset; q.action_stride = action_stride;
    const bool rows = gca_policy_obs_rows_shape(H, W, B) && ((uintptr_t)grid & 7u) == 0;
    const dim3 wgs((unsigned)E), wg(POL_VT);
    const size_t lds_bytes = (size_t)policy_lds_words(C) * 4;
    hipStream_t st = (hipStream_t)stream;
#define GCA_ADISP_LAUNCH(NWV)                                                                                       \
    hipLaunchKernelGGL(advanced_policy_act_display_kernel<NWV>, wgs, wg, lds_bytes, st, qq, grid, pos, is_night, \
                       time_step, choice, action, logits, value, local_out, coarse_out)
    if (rows && W == 256) GCA_ADISP_LAUNCH(1);
    else if (rows) GCA_ADISP_LAUNCH(2);
    else GCA_ADISP_LAUNCH(0);
#undef GCA_ADISP_LAUNCH
    GCA_CHECK_LAUNCH(who);
    return GCA_OK;
}
