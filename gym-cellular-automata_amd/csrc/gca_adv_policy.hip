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
