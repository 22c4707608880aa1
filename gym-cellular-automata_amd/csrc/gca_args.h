// gca_args.h — the argument contract of the entry points that libgca_hip.so (csrc/*.hip) and libgca_cpu.so
// (gca_cpu.cpp) both export: one check function per entry point, or per group of checks that several share, holding
// every refusal that does not depend on the build. Both builds call them first, so both refuse the same arguments
// with the same words in the same order. What only one build can know (LDS fit, workgroup counts, plane alignment,
// `scratch`, memset failures on the device; the walk's cap on the host) stays in that build, after the shared call;
// the idx scan of the policy_grad entry points, which only the host build can make, is here for its two callers.
// Plain C++, no device code, like the two plan headers.
#pragma once
#include <stdint.h>

#include "../../include/gca.h"
#include "gca_opt_plan.h"
#include "gca_ppo_plan.h"

// ----------------------------------------------------------------- errors
// Each library defines its own (gca_util.hip, gca_cpu.cpp); hidden, so that two libraries loaded into one process can
// never bind each other's copy and thread-local message.
__attribute__((visibility("hidden"))) void gca_set_error(const char* fmt, ...);

#define GCA_CHECK_ARG(cond, msg)                 \
    do {                                         \
        if (!(cond)) {                           \
            gca_set_error("argument: %s", msg);  \
            return GCA_ERR_ARG;                  \
        }                                        \
    } while (0)

// a refusal whose message the entry point `who` heads
static inline int gca_refuse(const char* who, const char* what) {
    gca_set_error("argument: %s: %s", who, what);
    return GCA_ERR_ARG;
}

// ----------------------------------------------------------------- util, Move / Modify, Drossel-Schwabl
static inline int gca_check_philox(const void* ctr, const void* out, int64_t n) {
    GCA_CHECK_ARG(ctr && out && n >= 0, "ctr/out required");
    return GCA_OK;
}

static inline int gca_check_count_cells(const void* grid, int E, int H, int W, const void* counts) {
    GCA_CHECK_ARG(grid && counts && E > 0 && H > 0 && W > 0, "grid/counts and positive sizes required");
    return GCA_OK;
}

static inline int gca_check_move_modify(const void* p, const void* action, const void* pos, int H, int W, int E) {
    GCA_CHECK_ARG(p && action && pos && E > 0 && H > 0 && W > 0, "move_modify: bad arguments");
    return GCA_OK;
}

static inline int gca_check_ds_count_draws(const void* grid, int E, int H, int W, const void* n_draws) {
    GCA_CHECK_ARG(grid && n_draws && E > 0 && H > 0 && W > 0, "ds_count_draws: bad arguments");
    GCA_CHECK_ARG((int64_t)H * W < (1 << 30), "ds_count_draws: grid too large");
    return GCA_OK;
}

static inline int gca_check_ds_step(const void* grid_in, const void* grid_out, int E, int H, int W,
                                    const void* thresholds, const void* uniforms, const void* uniform_offset) {
    GCA_CHECK_ARG(grid_in && grid_out && thresholds && E > 0 && H > 0 && W > 0, "ds_step: bad arguments");
    GCA_CHECK_ARG(grid_in != grid_out, "ds_step: in-place update is not supported");
    GCA_CHECK_ARG(!uniforms || uniform_offset, "ds_step: uniforms need uniform_offset");
    GCA_CHECK_ARG((int64_t)H * W < (1 << 30), "ds_step: grid too large");
    return GCA_OK;
}

// ----------------------------------------------------------------- the helicopter env
// The env arguments of gca_helicopter_step, gca_helicopter_rollout and gca_helicopter_policy_rollout.
static inline int gca_check_heli_env(const char* who, int empty, int tree, int fire, int max_freeze,
                                     const void* thresholds, const void* freeze, const void* rng_step,
                                     const void* parity, const void* buf0, const void* buf1, int H, int W,
                                     const void* pos, const void* counts, const void* hit, const void* reward,
                                     const void* steps_elapsed, int E) {
    if (!(thresholds && freeze && rng_step && parity && buf0 && buf1 && pos && counts && hit && reward &&
          steps_elapsed))
        return gca_refuse(who, "null argument");
    if (!(E > 0 && H > 0 && W > 0 && max_freeze >= 0)) return gca_refuse(who, "E, H, W > 0 and max_freeze >= 0");
    if (buf0 == buf1) return gca_refuse(who, "buf0 and buf1 must differ");
    if ((int64_t)H * W >= (1 << 30)) return gca_refuse(who, "grid too large");
    if (((empty | tree | fire) & ~0xFF) != 0 || empty == tree || tree == fire || empty == fire)
        return gca_refuse(who, "three distinct u8 codes");
    return GCA_OK;
}

static inline int gca_check_k(const char* who, int K) { return K >= 0 ? GCA_OK : gca_refuse(who, "K >= 0"); }

static inline int gca_check_bulldozer_reset_where(const gca_bulldozer_params* p, int64_t max_steps,
                                                  int64_t set_episode, const void* cdf, const void* values,
                                                  const void* done, const void* episode, const void* accu,
                                                  const void* parity, const void* buf0, const void* buf1, int H,
                                                  int W, const void* pos, const void* counts, const void* hit,
                                                  const void* steps_elapsed, int E) {
    GCA_CHECK_ARG(p && cdf && values && done && episode && accu && parity && buf0 && buf1 && pos && counts && hit &&
                      steps_elapsed,
                  "bulldozer_reset_where: null argument");
    GCA_CHECK_ARG(E > 0 && H > 0 && W > 0, "bulldozer_reset_where: E, H, W must be positive");
    GCA_CHECK_ARG(H < 32768 && W < 32768, "bulldozer_reset_where: H, W < 32768");
    GCA_CHECK_ARG(buf0 != buf1, "bulldozer_reset_where: buf0 and buf1 must differ");
    GCA_CHECK_ARG(max_steps >= 0 && set_episode >= -1 && set_episode <= 0xFFFFFFFFll,
                  "bulldozer_reset_where: max_steps >= 0 and set_episode in [-1, 2^32)");
    GCA_CHECK_ARG(p->env_offset >= 0, "bulldozer_reset_where: env_offset >= 0");
    return GCA_OK;
}

// ----------------------------------------------------------------- the policy observation
// the shapes the device's rows form takes; `form` 2 asks for it by name
static inline bool gca_policy_obs_rows_shape(int H, int W, int block) {
    return (W == 256 || W == 512) && (block == 8 || block == 16 || block == 32) && H % block == 0;
}

static inline int gca_check_policy_observation(const void* buf0, const void* buf1, const void* parity,
                                               const void* pos, int E, int H, int W, int empty, int tree, int fire,
                                               int radius, int block, int form, const void* local_out,
                                               const void* coarse_out) {
    GCA_CHECK_ARG(buf0 && (buf1 || !parity), "policy_observation: buf0 required, and buf1 with parity");
    GCA_CHECK_ARG(local_out || coarse_out, "policy_observation: local_out or coarse_out required");
    GCA_CHECK_ARG(pos || !local_out, "policy_observation: local_out needs pos");
    GCA_CHECK_ARG(E > 0 && H > 0 && W > 0, "policy_observation: E, H, W must be positive");
    GCA_CHECK_ARG((int64_t)H * W < (1 << 30), "policy_observation: grid too large (H * W < 2^30)");
    GCA_CHECK_ARG(((empty | tree | fire) & ~0xFF) == 0, "policy_observation: the codes must be u8 values");
    GCA_CHECK_ARG(radius >= 0 && radius <= 31, "policy_observation: radius in [0, 31]");
    GCA_CHECK_ARG(block >= 1 && block <= 64 && (block & (block - 1)) == 0,
                  "policy_observation: block must be a power of two in [1, 64]");
    GCA_CHECK_ARG(form >= 0 && form <= 2, "policy_observation: form 0 (by shape), 1 (generic) or 2 (rows)");
    GCA_CHECK_ARG(form != 2 || gca_policy_obs_rows_shape(H, W, block),
                  "policy_observation: form 2 (rows) needs W = 256 / 512, block = 8 / 16 / 32 and H % block == 0");
    return GCA_OK;
}

// ----------------------------------------------------------------- the helicopter policy
// The largest coarse map (C = 2 Hc Wc floats) of a policy: with the network's other LDS words (gca_policy_dev.h ties
// the two together) it fills the 64 KiB of a workgroup. The host build keeps the same limit.
constexpr int GCA_POLICY_C_MAX = 15088;

// two functions with gca_check_bdz_policy (below) only because the refusal texts differ: test_abi_refusals.py pins both
static inline int gca_check_policy(const gca_heli_policy* p) {
    GCA_CHECK_ARG(p && p->w_local && p->w_coarse && p->b1 && p->w_out && p->b2, "helicopter_policy: null weights");
    GCA_CHECK_ARG(p->radius >= 0 && p->radius <= 31, "helicopter_policy: radius in [0, 31]");
    GCA_CHECK_ARG(p->block >= 1 && p->block <= 64 && (p->block & (p->block - 1)) == 0,
                  "helicopter_policy: block must be a power of two in [1, 64]");
    GCA_CHECK_ARG(p->hidden >= 32 && p->hidden <= 256 && (p->hidden & (p->hidden - 1)) == 0,
                  "helicopter_policy: hidden must be a power of two in [32, 256]");
    return GCA_OK;
}

// the 16-B loads of the device's kernels; of a checked policy of either agent
static inline bool gca_policy_weights_aligned(const gca_policy* p) {
    return (((uintptr_t)p->w_local | (uintptr_t)p->w_coarse) & 15u) == 0;
}

static inline int gca_check_policy_c(const char* who, int C) {
    return (C >= 2 && C % 2 == 0 && C <= GCA_POLICY_C_MAX) ? GCA_OK : gca_refuse(who, "C = 2 Hc Wc, at most 15088");
}

static inline int gca_check_policy_act(const gca_heli_policy* p, int C, const void* local, const void* coarse,
                                       const void* rng_step, const void* action, int E) {
    if (const int st = gca_check_policy(p)) return st;
    GCA_CHECK_ARG(local && coarse && rng_step && action, "helicopter_policy_act: null argument");
    GCA_CHECK_ARG(E > 0, "helicopter_policy_act: E > 0");
    return gca_check_policy_c("helicopter_policy_act", C);
}

// gca_helicopter_policy_rollout's refusal of a coarse map of C floats: above 2^30 at once, above what a build can
// take where that build comes to need it
static inline int gca_check_rollout_coarse(int64_t C, int64_t limit) {
    GCA_CHECK_ARG(C <= limit, "helicopter_policy_rollout: coarse map too large");
    return GCA_OK;
}

static inline int gca_check_policy_rollout(int empty, int tree, int fire, int max_freeze, const gca_heli_policy* p,
                                           int K, const void* thresholds, const void* freeze, const void* rng_step,
                                           const void* parity, const void* buf0, const void* buf1, int H, int W,
                                           const void* pos, const void* counts, const void* hit, const void* reward,
                                           const void* steps_elapsed, int E) {
    const char* who = "helicopter_policy_rollout";
    if (const int st = gca_check_heli_env(who, empty, tree, fire, max_freeze, thresholds, freeze, rng_step, parity, buf0,
                                          buf1, H, W, pos, counts, hit, reward, steps_elapsed, E))
        return st;
    if (const int st = gca_check_k(who, K)) return st;
    GCA_CHECK_ARG(p && p->block >= 1, "helicopter_policy_rollout: policy required");
    const int64_t Hc = (H - 1) / p->block + 1, Wc = (W - 1) / p->block + 1;  // the ceilings, for any block >= 1
    if (const int st = gca_check_rollout_coarse(2 * Hc * Wc, (1 << 30) - 1)) return st;
    return gca_check_policy(p);
}

// ----------------------------------------------------------------- the bulldozer policy
// Every refusal names its argument. The dims are the helicopter policy's; the act kernel's LDS gives the same C limit.
static inline int gca_check_bdz_policy(const char* who, const gca_bulldozer_policy* p) {
    if (!p) return gca_refuse(who, "policy is null");
    if (!p->w_local) return gca_refuse(who, "policy.w_local is null");
    if (!p->w_coarse) return gca_refuse(who, "policy.w_coarse is null");
    if (!p->b1) return gca_refuse(who, "policy.b1 is null");
    if (!p->w_out) return gca_refuse(who, "policy.w_out is null");
    if (!p->b2) return gca_refuse(who, "policy.b2 is null");
    if (!(p->radius >= 0 && p->radius <= 31)) return gca_refuse(who, "policy.radius in [0, 31]");
    if (!(p->block >= 1 && p->block <= 64 && (p->block & (p->block - 1)) == 0))
        return gca_refuse(who, "policy.block must be a power of two in [1, 64]");
    if (!(p->hidden >= 32 && p->hidden <= 256 && (p->hidden & (p->hidden - 1)) == 0))
        return gca_refuse(who, "policy.hidden must be a power of two in [32, 256]");
    return GCA_OK;
}

// gca_bulldozer_policy_act's conditions under the name `who`: gca_extension_policy_act's are the same
static inline int gca_check_bdz_policy_act_as(const char* who, const gca_bulldozer_policy* p, int C, const void* local,
                                              const void* coarse, const void* steps_elapsed, const void* action,
                                              int E) {
    if (const int st = gca_check_bdz_policy(who, p)) return st;
    if (!local) return gca_refuse(who, "local is null");
    if (!coarse) return gca_refuse(who, "coarse is null");
    if (!steps_elapsed) return gca_refuse(who, "steps_elapsed is null");
    if (!action) return gca_refuse(who, "action is null");
    if (!(E > 0)) return gca_refuse(who, "E > 0");
    return gca_check_policy_c(who, C);
}

static inline int gca_check_bdz_policy_act(const gca_bulldozer_policy* p, int C, const void* local, const void* coarse,
                                           const void* steps_elapsed, const void* action, int E) {
    return gca_check_bdz_policy_act_as("bulldozer_policy_act", p, C, local, coarse, steps_elapsed, action, E);
}

// ----------------------------------------------------------------- the extension policy (gca.h "extension policy")
static inline int gca_check_advanced_display(const gca_obs_params* p, int E, int H, int W, const void* grid,
                                             const void* is_night, const void* choice, int choice_stride,
                                             const void* display_out) {
    const char* who = "advanced_display";
    if (!p) return gca_refuse(who, "params is null");
    if (!grid) return gca_refuse(who, "grid is null");
    if (!is_night) return gca_refuse(who, "is_night is null");
    if (!display_out) return gca_refuse(who, "display_out is null");
    if (!(E > 0 && H > 0 && W > 0)) return gca_refuse(who, "E, H, W must be positive");
    if (!((int64_t)H * W < (1 << 30))) return gca_refuse(who, "grid too large (H * W < 2^30)");
    if (!(p->n_ext >= 0 && p->n_ext <= GCA_OBS_MAX_EXT)) return gca_refuse(who, "0..4 extension channels");
    if (choice && !(choice_stride >= 1)) return gca_refuse(who, "choice_stride >= 1");
    const uintptr_t g0 = (uintptr_t)grid, d0 = (uintptr_t)display_out, n = (uintptr_t)E * (uintptr_t)H * (uintptr_t)W;
    if (g0 < d0 + n && d0 < g0 + n)
        return gca_refuse(who, "display_out may not overlap the grid (the blur reads neighbours)");
    return GCA_OK;
}

// gca_advanced_policy_act_display: the display's conditions, gca_advanced_policy_act's on the plane and the policy, and
// an action of three columns
static inline int gca_check_advanced_policy_act_display(const gca_bulldozer_policy* policy, const gca_obs_params* p,
                                                        const void* grid, const void* pos, const void* is_night,
                                                        const void* time_step, const void* choice, int choice_stride,
                                                        int E, int H, int W, const void* action, int action_stride) {
    const char* who = "advanced_policy_act_display";
    if (const int st = gca_check_bdz_policy(who, policy)) return st;
    if (!p) return gca_refuse(who, "params is null");
    if (!grid) return gca_refuse(who, "grid is null");
    if (!pos) return gca_refuse(who, "pos is null");
    if (!is_night) return gca_refuse(who, "is_night is null");
    if (!time_step) return gca_refuse(who, "time_step is null");
    if (!action) return gca_refuse(who, "action is null");
    if (!(E > 0 && H > 0 && W > 0)) return gca_refuse(who, "E, H, W must be positive");
    if (!((int64_t)H * W < (1 << 30))) return gca_refuse(who, "grid too large (H * W < 2^30)");
    if (((p->empty | p->tree | p->fire) & ~0xFF) != 0) return gca_refuse(who, "the codes must be u8 values");
    if (!(p->n_ext >= 0 && p->n_ext <= GCA_OBS_MAX_EXT)) return gca_refuse(who, "0..4 extension channels");
    if (choice && !(choice_stride >= 1)) return gca_refuse(who, "choice_stride >= 1");
    if (!(action_stride >= 3)) return gca_refuse(who, "action_stride >= 3");
    const int64_t Hc = (H - 1) / policy->block + 1, Wc = (W - 1) / policy->block + 1;
    if (2 * Hc * Wc > GCA_POLICY_C_MAX) return gca_refuse(who, "C = 2 Hc Wc, at most 15088");
    return gca_check_policy_c(who, (int)(2 * Hc * Wc));
}

// gca_advanced_policy_act: gca_policy_observation's conditions on the plane (parity NULL, both parts always built; the
// radius and the block are the policy's, checked with it), the bulldozer policy's, and the action's stride
static inline int gca_check_advanced_policy_act(const gca_bulldozer_policy* p, const void* grid, const void* pos,
                                                const void* time_step, int E, int H, int W, int empty, int tree,
                                                int fire, const void* action, int action_stride) {
    const char* who = "advanced_policy_act";
    if (const int st = gca_check_bdz_policy(who, p)) return st;
    if (!grid) return gca_refuse(who, "grid is null");
    if (!pos) return gca_refuse(who, "pos is null");
    if (!time_step) return gca_refuse(who, "time_step is null");
    if (!action) return gca_refuse(who, "action is null");
    if (!(E > 0 && H > 0 && W > 0)) return gca_refuse(who, "E, H, W must be positive");
    if (!((int64_t)H * W < (1 << 30))) return gca_refuse(who, "grid too large (H * W < 2^30)");
    if (((empty | tree | fire) & ~0xFF) != 0) return gca_refuse(who, "the codes must be u8 values");
    if (!(action_stride >= 2)) return gca_refuse(who, "action_stride >= 2");
    const int64_t Hc = (H - 1) / p->block + 1, Wc = (W - 1) / p->block + 1;
    if (2 * Hc * Wc > GCA_POLICY_C_MAX) return gca_refuse(who, "C = 2 Hc Wc, at most 15088");
    return gca_check_policy_c(who, (int)(2 * Hc * Wc));
}

// ----------------------------------------------------------------- the retardant observation (gca.h "advanced policy")
// C2 = 3 Hc Wc + S*S, rounded up to even: the floats of one env's feature vector
static inline int64_t gca_retardant_c2(int H, int W, int block, int radius) {
    const int64_t Hc = (H - 1) / block + 1, Wc = (W - 1) / block + 1, S = 2 * radius + 1;
    return (3 * Hc * Wc + S * S + 1) & ~(int64_t)1;
}

// what gca_advanced_policy_observation and gca_advanced_policy_act_retardant ask of the plane, its two retardant
// layers and the position
static inline int gca_check_retardant_state(const char* who, const void* grid, const void* dousing,
                                            const void* dous_bits, const void* pos, int E, int H, int W, int empty,
                                            int tree, int fire) {
    if (!grid) return gca_refuse(who, "grid is null");
    if (!dousing) return gca_refuse(who, "dousing is null");
    if (!pos) return gca_refuse(who, "pos is null");
    if (!(E > 0 && H > 0 && W > 0)) return gca_refuse(who, "E, H, W must be positive");
    if (!((int64_t)H * W < (1 << 30))) return gca_refuse(who, "grid too large (H * W < 2^30)");
    if (((empty | tree | fire) & ~0xFF) != 0) return gca_refuse(who, "the codes must be u8 values");
    if (dous_bits && W % 16 != 0) return gca_refuse(who, "dous_bits needs W % 16 == 0");
    if (((uintptr_t)dous_bits & 1u) != 0) return gca_refuse(who, "dous_bits must be 2-B aligned");
    return GCA_OK;
}

static inline int gca_check_advanced_policy_observation(const void* grid, const void* dousing, const void* dous_bits,
                                                        const void* pos, int E, int H, int W, int empty, int tree,
                                                        int fire, int radius, int block, const void* local_out,
                                                        const void* feat_out) {
    const char* who = "advanced_policy_observation";
    if (const int st = gca_check_retardant_state(who, grid, dousing, dous_bits, pos, E, H, W, empty, tree, fire))
        return st;
    if (!(local_out || feat_out)) return gca_refuse(who, "local_out or feat_out required");
    if (!(radius >= 0 && radius <= 31)) return gca_refuse(who, "radius in [0, 31]");
    if (!(block >= 1 && block <= 64 && (block & (block - 1)) == 0))
        return gca_refuse(who, "block must be a power of two in [1, 64]");
    if (!(gca_retardant_c2(H, W, block, radius) < (1ll << 31)))
        return gca_refuse(who, "feat too large (C2 = 3 Hc Wc + S*S < 2^31)");
    return GCA_OK;
}

static inline int gca_check_advanced_policy_act_retardant(const gca_bulldozer_policy* p, const void* grid,
                                                          const void* dousing, const void* dous_bits, const void* pos,
                                                          const void* time_step, int E, int H, int W, int empty,
                                                          int tree, int fire, const void* action, int action_stride) {
    const char* who = "advanced_policy_act_retardant";
    if (const int st = gca_check_bdz_policy(who, p)) return st;
    if (!time_step) return gca_refuse(who, "time_step is null");
    if (!action) return gca_refuse(who, "action is null");
    if (const int st = gca_check_retardant_state(who, grid, dousing, dous_bits, pos, E, H, W, empty, tree, fire))
        return st;
    if (!(action_stride >= 2)) return gca_refuse(who, "action_stride >= 2");
    if (gca_retardant_c2(H, W, p->block, p->radius) > GCA_POLICY_C_MAX)
        return gca_refuse(who, "C2 = 3 Hc Wc + S*S rounded up to even, at most 15088");
    return GCA_OK;
}

// ----------------------------------------------------------------- the PPO update
static inline int gca_check_gae(const void* reward, const void* value, const void* next_value, int K, int E,
                                const void* advantage, const void* returns) {
    if (const int st = gca_check_k("gae", K)) return st;
    GCA_CHECK_ARG(E > 0, "gae: E > 0");
    GCA_CHECK_ARG(reward && value && next_value && advantage && returns, "gae: null argument");
    return GCA_OK;
}

// The agent of a gca_*_policy_grad call: what heads its refusals, which policy check speaks, and the network's outputs
// (the logits of its heads and the value; ppo_plan's NOUT). The checks below are the three agents' alike.
struct GcaGradAgent {
    const char* who;       // heads every refusal of the call
    const char* who_ws;    // heads the workspace query's refusal
    const char* short_ws;  // the refusal of a short workspace, which names the query
    bool bdz;              // the policy check: gca_check_bdz_policy's texts, else gca_check_policy's
    int nout;
};
constexpr GcaGradAgent GCA_GRAD_HELI{"helicopter_policy_grad", "helicopter_policy_grad_workspace",
                                     "workspace smaller than gca_helicopter_policy_grad_workspace", false, 10};
constexpr GcaGradAgent GCA_GRAD_BDZ{"bulldozer_policy_grad", "bulldozer_policy_grad_workspace",
                                    "workspace smaller than gca_bulldozer_policy_grad_workspace", true, 12};
constexpr GcaGradAgent GCA_GRAD_EXT{"extension_policy_grad", "extension_policy_grad_workspace",
                                    "workspace smaller than gca_extension_policy_grad_workspace", true, 15};

// a workspace query answers -1 where this refuses
static inline int gca_check_policy_grad_workspace(const GcaGradAgent& a, const gca_policy* p, int C, int N) {
    if (!(p && p->radius >= 0 && p->radius <= 31 && p->hidden >= 32 && p->hidden <= 256 &&
          (p->hidden & (p->hidden - 1)) == 0 && C >= 2 && C % 2 == 0 && C <= GCA_POLICY_C_MAX && N >= 1))
        return gca_refuse(a.who_ws, "radius in [0, 31], hidden a power of two in [32, 256], "
                                    "C = 2 Hc Wc at most 15088, N >= 1");
    return GCA_OK;
}

static inline bool gca_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// *pl: the plan of the checked call. The alignment is the device's requirement, and the host build keeps it so that
// a workspace or a policy moves between the builds as it is.
static inline int gca_check_policy_grad(const GcaGradAgent& a, const gca_policy* p, int C, const void* local,
                                        const void* coarse, const void* action, const void* old_logits,
                                        const void* advantage, const void* returns, int64_t T, const void* idx, int N,
                                        float clip_coef, const void* g_w_local, const void* g_w_coarse,
                                        const void* g_b1, const void* g_w_out, const void* g_b2, const void* stats,
                                        const void* workspace, int64_t workspace_bytes, PpoPlan* pl) {
    if (const int st = a.bdz ? gca_check_bdz_policy(a.who, p) : gca_check_policy(p)) return st;
    if (!(local && coarse && action && old_logits && advantage && returns)) return gca_refuse(a.who, "null record");
    if (!(g_w_local && g_w_coarse && g_b1 && g_w_out && g_b2 && stats && workspace))
        return gca_refuse(a.who, "null output or workspace");
    if (const int st = gca_check_policy_c(a.who, C)) return st;
    if (!(T >= 1 && T < (1ll << 31))) return gca_refuse(a.who, "1 <= T < 2^31");
    if (!(N >= 1)) return gca_refuse(a.who, "N >= 1");
    if (!(idx || N <= T)) return gca_refuse(a.who, "N <= T without idx");
    if (!(clip_coef >= 0.0f)) return gca_refuse(a.who, "clip_coef >= 0");
    const int S = 2 * p->radius + 1, Hd = p->hidden;
    *pl = ppo_plan(S * S, C, Hd, N, a.nout);
    if (!(workspace_bytes >= pl->bytes)) return gca_refuse(a.who, a.short_ws);
    if (!(gca_policy_weights_aligned(p) && (((uintptr_t)workspace | (uintptr_t)p->b1) & 15u) == 0))
        return gca_refuse(a.who, "workspace, w_local, w_coarse and b1 16-B aligned");
    const int64_t wo = (int64_t)Hd * a.nout * 4, b2 = a.nout * 4ll;
    const void* ptrs[11] = {g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats,
                            p->w_local, p->w_coarse, p->b1, p->w_out, p->b2};
    const int64_t sizes[11] = {pl->off_wc * 4, (int64_t)C * Hd * 4, Hd * 4ll, wo, b2, 32,
                               pl->off_wc * 4, (int64_t)C * Hd * 4, Hd * 4ll, wo, b2};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 11; ++j)
            if (gca_overlap(ptrs[i], sizes[i], ptrs[j], sizes[j]))
                return gca_refuse(a.who, "the outputs may alias neither each other nor the weights");
    return GCA_OK;
}

// The agents of the gca_*_policy_grad_vclip calls: the plain entries' checks under their own names. The plain entries'
// workspace query serves them, so the refusal of a short workspace names that one.
constexpr GcaGradAgent GCA_GRAD_HELI_VCLIP{"helicopter_policy_grad_vclip", "helicopter_policy_grad_workspace",
                                           "workspace smaller than gca_helicopter_policy_grad_workspace", false, 10};
constexpr GcaGradAgent GCA_GRAD_BDZ_VCLIP{"bulldozer_policy_grad_vclip", "bulldozer_policy_grad_workspace",
                                          "workspace smaller than gca_bulldozer_policy_grad_workspace", true, 12};
constexpr GcaGradAgent GCA_GRAD_EXT_VCLIP{"extension_policy_grad_vclip", "extension_policy_grad_workspace",
                                          "workspace smaller than gca_extension_policy_grad_workspace", true, 15};

// What a _vclip call asks beyond gca_check_policy_grad (which speaks first): the recorded values, and a vstats (f32 [3],
// nullable) that overlaps neither the other outputs nor the weights.
static inline int gca_check_policy_grad_vclip(const GcaGradAgent& a, const gca_policy* p, int C, const void* local,
                                              const void* coarse, const void* action, const void* old_logits,
                                              const void* old_value, const void* advantage, const void* returns,
                                              int64_t T, const void* idx, int N, float clip_coef,
                                              const void* g_w_local, const void* g_w_coarse, const void* g_b1,
                                              const void* g_w_out, const void* g_b2, const void* stats,
                                              const void* vstats, const void* workspace, int64_t workspace_bytes,
                                              PpoPlan* pl) {
    if (const int st = gca_check_policy_grad(a, p, C, local, coarse, action, old_logits, advantage, returns, T, idx, N,
                                             clip_coef, g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats, workspace,
                                             workspace_bytes, pl))
        return st;
    if (!old_value) return gca_refuse(a.who, "null record");
    if (vstats) {
        const int Hd = p->hidden;
        const int64_t wo = (int64_t)Hd * a.nout * 4, b2 = a.nout * 4ll;
        const void* ptrs[11] = {g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats,
                                p->w_local, p->w_coarse, p->b1, p->w_out, p->b2};
        const int64_t sizes[11] = {pl->off_wc * 4, (int64_t)C * Hd * 4, Hd * 4ll, wo, b2, 32,
                                   pl->off_wc * 4, (int64_t)C * Hd * 4, Hd * 4ll, wo, b2};
        for (int j = 0; j < 11; ++j)
            if (gca_overlap(vstats, 12, ptrs[j], sizes[j]))
                return gca_refuse(a.who, "the outputs may alias neither each other nor the weights");
    }
    return GCA_OK;
}

// the host build alone can read idx (host memory there) before it indexes with it
static inline int gca_check_policy_grad_idx(const GcaGradAgent& a, const int32_t* idx, int N, int64_t T) {
    if (idx)
        for (int t = 0; t < N; ++t)
            if (!(idx[t] >= 0 && idx[t] < T)) return gca_refuse(a.who, "idx outside [0, T)");
    return GCA_OK;
}

// ----------------------------------------------------------------- the optimizer
// a workspace query answers -1 where this refuses
static inline int gca_check_adam_step_workspace(int64_t total_elements) {
    GCA_CHECK_ARG(total_elements >= 1, "adam_step_workspace: total_elements >= 1");
    return GCA_OK;
}

// *total: the elements of the checked call's tensors
static inline int gca_check_adam_step(const gca_adam_tensors* t, const void* state, float b1, float b2, float eps,
                                      int64_t steps_per_iteration, int64_t num_iterations, const void* info_out,
                                      const void* workspace, int64_t workspace_bytes, int64_t* total) {
    GCA_CHECK_ARG(t && state && workspace, "adam: null tensor table, state or workspace");
    GCA_CHECK_ARG(t->n >= 1 && t->n <= GCA_ADAM_MAX_TENSORS, "adam: 1 to 8 tensors");
    *total = 0;
    uintptr_t low = (uintptr_t)state | (uintptr_t)info_out;
    for (int i = 0; i < t->n; ++i) {
        GCA_CHECK_ARG(t->w[i] && t->g[i] && t->m[i] && t->v[i], "adam: null tensor pointer");
        GCA_CHECK_ARG(t->len[i] >= 1 && t->len[i] < (1ll << 31), "adam: tensor lengths in [1, 2^31)");
        *total += t->len[i];
        low |= (uintptr_t)t->w[i] | (uintptr_t)t->g[i] | (uintptr_t)t->m[i] | (uintptr_t)t->v[i];
    }
    GCA_CHECK_ARG((low & 3u) == 0, "adam: tensors, state and info_out 4-B aligned");
    GCA_CHECK_ARG(((uintptr_t)workspace & 7u) == 0, "adam: workspace 8-B aligned");
    GCA_CHECK_ARG(b1 >= 0.0f && b1 < 1.0f && b2 >= 0.0f && b2 < 1.0f, "adam: b1 and b2 in [0, 1)");
    GCA_CHECK_ARG(eps >= 0.0f, "adam: eps >= 0");
    GCA_CHECK_ARG((steps_per_iteration == 0 && num_iterations == 0) || (steps_per_iteration >= 1 && num_iterations >= 1),
                  "adam: steps_per_iteration and num_iterations both 0 (no annealing) or both >= 1");
    GCA_CHECK_ARG(workspace_bytes >= adam_workspace_bytes(*total), "adam: workspace smaller than gca_adam_step_workspace");
    return GCA_OK;
}

static inline int gca_check_permutation(const void* counter, int64_t T, int rows, const void* out) {
    GCA_CHECK_ARG(out, "permutation: null out");
    GCA_CHECK_ARG(T >= 1 && T < (1ll << 31), "permutation: 1 <= T < 2^31");
    GCA_CHECK_ARG(rows >= 1 && rows <= 65535, "permutation: 1 <= rows <= 65535");
    GCA_CHECK_ARG((((uintptr_t)out | (uintptr_t)counter) & 3u) == 0, "permutation: out and counter 4-B aligned");
    return GCA_OK;
}
