// gca_cpu.cpp — the host backend of the C-ABI (libgca_cpu.so): the same gca.h symbols as libgca_hip.so for the
// entry points whose work is O(1) per env or runs on tiny grids, with HOST pointers and `stream` ignored.
//
// Why it exists: BASELINE config 1 (ForestFireHelicopter5x5, "NumPy CPU operator path, no GPU") and the single-env
// Move / Modify / ModifyJax drop-ins on host arrays do a few dozen bytes of work per call; a device round trip per
// call costs 10-100x that work (VERDICT r02 "What's missing" 3). The Python layer dispatches here for host arrays of
// at most GCA_HOST_MAX_CELLS cells per env (and for the O(1) Move / Modify family on host arrays); device tensors
// and larger grids always take the HIP kernels. Product code, not the oracle: tests/ compare it with the oracle and
// with the reference's golden vectors exactly like the HIP path.
//
// Semantics (bit-identical to the HIP kernels of the same name):
//   gca_count_cells   ca_env.py:94-99                      (gca_util.hip)
//   gca_move_modify   move_modify.py:37-134                (gca_env.hip move_modify_kernel)
//   gca_ds_count_draws / gca_ds_step  ca_DrosselSchwabl.py:32-66 (gca_ds.hip), exact-stream and Philox modes
//   gca_helicopter_step  helicopter.py:220-236 + ca_env.py:27-48 (gca_heli.hip), the batched env step's twin
//   gca_helicopter_rollout  K of those steps with per-step records (gca_heli.hip), the resident rollout's twin
//   gca_bulldozer_reset_where  bulldozer.py:221-275 + ca_env.py:64-81 (gca_reset.hip), the per-env reset's twin
//   gca_policy_observation  the batched envs' policy observation (gca_policy_obs.hip), pinned by tests/_policy_obs_ref.py
//   gca_helicopter_policy_act / gca_helicopter_policy_rollout  the policy network and the closed-loop rollout
//                     (gca_heli.hip, gca_policy_dev.h), in gca.h's summation order
//   gca_bulldozer_policy_act  the bulldozer policy network alone (gca_policy_dev.h), in gca.h's summation order;
//                     gca_bulldozer_policy_rollout needs the Windy CA and is in the device build only
//   gca_advanced_policy_act  the Advanced env's observe-and-act (gca_adv_policy.hip) as the observation followed by
//                     the bulldozer policy
//   gca_advanced_policy_observation / gca_advanced_policy_act_retardant  the same with the env's retardant in the
//                     observation (gca_adv_policy.hip), pinned by tests/_retardant_obs_ref.py
//   gca_advanced_display / gca_extension_policy_act / gca_advanced_policy_act_display / gca_extension_policy_grad(..)
//                     the extension agent (gca_adv_policy.hip, gca_ppo.hip): the displayed plane in plain loops, the
//                     network with fifteen outputs, the one call as the three it is defined by, the three-head gradient;
//                     pinned by tests/_extension_policy_ref.py
//   gca_gae / gca_helicopter_policy_grad(_workspace) / gca_bulldozer_policy_grad(_workspace)  the PPO update
//                     (gca_ppo.hip): the GAE recurrence bit for bit, the loss gradient of either head layout in double
//                     as a second yardstick; gca_*_policy_grad_vclip the same with the reference's clipped value loss
//   gca_adam_step(_workspace) / gca_permutation  the optimizer and the minibatch shuffle (gca_opt.hip), bit for bit
//   gca_philox        Random123 Philox4x32-10 (KAT hook)
//
// Arguments: every entry point first calls its check function of gca_args.h, the same one the device build calls, so
// both builds refuse the same arguments with the same words. The only checks written here are the two that the host
// alone can make (the idx scan of the two policy_grad entry points, the permutation walk's cap) and the rollout's coarse-map
// limit, which the host applies for every K; each says so where it stands.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gca_args.h"

static thread_local char g_err[512] = "";

// this library's own copy of the setter that gca_args.h declares (hidden there)
void gca_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

struct u32x4 {
    uint32_t x, y, z, w;
};

inline u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)M0 * c.x;
        const uint64_t p1 = (uint64_t)M1 * c.z;
        c = u32x4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

inline double u01_f64(uint32_t hi, uint32_t lo) { return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1.0p-53; }

// Move.update (move_modify.py:37-67): the four set tests run in order on the running (row, col), each against the
// bounds of the position it started from.
inline void move_pos(int a, int& row, int& col, int H, int W, const gca_bulldozer_params& p) {
    const bool valid_up = row > 0, valid_down = row < H - 1, valid_left = col > 0, valid_right = col < W - 1;
    if (((p.up_mask >> a) & 1) && valid_up) row -= 1;
    if (((p.down_mask >> a) & 1) && valid_down) row += 1;
    if (((p.left_mask >> a) & 1) && valid_left) col -= 1;
    if (((p.right_mask >> a) & 1) && valid_right) col += 1;
}

// ForestFire.update's per-cell draw flag (ca_DrosselSchwabl.py:40-60): a TREE without a burning Moore neighbour
// (padding = EMPTY) and an EMPTY cell each consume one uniform.
inline bool has_fire_nb(const uint8_t* g, int r, int c, int H, int W, int fire) {
    for (int dr = -1; dr <= 1; ++dr) {
        const int rr = r + dr;
        if (rr < 0 || rr >= H) continue;
        for (int dc = -1; dc <= 1; ++dc) {
            const int cc = c + dc;
            if ((dr | dc) == 0 || cc < 0 || cc >= W) continue;
            if (g[rr * W + cc] == fire) return true;
        }
    }
    return false;
}

}  // namespace

extern "C" const char* gca_last_error(void) { return g_err; }
extern "C" int gca_version(void) { return 1; }

extern "C" int gca_philox(const uint32_t* ctr, uint32_t key0, uint32_t key1, uint32_t* out, int64_t n, void*) {
    if (const int st = gca_check_philox(ctr, out, n)) return st;
    for (int64_t i = 0; i < n; ++i) {
        const u32x4 x = philox4x32_10(u32x4{ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]}, key0, key1);
        out[4 * i] = x.x;
        out[4 * i + 1] = x.y;
        out[4 * i + 2] = x.z;
        out[4 * i + 3] = x.w;
    }
    return GCA_OK;
}

extern "C" int gca_count_cells(const uint8_t* grid, int E, int H, int W, int v0, int v1, int v2, int32_t* counts,
                               void*) {
    if (const int st = gca_check_count_cells(grid, E, H, W, counts)) return st;
    const int64_t HW = (int64_t)H * W;
    for (int e = 0; e < E; ++e) {
        int32_t hist[256] = {0};
        const uint8_t* g = grid + e * HW;
        for (int64_t i = 0; i < HW; ++i) ++hist[g[i]];
        counts[3 * e] = hist[v0 & 0xFF];
        counts[3 * e + 1] = hist[v1 & 0xFF];
        counts[3 * e + 2] = hist[v2 & 0xFF];
    }
    return GCA_OK;
}

extern "C" int gca_move_modify(const gca_bulldozer_params* p, const int32_t* action, int32_t* pos, uint8_t* grid, int H,
                               int W, uint8_t* hit, int E, void*) {
    if (const int st = gca_check_move_modify(p, action, pos, H, W, E)) return st;
    for (int e = 0; e < E; ++e) {
        int row = pos[2 * e], col = pos[2 * e + 1];
        const int a0 = action[2 * e], a1 = action[2 * e + 1];
        if (a0 >= 0 && a0 < 32) move_pos(a0, row, col, H, W, *p);
        pos[2 * e] = row;
        pos[2 * e + 1] = col;
        uint8_t h = 0;
        // MoveModify (move_modify.py:128-134): Modify at the NEW position; a position outside the grid (a caller's
        // own value, never produced by Move) is refused like the device's bounds of the grid buffer
        if (grid && a1) {
            if (row < 0 || row >= H || col < 0 || col >= W) {
                gca_set_error("move_modify: position (%d, %d) outside the %dx%d grid", row, col, H, W);
                return GCA_ERR_ARG;
            }
            uint8_t* g = grid + (int64_t)e * H * W + (int64_t)row * W + col;
            const int nv = p->effect[*g];
            if (nv >= 0) {
                *g = (uint8_t)nv;
                h = 1;
            }
        }
        if (hit) hit[e] = h;
    }
    return GCA_OK;
}

extern "C" int gca_ds_count_draws(const uint8_t* grid, int E, int H, int W, int empty, int tree, int fire,
                                  int32_t* n_draws, void*) {
    if (const int st = gca_check_ds_count_draws(grid, E, H, W, n_draws)) return st;
    const int64_t HW = (int64_t)H * W;
    for (int e = 0; e < E; ++e) {
        const uint8_t* g = grid + e * HW;
        int32_t n = 0;
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const int x = g[r * W + c];
                n += x == empty || (x == tree && !has_fire_nb(g, r, c, H, W, fire));
            }
        n_draws[e] = n;
    }
    return GCA_OK;
}

extern "C" int gca_ds_step(const uint8_t* grid_in, uint8_t* grid_out, int E, int H, int W, int empty, int tree,
                           int fire, const double* thresholds, const double* uniforms, const int64_t* uniform_offset,
                           uint64_t seed, const uint32_t* rng_step, int env_offset, int32_t* counts, void*) {
    if (const int st = gca_check_ds_step(grid_in, grid_out, E, H, W, thresholds, uniforms, uniform_offset)) return st;
    const int64_t HW = (int64_t)H * W;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int e = 0; e < E; ++e) {
        const uint8_t* g = grid_in + e * HW;
        uint8_t* o = grid_out + e * HW;
        const double thr_fire = thresholds[2 * e], thr_tree = thresholds[2 * e + 1];
        const uint32_t step = rng_step ? rng_step[e] : 0u;
        int64_t j = uniforms ? uniform_offset[e] : 0;
        int32_t cE = 0, cT = 0, cF = 0;
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const int cell = r * W + c;
                const int x = g[cell];
                int nx = x;
                if (x == fire) {
                    nx = empty;  // :58-59
                } else if (x == tree && has_fire_nb(g, r, c, H, W, fire)) {
                    nx = fire;  // :44-47
                } else if (x == tree || x == empty) {
                    double u;
                    if (uniforms) {
                        u = uniforms[j++];
                    } else {
                        const u32x4 rx =
                            philox4x32_10(u32x4{(uint32_t)cell, (uint32_t)(env_offset + e), step, GCA_TAG_DS_CELL}, k0, k1);
                        u = u01_f64(rx.x, rx.y);
                    }
                    if (x == tree) nx = u < thr_fire ? fire : tree;  // :48-53
                    else nx = u < thr_tree ? tree : empty;           // :54-57
                }
                o[cell] = (uint8_t)nx;
                cE += nx == empty;
                cT += nx == tree;
                cF += nx == fire;
            }
        if (counts) {
            counts[3 * e] = cE;
            counts[3 * e + 1] = cT;
            counts[3 * e + 2] = cF;
        }
    }
    return GCA_OK;
}

// One batched ForestFireHelicopter env step of every env (gca_heli.hip) in plain loops: helicopter.py:220-236 +
// ca_env.py:27-48. rec_reward / rec_hit (nullable): gca_helicopter_rollout's record rows of this step.
static void helicopter_step_host(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                                 const int32_t* action, uint64_t action_seed, int32_t* action_out,
                                 const double* thresholds, int32_t* freeze, uint32_t* rng_step, uint8_t* parity,
                                 uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts,
                                 uint8_t* hit, double* reward, int64_t* steps_elapsed, int E, double* rec_reward,
                                 uint8_t* rec_hit) {
    const int64_t HW = (int64_t)H * W;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    gca_bulldozer_params mv = {};  // the helicopter's action sets (helicopter.py:56-62); only the masks are read
    mv.up_mask = 0x007, mv.down_mask = 0x1C0, mv.left_mask = 0x049, mv.right_mask = 0x124;
    for (int e = 0; e < E; ++e) {
        const uint32_t rs = rng_step[e], env_id = (uint32_t)(env_offset + e);
        int32_t act;
        if (action) {
            act = action[e];
        } else {  // column 0 of gca_random_actions
            const u32x4 x = philox4x32_10(u32x4{0u, env_id, rs, GCA_TAG_ACTION}, (uint32_t)action_seed,
                                          (uint32_t)(action_seed >> 32));
            act = (int32_t)(((uint64_t)x.x * 9u) >> 32);
        }
        if (action_out) action_out[e] = act;
        int row = pos[2 * e], col = pos[2 * e + 1];
        move_pos(act < 0 ? 0 : (act > 8 ? 8 : act), row, col, H, W, mv);
        pos[2 * e] = row;
        pos[2 * e + 1] = col;
        const bool do_ca = freeze[e] == 0;
        uint8_t* g = (parity[e] ? buf1 : buf0) + e * HW;
        uint8_t h = 0;
        if (do_ca) {
            uint8_t* o = (parity[e] ? buf0 : buf1) + e * HW;
            const double thr_fire = thresholds[2 * e], thr_tree = thresholds[2 * e + 1];
            int32_t cE = 0, cT = 0, cF = 0;
            for (int r = 0; r < H; ++r)
                for (int c = 0; c < W; ++c) {
                    const int cell = r * W + c;
                    const int x = g[cell];
                    int nx = x;
                    if (x == fire) {
                        nx = empty;
                    } else if (x == tree && has_fire_nb(g, r, c, H, W, fire)) {
                        nx = fire;
                    } else if (x == tree || x == empty) {
                        const u32x4 rx = philox4x32_10(u32x4{(uint32_t)cell, env_id, rs, GCA_TAG_DS_CELL}, k0, k1);
                        const double u = u01_f64(rx.x, rx.y);
                        if (x == tree) nx = u < thr_fire ? fire : tree;
                        else nx = u < thr_tree ? tree : empty;
                    }
                    if (r == row && c == col && nx == fire) {  // Modify {FIRE: EMPTY} on the post-CA grid
                        nx = empty;
                        h = 1;
                    }
                    o[cell] = (uint8_t)nx;
                    cE += nx == empty;
                    cT += nx == tree;
                    cF += nx == fire;
                }
            counts[3 * e] = cE;
            counts[3 * e + 1] = cT;
            counts[3 * e + 2] = cF;
            parity[e] = parity[e] ? 0 : 1;
            freeze[e] = max_freeze;
        } else {
            if (row >= 0 && row < H && col >= 0 && col < W && g[(int64_t)row * W + col] == fire) {
                g[(int64_t)row * W + col] = (uint8_t)empty;
                h = 1;
                counts[3 * e] += 1;
                counts[3 * e + 2] -= 1;
            }
            freeze[e] -= 1;
        }
        hit[e] = h;
        const double n = (double)HW;
        const double qt = (double)counts[3 * e + 1] / n, qf = (double)counts[3 * e + 2] / n;
        reward[e] = qt - qf;  // helicopter.py:120-135 (built with -ffp-contract=off)
        if (rec_reward) rec_reward[e] = reward[e];
        if (rec_hit) rec_hit[e] = h;
        rng_step[e] = rs + 1u;
        steps_elapsed[e] += 1;
    }
}

// The batched ForestFireHelicopter env step (gca_heli.hip): `meet` is not used (nothing runs in parts here) and is
// left as it is.
extern "C" int gca_helicopter_step(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                                   const int32_t* action, uint64_t action_seed, int32_t* action_out,
                                   const double* thresholds, int32_t* freeze, uint32_t* rng_step, uint8_t* parity,
                                   uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts,
                                   uint8_t* hit, double* reward, int64_t* steps_elapsed, uint64_t*, int E, void*) {
    if (const int st = gca_check_heli_env("helicopter_step", empty, tree, fire, max_freeze, thresholds, freeze, rng_step,
                                          parity, buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E))
        return st;
    helicopter_step_host(empty, tree, fire, max_freeze, seed, env_offset, action, action_seed, action_out, thresholds,
                         freeze, rng_step, parity, buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E,
                         nullptr, nullptr);
    return GCA_OK;
}

// K env steps (gca_heli.hip's resident rollout) in plain loops: K times the step above, plus the records.
extern "C" int gca_helicopter_rollout(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                                      const int32_t* actions, uint64_t action_seed, int K, int32_t* action_out,
                                      double* reward_out, uint8_t* hit_out, const double* thresholds, int32_t* freeze,
                                      uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W,
                                      int32_t* pos, int32_t* counts, uint8_t* hit, double* reward,
                                      int64_t* steps_elapsed, int E, void*) {
    if (const int st = gca_check_heli_env("helicopter_rollout", empty, tree, fire, max_freeze, thresholds, freeze,
                                          rng_step, parity, buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E))
        return st;
    if (const int st = gca_check_k("helicopter_rollout", K)) return st;
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * (size_t)E;
        helicopter_step_host(empty, tree, fire, max_freeze, seed, env_offset, actions ? actions + o : nullptr,
                             action_seed, action_out ? action_out + o : nullptr, thresholds, freeze, rng_step, parity,
                             buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E,
                             reward_out ? reward_out + o : nullptr, hit_out ? hit_out + o : nullptr);
    }
    return GCA_OK;
}

// _seeding._splitmix64 / env_integers restated: an integer in [0, span) per (seed, global env id, tag).
static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static inline int32_t env_integer(uint64_t seed, uint64_t env_id, uint32_t tag, uint32_t span) {
    const uint64_t r = splitmix64(splitmix64(seed ^ (uint64_t)tag) ^ splitmix64(env_id));
    return (int32_t)(((r >> 32) * (uint64_t)span) >> 32);
}

// The per-env reset of the batched ForestFireBulldozer env (gca_reset.hip) in plain loops: bulldozer.py:221-275 +
// ca_env.py:64-81. buf1 is checked and left as it is.
extern "C" int gca_bulldozer_reset_where(const gca_bulldozer_params* p, uint64_t reset_seed, const uint8_t* mask,
                                         int64_t max_steps, int64_t set_episode, const float* cdf,
                                         const uint8_t* values, uint8_t* done, uint8_t* terminated_out,
                                         uint8_t* truncated_out, uint32_t* episode, int64_t* last_length_out,
                                         double* accu, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W,
                                         int32_t* pos, int32_t* counts, uint8_t* hit, int64_t* steps_elapsed, int E,
                                         void*) {
    if (const int st = gca_check_bulldozer_reset_where(p, max_steps, set_episode, cdf, values, done, episode, accu,
                                                       parity, buf0, buf1, H, W, pos, counts, hit, steps_elapsed, E))
        return st;
    const int64_t HW = (int64_t)H * W;
    const uint32_t k0 = (uint32_t)reset_seed, k1 = (uint32_t)(reset_seed >> 32);
    const uint32_t span_h = (uint32_t)(H / 12 > 1 ? H / 12 : 1), span_w = (uint32_t)(W / 12 > 1 ? W / 12 : 1);
    for (int e = 0; e < E; ++e) {
        const bool was_done = done[e] != 0;
        const int64_t se = steps_elapsed[e];
        const bool by_limit = max_steps > 0 && se >= max_steps;
        const bool selected = (mask ? mask[e] != 0 : was_done) || by_limit;
        if (terminated_out) terminated_out[e] = was_done ? 1 : 0;
        if (truncated_out) truncated_out[e] = (by_limit && !was_done) ? 1 : 0;
        if (!selected) continue;
        const uint32_t k = set_episode >= 0 ? (uint32_t)set_episode : episode[e] + 1u;
        const uint64_t env_id = (uint64_t)(p->env_offset + e);
        const uint32_t ktag = (k & 0xFFFFFFu) << 8;
        uint8_t* g = buf0 + e * HW;
        for (int64_t i = 0; i < HW; ++i) {
            const u32x4 x = philox4x32_10(u32x4{(uint32_t)(i >> 2), (uint32_t)env_id, k, GCA_TAG_INIT}, k0, k1);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
            const float u = (float)(xs[i & 3] >> 8) * 0x1.0p-24f;
            g[i] = u < cdf[0] ? values[0] : (u < cdf[1] ? values[1] : values[2]);
        }
        const int fr = 3 * H / 4 + env_integer(reset_seed, env_id, 1u | ktag, span_h);
        const int fc = W / 4 + env_integer(reset_seed, env_id, 2u | ktag, span_w);
        g[(int64_t)fr * W + fc] = (uint8_t)p->fire;
        int32_t cE = 0, cT = 0, cF = 0;
        for (int64_t i = 0; i < HW; ++i) {
            cE += g[i] == (uint8_t)p->empty;
            cT += g[i] == (uint8_t)p->tree;
            cF += g[i] == (uint8_t)p->fire;
        }
        counts[3 * e] = cE;
        counts[3 * e + 1] = cT;
        counts[3 * e + 2] = cF;
        pos[2 * e] = H / 4 + env_integer(reset_seed, env_id, 3u | ktag, span_h);
        pos[2 * e + 1] = 3 * W / 4 + env_integer(reset_seed, env_id, 4u | ktag, span_w);
        if (last_length_out) last_length_out[e] = se;
        episode[e] = k;
        parity[e] = 0;
        accu[e] = 0.0;
        done[e] = 0;
        hit[e] = 0;
        steps_elapsed[e] = 0;
    }
    return GCA_OK;
}

// The policy observation of the batched envs (gca_policy_obs.hip) in plain loops. `form` is validated with the other
// arguments and otherwise ignored.
extern "C" int gca_policy_observation(const uint8_t* buf0, const uint8_t* buf1, const uint8_t* parity,
                                      const int32_t* pos, int E, int H, int W, int empty, int tree, int fire, int radius,
                                      int block, int form, uint8_t* local_out, float* coarse_out, void*) {
    if (const int st = gca_check_policy_observation(buf0, buf1, parity, pos, E, H, W, empty, tree, fire, radius, block,
                                                    form, local_out, coarse_out))
        return st;
    const int64_t HW = (int64_t)H * W;
    const int S = 2 * radius + 1, Hc = (H + block - 1) / block, Wc = (W + block - 1) / block;
    const float inv = 1.0f / (float)(block * block);
    for (int e = 0; e < E; ++e) {
        const uint8_t* g = ((parity && parity[e]) ? buf1 : buf0) + e * HW;
        if (local_out) {
            uint8_t* out = local_out + (int64_t)e * S * S;
            for (int i = 0; i < S; ++i)
                for (int j = 0; j < S; ++j) {
                    const int64_t r = (int64_t)pos[2 * e] - radius + i, c = (int64_t)pos[2 * e + 1] - radius + j;
                    uint8_t cls = 3;
                    if (r >= 0 && r < H && c >= 0 && c < W) {
                        const int v = g[r * W + c];
                        cls = v == tree ? 1 : (v == fire ? 2 : 0);
                    }
                    out[i * S + j] = cls;
                }
        }
        if (coarse_out) {
            float* C = coarse_out + (int64_t)e * 2 * Hc * Wc;
            for (int bi = 0; bi < Hc; ++bi)
                for (int bj = 0; bj < Wc; ++bj) {
                    const int r1 = (bi + 1) * block < H ? (bi + 1) * block : H;
                    const int c1 = (bj + 1) * block < W ? (bj + 1) * block : W;
                    int32_t cT = 0, cF = 0;
                    for (int r = bi * block; r < r1; ++r)
                        for (int c = bj * block; c < c1; ++c) {
                            const int v = g[(int64_t)r * W + c];
                            cT += v == tree;
                            cF += v == fire;
                        }
                    C[bi * Wc + bj] = (float)cT * inv;
                    C[Hc * Wc + bi * Wc + bj] = (float)cF * inv;
                }
        }
    }
    return GCA_OK;
}

// ---------------------------------------------------------------- the helicopter policy (gca.h "helicopter policy")
// exp_f32 of gca_common.h restated with C99 fmaf / rintf (round to nearest even, the default mode): every step is one
// correctly rounded IEEE operation, so the bits are the device's.
static inline float exp_f32_host(float x) {
    x = fminf(fmaxf(x, -80.0f), 80.0f);
    const float kf = rintf(x * 1.44269504088896341f);
    const int k = (int)kf;
    float r = fmaf(kf, -0.693145751953125f, x);
    r = fmaf(kf, -1.42860682030941723212e-6f, r);
    float p = 1.98412698412698413e-4f;
    p = fmaf(p, r, 1.38888888888888889e-3f);
    p = fmaf(p, r, 8.33333333333333333e-3f);
    p = fmaf(p, r, 4.16666666666666667e-2f);
    p = fmaf(p, r, 1.66666666666666667e-1f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r * r, r);
    p = p + 1.0f;
    uint32_t bits;
    memcpy(&bits, &p, 4);
    bits += (uint32_t)k << 23;
    memcpy(&p, &bits, 4);
    return p;
}

// One env's NOUT outputs in gca.h's order, for both agents (10: the helicopter, 12: the bulldozer): the hidden layer
// and the heads. loc [S*S], coarse [C]; out [NOUT].
static void policy_outputs_host(const gca_policy* p, int NOUT, int C, const uint8_t* loc, const float* coarse,
                                float* out) {
    const int S = 2 * p->radius + 1, SS = S * S, N = SS + C, Hd = p->hidden, G = 1024 / Hd;
    float h[256];
    for (int j = 0; j < Hd; ++j) {
        float hj = p->b1[j];
        for (int g = 0; g < G; ++g) {
            float acc = 0.0f;
            for (int n = g; n < N; n += G) {
                if (n < SS) acc = acc + p->w_local[((size_t)n * 4 + (loc[n] & 3)) * Hd + j];
                else acc = acc + p->w_coarse[(size_t)(n - SS) * Hd + j] * coarse[n - SS];
            }
            hj = hj + acc;
        }
        h[j] = hj > 0.0f ? hj : 0.0f;
    }
    for (int o = 0; o < NOUT; ++o) {
        float q[16];
        for (int r = 0; r < 16; ++r) {
            float acc = 0.0f;
            for (int j = r; j < Hd; j += 16) acc = acc + p->w_out[j * NOUT + o] * h[j];
            q[r] = acc;
        }
        for (int half = 8; half >= 1; half >>= 1)
            for (int r = 0; r < half; ++r) q[r] = q[r] + q[r + half];
        out[o] = p->b2[o] + q[0];
    }
}

static inline float u01_f32_host(uint32_t x) { return (float)(x >> 8) * 0x1.0p-24f; }

// The move rule both agents use on the nine logits l (gca.h "sampling"): the first maximum when greedy, else the
// first i with t < c_i under the uniform of the Philox word x.
static int32_t policy_move_host(const float* l, int greedy, uint32_t x) {
    float m = l[0];
    int32_t first = 0;
    for (int i = 1; i < 9; ++i)
        if (l[i] > m) {
            m = l[i];
            first = i;
        }
    if (greedy) return first;
    float c[9], s = 0.0f;
    for (int i = 0; i < 9; ++i) {
        s = s + exp_f32_host(l[i] - m);
        c[i] = s;
    }
    const float t = u01_f32_host(x) * c[8];
    for (int i = 0; i < 8; ++i)
        if (t < c[i]) return i;
    return 8;
}

// One env's outputs (out [10]: the logits and the value) and action: outputs, draw, sample.
static int32_t policy_eval_host(const gca_heli_policy* p, int C, const uint8_t* loc, const float* coarse,
                                uint32_t env_id, uint32_t rs, uint64_t policy_seed, int greedy, float* out) {
    policy_outputs_host(p, 10, C, loc, coarse, out);
    const u32x4 x = philox4x32_10(u32x4{0u, env_id, rs, GCA_TAG_POLICY}, (uint32_t)policy_seed,
                                  (uint32_t)(policy_seed >> 32));
    return policy_move_host(out, greedy, x.x);
}

static void policy_act_host(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                            const uint32_t* rng_step, int env_offset, uint64_t policy_seed, int greedy,
                            int32_t* action, float* logits, float* value, int E) {
    const size_t SS = (size_t)(2 * p->radius + 1) * (2 * p->radius + 1);
    for (int e = 0; e < E; ++e) {
        float out[10];
        action[e] = policy_eval_host(p, C, local + e * SS, coarse + (size_t)e * C, (uint32_t)(env_offset + e),
                                     rng_step[e], policy_seed, greedy, out);
        if (logits) memcpy(logits + (size_t)e * 9, out, 9 * sizeof(float));
        if (value) value[e] = out[9];
    }
}

extern "C" int gca_helicopter_policy_act(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                                         const uint32_t* rng_step, int env_offset, uint64_t policy_seed, int greedy,
                                         int32_t* action, float* logits, float* value, int E, void*) {
    if (const int st = gca_check_policy_act(p, C, local, coarse, rng_step, action, E)) return st;
    policy_act_host(p, C, local, coarse, rng_step, env_offset, policy_seed, greedy, action, logits, value, E);
    return GCA_OK;
}

// K x (observation, act, step) in plain loops, the records' rows written as they come; `scratch` is not needed here.
extern "C" int gca_helicopter_policy_rollout(int empty, int tree, int fire, int max_freeze, uint64_t seed,
                                             int env_offset, const gca_heli_policy* p, uint64_t policy_seed, int greedy,
                                             int K, int32_t* action_out, float* logits_out, float* value_out,
                                             double* reward_out, uint8_t* hit_out, uint8_t* local_out,
                                             float* coarse_out, void*, const double* thresholds, int32_t* freeze,
                                             uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H,
                                             int W, int32_t* pos, int32_t* counts, uint8_t* hit, double* reward,
                                             int64_t* steps_elapsed, int E, void*) {
    if (const int st = gca_check_policy_rollout(empty, tree, fire, max_freeze, p, K, thresholds, freeze, rng_step, parity,
                                                buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E))
        return st;
    const int S = 2 * p->radius + 1, Hc = (H + p->block - 1) / p->block, Wc = (W + p->block - 1) / p->block;
    const int C = 2 * Hc * Wc;
    // the host build has one path and refuses this for every K; the device build only on its way to a launch
    if (const int st = gca_check_rollout_coarse(C, GCA_POLICY_C_MAX)) return st;
    const size_t SS = (size_t)S * S;
    std::vector<int32_t> act((size_t)E);
    std::vector<uint8_t> loc((size_t)E * SS);
    std::vector<float> coa((size_t)E * C);
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * (size_t)E;
        int32_t* act_k = action_out ? action_out + o : act.data();
        uint8_t* loc_k = local_out ? local_out + o * SS : loc.data();
        float* coa_k = coarse_out ? coarse_out + o * C : coa.data();
        if (const int st = gca_policy_observation(buf0, buf1, parity, pos, E, H, W, empty, tree, fire, p->radius,
                                                  p->block, 0, loc_k, coa_k, nullptr))
            return st;
        policy_act_host(p, C, loc_k, coa_k, rng_step, env_offset, policy_seed, greedy, act_k,
                        logits_out ? logits_out + o * 9 : nullptr, value_out ? value_out + o : nullptr, E);
        helicopter_step_host(empty, tree, fire, max_freeze, seed, env_offset, act_k, 0, nullptr, thresholds, freeze,
                             rng_step, parity, buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E,
                             reward_out ? reward_out + o : nullptr, hit_out ? hit_out + o : nullptr);
    }
    return GCA_OK;
}

// ---------------------------------------------------------------- the bulldozer policy (gca.h "bulldozer policy")
// One env's twelve outputs and its (move, shoot): outputs, draw, sample -- the helicopter's move rule, then the shoot
// head.
static void bdz_policy_eval_host(const gca_bulldozer_policy* p, int C, const uint8_t* loc, const float* coarse,
                                 uint32_t step, uint32_t env_id, uint32_t ep, uint64_t policy_seed, int greedy,
                                 float* out, int32_t* act) {
    policy_outputs_host(p, 12, C, loc, coarse, out);
    const u32x4 x = philox4x32_10(u32x4{step, env_id, ep, GCA_TAG_BPOLICY}, (uint32_t)policy_seed,
                                  (uint32_t)(policy_seed >> 32));
    act[0] = policy_move_host(out, greedy, x.x);
    const float s0 = out[9], s1 = out[10];
    if (greedy) {
        act[1] = s1 > s0 ? 1 : 0;
        return;
    }
    const float ms = s1 > s0 ? s1 : s0;
    const float c0 = exp_f32_host(s0 - ms), c1 = c0 + exp_f32_host(s1 - ms);
    act[1] = u01_f32_host(x.y) * c1 < c0 ? 0 : 1;
}

extern "C" int gca_bulldozer_policy_act(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                                        const int64_t* steps_elapsed, const uint32_t* episode, int env_offset,
                                        uint64_t policy_seed, int greedy, int32_t* action, float* logits, float* value,
                                        int E, void*) {
    if (const int st = gca_check_bdz_policy_act(p, C, local, coarse, steps_elapsed, action, E)) return st;
    const size_t SS = (size_t)(2 * p->radius + 1) * (2 * p->radius + 1);
    for (int e = 0; e < E; ++e) {
        float out[12];
        bdz_policy_eval_host(p, C, local + e * SS, coarse + (size_t)e * C, (uint32_t)steps_elapsed[e],
                             (uint32_t)(env_offset + e), episode ? episode[e] : 0u, policy_seed, greedy, out,
                             action + 2 * (size_t)e);
        if (logits) memcpy(logits + (size_t)e * 11, out, 11 * sizeof(float));
        if (value) value[e] = out[11];
    }
    return GCA_OK;
}

// ---------------------------------------------------------------- the extension policy (gca.h "extension policy")
// The bulldozer policy with fifteen outputs: move and shoot by bdz_policy_eval_host's statements on the same draw, the
// extension by the move rule over three logits on the draw's word 2.
static int32_t policy_pick3_host(const float* l, int greedy, uint32_t x) {
    float m = l[0];
    int32_t first = 0;
    for (int i = 1; i < 3; ++i)
        if (l[i] > m) {
            m = l[i];
            first = i;
        }
    if (greedy) return first;
    float c[3], s = 0.0f;
    for (int i = 0; i < 3; ++i) {
        s = s + exp_f32_host(l[i] - m);
        c[i] = s;
    }
    const float t = u01_f32_host(x) * c[2];
    for (int i = 0; i < 2; ++i)
        if (t < c[i]) return i;
    return 2;
}

extern "C" int gca_extension_policy_act(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                                        const int64_t* steps_elapsed, const uint32_t* episode, int env_offset,
                                        uint64_t policy_seed, int greedy, int32_t* action, float* logits, float* value,
                                        int E, void*) {
    if (const int st = gca_check_bdz_policy_act_as("extension_policy_act", p, C, local, coarse, steps_elapsed, action, E))
        return st;
    const size_t SS = (size_t)(2 * p->radius + 1) * (2 * p->radius + 1);
    for (int e = 0; e < E; ++e) {
        float out[15];
        policy_outputs_host(p, 15, C, local + e * SS, coarse + (size_t)e * C, out);
        const u32x4 x = philox4x32_10(u32x4{(uint32_t)steps_elapsed[e], (uint32_t)(env_offset + e),
                                            episode ? episode[e] : 0u, GCA_TAG_BPOLICY},
                                      (uint32_t)policy_seed, (uint32_t)(policy_seed >> 32));
        int32_t* act = action + 3 * (size_t)e;
        act[0] = policy_move_host(out, greedy, x.x);
        const float s0 = out[9], s1 = out[10];
        if (greedy) {
            act[1] = s1 > s0 ? 1 : 0;
        } else {
            const float ms = s1 > s0 ? s1 : s0;
            const float c0 = exp_f32_host(s0 - ms), c1 = c0 + exp_f32_host(s1 - ms);
            act[1] = u01_f32_host(x.y) * c1 < c0 ? 0 : 1;
        }
        act[2] = policy_pick3_host(out + 11, greedy, x.z);
        if (logits) memcpy(logits + (size_t)e * 14, out, 14 * sizeof(float));
        if (value) value[e] = out[14];
    }
    return GCA_OK;
}

// The displayed plane (gca.h "extension policy") in plain loops: per env the day/night, the active channels, the
// selection scan over ROWS, then every cell's value of the channel shown.
extern "C" int gca_advanced_display(const gca_obs_params* p, int E, int H, int W, const uint8_t* grid,
                                    const int32_t* is_night, const int32_t* time_step, const int32_t* choice,
                                    int choice_stride, uint8_t* display_out, void*) {
    if (const int st = gca_check_advanced_display(p, E, H, W, grid, is_night, choice, choice_stride, display_out))
        return st;
    const int64_t HW = (int64_t)H * W;
    for (int e = 0; e < E; ++e) {
        const uint8_t* g = grid + e * HW;
        uint8_t* out = display_out + e * HW;
        bool night = is_night[e] != 0;
        if (time_step && p->day_length > 0 && time_step[e] % p->day_length == 0) night = !night;
        uint32_t on = 0u;
        if (p->enable_extensions && p->n_choices > 0) {
            int c = choice ? choice[(int64_t)e * choice_stride] : 0;
            const int top = (p->n_choices < 8 ? p->n_choices : 8) - 1;
            c = c < 0 ? 0 : (c > top ? top : c);
            for (int i = 0; i < p->n_ext; ++i) on |= (p->ext_lookup[c][i] != 0 ? 1u : 0u) << i;
        }
        auto blur = [&](int r, int c) {
            int s = 0;
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    const int rr = r + dr < 0 ? 0 : (r + dr > H - 1 ? H - 1 : r + dr);
                    const int cc = c + dc < 0 ? 0 : (c + dc > W - 1 ? W - 1 : c + dc);
                    s += g[(int64_t)rr * W + cc];
                }
            return (2 * s + 9) / 18;
        };
        auto transform = [&](int r, int c, int skip_vis, int skip_blur) {
            int v = skip_blur ? g[(int64_t)r * W + c] : blur(r, c);
            if (!skip_vis && v == 3 && !night) v = 0;
            return v;
        };
        auto ext = [&](int i, int r, int c) {
            return ((on >> i) & 1u) ? transform(r, c, p->ext_skip_visibility[i], p->ext_skip_blur[i]) : 0;
        };
        int sel = -1;
        if (on) {
            int fv = -1;
            for (int r = 0; r < H && fv < 0; ++r)
                for (int c = 0; c < W && fv < 0; ++c)
                    for (int i = 0; i < p->n_ext; ++i)
                        if (ext(i, r, c) > 0) fv = r;
            if (fv >= 0) sel = fv < p->n_ext - 1 ? fv : p->n_ext - 1;
        }
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c)
                out[(int64_t)r * W + c] = (uint8_t)(sel >= 0 ? ext(sel, r, c)
                                                            : (p->should_transform ? transform(r, c, 0, 0)
                                                                                   : g[(int64_t)r * W + c]));
    }
    return GCA_OK;
}

// Observe the displayed plane and act (gca.h "extension policy") as the three host functions it is defined by. `choice`
// may be column 2 of `action`: it is read (by the display) before any action is written.
extern "C" int gca_advanced_policy_act_display(const gca_bulldozer_policy* policy, const gca_obs_params* p,
                                               const uint8_t* grid, const int32_t* pos, const int32_t* is_night,
                                               const int32_t* time_step, const int32_t* choice, int choice_stride,
                                               int E, int H, int W, int env_offset, uint64_t policy_seed, int greedy,
                                               int32_t* action, int action_stride, float* logits, float* value,
                                               uint8_t* local_out, float* coarse_out, void*) {
    if (const int st = gca_check_advanced_policy_act_display(policy, p, grid, pos, is_night, time_step, choice,
                                                             choice_stride, E, H, W, action, action_stride))
        return st;
    const int B = policy->block, S = 2 * policy->radius + 1;
    const int C = 2 * ((H + B - 1) / B) * ((W + B - 1) / B);
    std::vector<uint8_t> plane((size_t)E * H * W);
    if (const int st = gca_advanced_display(p, E, H, W, grid, is_night, time_step, choice, choice_stride, plane.data(),
                                            nullptr))
        return st;
    std::vector<uint8_t> loc(local_out ? 0 : (size_t)E * S * S);
    std::vector<float> coa(coarse_out ? 0 : (size_t)E * C);
    uint8_t* loc_p = local_out ? local_out : loc.data();
    float* coa_p = coarse_out ? coarse_out : coa.data();
    if (const int st = gca_policy_observation(plane.data(), nullptr, nullptr, pos, E, H, W, p->empty, p->tree, p->fire,
                                              policy->radius, B, 0, loc_p, coa_p, nullptr))
        return st;
    std::vector<int64_t> se((size_t)E);
    std::vector<int32_t> act(3 * (size_t)E);
    for (int e = 0; e < E; ++e) se[e] = (int64_t)time_step[e];
    if (const int st = gca_extension_policy_act(policy, C, loc_p, coa_p, se.data(), nullptr, env_offset, policy_seed,
                                                greedy, act.data(), logits, value, E, nullptr))
        return st;
    for (int e = 0; e < E; ++e)
        for (int j = 0; j < 3; ++j) action[(size_t)e * action_stride + j] = act[3 * (size_t)e + j];
    return GCA_OK;
}

// The Advanced env's observe-and-act (gca.h "advanced policy") as the two host functions it is defined by: the
// observation of the one plane, then the bulldozer policy on the widened time_step; a record the caller does not keep
// lives in a vector.
extern "C" int gca_advanced_policy_act(const gca_bulldozer_policy* policy, const uint8_t* grid, const int32_t* pos,
                                       const int32_t* time_step, int E, int H, int W, int empty, int tree, int fire,
                                       int env_offset, uint64_t policy_seed, int greedy, int32_t* action,
                                       int action_stride, float* logits, float* value, uint8_t* local_out,
                                       float* coarse_out, void*) {
    if (const int st = gca_check_advanced_policy_act(policy, grid, pos, time_step, E, H, W, empty, tree, fire, action,
                                                     action_stride))
        return st;
    const int B = policy->block, S = 2 * policy->radius + 1;
    const int C = 2 * ((H + B - 1) / B) * ((W + B - 1) / B);
    std::vector<uint8_t> loc(local_out ? 0 : (size_t)E * S * S);
    std::vector<float> coa(coarse_out ? 0 : (size_t)E * C);
    uint8_t* loc_p = local_out ? local_out : loc.data();
    float* coa_p = coarse_out ? coarse_out : coa.data();
    if (const int st = gca_policy_observation(grid, nullptr, nullptr, pos, E, H, W, empty, tree, fire, policy->radius, B,
                                              0, loc_p, coa_p, nullptr))
        return st;
    std::vector<int64_t> se((size_t)E);
    std::vector<int32_t> act(2 * (size_t)E);
    for (int e = 0; e < E; ++e) se[e] = (int64_t)time_step[e];
    if (const int st = gca_bulldozer_policy_act(policy, C, loc_p, coa_p, se.data(), nullptr, env_offset, policy_seed,
                                                greedy, act.data(), logits, value, E, nullptr))
        return st;
    for (int e = 0; e < E; ++e) {
        action[(size_t)e * action_stride] = act[2 * (size_t)e];
        action[(size_t)e * action_stride + 1] = act[2 * (size_t)e + 1];
    }
    return GCA_OK;
}

// The observation with the retardant in it (gca.h "advanced policy") in plain loops on `dousing`: the window and the
// grid's two channels are gca_policy_observation's, copied into the head of each env's feature vector. dous_bits is
// validated and not read.
extern "C" int gca_advanced_policy_observation(const uint8_t* grid, const uint8_t* dousing, const uint16_t* dous_bits,
                                               const int32_t* pos, int E, int H, int W, int empty, int tree, int fire,
                                               int radius, int block, uint8_t* local_out, float* feat_out, void*) {
    if (const int st = gca_check_advanced_policy_observation(grid, dousing, dous_bits, pos, E, H, W, empty, tree, fire,
                                                             radius, block, local_out, feat_out))
        return st;
    const int S = 2 * radius + 1, Hc = (H + block - 1) / block, Wc = (W + block - 1) / block;
    const int64_t HW = (int64_t)H * W, HcWc = (int64_t)Hc * Wc, C2 = gca_retardant_c2(H, W, block, radius);
    std::vector<float> coa(feat_out ? (size_t)E * 2 * HcWc : 0);
    if (const int st = gca_policy_observation(grid, nullptr, nullptr, pos, E, H, W, empty, tree, fire, radius, block, 0,
                                              local_out, feat_out ? coa.data() : nullptr, nullptr))
        return st;
    if (!feat_out) return GCA_OK;
    const float inv = 1.0f / (float)(block * block);
    for (int e = 0; e < E; ++e) {
        const uint8_t* d = dousing + e * HW;
        float* f = feat_out + e * C2;
        memcpy(f, coa.data() + (size_t)e * 2 * HcWc, (size_t)(2 * HcWc) * sizeof(float));
        for (int bi = 0; bi < Hc; ++bi)
            for (int bj = 0; bj < Wc; ++bj) {
                const int r1 = (bi + 1) * block < H ? (bi + 1) * block : H;
                const int c1 = (bj + 1) * block < W ? (bj + 1) * block : W;
                int32_t cD = 0;
                for (int r = bi * block; r < r1; ++r)
                    for (int c = bj * block; c < c1; ++c) cD += d[(int64_t)r * W + c] != 0;
                f[2 * HcWc + (int64_t)bi * Wc + bj] = (float)cD * inv;
            }
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const int64_t r = (int64_t)pos[2 * e] - radius + i, c = (int64_t)pos[2 * e + 1] - radius + j;
                const bool in = r >= 0 && r < H && c >= 0 && c < W;
                f[3 * HcWc + i * S + j] = in && d[r * W + c] != 0 ? 1.0f : 0.0f;
            }
        if (3 * HcWc + S * S < C2) f[C2 - 1] = 0.0f;
    }
    return GCA_OK;
}

// gca_advanced_policy_act on that observation, as the two host functions it is defined by.
extern "C" int gca_advanced_policy_act_retardant(const gca_bulldozer_policy* policy, const uint8_t* grid,
                                                 const uint8_t* dousing, const uint16_t* dous_bits, const int32_t* pos,
                                                 const int32_t* time_step, int E, int H, int W, int empty, int tree,
                                                 int fire, int env_offset, uint64_t policy_seed, int greedy,
                                                 int32_t* action, int action_stride, float* logits, float* value,
                                                 uint8_t* local_out, float* feat_out, void*) {
    if (const int st = gca_check_advanced_policy_act_retardant(policy, grid, dousing, dous_bits, pos, time_step, E, H, W,
                                                               empty, tree, fire, action, action_stride))
        return st;
    const int S = 2 * policy->radius + 1;
    const int C2 = (int)gca_retardant_c2(H, W, policy->block, policy->radius);
    std::vector<uint8_t> loc(local_out ? 0 : (size_t)E * S * S);
    std::vector<float> fea(feat_out ? 0 : (size_t)E * C2);
    uint8_t* loc_p = local_out ? local_out : loc.data();
    float* fea_p = feat_out ? feat_out : fea.data();
    if (const int st = gca_advanced_policy_observation(grid, dousing, dous_bits, pos, E, H, W, empty, tree, fire,
                                                       policy->radius, policy->block, loc_p, fea_p, nullptr))
        return st;
    std::vector<int64_t> se((size_t)E);
    std::vector<int32_t> act(2 * (size_t)E);
    for (int e = 0; e < E; ++e) se[e] = (int64_t)time_step[e];
    if (const int st = gca_bulldozer_policy_act(policy, C2, loc_p, fea_p, se.data(), nullptr, env_offset, policy_seed,
                                                greedy, act.data(), logits, value, E, nullptr))
        return st;
    for (int e = 0; e < E; ++e) {
        action[(size_t)e * action_stride] = act[2 * (size_t)e];
        action[(size_t)e * action_stride + 1] = act[2 * (size_t)e + 1];
    }
    return GCA_OK;
}

// ---------------------------------------------------------------- the PPO update (gca.h "PPO update")
// The recurrence of gca.h, one rounded f32 operation at a time (the file is built with -ffp-contract=off).
extern "C" int gca_gae(const double* reward, const float* value, const float* next_value, const uint8_t* terminal,
                       float gamma, float gamma_lambda, int K, int E, float* advantage, float* returns, void*) {
    if (const int st = gca_check_gae(reward, value, next_value, K, E, advantage, returns)) return st;
    for (int e = 0; e < E; ++e) {
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
    return GCA_OK;
}

static int64_t policy_grad_workspace_host(const GcaGradAgent& ag, const gca_policy* p, int C, int N) {
    if (gca_check_policy_grad_workspace(ag, p, C, N)) return -1;
    const int S = 2 * p->radius + 1;
    return ppo_plan(S * S, C, p->hidden, N, ag.nout).bytes;
}

extern "C" int64_t gca_helicopter_policy_grad_workspace(const gca_heli_policy* p, int C, int N) {
    return policy_grad_workspace_host(GCA_GRAD_HELI, p, C, N);
}

extern "C" int64_t gca_bulldozer_policy_grad_workspace(const gca_bulldozer_policy* p, int C, int N) {
    return policy_grad_workspace_host(GCA_GRAD_BDZ, p, C, N);
}

static double lse_host(const double* l, int n) {
    double m = l[0];
    for (int i = 1; i < n; ++i) m = l[i] > m ? l[i] : m;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += exp(l[i] - m);
    return m + log(s);
}

// Both agents' gradient in plain loops over the head layout (nh heads of heads[h] logits, then the value): the network,
// the per-head loss of gca.h and every gradient sum in double, rounded to f32 once. The workspace is checked as on the
// device and not used. vclip (the _vclip entries, with old_value and vstats): gca.h's clipped value loss in place of
// 0.5 (v - R)^2, with U and every comparison in double; a first pass over the minibatch forms the values and U.
static int policy_grad_host(const GcaGradAgent& ag, int nh, const int* heads, const gca_policy* p, int C,
                            const uint8_t* local, const float* coarse, const int32_t* action, const float* old_logits,
                            const float* advantage, const float* returns, int64_t T, const int32_t* idx, int N,
                            float clip_coef, float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                            float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats, void* workspace,
                            int64_t workspace_bytes, bool vclip = false, const float* old_value = nullptr,
                            float* vstats = nullptr) {
    PpoPlan pl;
    if (const int st = vclip ? gca_check_policy_grad_vclip(ag, p, C, local, coarse, action, old_logits, old_value,
                                                           advantage, returns, T, idx, N, clip_coef, g_w_local,
                                                           g_w_coarse, g_b1, g_w_out, g_b2, stats, vstats, workspace,
                                                           workspace_bytes, &pl)
                             : gca_check_policy_grad(ag, p, C, local, coarse, action, old_logits, advantage, returns, T,
                                                     idx, N, clip_coef, g_w_local, g_w_coarse, g_b1, g_w_out, g_b2,
                                                     stats, workspace, workspace_bytes, &pl))
        return st;
    if (const int st = gca_check_policy_grad_idx(ag, idx, N, T)) return st;
    const int S = 2 * p->radius + 1, SS = S * S, Hd = p->hidden, NO = ag.nout, NL = NO - 1;
    auto row_of = [&](int t) { return idx ? (size_t)idx[t] : (size_t)t; };
    double mean = 0.0, var = 0.0;
    for (int t = 0; t < N; ++t) mean += advantage[row_of(t)];
    mean /= N;
    for (int t = 0; t < N; ++t) {
        const double d = advantage[row_of(t)] - mean;
        var += d * d;
    }
    const double sd = sqrt(var / N), inv_n = 1.0 / N, inv_nh = 1.0 / ((double)N * nh);
    std::vector<double> gwl((size_t)SS * 4 * Hd, 0.0), gwc((size_t)C * Hd, 0.0), gb1(Hd, 0.0), gwo((size_t)Hd * NO, 0.0);
    std::vector<double> a(Hd), h(Hd), da(Hd), out(NO), d(NO), gb2(NO, 0.0), lo(NL), pr(NL), lp(NL);
    double st[5] = {0};
    // the network on one record row: pre-activations a, hidden h, outputs out
    auto forward = [&](size_t row) {
        const uint8_t* loc = local + row * SS;
        const float* co = coarse + row * C;
        for (int j = 0; j < Hd; ++j) a[j] = p->b1[j];
        for (int n = 0; n < SS; ++n) {
            const float* w = p->w_local + ((size_t)n * 4 + (loc[n] & 3)) * Hd;
            for (int j = 0; j < Hd; ++j) a[j] += w[j];
        }
        for (int c = 0; c < C; ++c) {
            const float* w = p->w_coarse + (size_t)c * Hd;
            const double x = co[c];
            for (int j = 0; j < Hd; ++j) a[j] += w[j] * x;
        }
        for (int o = 0; o < NO; ++o) out[o] = p->b2[o];
        for (int j = 0; j < Hd; ++j) {
            h[j] = a[j] > 0.0 ? a[j] : 0.0;
            for (int o = 0; o < NO; ++o) out[o] += (double)p->w_out[j * NO + o] * h[j];
        }
    };
    // the clipped value loss's minibatch scalars (gca.h): U, then n_U and the samples outside the clip against that U
    const double cc = (double)clip_coef;
    double U = 0.0, share_u = 0.0;
    struct VTerms {
        double dcr, q;
        bool in, u;
    };
    auto vterms = [&](double v, size_t row) {
        const double vo = old_value[row], diff = v - vo;
        VTerms t;
        t.in = fabs(diff) <= cc;
        t.dcr = (vo + (diff < -cc ? -cc : (diff > cc ? cc : diff))) - (double)returns[row];
        t.q = t.dcr * t.dcr;
        t.u = U >= t.q;
        return t;
    };
    if (vclip) {
        std::vector<double> vs(N);
        for (int t = 0; t < N; ++t) {
            forward(row_of(t));
            vs[t] = out[NL];
            const double dv = vs[t] - returns[row_of(t)];
            U += 0.5 * dv * dv;
        }
        U *= inv_n;
        int64_t nu = 0, nc = 0;
        for (int t = 0; t < N; ++t) {
            const VTerms vt = vterms(vs[t], row_of(t));
            nu += vt.u ? 1 : 0;
            nc += vt.in ? 0 : 1;
        }
        share_u = (double)nu / N;
        if (vstats) {
            vstats[0] = (float)U;
            vstats[1] = (float)share_u;
            vstats[2] = (float)((double)nc / N);
        }
    }
    for (int t = 0; t < N; ++t) {
        const size_t row = row_of(t);
        const uint8_t* loc = local + row * SS;
        const float* co = coarse + row * C;
        forward(row);
        double adv = advantage[row];
        if (norm_adv) adv = (adv - mean) / (sd + 1e-8);
        const double lo_c = 1.0 - (double)clip_coef, hi_c = 1.0 + (double)clip_coef;
        for (int hd = 0, off = 0; hd < nh; off += heads[hd], ++hd) {
            const int n = heads[hd];
            const double* l = out.data() + off;
            for (int i = 0; i < n; ++i) lo[i] = old_logits[row * NL + off + i];
            const int32_t ar = action[row * nh + hd];
            const int act = ar < 0 ? 0 : (ar > n - 1 ? n - 1 : ar);
            const double lse = lse_host(l, n), lse_old = lse_host(lo.data(), n);
            const double logratio = (l[act] - lse) - (lo[act] - lse_old), ratio = exp(logratio);
            const bool clipped = ratio < lo_c || ratio > hi_c;
            const double pg1 = -adv * ratio, pg2 = -adv * (ratio < lo_c ? lo_c : (ratio > hi_c ? hi_c : ratio));
            const double dpg_dr = (!clipped || pg1 > pg2) ? -adv : 0.0;
            double ent = 0.0;
            for (int i = 0; i < n; ++i) {
                lp[i] = l[i] - lse;
                pr[i] = exp(lp[i]);
                ent -= pr[i] * lp[i];
            }
            for (int i = 0; i < n; ++i)
                d[off + i] = (dpg_dr * ratio * ((i == act ? 1.0 : 0.0) - pr[i]) +
                              (double)ent_coef * pr[i] * (lp[i] + ent)) * inv_nh;
            st[0] += pg1 > pg2 ? pg1 : pg2;
            st[2] += ent;
            st[3] += (ratio - 1.0) - logratio;
            st[4] += clipped ? 1.0 : 0.0;
        }
        const double dv = out[NL] - returns[row];
        if (vclip) {
            const VTerms vt = vterms(out[NL], row);
            d[NL] = (double)vf_coef * (0.5 * inv_n) * (share_u * dv + ((!vt.u && vt.in) ? 2.0 * vt.dcr : 0.0));
            st[1] += 0.5 * (vt.u ? U : vt.q);
        } else {
            d[NL] = (double)vf_coef * dv * inv_n;
            st[1] += 0.5 * dv * dv;
        }
        for (int o = 0; o < NO; ++o) gb2[o] += d[o];
        for (int j = 0; j < Hd; ++j) {
            double dh = 0.0;
            for (int o = 0; o < NO; ++o) {
                gwo[(size_t)j * NO + o] += h[j] * d[o];
                dh += (double)p->w_out[j * NO + o] * d[o];
            }
            da[j] = a[j] > 0.0 ? dh : 0.0;
            gb1[j] += da[j];
        }
        for (int n = 0; n < SS; ++n) {
            double* g = gwl.data() + ((size_t)n * 4 + (loc[n] & 3)) * Hd;
            for (int j = 0; j < Hd; ++j) g[j] += da[j];
        }
        for (int c = 0; c < C; ++c) {
            double* g = gwc.data() + (size_t)c * Hd;
            const double x = co[c];
            for (int j = 0; j < Hd; ++j) g[j] += x * da[j];
        }
    }
    for (size_t i = 0; i < gwl.size(); ++i) g_w_local[i] = (float)gwl[i];
    for (size_t i = 0; i < gwc.size(); ++i) g_w_coarse[i] = (float)gwc[i];
    for (int j = 0; j < Hd; ++j) g_b1[j] = (float)gb1[j];
    for (size_t i = 0; i < gwo.size(); ++i) g_w_out[i] = (float)gwo[i];
    for (int o = 0; o < NO; ++o) g_b2[o] = (float)gb2[o];
    const double pg = st[0] * inv_nh, vl = st[1] * inv_n, en = st[2] * inv_nh;
    stats[0] = (float)(pg - (double)ent_coef * en + (double)vf_coef * vl);
    stats[1] = (float)pg;
    stats[2] = (float)vl;
    stats[3] = (float)en;
    stats[4] = (float)(st[3] * inv_nh);
    stats[5] = (float)(st[4] * inv_nh);
    stats[6] = (float)mean;
    stats[7] = (float)sd;
    return GCA_OK;
}

extern "C" int gca_helicopter_policy_grad(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                                          const int32_t* action, const float* old_logits, const float* advantage,
                                          const float* returns, int64_t T, const int32_t* idx, int N, float clip_coef,
                                          float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                                          float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats,
                                          void* workspace, int64_t workspace_bytes, void*) {
    const int heads[1] = {9};
    return policy_grad_host(GCA_GRAD_HELI, 1, heads, p, C, local, coarse, action, old_logits, advantage, returns, T, idx,
                            N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats,
                            workspace, workspace_bytes);
}

extern "C" int gca_bulldozer_policy_grad(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                         const float* coarse, const int32_t* action, const float* old_logits,
                                         const float* advantage, const float* returns, int64_t T, const int32_t* idx,
                                         int N, float clip_coef, float ent_coef, float vf_coef, int norm_adv,
                                         float* g_w_local, float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2,
                                         float* stats, void* workspace, int64_t workspace_bytes, void*) {
    const int heads[2] = {9, 2};
    return policy_grad_host(GCA_GRAD_BDZ, 2, heads, p, C, local, coarse, action, old_logits, advantage, returns, T, idx,
                            N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats,
                            workspace, workspace_bytes);
}

extern "C" int gca_helicopter_policy_grad_vclip(const gca_heli_policy* p, int C, const uint8_t* local,
                                                const float* coarse, const int32_t* action, const float* old_logits,
                                                const float* old_value, const float* advantage, const float* returns,
                                                int64_t T, const int32_t* idx, int N, float clip_coef, float ent_coef,
                                                float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                                                float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                                                void* workspace, int64_t workspace_bytes, void*) {
    const int heads[1] = {9};
    return policy_grad_host(GCA_GRAD_HELI_VCLIP, 1, heads, p, C, local, coarse, action, old_logits, advantage, returns,
                            T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local, g_w_coarse, g_b1, g_w_out,
                            g_b2, stats, workspace, workspace_bytes, true, old_value, vstats);
}

extern "C" int gca_bulldozer_policy_grad_vclip(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                               const float* coarse, const int32_t* action, const float* old_logits,
                                               const float* old_value, const float* advantage, const float* returns,
                                               int64_t T, const int32_t* idx, int N, float clip_coef, float ent_coef,
                                               float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                                               float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                                               void* workspace, int64_t workspace_bytes, void*) {
    const int heads[2] = {9, 2};
    return policy_grad_host(GCA_GRAD_BDZ_VCLIP, 2, heads, p, C, local, coarse, action, old_logits, advantage, returns,
                            T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local, g_w_coarse, g_b1, g_w_out,
                            g_b2, stats, workspace, workspace_bytes, true, old_value, vstats);
}

extern "C" int64_t gca_extension_policy_grad_workspace(const gca_bulldozer_policy* p, int C, int N) {
    return policy_grad_workspace_host(GCA_GRAD_EXT, p, C, N);
}

extern "C" int gca_extension_policy_grad(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                         const float* coarse, const int32_t* action, const float* old_logits,
                                         const float* advantage, const float* returns, int64_t T, const int32_t* idx,
                                         int N, float clip_coef, float ent_coef, float vf_coef, int norm_adv,
                                         float* g_w_local, float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2,
                                         float* stats, void* workspace, int64_t workspace_bytes, void*) {
    const int heads[3] = {9, 2, 3};
    return policy_grad_host(GCA_GRAD_EXT, 3, heads, p, C, local, coarse, action, old_logits, advantage, returns, T, idx,
                            N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats,
                            workspace, workspace_bytes);
}

extern "C" int gca_extension_policy_grad_vclip(const gca_bulldozer_policy* p, int C, const uint8_t* local,
                                               const float* coarse, const int32_t* action, const float* old_logits,
                                               const float* old_value, const float* advantage, const float* returns,
                                               int64_t T, const int32_t* idx, int N, float clip_coef, float ent_coef,
                                               float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                                               float* g_b1, float* g_w_out, float* g_b2, float* stats, float* vstats,
                                               void* workspace, int64_t workspace_bytes, void*) {
    const int heads[3] = {9, 2, 3};
    return policy_grad_host(GCA_GRAD_EXT_VCLIP, 3, heads, p, C, local, coarse, action, old_logits, advantage, returns,
                            T, idx, N, clip_coef, ent_coef, vf_coef, norm_adv, g_w_local, g_w_coarse, g_b1, g_w_out,
                            g_b2, stats, workspace, workspace_bytes, true, old_value, vstats);
}

// ---------------------------------------------------------------- the optimizer (gca.h "optimizer")
// gca_adam_step in gca.h's order: the lanes, the chunks and the trees of the device's sum as plain loops, then one
// rounded f32 operation at a time per element (the file is built with -ffp-contract=off).
static double adam_tree_host(double* s) {
    for (int h = ADAM_THREADS / 2; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l) s[l] = s[l] + s[l + h];
    return s[0];
}

extern "C" int64_t gca_adam_step_workspace(int64_t total_elements) {
    if (gca_check_adam_step_workspace(total_elements)) return -1;
    return adam_workspace_bytes(total_elements);
}

extern "C" int gca_adam_step(const gca_adam_tensors* t, void* state, float lr0, float b1, float b2, float eps,
                             float max_norm, int64_t steps_per_iteration, int64_t num_iterations, float* info_out,
                             void* workspace, int64_t workspace_bytes, void*) {
    int64_t total;
    if (const int st = gca_check_adam_step(t, state, b1, b2, eps, steps_per_iteration, num_iterations, info_out,
                                           workspace, workspace_bytes, &total))
        return st;
    const int64_t CH = adam_chunk(total);
    std::vector<double> part;
    double s[ADAM_THREADS];
    for (int i = 0; i < t->n; ++i) {
        for (int64_t base = 0; base < t->len[i]; base += CH) {
            const int64_t cnt = t->len[i] - base < CH ? t->len[i] - base : CH;
            for (int l = 0; l < ADAM_THREADS; ++l) s[l] = 0.0;
            const float* g = t->g[i] + base;
            for (int64_t e = 0; e < cnt; ++e) {  // increasing e is increasing (k, j) for every lane
                double& a = s[(e / 4) % ADAM_THREADS];
                a = a + (double)g[e] * (double)g[e];
            }
            part.push_back(adam_tree_host(s));
        }
    }
    for (int l = 0; l < ADAM_THREADS; ++l) s[l] = 0.0;
    for (size_t p = 0; p < part.size(); ++p) s[p % ADAM_THREADS] = s[p % ADAM_THREADS] + part[p];
    const float norm = sqrtf((float)adam_tree_host(s));
    int32_t* sw = reinterpret_cast<int32_t*>(state);
    float* sf = reinterpret_cast<float*>(state);
    const int32_t count = sw[ADAM_COUNT];
    const float b1p = sf[ADAM_B1POW] * b1, b2p = sf[ADAM_B2POW] * b2;
    const float lr = adam_lr(lr0, count, steps_per_iteration, num_iterations);
    const float omb1 = 1.0f - b1, omb2 = 1.0f - b2, c1 = 1.0f - b1p, c2 = 1.0f - b2p;
    const bool clip = max_norm > 0.0f && !(norm < max_norm);
    for (int i = 0; i < t->n; ++i) {
        float *w = t->w[i], *m = t->m[i], *v = t->v[i];
        const float* g = t->g[i];
        for (int64_t e = 0; e < t->len[i]; ++e) {
            const float gc = clip ? (g[e] / norm) * max_norm : g[e];
            m[e] = (b1 * m[e]) + (omb1 * gc);
            v[e] = (b2 * v[e]) + ((omb2 * gc) * gc);
            const float mhat = m[e] / c1, vhat = v[e] / c2;
            w[e] = w[e] - (lr * (mhat / (sqrtf(vhat) + eps)));
        }
    }
    sw[ADAM_COUNT] = sw[ADAM_PENDING + ADAM_COUNT] = count + 1;
    sf[ADAM_B1POW] = sf[ADAM_PENDING + ADAM_B1POW] = b1p;
    sf[ADAM_B2POW] = sf[ADAM_PENDING + ADAM_B2POW] = b2p;
    sf[ADAM_NORM] = norm;
    sf[ADAM_LR] = sf[ADAM_PENDING + ADAM_LR] = lr;
    if (info_out) {
        info_out[0] = norm;
        info_out[1] = lr;
    }
    return GCA_OK;
}

extern "C" int gca_permutation(uint64_t seed, uint32_t epoch0, const int32_t* counter, int64_t T, int rows,
                               int32_t* out, void*) {
    if (const int st = gca_check_permutation(counter, T, rows, out)) return st;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const auto f = [k0, k1](uint32_t right, uint32_t round, uint32_t row_key) {
        return philox4x32_10(u32x4{right, round, row_key, GCA_TAG_PERM}, k0, k1).x;
    };
    const int h = perm_half_bits(T);
    bool capped = false;
    for (int r = 0; r < rows; ++r) {
        const uint32_t row_key = epoch0 + (uint32_t)r + (counter ? (uint32_t)counter[0] : 0u);
        for (int64_t i = 0; i < T; ++i)
            out[(size_t)r * T + i] = (int32_t)perm_walk((uint32_t)i, (uint32_t)T, h, row_key, f, &capped);
    }
    // the host build alone sees its walks: a kernel cannot report one that reached the cap
    if (capped) {
        gca_set_error("internal: %s", "permutation: the walk reached its cap");
        return GCA_ERR_UNSUPPORTED;
    }
    return GCA_OK;
}
