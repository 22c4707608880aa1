/*
 * gca.h — C-ABI of libgca_hip.so, the MI355X (gfx950) forest-fire CA hot path.
 *
 * Boundary contract:
 *   - plain extern "C", int status (GCA_OK = 0), gca_last_error() for the message;
 *   - every array argument is a DEVICE pointer owned by the caller (e.g. a torch
 *     tensor's data_ptr()); parameter structs are HOST pointers read at call time;
 *   - `stream` is a hipStream_t (NULL = legacy default stream); calls only enqueue
 *     work: no allocation, no synchronisation, so they can be captured in a hipGraph;
 *   - one caller per stream (thread-compatible, not thread-safe).
 *
 * Cell grids are u8, laid out (env, row, col) row-major. Cell codes are the
 * reference's integer values (ForestFireBulldozer EMPTY=0 TREE=3 FIRE=25,
 * Advanced/Helicopter 0/1/2); the host side checks they fit in u8.
 *
 * RNG: counter-based Philox4x32-10 (Random123), key = (seed lo, seed hi),
 * counter = (slot, global env id, per-env step, stream tag). See DESIGN.md §RNG.
 */
#ifndef GCA_H
#define GCA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCA_OK 0
#define GCA_ERR_ARG 1
#define GCA_ERR_HIP 2
#define GCA_ERR_UNSUPPORTED 3

#define GCA_MAX_RADIUS 8     /* heat-kernel radius ceil(log2 N)-2 <= 8  <=>  N <= 1024 */

/* Philox stream tags (counter word 3). */
#define GCA_TAG_WINDY_ROLL 0x574E4459u /* 'WNDY' : 3x3 roll of WindyForestFire      */
#define GCA_TAG_ALEX_CELL  0x414C5843u /* 'ALXC' : per-cell draws of Alexandridis (one block per 4 cells) */
#define GCA_TAG_ALEX_AGE   0x414C5841u /* 'ALXA' : ages of a 4-cell group's 2nd..4th new fires            */
#define GCA_TAG_ALEX_WIND  0x414C5857u /* 'ALXW' : per-env wind change               */
#define GCA_TAG_ACTION     0x41435449u /* 'ACTI' : synthetic actions (bench)          */
#define GCA_TAG_INIT       0x494E4954u /* 'INIT' : synthetic initial states           */
#define GCA_TAG_DS_CELL    0x44534345u /* 'DSCE' : Drossel-Schwabl per-cell draws     */
#define GCA_TAG_PINE       0x50494E45u /* 'PINE' (+1+m): pinecone count / pinecone m  */
#define GCA_TAG_PINE_AGE   0x50494E41u /* 'PINA' : age of a pinecone-ignited cell     */
#define GCA_TAG_HIDDEN     0x48494444u /* 'HIDD' : per-env hidden-layer plan (patches, hills, slopes) */
#define GCA_TAG_HIDDEN_CELL 0x48494443u /* 'HIDC' : per-cell hidden-layer draws          */
#define GCA_TAG_PINEC      0x50434C00u /* 'PCL\0' (+1+m): classic pinecone count / pinecone m */
#define GCA_TAG_PINEC_AGE  0x50434C41u /* 'PCLA' : age of a classic pinecone ignition        */
#define GCA_TAG_POLICY     0x504F4C49u /* 'POLI' : the helicopter policy's action draw          */

/* ------------------------------------------------------------------ generic */

const char* gca_last_error(void);
int gca_version(void);

/* Philox4x32-10 over n counters (ctr[n][4] device, out[n][4] device). KAT hook. */
int gca_philox(const uint32_t* ctr, uint32_t key0, uint32_t key1, uint32_t* out, int64_t n, void* stream);

/* counts[e][0..2] = #cells == v0/v1/v2 in grid e (overwrites). ca_env.py:94-99 count_cells. */
int gca_count_cells(const uint8_t* grid, int E, int H, int W, int v0, int v1, int v2, int32_t* counts, void* stream);

/* ------------------------------------------------------- WindyForestFire ---
 * Replaces WindyForestFire._get_failed_propagations_mask + _get_kernel
 * (ca_windy.py:53-77): dir_mask[e] bit d (d = 3x3 index row-major, centre
 * skipped) is set iff roll[d] < wind[d]  (the reference keeps d iff NOT wind<=roll).
 * wind: [E][9] f64 with env stride wind_stride (0 = one wind shared by all envs).
 * roll: [E][9] f64 injected uniforms, or NULL -> Philox(seed, (d/2, env_offset+e,
 *       rng_step[e] + pass, GCA_TAG_WINDY_ROLL)), 53-bit doubles.
 * Only envs with steps == NULL || steps[e] > pass are written; dir_mask[e] of every
 * other env keeps its value. roll < wind is strict: a tie leaves the bit clear.
 * rng_step == NULL draws step `pass` for every env; rng_step[e] + pass wraps at 2^32. */
int gca_windy_dirmask(const double* wind, int64_t wind_stride, const double* roll, uint64_t seed,
                      const uint32_t* rng_step, const int32_t* steps, int pass, int env_offset,
                      uint8_t* dir_mask, int E, void* stream);

/* One WindyForestFire CA step (ca_windy.py:41-51, scipy convolve2d mode="same",
 * fill=empty, then the 3 thresholds of _translate_analogic_to_discrete :102-139).
 * Env e participates iff steps == NULL || steps[e] > pass; it reads
 * buf[parity ? parity[e] : 0] and writes the other buffer (parity is NOT flipped here).
 * force_exact = 1 selects the literal threshold kernel; 0 lets the library use the
 * SWAR kernel when it is exact (empty == 0, all cells in {empty, tree, fire}: the
 * caller guarantees the latter; W = 16*2^j <= 1024, 16-B aligned buffers).
 * counts (nullable, [E][3] empty/tree/fire of the NEW grid) are ACCUMULATED with
 * atomics: the caller zeroes the participating rows first.
 * An env that does not participate is not touched: neither of its buffers, nor its
 * counts row. A participating env's source buffer is only read.
 * The SWAR kernels apply the closed-form rule (TREE -> FIRE iff an active direction
 * sees FIRE, FIRE -> EMPTY, else unchanged). It equals the thresholds on every grid of
 * the three codes iff the codes satisfy the reference constructor's inequalities
 * (ca_windy.py:163-173; with empty = 0: 8*tree < fire < 32*tree), which this entry
 * point does NOT check: with other codes (e.g. 0, 2, 9) pass force_exact = 1 to get
 * the thresholds (there a TREE ignites on the weight of its TREE neighbours alone).
 * W = 256 and 512 take the row-stream kernel, every other eligible W the lane-tile
 * kernel; any other W, an unaligned buffer or empty != 0 the literal kernel.   */
int gca_windy_step(uint8_t* buf0, uint8_t* buf1, const uint8_t* parity, const int32_t* steps, int pass,
                   const uint8_t* dir_mask, int E, int H, int W, int empty, int tree, int fire,
                   int force_exact, int32_t* counts, void* stream);

/* --------------------------------------------- ForestFireBulldozer (batched)
 * bulldozer.py:393-400 MDP = RepeatCA (repeat_ca.py:32-45) then MoveModify
 * (move_modify.py:128-134); reward/done bulldozer.py:180-216.                 */
typedef struct {
    double t_move[9];        /* _movement_timings (bulldozer.py:277-286)      */
    double t_shoot[2];       /* _shooting_timings                              */
    double t_any;            /* time_per_state (bulldozer.py:297)              */
    uint64_t seed;           /* Philox key for the windy roll                  */
    int32_t env_offset;      /* global id of env 0 of this shard               */
    int32_t empty, tree, fire;
    int32_t up_mask, down_mask, left_mask, right_mask; /* action sets as bitmasks over 0..8 */
    int16_t effect[256];     /* Modify effects: new value, or -1 if not a key  */
} gca_bulldozer_params;

/* Before the CA passes: for live envs (done[e]==0) accu += (t_move[a0]+t_shoot[a1]) + t_any,
 * (accu, steps) = modf(accu); zero counts of stepping envs; dir_mask for pass 0.
 * Done envs (done nullable: NULL = every env is live) get steps = -1 and nothing
 * else: their accu, counts and dir_mask keep their values, as do the counts and
 * dir_mask of live envs with steps == 0.                                        */
int gca_bulldozer_pre(const gca_bulldozer_params* p, const int32_t* action, double* accu, int32_t* steps,
                      const uint8_t* done, const double* wind, int64_t wind_stride, const uint32_t* rng_step,
                      uint8_t* dir_mask, int32_t* counts, int E, void* stream);
/* Between CA passes `pass` and `pass+1`: flip parity of envs that stepped in `pass`;
 * for envs stepping again (steps[e] > pass + 1), zero their counts and draw the
 * dir_mask for pass+1 at Philox step rng_step[e] + pass + 1.                     */
int gca_bulldozer_interpass(const gca_bulldozer_params* p, int pass, const int32_t* steps, uint8_t* parity,
                            const double* wind, int64_t wind_stride, const uint32_t* rng_step, uint8_t* dir_mask,
                            int32_t* counts, int E, void* stream);
/* After the last pass (index last_pass): flip parity, Move, Modify (in place on the
 * current buffer), adjust counts, reward = -(f/(t+f)) (NaN if t+f==0), done = (f==0),
 * rng_step += steps. Done-on-entry envs (steps[e] < 0): reward 0, nothing else is
 * written (pos, hit, done, counts, parity, rng_step keep their values).
 * parity == NULL: no flip, Modify on buf0 (buf1 may be NULL). A Modify whose old or
 * new value is none of the three codes changes only the count of the one that is.   */
int gca_bulldozer_post(const gca_bulldozer_params* p, int last_pass, const int32_t* action, const int32_t* steps,
                       uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos,
                       int32_t* counts, uint32_t* rng_step, uint8_t* done, uint8_t* hit, double* reward,
                       int E, void* stream);

/* The whole ForestFireBulldozer env step in one launch (bulldozer.py:393-400 MDP.update + ca_env.py:27-62 reward /
 * done), one workgroup per env: the gca_bulldozer_pre bookkeeping, when a CA step is due (steps[e] = 1) the Windy
 * direction mask and the row-stream CA of gca_windy_step on the env's grid, then gca_bulldozer_post's Move / Modify,
 * counts, reward, done, hit, rng_step and parity; steps_elapsed (nullable) += 1 for live envs. Identical results to
 * the three-kernel sequence. Requires W = 256 or 512, empty = 0 < tree < fire, 16-B aligned buffers and one CA pass
 * at most per env step ((t_move + t_shoot) + t_any < 1 for every action; otherwise GCA_ERR_ARG).
 * meet (nullable): E 64-bit slots, zero-initialised once by the caller (every launch leaves them zero); with them the
 * step runs as 2 (W = 256) / 4 (W = 512) workgroups per env that meet in one atomic per env, the last to arrive writing
 * the env's outputs — the same results; NULL: one workgroup per env. Not shared between concurrent launches. The
 * slots pack 20-bit counts, so grids with H*W + 1 >= 2^20 cells ignore `meet` and run one workgroup per env.   */
int gca_bulldozer_step_fused(const gca_bulldozer_params* p, const int32_t* action, double* accu, int32_t* steps,
                             uint8_t* done, const double* wind, int64_t wind_stride, uint32_t* rng_step,
                             uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos,
                             int32_t* counts, uint8_t* hit, double* reward, int64_t* steps_elapsed, uint64_t* meet,
                             int E, void* stream);
/* gca_bulldozer_step_fused under a random policy: every env's action is drawn inside the step exactly as
 * gca_random_actions(action, E, p->env_offset, action_seed, rng_step) draws it before the step (move randint[0, 9),
 * shoot the top bit, Philox keyed by the global env id and rng_step[e]) -- the pair of launches in one, bit for bit --
 * and written to action_out (nullable, [E][2]). For random rollouts (action_space.sample() per env per step).       */
int gca_bulldozer_step_fused_random(const gca_bulldozer_params* p, uint64_t action_seed, int32_t* action_out,
                                    double* accu, int32_t* steps, uint8_t* done, const double* wind,
                                    int64_t wind_stride, uint32_t* rng_step, uint8_t* parity, uint8_t* buf0,
                                    uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts, uint8_t* hit,
                                    double* reward, int64_t* steps_elapsed, uint64_t* meet, int E, void* stream);
/* K env steps of every env in ONE launch under gca_bulldozer_step_fused_random's random policy (r06): bit for bit K
 * consecutive gca_bulldozer_step_fused_random calls with the same action_seed (the batched form of K iterations of the
 * reference loop `env.step(env.action_space.sample())`, bulldozer.py:393-400, ca_env.py:27-62); one workgroup per env
 * keeps the env's state in registers across the K steps. Optional per-step outputs: action_out (K, E, 2) int32,
 * reward_out (K, E) f64, done_out (K, E) u8 (as `done` after each step). Same contract as gca_bulldozer_step_fused
 * (W = 256 / 512, one CA pass at most per env step, empty = 0 < tree < fire). */
int gca_bulldozer_rollout_random(const gca_bulldozer_params* p, uint64_t action_seed, int K, int32_t* action_out,
                                 double* reward_out, uint8_t* done_out, double* accu, int32_t* steps, uint8_t* done,
                                 const double* wind, int64_t wind_stride, uint32_t* rng_step, uint8_t* parity,
                                 uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts, uint8_t* hit,
                                 double* reward, int64_t* steps_elapsed, int E, void* stream);
/* K env steps of every env in ONE launch with the caller's actions and, optionally, same-step autoreset: the batched
 * form of K iterations of `env.step(action)` (bulldozer.py:393-400, ca_env.py:27-62) followed, under autoreset, by the
 * reference's conditional reset of the envs that finished (ca_env.py:64-81). Bit for bit K consecutive
 * gca_bulldozer_step_fused calls on actions[k] (actions (K, E, 2) int32, decided before the call; NULL: K
 * gca_bulldozer_step_fused_random calls under action_seed), each followed when autoreset != 0 by
 * gca_bulldozer_reset_where(mask = NULL, max_steps, set_episode = -1): one workgroup per env keeps the env's state in
 * registers across the K steps, and an env's reset (grid into buf0 keyed by (reset_seed, global env id, episode + 1),
 * fire cell, position, counts; parity, accu, done, hit, steps_elapsed = 0; rng_step runs on, reward and steps stay)
 * overlaps every other env's steps. An env that is done on entry takes the no-op step (reward 0) and is then reset.
 * Per-step records, all nullable: action_out (K, E, 2) int32 the actions taken, unclamped; reward_out (K, E) f64 what
 * step k leaves in `reward`; terminated_out / truncated_out (K, E) u8: under autoreset the flags the reset after step k
 * saw (done, and the time limit reached without done), otherwise `done` after step k and zeros.
 * autoreset == 0: reset_seed, max_steps, cdf, values, episode, last_length, terminated, truncated are not used (max_steps
 * is ignored as gca_bulldozer_step_fused ignores it). autoreset != 0: cdf [3] f32, values [3] u8 (device arrays),
 * episode and steps_elapsed are required; last_length (written for the envs that reset), terminated and truncated (the
 * last step's flags, every env) are nullable. Same contract as gca_bulldozer_step_fused (W = 256 / 512, one CA pass at
 * most per env step, empty = 0 < tree < fire, 16-B aligned buffers) and gca_bulldozer_reset_where (buf0 != buf1,
 * H < 32768, max_steps >= 0, env_offset >= 0). K = 0 launches nothing. */
int gca_bulldozer_rollout(const gca_bulldozer_params* p, const int32_t* actions, uint64_t action_seed, int K,
                          int32_t* action_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                          int autoreset, uint64_t reset_seed, int64_t max_steps, const float* cdf,
                          const uint8_t* values, uint32_t* episode, int64_t* last_length, uint8_t* terminated,
                          uint8_t* truncated, double* accu, int32_t* steps, uint8_t* done, const double* wind,
                          int64_t wind_stride, uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H,
                          int W, int32_t* pos, int32_t* counts, uint8_t* hit, double* reward, int64_t* steps_elapsed,
                          int E, void* stream);

/* Per-env reset of the batched ForestFireBulldozer env on the device, one launch, device pointers only (capturable):
 * the initial distribution of bulldozer.py:221-275 and the fresh-episode state of ca_env.py:64-81 for the selected envs.
 *   selected  (mask ? mask[e] != 0 : done[e] != 0) || (max_steps > 0 && steps_elapsed[e] >= max_steps)
 *   flags     terminated_out[e] = done[e] on entry, truncated_out[e] = selected by the time limit and not done: both
 *             nullable, written for EVERY env; last_length_out[e] (nullable) = steps_elapsed[e], selected envs only
 *   episode   k = set_episode >= 0 ? (uint32)set_episode : episode[e] + 1, stored to episode[e]
 *   grid      buf0[e]: flat cell i = values[first j with u < cdf[j]], u = u01_f32 of word i & 3 of Philox((i >> 2,
 *             p->env_offset + e, k, GCA_TAG_INIT), reset_seed) -- gca_fill_categorical (n_values = 3) with counter
 *             word 2 = k -- then p->fire at (3H/4 + n1, W/4 + n2); pos[e] = (H/4 + n3, 3W/4 + n4), where n_t is
 *             _seeding.env_integers(reset_seed, global env id, tag = t | ((k & 0xFFFFFF) << 8), 0, max(1, N/12)):
 *             episode 0 is BatchedForestFireBulldozerEnv.reset(seed = reset_seed)'s own state
 *   counts    [e][3] p->empty / p->tree / p->fire cells of the new grid, summed in the same launch (no atomics)
 *   state     parity, accu, done, hit, steps_elapsed = 0. rng_step is not a parameter: the Windy rolls and sampled
 *             actions of the new episode continue the env's stream. buf1 and every byte of an unselected env are left
 *             untouched.
 * cdf [3] f32 and values [3] u8 are device arrays. H, W < 32768; any H*W (a partial last quad and unaligned env bases
 * take byte stores). One workgroup per env; unselected envs leave after their per-env loads. */
int gca_bulldozer_reset_where(const gca_bulldozer_params* p, uint64_t reset_seed, const uint8_t* mask,
                              int64_t max_steps, int64_t set_episode, const float* cdf, const uint8_t* values,
                              uint8_t* done, uint8_t* terminated_out, uint8_t* truncated_out, uint32_t* episode,
                              int64_t* last_length_out, double* accu, uint8_t* parity, uint8_t* buf0, uint8_t* buf1,
                              int H, int W, int32_t* pos, int32_t* counts, uint8_t* hit, int64_t* steps_elapsed, int E,
                              void* stream);

/* Move then Modify for E envs (move_modify.py:37-134): action[e] = (move, shoot);
 * uses p->up/down/left/right_mask and p->effect; grid may be NULL (Move only); hit nullable. */
int gca_move_modify(const gca_bulldozer_params* p, const int32_t* action, int32_t* pos, uint8_t* grid, int H, int W,
                    uint8_t* hit, int E, void* stream);

/* -------------------------------------------- Alexandridis (advanced env CA) */
typedef struct {
    int32_t R;                 /* burn_kernel_radius (ca_alexandridis_jax.py:62)              */
    float heat_dw[GCA_MAX_RADIUS + 1]; /* w_k - w_{k+1} (f32), w_k = heat weight at Chebyshev distance k (k=0 centre, w_{R+1}=0), :108-153 */
    float dous_inner, dous_border;    /* 5x5 dousing weights :64-105                          */
    float veg1p[6], den1p[6];  /* 1 + veg_probs / den_probs, f32 (:170-184, clip 1..5)        */
    float p_tree;              /* shared_context["p_tree"] (:386)                              */
    int32_t age_lo, age_hi;    /* randint(fire_age_min, fire_age_max) bounds, truncated (:368) */
    uint64_t seed;
    int32_t env_offset;
    int32_t empty, tree, fire; /* 0, 1, 2 in AdvancedForestFireBulldozerEnv                  */
    int32_t n_winds;
    float winds[16][9];        /* shared_context["winds"][i][0] wind matrices (row-major 3x3)  */
    float heat0;               /* initial value of the heat sum: 0 for the JAX rule; the classic
                                  PartiallyObservableForestFire's constant p_h = 0.58 with every
                                  heat_dw / dousing weight 0 (ca_alexandridis.py:94)             */
    int32_t burnout_eq1;       /* 0: FIRE -> EMPTY iff age <= 1 (ca_alexandridis_jax.py:389);
                                  1: iff age == 1, i.e. the decremented age hits 0 (classic
                                  ca_alexandridis.py:181-183). Ages are decremented either way. */
    int32_t vd_uniform;        /* gca_alex_step_march* with vd = NULL (uniform layers, flat terrain only): the packed
                                  byte vegetation | density << 4 of every cell of every env (init_vegetation_same /
                                  init_density_same, advanced_bulldozer.py:190-195); unused otherwise */
} gca_alex_params;

/* p_slope[e][d][r][c] = slope_factor(0.078f * slope[e][r][c][d']) for the 8 non-centre d'
 * (ca_alexandridis_jax.py:199-200: exp(0.078 * slope)); slope_factor(a) = exp_f32(a) for a >= 0 and
 * 1 / exp_f32(-a) for a < 0 (IEEE division), exp_f32 the deterministic expf of DESIGN.md. */
int gca_alex_prepare_slope(const float* slope, float* p_slope, int E, int H, int W, void* stream);

/* One CA step of PartiallyObservableForestFireJax._update_grid (ca_alexandridis_jax.py:321-424).
 * grid u8, fire_age i16, vegetation/density/dousing u8 (E,H,W); p_slope (E,8,H,W) f32.
 * Draws: inj_burn [E][H][W][9] f32, inj_grow [E][H][W] f32, inj_age [E][H][W] i32 (all three
 *        given = injected mode, the reference rule verbatim), or all NULL = Philox mode
 *        (burn test against 1 - prod(1 - clamp01(p_d)); one Philox4x32-10 block per 4 cells (r, 4g .. 4g+3),
 *        counter (r * ceil(W/4) + g, env_offset + e, rng_step[e], ALXC): cell j tests word j's high 24 bits,
 *        the group's first new fire takes randint of the words' low bytes, its 2nd..4th words 0..2 of the
 *        ALXA block of the same counter).
 * prob_out (nullable, debug) [E][H][W][8] f32 burn probabilities of every cell.
 * counts (nullable) [E][3] of the NEW grid, OVERWRITTEN (memset inside).          */
int gca_alex_step(const gca_alex_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                  const int16_t* age_in, int16_t* age_out, const uint8_t* veg, const uint8_t* den,
                  const uint8_t* dousing, const float* p_slope, const int32_t* wind_index, const uint32_t* rng_step,
                  const float* inj_burn, const float* inj_grow, const int32_t* inj_age, float* prob_out,
                  int32_t* counts, void* stream);

/* gca_alex_step with the slopes in the antisymmetric edge layout of gca_alex_edge_slope_from_altitude
 * (16 B per cell instead of p_slope's 32): edge_slope (E,4,H,W) f32. Valid for slopes that come from an
 * altitude field through get_slope (init_utils.py:166-200), the only slopes the Advanced env has
 * (advanced_bulldozer.py:182-204); results are bit-identical to gca_alex_step on the p_slope that
 * gca_alex_slope_from_altitude builds from the same altitude. Same replaced code and draws as above. */
int gca_alex_step_es(const gca_alex_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                     const int16_t* age_in, int16_t* age_out, const uint8_t* veg, const uint8_t* den,
                     const uint8_t* dousing, const float* edge_slope, const int32_t* wind_index,
                     const uint32_t* rng_step, const float* inj_burn, const float* inj_grow, const int32_t* inj_age,
                     float* prob_out, int32_t* counts, void* stream);

/* gca_alex_step_es on the Advanced env's packed layout (Philox mode, W % 256 == 0, H % 16 == 0, 16-B aligned
 * arrays): vd[e][r][c] = min(veg, 7) | min(den, 7) << 4; dous_bits[e][r][c / 16] bit c % 16 = (dousing != 0)
 * (the env's dousing counts are 0/1: ModifyJax writes 1, move_modify_jax.py:102-114); edge_slope_coal = the edge
 * layout with every 256-column row segment of a plane in coalesced order (gca_alex_edge_slope_coalesce).
 * Results are bit-identical to gca_alex_step_es on the unpacked arrays. Same replaced code as gca_alex_step.
 * Tile activity map (nullable): act_out[e][tile] (u8, tiles of 16 rows x 256 columns, row-major) receives 1 iff
 * the step leaves a FIRE in that tile; with act_in = the previous step's act_out (or all ones), a tile whose 3 x 3
 * tile neighbourhood has no fire is copied instead of stepped (exact when p_tree == 0: act_in is ignored
 * otherwise). act_out is required with act_in; act_out alone just records the map. */
int gca_alex_step_packed(const gca_alex_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                         const int16_t* age_in, int16_t* age_out, const uint8_t* vd, const uint16_t* dous_bits,
                         const float* edge_slope_coal, const int32_t* wind_index, const uint32_t* rng_step,
                         int32_t* counts, const uint8_t* act_in, uint8_t* act_out, void* stream);
/* gca_alex_step_packed that ALSO writes the env's step observation of the plain case (enable_extensions = False, the
 * reference's default; advanced_bulldozer.py:1035-1101, :1120): rgb [E][H][W][3] f32 of every cell = the colour of its
 * NEW state (empty / tree / fire; other codes the empty colour) under the PRE-step is_night[e], water-tinted where its
 * PRE-step dousing bit is set (the MDP renders with the input per_env_context, :1121) — the frame gca_adv_observation
 * (mode 0) renders from the same inputs, minus the bulldozer's pixel, which gca_obs_position adds once the env step
 * has moved it. color_table [2][3][2][4] f32 from gca_obs_color_table (16-B aligned, like rgb). */
int gca_alex_step_packed_rgb(const gca_alex_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                             const int16_t* age_in, int16_t* age_out, const uint8_t* vd, const uint16_t* dous_bits,
                             const float* edge_slope_coal, const int32_t* wind_index, const uint32_t* rng_step,
                             int32_t* counts, const uint8_t* act_in, uint8_t* act_out, const float* color_table,
                             const int32_t* is_night, float* rgb, void* stream);
/* gca_alex_step_packed / _rgb in marching form for W == 256 (H % 16 == 0): one wave walks one 16 x 256 tile row by
 * row (gca_alex_march.hip), every slope byte read once. Same replaced code, arguments, results (bit for bit), tile
 * activity map and frame, except edge_slope: the edge layout (E,4,H,W) in natural column order (the output of
 * gca_alex_edge_slope_from_altitude, not coalesced), or NULL for flat terrain: every slope factor 1, as when every edge
 * value is +-1 (use_hidden=False: init_altitude_same, advanced_bulldozer.py:190-197, gives zero slopes) — no slope
 * planes are read (7.125 instead of 23.125 B / cell) and the results are those of the all-ones planes, bit for bit.
 * With edge_slope = NULL, vd may be NULL too: every cell's packed layer byte is p->vd_uniform (6.125 B / cell). */
int gca_alex_step_march(const gca_alex_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                        const int16_t* age_in, int16_t* age_out, const uint8_t* vd, const uint16_t* dous_bits,
                        const float* edge_slope, const int32_t* wind_index, const uint32_t* rng_step, int32_t* counts,
                        const uint8_t* act_in, uint8_t* act_out, void* stream);
int gca_alex_step_march_rgb(const gca_alex_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                            const int16_t* age_in, int16_t* age_out, const uint8_t* vd, const uint16_t* dous_bits,
                            const float* edge_slope, const int32_t* wind_index, const uint32_t* rng_step,
                            int32_t* counts, const uint8_t* act_in, uint8_t* act_out, const float* color_table,
                            const int32_t* is_night, float* rgb, void* stream);
/* vd (nullable) and dous_bits of gca_alex_step_packed from veg / den / dousing (E,H,W) u8; W % 16 == 0. */
int gca_alex_pack_layers(const uint8_t* veg, const uint8_t* den, const uint8_t* dousing, uint8_t* vd,
                         uint16_t* dous_bits, int E, int H, int W, void* stream);
/* edge_slope (E,4,H,W) -> coalesced order: inside every 256-column segment of a row, column 16q + 4m + j moves
 * to position 64m + 4q + j (W % 256 == 0). */
int gca_alex_edge_slope_coalesce(const float* edge_slope, float* edge_slope_coal, int E, int H, int W, void* stream);

/* Edge-slope layout for gca_alex_step_es from altitude [E][H][W] f64 (NULL = flat): edge_slope[e][k][r][c] =
 * V = +exp_f32(a) if a >= 0 else -exp_f32(-a), a = 0.078f * s, s = f32(degrees(atan((alt[r][c] - alt[n]) /
 * (1.414 if diagonal)))) toward neighbour n = k-th of (-1,-1), (-1,0), (-1,+1), (0,-1) (s = 0 where n is
 * outside the grid): get_slope (init_utils.py:166-200) without its border zeroing, which the step applies
 * per cell. p_slope everywhere is slope_factor(a) = exp_f32(a) (a >= 0) or 1/exp_f32(-a) (a < 0), so
 * both directions of an edge come from V: P(a) = V > 0 ? V : 1/|V|, P(-a) = V < 0 ? |V| : 1/|V|.      */
int gca_alex_edge_slope_from_altitude(const double* altitude, float* edge_slope, int E, int H, int W, void* stream);
/* (own, neighbour) factors the step derives from n edge values V, with the step's own arithmetic
 * (v_rcp_f32 + Newton reciprocal): the hook the exhaustive reciprocal test calls.                   */
int gca_alex_edge_factors(const float* v, float* own, float* nbr, int64_t n, void* stream);

/* Wind change of PartiallyObservableForestFireJax.update (ca_alexandridis_jax.py:442-451) for E envs:
 * u < p_wind_change -> wind_index = (wind_index + k) % n_winds, k in [1, 8).
 * inj_u/inj_k injected draws, or both NULL -> Philox((0, env_offset+e, rng_step[e], ALXW)) words 0/1. */
int gca_alex_wind_change(float p_wind_change, int n_winds, uint64_t seed, int env_offset, const uint32_t* rng_step,
                         const float* inj_u, const int32_t* inj_k, int32_t* wind_index, int E, void* stream);

/* get_slope (init_utils.py:166-200) on the device from altitude [E][H][W] f64 (NULL = flat),
 * f64 -> f32 like jnp.array, then p_slope as in gca_alex_prepare_slope. slope_out (nullable)
 * receives the f32 slope [E][H][W][3][3]. */
int gca_alex_slope_from_altitude(const double* altitude, float* p_slope, float* slope_out, int E, int H, int W,
                                 void* stream);

/* init_altitude's arithmetic (bulldozer/utils/init_utils.py:76-116) on the device. altitude [E][H][W]
 * holds the noise field on entry (the reference's uniform(0, 5) draws) and the altitude on return:
 * per cell, in the reference's order, += height * cos(dist / radius * pi / 2) for every hill with
 * dist < radius, += height_diff * (row - start_row) / height inside every slope rectangle, then / 10.
 * hills [E][GCA_MAX_HILLS][4] = (centre row, centre col, radius, height), n_hills [E] (<= 10);
 * slopes [E][GCA_MAX_SLOPES][5] = (start row, start col, width, height, height_diff), n_slopes [E] (<= 8).
 * Integer fields are stored as doubles. The random draws stay on the host (legacy np.random order). */
#define GCA_MAX_HILLS 10
#define GCA_MAX_SLOPES 8
int gca_alex_altitude_apply(double* altitude, int E, int H, int W, const int32_t* n_hills, const double* hills,
                            const int32_t* n_slopes, const double* slopes, void* stream);

/* Hidden layers drawn on the device (init_utils.py:10-116's recipe, Philox draws keyed by the GLOBAL env id,
 * so sharded runs draw what the unsharded run draws; not the reference's np.random stream — the envs'
 * hidden_rng="philox" mode). Per env (counter (slot, env_offset + e, 0, GCA_TAG_HIDDEN)):
 *   vegetation / density: randint(4, 8) patches (centre randint(0, R) x randint(0, C), size randint(3, max(4,
 *     R//2)) x randint(3, max(4, C//2)), value randint(1, 6)), later patches over earlier ones, uncovered cells
 *     randint(1, 4);
 *   altitude: noise uniform(0, 5) per cell into `altitude`, and the hills / slopes plan of
 *     gca_alex_altitude_apply (randint(6, 10) hills: centre, radius randint(2, max(3, min(R, C)//4)), height
 *     uniform(2, 6); randint(4, 8) slopes: start randint(0, max(1, R-4)) x randint(0, max(1, C-4)), width
 *     randint(3, max(4, C//4)), height randint(3, max(4, R//4)), height_diff uniform(1, 4)).
 * Per cell (counter (r * W + c, env_offset + e, 0, GCA_TAG_HIDDEN_CELL)): word 0 -> vegetation fill, word 1
 * -> density fill, words 2:3 -> noise. Follow with gca_alex_altitude_apply to finish the altitude.          */
int gca_hidden_init(uint64_t seed, int env_offset, int E, int H, int W, uint8_t* vegetation, uint8_t* density,
                    double* altitude, int32_t* n_hills, double* hills, int32_t* n_slopes, double* slopes,
                    void* stream);

/* Pinecone spotting (ca_alexandridis_jax.py:229-319, the scatter :400-420 — disabled in the reference's
 * live path, enabled in our env / operator with pinecones=True), after gca_alex_step* on its output:
 * every FIRE cell of grid_in throws n = min(Poisson(1), max_pinecones) pinecones in direction d (uniform
 * over 8) with integer thrust s = round(N(0,1) * ft[ft_lookup[d]]) of the env's current wind; a pinecone
 * landing on a TREE of grid_out at (clip(r + dx[d] s), clip(c + dy[d] s)) burns it with probability
 * (scale * veg1p[clip(veg)]) * den1p[clip(den)] of the target; the target becomes FIRE with age
 * randint(age_lo, age_hi) and one count moves tree -> fire. Any burning pinecone ignites its target
 * (duplicates). s_cdf [n_winds][8][GCA_PINE_CDF] u32: per (wind, direction) t[0] = 2K, t[1..2K] = 32-bit
 * thresholds of P(s <= -K + j) (gymca_amd/forest_fire/operators/pinecones.py). Draws: Philox blocks
 * (lin, env, step, PINE + 0 / 1 + m) and (target lin, env, step, PINA), see gca_pine.hip. act_tiles
 * (nullable): gca_alex_step_packed's act_out of the same step — the tile of every ignited target is set to 1. */
#define GCA_PINE_MAX 8
#define GCA_PINE_CDF 17
typedef struct {
    uint32_t n_cdf[GCA_PINE_MAX]; /* P(Poisson(1) <= j) * 2^32, j = 0..7                         */
    int32_t max_pinecones;        /* 5 (:230)                                                      */
    int32_t dx[8], dy[8];         /* E, NE, N, NW, W, SW, S, SE tables (:259-260)                  */
    float scale;                  /* 0.48 (:227)                                                    */
    float veg1p[6], den1p[6];     /* 1 + veg_probs / den_probs, f32 (:211-214)                     */
    int32_t age_lo, age_hi;       /* randint(4, 11) (:409)                                          */
    uint64_t seed;
    int32_t env_offset;
    int32_t empty, tree, fire;
} gca_pine_params;
int gca_alex_pinecones(const gca_pine_params* p, int E, int H, int W, const uint8_t* grid_in, uint8_t* grid_out,
                       int16_t* age_out, const uint8_t* veg, const uint8_t* den, const int32_t* wind_index,
                       const uint32_t* s_cdf, const uint32_t* rng_step, int32_t* counts, uint8_t* act_tiles, void* stream);

/* Classic pinecone spotting: PartiallyObservableForestFire.update's sequential skip-list pass
 * (ca_alexandridis.py:184-210, sampling :35-69, ignition :113-133), after gca_alex_step (classic params) on
 * its output. Every FIRE cell s of grid_in, in row-major order, throws N ~ Poisson(1) pinecones (tail folded at
 * GCA_PINEC_NMAX); pinecone m has direction d uniform over 8 and integer thrust s_m = round(3 N(0,1) ft[lookup[d]])
 * (:189-190, ft of the env's current wind), landing at (r + dx[d] s_m, c + dy[d] s_m). A landing inside the grid
 * and not on s itself ignites its target - WHATEVER the target's state - iff u < 0.58 (1 + p_veg) (1 + p_den)
 * of the target (burn_thr: u24 < thr), with a fresh age randint(4, 11). A target that ignites and comes LATER
 * in the scan is skipped by the reference's loop (:151-152): when that target is itself a FIRE cell of grid_in it
 * throws no pinecones. The device resolves that order dependence exactly: one workgroup per env iterates
 * "s is active iff no active earlier source ignites it" to its fixed point (the dependence is a DAG in scan
 * order), then applies the landings of the active sources. Ages are keyed by the target (the last of several
 * ignitions of one target draws a fresh uniform age in the reference: the same law). counts (nullable):
 * one count moves from the target's previous state to FIRE per ignited target.
 * s_cdf [n_winds][8][GCA_PINEC_CDF] u32: per (wind, direction) t[0] = 2K, t[1..2K] thresholds of
 * P(round(3 ft Z) <= -K + j) * 2^32. scratch: NULL when 16 * ceil(H W / 32) bytes fit one workgroup's LDS
 * (H W <= 262144 = 512 x 512), else E * 4 * ceil(H W / 32) u32 of device memory (the kernel clears it).
 * Draws: Philox (lin, env, step, PINEC + 0) -> N, (lin, env, step, PINEC + 1 + m) -> s (word 0), u (word 1 >> 8),
 * d (word 2 >> 29); (target lin, env, step, PINEC_AGE) word 0 -> age. */
#define GCA_PINEC_NMAX 16
#define GCA_PINEC_CDF 48
#define GCA_PINEC_LDS_MAX_HW 262144
typedef struct {
    uint32_t n_cdf[GCA_PINEC_NMAX]; /* P(Poisson(1) <= j) * 2^32, j = 0..15 (N_p = poisson(), :37)              */
    int32_t dx[8], dy[8];           /* dx_lookup / dy_lookup (:63-64)                                          */
    uint32_t burn_thr[6][6];        /* [veg][den]: ceil(p * 2^24), p = 0.58 * (1 + p_veg) * (1 + p_den) in f64 */
    int32_t age_lo, age_hi;         /* integers(4, 11) (:131)                                                  */
    uint64_t seed;
    int32_t env_offset;
    int32_t empty, tree, fire;
} gca_pine_classic_params;
int gca_alex_pinecones_classic(const gca_pine_classic_params* p, int E, int H, int W, const uint8_t* grid_in,
                               uint8_t* grid_out, int16_t* age_out, const uint8_t* veg, const uint8_t* den,
                               const int32_t* wind_index, const uint32_t* s_cdf, const uint32_t* rng_step,
                               int32_t* counts, uint32_t* scratch, void* stream);

/* --------------------------------- AdvancedForestFireBulldozer env step (batched)
 * advanced_bulldozer.py:1103-1133 minus observations, + _award/_is_done :597-633.  */
typedef struct {
    float t_move[9], t_shoot[2], t_any;  /* f32 like the JAX env (all moves cost t_move: :745-760) */
    float p_wind_change;                 /* 0.06 (:210)                                            */
    int32_t day_length;                  /* 400 (:733)                                             */
    uint64_t seed;
    int32_t env_offset;
    int32_t n_winds;
    int32_t up_mask, down_mask, left_mask, right_mask;
} gca_advenv_params;

/* After gca_alex_step: wind change (repeat: ca_alexandridis_jax.py:442-451), time
 * accumulation (repeat_ca_jax.py:191-198, f32), MoveJax, ModifyJax (dousing[r][c] = 1
 * if shoot==1), time_step += 1, is_night toggle, reward = -(f/(t+f+1e-8)) f32,
 * done = no fire, rng_step += 1. dous_bits (nullable): the packed layout's dousing bits, set with dousing.
 * steps_elapsed / reward_accumulated (nullable, f32 [E]): stateless_step's episode statistics
 * info["steps_elapsed"] += 1, info["reward_accumulated"] += reward (advanced_bulldozer.py:396-397).    */
int gca_advenv_post(const gca_advenv_params* p, const int32_t* action, int32_t* pos, float* accu,
                    int32_t* wind_index, int32_t* time_step, int32_t* is_night, uint8_t* dousing, uint16_t* dous_bits,
                    int H, int W, const int32_t* counts, uint32_t* rng_step, float* reward, uint8_t* done,
                    float* steps_elapsed, float* reward_accumulated, int E, void* stream);

/* conditional_reset (advanced_bulldozer.py:422-518): envs with done[e] copy their
 * initial grid/age/dousing/position/time/wind_index (and clear done); dous_bits (nullable, packed layout)
 * are zeroed (only without dousing0).                                             */
int gca_reset_where(const uint8_t* done, int E, int H, int W, uint8_t* grid, const uint8_t* grid0,
                    int16_t* age, const int16_t* age0, uint8_t* dousing, const uint8_t* dousing0,
                    uint16_t* dous_bits, int32_t* pos, const int32_t* pos0, float* accu, int32_t* wind_index,
                    const int32_t* wind_index0, void* stream);

/* ------------------------------------------- Advanced env observations (RGB)
 * MDP.build_observation_on_extensions + grid_to_rgb_with_extensions + grid_to_rgb
 * (advanced_bulldozer.py:988-1101) with apply_blur / apply_visibility / transform_grid /
 * apply_extensions (bulldozer/utils/extension_utils.py:89-196).                       */
#define GCA_OBS_MAX_EXT 4
typedef struct {
    int32_t empty, tree, fire;
    int32_t n_ext;                              /* extension channels (reference registry: 2)       */
    int32_t ext_skip_visibility[GCA_OBS_MAX_EXT];
    int32_t ext_skip_blur[GCA_OBS_MAX_EXT];     /* (unblur: 0/1, see_invisible_fires: 1/0)          */
    int32_t enable_extensions;                  /* MDP.enable_extensions                             */
    int32_t should_transform;                   /* MDP.should_transform_grid                         */
    int32_t day_length;                         /* > 0 with time_step: undo the step's is_night toggle */
    float color_day[4][3];                      /* empty, tree, fire, position (0..255 as f32)       */
    float color_night[4][3];
    float tint_day[3], tint_night[3];           /* water tint of doused cells                        */
    int32_t n_choices;                          /* extension-choice ids (create_up_to_k_mappings)     */
    int32_t ext_lookup[8][GCA_OBS_MAX_EXT];     /* id -> binary extension flags                       */
} gca_obs_params;

/* rgb [E][H][W][3] f32 (and, nullable, channels [E][H][W][3 + n_ext] u8 = transformed grid, 0, 0,
 * extension channels) for E envs.
 * mode 0 (env step, advanced_bulldozer.py:1120): grid/position after the step, dousing and is_night
 *   before it (pass the post-step is_night with time_step to undo its toggle); action [E][action_stride]
 *   full actions (move, shoot, extension choice): the choice (column 2, clamped to n_choices - 1) maps
 *   to binary extension flags through ext_lookup (_create_full_actions :308-330); action NULL or
 *   action_stride < 3 = no extension active.
 * mode 1 (reset, :401-411): the reference applies grid_to_rgb_with_extensions to the raw (H, W)
 *   grid; its broadcasting gives rgb[r][c] = colour(grid[c][k]) with k = 3 + the first row holding a
 *   positive value in columns 3.. (clamped), or k = 0 — reproduced as is (square grids only).
 * env_mask (nullable, u8 [E]): only envs with env_mask[e] != 0 are rendered, the others' rgb/channels
 *   are left untouched — conditional_reset's per-env jnp.where(terminated, new obs, old obs) (:464-481). */
int gca_adv_observation(const gca_obs_params* p, int mode, int E, int H, int W, const uint8_t* grid,
                        const uint8_t* dousing, const int32_t* pos, const int32_t* is_night, const int32_t* time_step,
                        const int32_t* action, int action_stride, float* rgb, uint8_t* channels,
                        const uint8_t* env_mask, void* stream);

/* gca_alex_step_march_rgb for the extension pipeline (W = 256, codes 0 / 1 / 2): the frame of gca_adv_observation
 * mode 0 (action = the full actions, action_stride >= 3) from the CA step's epilogue, minus the bulldozer's pixel
 * (gca_obs_position), for every env whose display is channel 0 of the extended grid -- the grid itself (the unblur
 * choice) or all zeros (see_invisible_fires: its blur is shown only when row 0 of the blur is empty; the reference's
 * row-vs-channel display scan, advanced_bulldozer.py:1035-1064). The kernel checks that speculation on row 0 of the
 * new grid and sets refit[e] = 1 (else 0) when it fails or when the display needs the blurred grid (no extension
 * chosen with should_transform): those envs' frames are left for gca_adv_observation with env_mask = refit, after
 * the env step. Results of the pair are bit for bit gca_adv_observation's. */
int gca_alex_step_march_rgb_ext(const gca_alex_params* p, const gca_obs_params* op, int E, int H, int W,
                                const uint8_t* grid_in, uint8_t* grid_out, const int16_t* age_in, int16_t* age_out,
                                const uint8_t* vd, const uint16_t* dous_bits, const float* edge_slope,
                                const int32_t* wind_index, const uint32_t* rng_step, int32_t* counts,
                                const uint8_t* act_in, uint8_t* act_out, const float* color_table,
                                const int32_t* is_night, float* rgb, const int32_t* action, int action_stride,
                                uint8_t* refit, void* stream);

/* [night][kind empty / tree / fire][dousing 0 / 1] float4 colours (rgb, 0) of grid_to_rgb (advanced_bulldozer.py:1041-1093),
 * the table gca_alex_step_packed_rgb reads: table[12][4] f32 device, 16-B aligned. */
int gca_obs_color_table(const gca_obs_params* p, float* table, void* stream);
/* rgb[e][pos[e]] = the position colour of the PRE-step day / night (is_night after the env step, time_step to undo its
 * toggle; time_step NULL = is_night as given): grid_to_rgb's .at[position].set (:1095-1099) over a fused frame. */
int gca_obs_position(const gca_obs_params* p, int E, int H, int W, const int32_t* pos, const int32_t* is_night,
                     const int32_t* time_step, float* rgb, void* stream);

/* Synthetic inputs for benches/tests (Philox, GCA_TAG_INIT / GCA_TAG_ACTION).
 * gca_fill_categorical: out[e][i] (u8, [E][n_per_env]) = values[k], u = u01_f32 of word i & 3 of Philox((i >> 2,
 *   env_offset + e, 0, GCA_TAG_INIT), seed), k the first index < n_values - 1 with u < cdf[k]; a u at or above every
 *   one of those entries FALLS THROUGH to the last value, values[n_values - 1] (cdf[n_values - 1] is never read, and
 *   n_values = 1 fills with values[0]). cdf f32 and values u8 are device arrays.
 * gca_random_actions: action[e] = (randint_ms(x.x, 0, 9), x.y >> 31), x = Philox((0, env_offset + e, rng_step[e]
 *   (NULL: 0), GCA_TAG_ACTION), seed). */
int gca_fill_categorical(uint8_t* out, int64_t n_per_env, int E, int env_offset, uint64_t seed,
                         const float* cdf, const uint8_t* values, int n_values, void* stream);
int gca_random_actions(int32_t* action, int E, int env_offset, uint64_t seed, const uint32_t* rng_step,
                       void* stream);

/* ------------------------------------------ Drossel-Schwabl (helicopter CA)
 * ForestFire.update (ca_DrosselSchwabl.py:32-66). The reference draws one f64
 * uniform per TREE-without-burning-neighbour and per EMPTY cell, in row-major
 * order, from op.np_random. Exact-stream mode: uniforms[] holds those draws in
 * order (n = gca_ds_count_draws). One workgroup per env (scan over the grid).
 * uniforms is ONE array shared by all envs: env e's j-th draw is uniforms[uniform_offset[e] + j], so uniform_offset
 * [E] indexes that array (typically the exclusive sum of n_draws), not a per-env slice. uniforms = NULL: Philox mode,
 * u = u01_f64 of Philox((cell, env_offset + e, rng_step[e] or 0, GCA_TAG_DS_CELL), seed), uniform_offset unused.
 * counts (nullable) [E][3] EMPTY / TREE / FIRE cells of grid_out, OVERWRITTEN (the caller need not zero them).   */
int gca_ds_count_draws(const uint8_t* grid, int E, int H, int W, int empty, int tree, int fire,
                       int32_t* n_draws, void* stream);
int gca_ds_step(const uint8_t* grid_in, uint8_t* grid_out, int E, int H, int W, int empty, int tree, int fire,
                const double* thresholds /*[E][2]: cdf0 of choice([T,F], p=[p_fire,1-p_fire]), same for p_tree*/,
                const double* uniforms, const int64_t* uniform_offset, uint64_t seed, const uint32_t* rng_step,
                int env_offset, int32_t* counts, void* stream);

/* The whole ForestFireHelicopter env step for E envs in one launch (helicopter.py:220-236 MDP.update + ca_env.py:27-48
 * step / reward; operators: move_modify.py:37-67 Move, :128-134 MoveModify, ca_DrosselSchwabl.py:32-66 ForestFire):
 *   action   action[e] clamped to [0, 8]; action == NULL: randint_ms(x.x, 0, 9) of Philox((0, env_offset+e,
 *            rng_step[e], GCA_TAG_ACTION), action_seed), column 0 of gca_random_actions, written to action_out[e]
 *            (nullable; with a caller's action it receives that action unclamped)
 *   Move     pos[e] under the helicopter's action sets up {0,1,2}, down {6,7,8}, left {0,3,6}, right {2,5,8}
 *   CA       iff freeze[e] == 0: one Drossel-Schwabl step from buf[parity[e]][e] into buf[parity[e]^1][e], parity
 *            flipped; bit-identical to gca_ds_step(..., uniforms = NULL, seed, rng_step, env_offset) on that grid
 *   Modify   always on, at the moved position on the post-CA grid: FIRE -> EMPTY and hit[e] = 1, else hit[e] = 0
 *   freeze   max_freeze after a CA step, else freeze - 1
 *   counts   [E][3] EMPTY / TREE / FIRE of the env's grid after the step (in: of its grid before the step)
 *   reward   (double)T / n - (double)F / n, n = H*W: two IEEE divisions and one subtraction, which is
 *            np.dot([0, 1, -1], counts / ncells) (helicopter.py:120-135) bit for bit
 *   rng_step[e] += 1, steps_elapsed[e] += 1; the env never terminates (helicopter.py:137-138).
 * thresholds [E][2] as gca_ds_step's. Any H, W >= 1 with H*W < 2^30; W % 256 == 0 with 4-byte aligned grids takes the
 * dword path. Three distinct u8 codes; cells holding another value are copied and not counted.
 * meet (nullable): E 64-bit slots, zero-initialised once by the caller (every launch leaves them zero); with them a
 * small launch (E * P < 1024) splits each env's rows over P <= 8 workgroups that meet in one atomic per env, the last
 * to arrive writing the env's outputs -- the same results; NULL, or H*W + 1 >= 2^20: one workgroup per env. Not
 * shared between concurrent launches. The host build runs plain loops and ignores meet. */
int gca_helicopter_step(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                        const int32_t* action, uint64_t action_seed, int32_t* action_out, const double* thresholds,
                        int32_t* freeze, uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H,
                        int W, int32_t* pos, int32_t* counts, uint8_t* hit, double* reward, int64_t* steps_elapsed,
                        uint64_t* meet, int E, void* stream);

/* K consecutive ForestFireHelicopter env steps of E envs (K x helicopter.py:220-236 MDP.update + ca_env.py:27-48 step /
 * reward): exactly K calls of gca_helicopter_step on the same state tensors, step k taking actions + k*E. actions
 * (K, E) int32, decided before the launch (frame-skip, open-loop planners, recorded trajectories); actions == NULL:
 * step k draws its actions inside the step from action_seed, keyed by the env's rng_step at that step, as
 * gca_helicopter_step's action == NULL does. Afterwards every state tensor (both planes of buf, parity, freeze, pos,
 * counts, rng_step (mod 2^32), hit and reward of the last step, steps_elapsed) holds bit for bit what the K calls
 * leave. Records, each (K, E) and nullable: row k of action_out / reward_out / hit_out = what step k writes to
 * action_out (the raw action, unclamped) / reward / hit.
 * A grid whose two 4-byte-pitched, EMPTY-padded planes fit in 64 KiB of LDS (4 * (1 + (H + 2) * (ceil(W / 4) + 1))
 * bytes each) runs all K steps in ONE launch, one workgroup per env, the grid resident in LDS and the env's scalars
 * in registers; global memory is touched at entry, at exit and for the records. Other shapes run K launches of the
 * step kernel (one workgroup per env, no meet) on the same stream: the same results, the caller need not know which.
 * Launches only (no sync, no allocation, no memset): capturable. K == 0 is a no-op, K < 0 an argument error; the other
 * arguments and limits are gca_helicopter_step's. The host build runs plain loops. */
int gca_helicopter_rollout(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                           const int32_t* actions, uint64_t action_seed, int K, int32_t* action_out,
                           double* reward_out, uint8_t* hit_out, const double* thresholds, int32_t* freeze,
                           uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W,
                           int32_t* pos, int32_t* counts, uint8_t* hit, double* reward, int64_t* steps_elapsed, int E,
                           void* stream);

/* ------------------------------------------ policy observation of the batched envs (no reference counterpart)
 * A compact observation of every env of a batched bulldozer / helicopter env, both parts in ONE launch that reads each
 * env's current plane buf[parity[e]][e] (u8 [E][H][W]) once; pinned by the numpy restatement tests/_policy_obs_ref.py.
 *   local_out  u8 [E][S][S], S = 2 radius + 1: entry (i, j) is the class of cell (pos[e][0] - radius + i,
 *              pos[e][1] - radius + j): 1 the cell equals `tree`, 2 it equals `fire`, 0 any other in-grid cell, 3 outside
 *              the grid. A position outside the grid is no error: the window is class 3 wherever it misses the grid.
 *   coarse_out f32 [E][2][Hc][Wc], Hc = ceil(H / block), Wc = ceil(W / block): channel 0 the number of `tree` cells of
 *              block (bi, bj) times 1 / block^2, channel 1 the same for `fire`; a block that sticks out of the grid
 *              counts its in-grid cells only. Counts <= 4096 and the scale is a power of two: every value is exact.
 * Classification is by equality with the codes (three values in [0, 255]) in every form. radius in [0, 31]; block a
 * power of two in [1, 64]; H * W < 2^30. local_out or coarse_out may be NULL (that part is skipped; both NULL is an
 * argument error). parity == NULL: every env reads buf0 (buf1 may then be NULL).
 * form: 1 the generic form (any H, W, block); 2 the rows form, for W = 256 / 512, block = 8 / 16 / 32, H % block == 0
 * and 8-B aligned planes (anything else is an argument error): a wave holds whole image rows, sums SWAR equality flags
 * per byte over a block-row and adds them across the lanes of a block by DPP; 0 picks the rows form exactly when it
 * applies. Both forms give the same bytes. One launch, no allocation, no sync, no atomics: capturable. The host build
 * runs plain loops (`form` is validated the same way, alignment aside, and otherwise ignored). */
int gca_policy_observation(const uint8_t* buf0, const uint8_t* buf1, const uint8_t* parity, const int32_t* pos, int E,
                           int H, int W, int empty, int tree, int fire, int radius, int block, int form,
                           uint8_t* local_out, float* coarse_out, void* stream);

/* ------------------------------------------ helicopter policy (the agent of the reference's PPO collection loop,
 * agents/jax_ppo.py:866-899: observe, network, softmax sample, step, record -- here inside the env's own launches)
 * A two-layer MLP over gca_policy_observation(radius, block)'s tensors. S = 2 radius + 1, C = 2 Hc Wc, Hd = hidden, a
 * power of two in [32, 256]. All f32; every multiply and every add below is rounded on its own (no fma).
 *   inputs   term n, n = 0 .. S*S + C - 1:  n < S*S:  t_n[j] = w_local[n][local_n][j]  (a table lookup, no multiply;
 *            local_n the class 0..3 of window cell n, row-major; a class above 3 counts modulo 4)
 *            n >= S*S: t_n[j] = w_coarse[c][j] * coarse_c, c = n - S*S (coarse flattened (2, Hc, Wc) row-major)
 *   hidden   G = 1024 / Hd groups. p_g[j] = ((0 + t_g[j]) + t_{g+G}[j]) + t_{g+2G}[j] + ...: group g's terms in
 *            increasing n, left to right, starting from 0.0f (a group without terms is 0.0f).
 *            h_j = relu(((b1[j] + p_0[j]) + p_1[j]) + ... + p_{G-1}[j]), relu(x) = x > 0 ? x : 0.
 *   heads    out_o, o = 0..9: q_r = ((0 + w_out[r][o] * h_r) + w_out[r+16][o] * h_{r+16}) + ..., r = 0..15 (j = r,
 *            r + 16, ... < Hd, left to right from 0.0f); then the pairwise tree a_r = q_r + q_{r+8} (r < 8),
 *            b_r = a_r + a_{r+4} (r < 4), c_r = b_r + b_{r+2} (r < 2), d = c_0 + c_1; out_o = b2[o] + d.
 *            Outputs 0..8 are the action logits l_i, output 9 is the value.
 *   sampling m = l_0, then for i = 1..8: if l_i > m then m = l_i (the first maximum). greedy != 0: the action is the
 *            index of that first maximum, nothing is drawn. Otherwise p_i = exp_f32(l_i - m) (the deterministic expf of
 *            DESIGN.md), c_i = c_{i-1} + p_i for i = 0..8 (c_{-1} = 0.0f), u = u01_f32(x.x) of Philox((0, env_offset +
 *            e, rng_step[e], GCA_TAG_POLICY), policy_seed); the action is the first i with u * c_8 < c_i, else 8.
 *            Non-finite weights still give an action in [0, 8]; nothing else is promised for them.
 * The order depends on (S, C, Hd) only: never on E, K, the launch shape or the path that runs. The device (one workgroup
 * per env runs policy_outputs of csrc/gca_policy_dev.h, the one implementation both agents share: a thread owns four
 * consecutive units, Hd / 4 threads a weight row, which leaves the G groups; 16 lanes per output meet in an xor
 * butterfly), the host build (policy_outputs_host, gca_cpu.cpp) and the numpy restatement
 * tests/_helicopter_policy_ref.py all follow it, so they agree bit for bit.
 * Layouts: w_local f32 [S*S][4][Hd] and w_coarse f32 [C][Hd] (both 16-B aligned on the device), b1 f32 [Hd], w_out
 * f32 [Hd][10], b2 f32 [10] (device arrays; the struct itself is a host struct read at call time). gca_policy is the
 * struct of both agents' networks (the bulldozer's w_out and b2 have twelve columns). */
typedef struct {
    int32_t radius, block;     /* gca_policy_observation's: radius in [0, 31], block a power of two in [1, 64] */
    int32_t hidden;            /* Hd, a power of two in [32, 256]                                               */
    int32_t reserved;          /* 0                                                                             */
    const float* w_local;
    const float* w_coarse;
    const float* b1;
    const float* w_out;
    const float* b2;
} gca_policy;
typedef gca_policy gca_heli_policy;

/* The policy's action for E envs on a given observation, ONE launch (a workgroup per env), no allocation, no sync:
 * capturable. local u8 [E][S][S] and coarse f32 [E][C] as gca_policy_observation writes them (C = 2 Hc Wc is given; the
 * network has no other use for the grid's shape and p->block is not read). Writes action i32 [E], logits f32 [E][9]
 * (nullable) and value f32 [E] (nullable). No env state changes: rng_step is read only, so the value of the state after
 * a rollout (the bootstrap) is free of side effects. C even, and small enough for the coarse map in LDS (C <= 15088). */
int gca_helicopter_policy_act(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                              const uint32_t* rng_step, int env_offset, uint64_t policy_seed, int greedy,
                              int32_t* action, float* logits, float* value, int E, void* stream);

/* K closed-loop env steps of E envs: bit for bit K x (gca_policy_observation(p->radius, p->block) of the state before the
 * step -- the position before the move, the current plane after the previous step --, gca_helicopter_policy_act on it,
 * gca_helicopter_step with that action). The arguments are gca_helicopter_rollout's with the actions replaced by the
 * policy. Records, each nullable, row k = what step k saw and did: action_out i32 (K, E), logits_out f32 (K, E, 9),
 * value_out f32 (K, E), reward_out f64 (K, E), hit_out u8 (K, E), local_out u8 (K, E, S, S), coarse_out f32
 * (K, E, 2, Hc, Wc). The state tensors afterwards are those of the K x 3 calls.
 * Where the two LDS planes of gca_helicopter_rollout plus 4 * (C rounded up to 4 + 1296) bytes of the network fit in
 * 64 KiB, everything runs in ONE launch: the window and the block counts come from the LDS plane, the hidden partials
 * and the outputs live in LDS, the weights are read from global memory; five barriers per step. Other shapes run the
 * K x 3 launches on the stream with the same results; they keep a step's action, window and coarse map in the record
 * rows, or, for a record the caller does not keep, in `scratch`: E * (4 + 4 C + S*S) bytes of device memory, 4-byte
 * aligned (nullable when the three records are given or the shape is resident; pass it always to be shape-agnostic).
 * Launches only: capturable. K == 0 is a no-op, K < 0 and every other argument error is reported before any launch. */
int gca_helicopter_policy_rollout(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                                  const gca_heli_policy* p, uint64_t policy_seed, int greedy, int K,
                                  int32_t* action_out, float* logits_out, float* value_out, double* reward_out,
                                  uint8_t* hit_out, uint8_t* local_out, float* coarse_out, void* scratch,
                                  const double* thresholds, int32_t* freeze, uint32_t* rng_step, uint8_t* parity,
                                  uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts,
                                  uint8_t* hit, double* reward, int64_t* steps_elapsed, int E, void* stream);

/* ------------------------------------------ bulldozer policy (the two-headed agent of the reference's PPO collection
 * loop on the bulldozer env: Actor(action_dims=[9, 2]), agents/jax_ppo.py:305-356, 866-899)
 * The helicopter policy's network with TWELVE outputs. Inputs, hidden layer and summation order are exactly those of
 * "helicopter policy" above: the G = 1024 / Hd groups, a group's terms in increasing n from 0.0f, the relu, and per
 * output the 16 partial sums q_r (j = r, r + 16, ... left to right from 0.0f) that meet in the 8-4-2-1 tree;
 * out_o = b2[o] + d for o = 0..11. out[0..8] are the move logits l_i, out[9..10] the shoot logits s_0, s_1, out[11] the
 * value. All f32, every multiply and add rounded on its own (no fma).
 *   draw     x = Philox((uint32)steps_elapsed[e], env_offset + e, episode ? episode[e] : 0, GCA_TAG_BPOLICY) under
 *            policy_seed. Not keyed by rng_step: in this env it counts CA passes, not env steps, and would repeat one
 *            uniform over several steps.
 *   move     the helicopter rule on l_0..l_8 with u = u01_f32(x.x): m the first maximum, p_i = exp_f32(l_i - m),
 *            c_i = c_{i-1} + p_i, the first i with u * c_8 < c_i, else 8.
 *   shoot    m the first maximum of (s_0, s_1) (m = s_0; if s_1 > m then m = s_1), p_i = exp_f32(s_i - m), c_0 = p_0,
 *            c_1 = c_0 + p_1, u = u01_f32(x.y): shoot = 0 if u * c_1 < c_0, else 1.
 *   greedy   != 0: the index of the first maximum of each head, nothing drawn.
 * Non-finite weights still give a move in [0, 8] and a shoot in {0, 1}; nothing else is promised for them.
 * The order depends on (S, C, Hd) only: never on E, K, the number of waves of the launch or the path that runs. The
 * device (the same policy_outputs of csrc/gca_policy_dev.h with twelve outputs: its 256 float4 "virtual threads" are
 * looped over the workgroup's real threads, so any wave count gives the same sums), the host build (the same
 * policy_outputs_host) and tests/_bulldozer_policy_ref.py follow it and agree bit for bit.
 * Layouts: w_local f32 [S*S][4][Hd] and w_coarse f32 [C][Hd] (16-B aligned on the device), b1 f32 [Hd], w_out f32
 * [Hd][12], b2 f32 [12] (device arrays; the struct itself is a host struct read at call time). */
#define GCA_TAG_BPOLICY 0x42504F4Cu /* 'BPOL' : the bulldozer policy's draw (word 0 move, word 1 shoot) */
typedef gca_policy gca_bulldozer_policy;

/* The policy's action for E envs on a given observation, ONE launch (a workgroup per env), no allocation, no sync:
 * capturable. local u8 [E][S][S] and coarse f32 [E][C] as gca_policy_observation writes them (C = 2 Hc Wc even, at most
 * 15088; p->block is not read). steps_elapsed i64 [E] and episode u32 [E] (nullable: 0) key the draw and are the only
 * env state read; nothing is changed, so the value of the state after a rollout (the bootstrap) is free of side
 * effects. Writes action i32 [E][2] (move, shoot), logits f32 [E][11] (nullable: the nine move logits, then the two
 * shoot logits) and value f32 [E] (nullable). The host build runs plain loops in the same order. */
int gca_bulldozer_policy_act(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                             const int64_t* steps_elapsed, const uint32_t* episode, int env_offset,
                             uint64_t policy_seed, int greedy, int32_t* action, float* logits, float* value, int E,
                             void* stream);

/* K closed-loop env steps of E bulldozer envs: bit for bit K x (gca_policy_observation(p->radius, p->block) of the state
 * before the step, gca_bulldozer_policy_act on it, gca_bulldozer_step_fused (meet = NULL) with that action, and then,
 * when autoreset != 0, gca_bulldozer_reset_where(mask = NULL, max_steps, set_episode = -1)). The arguments are
 * gca_bulldozer_rollout's with actions / action_seed replaced by the policy. An env that is done without autoreset still
 * observes, acts and records every step; its step is the no-op (reward 0, steps_elapsed unchanged, so a fixed seed
 * repeats its action). Records, each nullable, row k = what step k saw and did: action_out i32 (K, E, 2), logits_out
 * f32 (K, E, 11), value_out f32 (K, E), reward_out f64 (K, E), terminated_out / truncated_out u8 (K, E) as
 * gca_bulldozer_rollout defines them, local_out u8 (K, E, S, S), coarse_out f32 (K, E, 2, Hc, Wc). steps_elapsed is
 * required; episode only under autoreset (NULL keys the draw with 0).
 * ONE launch, one workgroup per env with the env's state in registers, where the observation's rows form applies
 * (block 8 / 16 / 32, H % block == 0) and the coarse map plus the network's words fit in a workgroup's 64 KiB of LDS
 * (4 * (C rounded up to 4) + 5184 bytes, plus 512 of the kernel's own: C = 8192 for 512 x 512 at block 8 fits). The
 * coarse map then lives in LDS for the whole launch: counted from the current plane on entry, after every CA pass and
 * after every in-launch reset, and adjusted by -+ 1 / block^2 where Modify changes a cell in between (every value is a
 * multiple of 1 / block^2 that is at most 1, so the adjusted map equals a recount exactly). Every other shape runs the
 * K x 3 (+ reset, + one small launch that writes the reward / flag rows) launches on the stream with the same results;
 * they keep a step's action, window and coarse map in the record rows, or, for a record the caller does not keep, in
 * `scratch`: E * (8 + 4 C + S*S) bytes of device memory, 4-byte aligned (nullable when action_out, local_out and
 * coarse_out are given or the shape is resident; pass it always to be shape-agnostic). Launches only: capturable.
 * K == 0 is a no-op; K < 0 and every other argument error is reported before any launch. Device build only (the host
 * build has no Windy CA for these sizes). */
int gca_bulldozer_policy_rollout(const gca_bulldozer_params* p, const gca_bulldozer_policy* policy,
                                 uint64_t policy_seed, int greedy, int K, int32_t* action_out, float* logits_out,
                                 float* value_out, double* reward_out, uint8_t* terminated_out, uint8_t* truncated_out,
                                 uint8_t* local_out, float* coarse_out, void* scratch, int autoreset,
                                 uint64_t reset_seed, int64_t max_steps, const float* cdf, const uint8_t* values,
                                 uint32_t* episode, int64_t* last_length, uint8_t* terminated, uint8_t* truncated,
                                 double* accu, int32_t* steps, uint8_t* done, const double* wind, int64_t wind_stride,
                                 uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W,
                                 int32_t* pos, int32_t* counts, uint8_t* hit, double* reward, int64_t* steps_elapsed,
                                 int E, void* stream);

/* ------------------------------------------ advanced policy (the bulldozer policy on the Advanced bulldozer env, the
 * env the reference's PPO agent trains on: observe and act in one launch)
 * The results are bit for bit those of two calls in sequence:
 *   1. gca_policy_observation(grid, NULL, NULL, pos, E, H, W, empty, tree, fire, policy->radius, policy->block, 0,
 *      local, coarse)
 *   2. gca_bulldozer_policy_act(policy, C, local, coarse, steps_elapsed, NULL, env_offset, policy_seed, greedy, ...)
 *      with steps_elapsed[e] = (int64)time_step[e] and C = 2 Hc Wc of (H, W, policy->block).
 * The network, its summation order and both samplers are those of "bulldozer policy" above. The draw is
 * Philox(((uint32)time_step[e], env_offset + e, 0, GCA_TAG_BPOLICY), policy_seed): the env's time_step advances by one
 * per env step and is kept across its conditional reset, so a draw never repeats within an env's life.
 * grid u8 [E][H][W] is the env's current plane, pos i32 [E][2], time_step i32 [E]. action i32 [E][action_stride],
 * action_stride >= 2: only columns 0 (move) and 1 (shoot) are written, a third column (the env's extension choice)
 * stays the caller's. logits f32 [E][11], value f32 [E], local_out u8 [E][S][S] and coarse_out f32 [E][C] are nullable;
 * the last two record what the network saw. No env state changes.
 * Always ONE launch, one 256-thread workgroup per env: the coarse map is counted straight into LDS (the observation's
 * rows form where W = 256 / 512, block = 8 / 16 / 32, H % block == 0 and grid is 8-B aligned, else its generic form;
 * same bytes), the window is read from the plane. No scratch, no allocation, no sync, no atomics: capturable. H * W <
 * 2^30, C at most 15088, u8 codes; argument errors are reported before the launch. The host build runs the two host
 * functions above in plain loops. */
int gca_advanced_policy_act(const gca_bulldozer_policy* policy, const uint8_t* grid, const int32_t* pos,
                            const int32_t* time_step, int E, int H, int W, int empty, int tree, int fire,
                            int env_offset, uint64_t policy_seed, int greedy, int32_t* action, int action_stride,
                            float* logits, float* value, uint8_t* local_out, float* coarse_out, void* stream);

/* The observation with the retardant in it. On the Advanced env the agent's second head drops retardant, which the env
 * keeps in its `dousing` layer and not in the grid (the reference's agent sees it in its RGB frame, whose colours are
 * indexed [kind][dousing 0/1]: advanced_bulldozer.py:1041-1093); gca_policy_observation reads the grid alone. This one
 * replaces it for that env: `local_out` u8 [E][S][S] is gca_policy_observation's window unchanged, and feat_out f32
 * [E][C2], C2 = 3 Hc Wc + S*S rounded up to even, is the vector the network takes in the coarse map's place:
 *   [0, 2 Hc Wc)               gca_policy_observation's coarse map, the same values in the same order
 *   [2 Hc Wc, 3 Hc Wc)         block (bi, bj), row-major: the number of its in-grid cells with dousing != 0, times
 *                              1 / block^2 (exact: a count of at most 4096 times a power of two)
 *   [3 Hc Wc, 3 Hc Wc + S*S)   window cell n = i * S + j at (pos[e][0] - radius + i, pos[e][1] - radius + j): 1.0f if the
 *                              cell is inside the grid and dousing != 0 there, else 0.0f
 *   one more word, 0.0f, when 3 Hc Wc + S*S is odd
 * dousing u8 [E][H][W]. dous_bits u16 [E][H][W / 16], nullable and allowed only when W % 16 == 0 (2-B aligned): bit
 * c % 16 of word [r][c / 16] is set iff dousing[r][c] != 0, as the env's packed layout keeps it. With dous_bits the
 * launch takes the retardant from the bits and does not read the u8 layer; without, it reads the u8 layer. The block
 * counts come from the bits by popcount -- a dword of a bit row holds four, two or one tile rows at block 8 / 16 / 32
 * (W % 32 == 0, 4-B aligned bits), any other shape masks the tile's bit range out of its words -- and from the u8 layer
 * by byte loops; the grid's two channels come as in gca_advanced_policy_act. Either output may be NULL, not both;
 * radius, block, the codes and H * W as gca_policy_observation; C2 < 2^31. ONE launch, a 256-thread workgroup per env,
 * no allocation, no sync, no atomics: capturable. The host build runs plain loops on `dousing`; it validates dous_bits
 * the same way and does not read it. Pinned by tests/_retardant_obs_ref.py. */
int gca_advanced_policy_observation(const uint8_t* grid, const uint8_t* dousing, const uint16_t* dous_bits,
                                    const int32_t* pos, int E, int H, int W, int empty, int tree, int fire, int radius,
                                    int block, uint8_t* local_out, float* feat_out, void* stream);

/* gca_advanced_policy_act on that observation: observe and act in one launch for a policy that sees the retardant. The
 * results are bit for bit those of
 *   1. gca_advanced_policy_observation(grid, dousing, dous_bits, pos, E, H, W, empty, tree, fire, policy->radius,
 *      policy->block, local, feat)
 *   2. gca_bulldozer_policy_act(policy, C2, local, feat, steps_elapsed, NULL, env_offset, policy_seed, greedy, ...) with
 *      steps_elapsed[e] = (int64)time_step[e]
 * The network is "bulldozer policy" with C = C2, so policy->w_coarse is f32 [C2][Hd]; its summation order depends on
 * (S, C, Hd) only. The draw is keyed as gca_advanced_policy_act keys it. Only action columns 0 and 1 are written;
 * logits, value, local_out and feat_out f32 [E][C2] are nullable. No env state changes.
 * Always ONE launch, one 256-thread workgroup per env: the feature vector is built straight into the network's LDS
 * words, every word by one thread, and is complete at the network's first barrier. No scratch, no atomics:
 * capturable. C2 at most 15088 (the LDS of a workgroup), checked before the launch with the other arguments, which are
 * those of the two calls. The host build runs the two host functions. */
int gca_advanced_policy_act_retardant(const gca_bulldozer_policy* policy, const uint8_t* grid, const uint8_t* dousing,
                                      const uint16_t* dous_bits, const int32_t* pos, const int32_t* time_step, int E,
                                      int H, int W, int empty, int tree, int fire, int env_offset,
                                      uint64_t policy_seed, int greedy, int32_t* action, int action_stride,
                                      float* logits, float* value, uint8_t* local_out, float* feat_out, void* stream);

/* ------------------------------------------ extension policy (the three-headed agent the reference trains on the
 * Advanced bulldozer env: Actor(action_dims=[9, 2], choose_k=[(2, 1)]), agents/jax_ppo.py:305-356, 708-710; it observes
 * the frame of build_observation_on_extensions, advanced_bulldozer.py:988-1033, not the true grid)
 *
 * gca_advanced_display: for every env the u8 value plane that gca_adv_observation mode 0 colours -- display_grid of
 * grid_to_rgb_with_extensions before the colour lookup, with no dousing and no position. grid u8 [E][H][W], is_night i32
 * [E]; time_step i32 [E], nullable: when given, the pre-step day/night is recovered as gca_adv_observation recovers it
 * (is_night flipped where time_step % day_length == 0), when NULL is_night is used as it is. choice i32, env e's at
 * choice[e * choice_stride], nullable (NULL: 0 for every env), clamped to [0, n_choices - 1]: ext_lookup[choice] names the
 * active extension channels (none unless enable_extensions). display_out u8 [E][H][W]; its E H W bytes may not overlap the
 * grid's anywhere (the blur reads neighbours; an overlap is an argument error). Every quirk of the
 * frame is kept: blur = floor((2 S + 9) / 18) of the edge-padded 3 x 3 sum S; visibility turns the literal value 3 into 0
 * by day; the first ROW of the channel-last stack holding a positive extension value gives, clamped to n_ext - 1, the
 * CHANNEL displayed everywhere (a switched-off channel is all zeros); with no positive extension value the base channel
 * is displayed (the transformed grid with should_transform, else the grid). One launch, no allocation, no sync:
 * capturable. The host build runs plain loops. Pinned by tests/_extension_policy_ref.py against oracle/observation.py. */
int gca_advanced_display(const gca_obs_params* p, int E, int H, int W, const uint8_t* grid, const int32_t* is_night,
                         const int32_t* time_step, const int32_t* choice, int choice_stride, uint8_t* display_out,
                         void* stream);

/* gca_extension_policy_act: the "bulldozer policy" above with FIFTEEN outputs: out[0..8] the move logits, out[9..10] the
 * shoot logits, out[11..13] the extension logits, out[14] the value; w_out f32 [Hd][15], b2 f32 [15]. Inputs, hidden
 * layer and summation order are unchanged (the heads take 16 * 15 = 240 of 256 lanes). The draw is the bulldozer's,
 * Philox(((uint32)steps_elapsed[e], env_offset + e, episode ? episode[e] : 0, GCA_TAG_BPOLICY), policy_seed): word 0
 * draws the move and word 1 the shoot by the rules above, so a seed gives the two-head agent's move and shoot for equal
 * logits; word 2 draws the extension by the move rule over three logits: m the first maximum of e_0..e_2, p_i =
 * exp_f32(e_i - m), c_i = c_{i-1} + p_i, u = u01_f32(x.z), the first i with u * c_2 < c_i, else 2. greedy != 0: the first
 * maximum of each head, nothing drawn. Non-finite weights still give an extension in [0, 2].
 * action i32 [E][3] (move, shoot, extension), logits f32 [E][14] (nullable), value f32 [E] (nullable); the other
 * arguments and checks are gca_bulldozer_policy_act's. ONE launch, a workgroup per env; the host build runs plain loops
 * in the same order and agrees bit for bit. */
int gca_extension_policy_act(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                             const int64_t* steps_elapsed, const uint32_t* episode, int env_offset,
                             uint64_t policy_seed, int greedy, int32_t* action, float* logits, float* value, int E,
                             void* stream);

/* gca_advanced_policy_act_display: observe the DISPLAYED plane and act, in ONE launch. Bit for bit three calls in
 * sequence:
 *   1. gca_advanced_display(p, E, H, W, grid, is_night, time_step, choice, choice_stride, plane)
 *   2. gca_policy_observation(plane, NULL, NULL, pos, E, H, W, p->empty, p->tree, p->fire, policy->radius,
 *      policy->block, 0, local, coarse)
 *   3. gca_extension_policy_act(policy, C, local, coarse, steps_elapsed, NULL, env_offset, policy_seed, greedy, ...) with
 *      steps_elapsed[e] = (int64)time_step[e] and C = 2 Hc Wc of (H, W, policy->block).
 * The displayed plane never exists: one 256-thread workgroup per env counts the TREE / FIRE shares of the displayed
 * values straight into the network's LDS words and computes the window's classes from the plane, the blur on the fly.
 * action i32 [E][action_stride], action_stride >= 3: columns 0, 1 and 2 are written. logits f32 [E][14], value f32 [E],
 * local_out u8 [E][S][S] and coarse_out f32 [E][C] are nullable; the last two record what the network saw. time_step is
 * required (it keys the draw, as in gca_advanced_policy_act). `choice` MAY point at column 2 of the same `action` rows
 * (choice_stride = action_stride): workgroup e reads env e's choice, and no other env's, before any of its threads
 * writes env e's action (the network's first barrier lies between). No env state changes. No scratch, no allocation, no
 * sync, no atomics: capturable. The host build runs the three host functions. */
int gca_advanced_policy_act_display(const gca_bulldozer_policy* policy, const gca_obs_params* p, const uint8_t* grid,
                                    const int32_t* pos, const int32_t* is_night, const int32_t* time_step,
                                    const int32_t* choice, int choice_stride, int E, int H, int W, int env_offset,
                                    uint64_t policy_seed, int greedy, int32_t* action, int action_stride,
                                    float* logits, float* value, uint8_t* local_out, float* coarse_out, void* stream);

/* gca_extension_policy_grad(_workspace, _vclip): gca_bulldozer_policy_grad for the three heads (9, 2, 3): action i32
 * [T][3], old_logits f32 [T][14], fifteen outputs, the value in column 14, NH = 3. Every mean of pg, entropy, approx_kl
 * and the clip fraction runs over the N x 3 (sample, head) pairs -- the reference stacks the per-head log-probabilities
 * and entropies and never sums over heads (jax_ppo.py:913-926) -- and everything else said of the two-head calls below
 * ("PPO update") holds, with gca_extension_policy_grad_workspace. */
int64_t gca_extension_policy_grad_workspace(const gca_bulldozer_policy* p, int C, int N);
int gca_extension_policy_grad(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                              const int32_t* action, const float* old_logits, const float* advantage,
                              const float* returns, int64_t T, const int32_t* idx, int N, float clip_coef,
                              float ent_coef, float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                              float* g_b1, float* g_w_out, float* g_b2, float* stats, void* workspace,
                              int64_t workspace_bytes, void* stream);
int gca_extension_policy_grad_vclip(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                                    const int32_t* action, const float* old_logits, const float* old_value,
                                    const float* advantage, const float* returns, int64_t T, const int32_t* idx, int N,
                                    float clip_coef, float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                                    float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats,
                                    float* vstats, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------ PPO update (the learner's half of the reference's main loop:
 * agents/jax_ppo.py:932-984 compute_gae, :987-1043 ppo_loss and its gradient), on rollout_policy's records
 * gca_gae: reward f64 (K, E) and value f32 (K, E) as gca_helicopter_policy_rollout records them, next_value f32 (E) the
 * value of the state after the rollout (gca_helicopter_policy_act gives it without side effects), terminal u8 (K, E),
 * nullable: terminal[k][e] != 0 means step k ended env e's episode, nothing is bootstrapped across k -> k + 1 (the
 * reference's dones[1:] with next_done as the last row; NULL = never, the helicopter env never ends). For k = K-1 .. 0,
 * A = 0.0f before the first iteration, every operation an individually rounded f32 one (no fma) in this order:
 *   r = (float)reward; nn = terminal ? 0.0f : 1.0f; nv = k == K-1 ? next_value[e] : value[k+1][e];
 *   delta = (r + (gamma * nv) * nn) - value[k][e];  A = delta + (gamma_lambda * nn) * A;
 *   advantage[k][e] = A;  returns[k][e] = A + value[k][e].
 * gamma_lambda is the caller's float(gamma * gae_lambda) computed in double (jax's weak-typed Python scalars). One launch,
 * a thread per env, no allocation, no sync: capturable. K == 0 is a no-op; argument errors come before any launch. The
 * device, the host build and tests/_ppo_ref.py agree bit for bit. */
int gca_gae(const double* reward, const float* value, const float* next_value, const uint8_t* terminal, float gamma,
            float gamma_lambda, int K, int E, float* advantage, float* returns, void* stream);

/* gca_helicopter_policy_grad: the PPO clipped-surrogate loss (jax_ppo.py:987-1041 with clip_vloss off), its statistics
 * and d loss / d each of the five policy tensors over a minibatch of recorded samples. The T = K E rows are
 * rollout_policy's records flattened: local u8 [T][S][S], coarse f32 [T][C], action i32 [T], old_logits f32 [T][9];
 * advantage / returns f32 [T] are gca_gae's. The minibatch is rows idx[0..N) (NULL: rows 0..N-1, N <= T; repeats
 * allowed; nothing is gathered into a copy). Per sample, with (l, v) the policy's logits and value on that row (class
 * & 3, relu'(0) = 0): logp_new = l[a] - logsumexp(l); logp_old the same function of old_logits; ratio = exp(logp_new -
 * logp_old); A^ the advantage, with norm_adv != 0 (A - mean) / (std + 1e-8) over the minibatch (population std;
 * constants, not differentiated); pg = max(-A^ ratio, -A^ clip(ratio, 1 - c, 1 + c)); vl = 0.5 (v - R)^2; ent = -sum p_i
 * log p_i. loss = mean(pg) - ent_coef mean(ent) + vf_coef mean(vl).
 * stats[8] = {loss, mean pg, mean vl, mean ent, approx_kl = mean((ratio - 1) - logratio), clip fraction = the share of
 * samples with ratio outside [1 - c, 1 + c], adv mean, adv std}.
 * The reference's clipped value loss (clip_vloss, :1021-1030) takes the batch mean BEFORE its maximum, a quirk; it is
 * gca_helicopter_policy_grad_vclip / gca_bulldozer_policy_grad_vclip below.
 * Outputs: g_* f32 in the weights' own layouts, every element written (a (cell, class) row no sample selects is exactly
 * 0.0f), never read, and they may alias neither each other nor the weights. All accumulation is f32 (the scalar loss
 * chain of ONE sample -- the two logsumexps, the ratio, the entropy -- runs in double and is rounded once), no floating-point
 * atomics: partial sums go to `workspace` (gca_helicopter_policy_grad_workspace bytes; a smaller one is an argument
 * error; the workspace, w_local, w_coarse and b1 must be 16-B aligned, which both builds check; the outputs need no
 * alignment) and are added in a fixed order, so equal arguments give equal bits; the result may depend on N and on
 * the launch shape derived from (S, C, Hd, N), on nothing else. The forward inside does NOT follow the act kernels'
 * summation order: logits recomputed with unchanged weights agree with the recorded ones within rounding, not bit for
 * bit. An action outside [0, 8] is clamped. The host build checks idx against [0, T) (an argument error); the device
 * cannot without a sync and clamps each index into [0, T). Launches only: capturable, no allocation, no sync. The host
 * build runs plain loops with the network and the gradient sums in double, rounded once. */
int64_t gca_helicopter_policy_grad_workspace(const gca_heli_policy* p, int C, int N);
int gca_helicopter_policy_grad(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                               const int32_t* action, const float* old_logits, const float* advantage,
                               const float* returns, int64_t T, const int32_t* idx, int N, float clip_coef,
                               float ent_coef, float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                               float* g_b1, float* g_w_out, float* g_b2, float* stats, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* gca_bulldozer_policy_grad: the same loss for the bulldozer's two heads (the reference's Actor(action_dims=[9, 2])),
 * taken PER HEAD as the reference's ppo_loss takes it (agents/jax_ppo.py:902-930 get_action_and_value2 stacks the heads'
 * log-probabilities and entropies to (N, heads), its .sum(axis=1) commented out; update_ppo :1066-1072 repeats the
 * advantages per head, and every .mean() of ppo_loss :987-1041 runs over N x heads). The records are
 * gca_bulldozer_policy_rollout's: action i32 [T][2] (move, shoot), old_logits f32 [T][11] (nine move logits, two shoot
 * logits); the network has twelve outputs, the value in column 11. With NH = 2 heads, head h has logits l_h (9 or 2 of
 * them), recorded logits lo_h and action a_h; A^ is the sample's (optionally normalised) advantage as above:
 *   logratio_h = (l_h[a_h] - lse(l_h)) - (lo_h[a_h] - lse(lo_h)), ratio_h = exp(logratio_h)
 *   pg_h = max(-A^ ratio_h, -A^ clip(ratio_h, 1 - c, 1 + c)); ent_h = -sum p log p over head h; vl = 0.5 (v - R)^2
 *   loss = mean_{s,h} pg - ent_coef mean_{s,h} ent + vf_coef mean_s vl
 * stats[8] in the order above: pg, entropy, approx_kl = mean((ratio - 1) - logratio) and the clip fraction are means
 * over the N NH (sample, head) pairs; v_loss, adv mean and adv std are means over the N samples.
 *   d loss / d l_h[i] = (1 / (N NH)) [dpg_dr_h ratio_h (1[i = a_h] - p_i) + ent_coef p_i (log p_i + ent_h)], with
 *   dpg_dr_h = -A^ where the unclipped branch is the maximum (not clipped, or pg1 > pg2), else 0;
 *   d loss / d v = vf_coef (v - R) / N.
 * An action of head h outside [0, n_h - 1] is clamped. With one head this is gca_helicopter_policy_grad's loss exactly,
 * and everything else said there (outputs, workspace, alignment, fixed summation order, idx, capturability, the host
 * build) holds here with gca_bulldozer_policy_grad_workspace; one sample's terms of a statistic are added over its
 * heads in double and rounded once. */
int64_t gca_bulldozer_policy_grad_workspace(const gca_bulldozer_policy* p, int C, int N);
int gca_bulldozer_policy_grad(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                              const int32_t* action, const float* old_logits, const float* advantage,
                              const float* returns, int64_t T, const int32_t* idx, int N, float clip_coef,
                              float ent_coef, float vf_coef, int norm_adv, float* g_w_local, float* g_w_coarse,
                              float* g_b1, float* g_w_out, float* g_b2, float* stats, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* gca_helicopter_policy_grad_vclip / gca_bulldozer_policy_grad_vclip: the two calls above with the reference's clipped
 * value loss (args.ppo.clip_vloss, its default; agents/jax_ppo.py:1021-1030) in place of vl = 0.5 (v - R)^2. Two more
 * arguments: old_value f32 [T], the RECORDED value (rollout_policy's `value`), indexed through idx like the other
 * records, and vstats f32 [3], nullable. Per minibatch of N samples, with v_s the value output on row s, R_s the return,
 * vo_s the recorded value and c = clip_coef (the ratio clip's coefficient, as in the reference):
 *   U    = 0.5 mean_s (v_s - R_s)^2                  a scalar: the reference takes the batch mean BEFORE its maximum
 *   vc_s = vo_s + clip(v_s - vo_s, -c, +c);  q_s = (vc_s - R_s)^2           (no 0.5)
 *   v_loss = 0.5 mean_s max(U, q_s);  loss = mean pg - ent_coef mean ent + vf_coef v_loss
 * Every other term and statistic is the plain call's. With in_s = 1[|v_s - vo_s| <= c], u_s = 1[U >= q_s] and
 * n_U = sum_s u_s:
 *   d loss / d v_s = vf_coef (0.5 / N) [ (n_U / N) (v_s - R_s) + (1 - u_s) in_s 2 (vc_s - R_s) ]
 * so every sample's gradient depends on two minibatch-wide scalars. Ties: U >= q_s goes to the U branch and
 * |v_s - vo_s| == c to the inside (jax splits a tie's gradient evenly; ties have measure zero). With N = 1 and the
 * sample inside this is the plain 0.5 (v - R)^2 and its gradient.
 * stats[8] keeps its order: v_loss (index 2) and loss (index 0) are the clipped ones.
 * vstats = {U, n_U / N, the share of samples with |v_s - vo_s| > c}; the counts are integer sums, each share the
 * double quotient rounded to f32.
 * Precision. One sample's chain (v_s - R_s, vc_s, q_s, the bracket above) runs in double from the f32 v_s, R_s, vo_s and
 * is rounded to f32 once per term. Device build: U = (sum_s f32(0.5 (v_s - R_s)^2)) * f32(1 / N), an f32 sum in a fixed
 * order (the pairwise tree over a tile's samples that the plain call's v_loss takes, then over the tiles a sequential
 * partial per thread of one 1024-thread workgroup and a tree) and one f32 product; u_s compares (double)U with the
 * double q_s, and both kernels that need u_s and in_s evaluate the same expression on the same words. Host build: U is
 * the double sum times 1 / N in double, compared in double. No floating-point atomics; equal arguments give equal bits.
 * Eight launches instead of four (the value column waits for U, and d loss / d v_s for n_U: after the forward one
 * workgroup forms U from the tiles' sums, a wave per tile counts u_s and the samples outside the clip, one workgroup
 * adds the counts, and a workgroup per tile writes d loss / d v_s, adds its term to d loss / d pre-activations last, as
 * the plain call does, and forms the tile's v_loss and b2[value] sums in the plain call's tree), all on the caller's
 * stream: capturable, no allocation, no sync. With vf_coef = 0 the five gradients and stats 1, 3, 4, 5, 6, 7 equal the plain
 * call's on the same arguments as numbers (the value term contributes +-0, added last).
 * The plain calls' workspace queries serve these (header words 2..4 hold U and the counts). Checks, alignment,
 * aliasing (vstats included), idx and the host build are as for the plain calls. */
int gca_helicopter_policy_grad_vclip(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                                     const int32_t* action, const float* old_logits, const float* old_value,
                                     const float* advantage, const float* returns, int64_t T, const int32_t* idx, int N,
                                     float clip_coef, float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                                     float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats,
                                     float* vstats, void* workspace, int64_t workspace_bytes, void* stream);
int gca_bulldozer_policy_grad_vclip(const gca_bulldozer_policy* p, int C, const uint8_t* local, const float* coarse,
                                    const int32_t* action, const float* old_logits, const float* old_value,
                                    const float* advantage, const float* returns, int64_t T, const int32_t* idx, int N,
                                    float clip_coef, float ent_coef, float vf_coef, int norm_adv, float* g_w_local,
                                    float* g_w_coarse, float* g_b1, float* g_w_out, float* g_b2, float* stats,
                                    float* vstats, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------ optimizer (the rest of the reference's update_ppo, agents/jax_ppo.py:1045-1114:
 * optax.chain(clip_by_global_norm(max_norm), adam(lr, b1, b2, eps)) with linear_schedule, :677-702 and :775-783)
 * gca_adam_step: one optimizer step over n <= GCA_ADAM_MAX_TENSORS parameter tensors in TWO launches, no floating-point
 * atomics, no allocation, no sync: capturable, and equal inputs give equal bits. Tensor t has len[t] >= 1 elements in
 * four f32 arrays: the parameters w (updated in place), the gradient g (read only), the moments m and v (updated in
 * place). Contiguous, 4-byte alignment suffices: a tensor whose four pointers are 16-B aligned takes 16-B accesses,
 * any other a scalar path with the same results. The table is a host struct read at call time.
 * state: GCA_ADAM_STATE_WORDS 4-byte words of device memory that the host never reads: [0] count i32, [1] b1_pow f32,
 * [2] b2_pow f32, [3] the last step's pre-clip gradient norm f32, [4] the last learning rate f32, [5..7] unused,
 * [8..15] the slot the next scalars wait in between the two launches. Before step 1: count = 0, b1_pow = b2_pow = 1.0f
 * (the caller writes them once), everything else 0. A replayed capture advances the count like any other step.
 * Arithmetic: every operation an individually rounded IEEE f32 one (correctly rounded divide and square root, no fma),
 * in exactly this order, but for the sum under the norm and the learning rate, which run in double:
 *   count' = count + 1; b1_pow' = b1_pow * b1; b2_pow' = b2_pow * b2
 *   lr     = lr0 without annealing (steps_per_iteration == 0 and num_iterations == 0); with it (both >= 1), in double
 *            and rounded to f32 once: frac = 1 - ((count / steps_per_iteration) / num_iterations), the first division
 *            an integer one on the count BEFORE this step, the second a real one; lr = lr0 * max(frac, 0). That is the
 *            reference's linear_schedule; the reference never leaves frac >= 0, the clamp at zero is ours.
 *   norm   CH = 1024 * max(1, ceil(total / 2097152)), total = the sum of the lengths. Tensor t is cut into chunks of CH
 *            elements (the last one shorter), and the chunks are numbered through the tensors in argument order. In a
 *            chunk, lane l of 256 adds the squares (each exact in double) of its elements to a double that starts at
 *            0.0, in increasing k and, inside a k, increasing j: elements 4 (l + 256 k) + j, j = 0..3, of the chunk.
 *            The 256 lane sums meet in the tree s[l] = s[l] + s[l + h] for l < h, h = 128, 64, .., 1; s[0] is the
 *            chunk's partial. The partials are summed the same way: lane l adds partials l, l + 256, .. in increasing
 *            order from 0.0, then the same tree. norm = sqrtf((float)sum).
 *   clip   clip_by_global_norm's operations: g' = norm < max_norm ? g : (g / norm) * max_norm; max_norm <= 0: g' = g
 *            (the norm is still computed and recorded).
 *   m      m' = (b1 * m) + ((1.0f - b1) * g')
 *   v      v' = (b2 * v) + (((1.0f - b2) * g') * g')
 *   w      mhat = m' / (1.0f - b1_pow'); vhat = v' / (1.0f - b2_pow'); w' = w - (lr * (mhat / (sqrtf(vhat) + eps)))
 * info_out (nullable, device f32 [2]) receives {norm, lr}. workspace: gca_adam_step_workspace(total) bytes, 8-B
 * aligned; a shorter one is an argument error. Argument errors come before any launch, the same in both builds. The
 * device, the host build and tests/_adam_ref.py follow the order above, so they agree bit for bit. */
#define GCA_ADAM_MAX_TENSORS 8
#define GCA_ADAM_STATE_WORDS 16
typedef struct {
    int32_t n;                 /* tensors in use, 1 .. GCA_ADAM_MAX_TENSORS */
    int32_t reserved;          /* 0 */
    int64_t len[GCA_ADAM_MAX_TENSORS];
    float* w[GCA_ADAM_MAX_TENSORS];
    const float* g[GCA_ADAM_MAX_TENSORS];
    float* m[GCA_ADAM_MAX_TENSORS];
    float* v[GCA_ADAM_MAX_TENSORS];
} gca_adam_tensors;
int64_t gca_adam_step_workspace(int64_t total_elements);
int gca_adam_step(const gca_adam_tensors* t, void* state, float lr0, float b1, float b2, float eps, float max_norm,
                  int64_t steps_per_iteration, int64_t num_iterations, float* info_out, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* gca_permutation: rows permutations of [0, T) in one launch (the minibatch shuffle of update_ppo, jax_ppo.py:1062-1067;
 * our own Philox stream, not jax's). out i32 [rows][T]; every out[r][i] is computed on its own: no sort, no atomic, no
 * second pass. Row r is keyed by k_r = epoch0 + r + (counter ? *counter : 0) (mod 2^32; counter a device i32, read
 * only: a replayed capture draws fresh rows when the counter moves, e.g. the optimizer's count). h = the smallest
 * integer >= 1 with 2^(2h) >= T. The balanced Feistel network on x = (L, R), L = x >> h, R = x & (2^h - 1), runs four
 * rounds (L, R) <- (R, L ^ (F & (2^h - 1))), round = 0..3, F = word 0 of Philox4x32-10 over the counter (R, round, k_r,
 * GCA_TAG_PERM) with the key (seed lo, seed hi); x' = (L << h) | R. Starting from x = i the network is applied until
 * x < T: a bijection of [0, 2^(2h)) walked cyclically is a permutation of [0, T). The walk is capped at 1024
 * applications (probability below (3/4)^1024); a thread that reaches the cap writes i, the host build reports
 * GCA_ERR_UNSUPPORTED ("internal: ..."). 1 <= T < 2^31, 1 <= rows <= 65535. The device, the host build and
 * tests/_adam_ref.py agree bit for bit. */
#define GCA_TAG_PERM 0x5045524Du /* 'PERM' : the minibatch permutation's round function */
int gca_permutation(uint64_t seed, uint32_t epoch0, const int32_t* counter, int64_t T, int rows, int32_t* out,
                    void* stream);

/* ------------------------------------------ measurement yardsticks (bench.py; no reference counterpart)
 * gca_bench_copy: a 16-B device copy of nbytes (one element per thread, one pass) (a multiple of 16, 16-B aligned), nt != 0 non-temporal
 * loads and stores: the practical HBM ceiling the bench reports beside the 8 TB/s spec.
 * gca_bench_march_pattern: the loads and stores of gca_alex_step_march at W = 256 (radius R in 4..7; with rgb != NULL
 * also the fused frame's f32 RGB stores) with trivial arithmetic, on the env's packed-layout buffers: the floor of
 * that access pattern on this device; edge_slopes = NULL: the flat-terrain step's pattern (no slope planes), and vd =
 * NULL with it the uniform-layers step's (no vd layer either). Outputs are scratch (their values mean nothing). */
int gca_bench_copy(const void* src, void* dst, int64_t nbytes, int nt, void* stream);
int gca_bench_march_pattern(int R, int E, int H, int W, const uint8_t* grid, uint8_t* grid_out, const int16_t* age,
                            int16_t* age_out, const uint8_t* vd, const uint16_t* dous_bits, const float* edge_slopes,
                            float* rgb, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCA_H */
