// gca_heli.hip — the whole ForestFireHelicopter env step for E envs in one launch on gfx950
// (helicopter.py:220-236 MDP.update + ca_env.py:27-48 reward): action, Move (move_modify.py:37-67), when the env's
// freeze countdown is 0 one Drossel–Schwabl step (ca_DrosselSchwabl.py:32-66, the Philox mode of gca_ds_step bit for
// bit) from buf[parity] into buf[parity ^ 1], Modify {FIRE: EMPTY} at the moved position on the post-CA grid
// (move_modify.py:128-134), freeze, counts, reward, rng_step and steps_elapsed.
//
// Layout: an env's rows are split over P workgroups of 4 waves (P = 1 without `meet`). W % 256 == 0: a wave takes
// (strip of HELI_SH rows) x (256 columns), a lane 4 cells of a row as one dword; the FIRE flags are byte masks, the
// left / right neighbours come from the adjacent lanes (DPP wave shifts), a row is loaded once per strip and its
// horizontal 3-cell OR is carried down the strip. Other widths: a cell per thread, nine byte loads.
// No prefix scan: a cell's draw is keyed by its index (Philox (cell, global env id, rng_step, DSCE)), not by its rank.
// `u < thr` is the integer test (bits >> 11) < ceil(thr * 2^53) (scaling by 2^53 is exact), the two integer
// thresholds computed once per env.
// Modify is folded into the CA's own store of that cell: the thread that computes the helicopter's cell writes EMPTY
// instead of FIRE and reports the hit, so there is no second pass over the grid and no barrier between CA and Modify.
// On a step without a CA pass one thread patches the byte in place.
// The parts meet like bulldozer_step_fused_parts_kernel: one 64-bit atomic per env carries the part's E | T | F counts
// (20 bits each), the hit bit and an arrival count in the top 3 bits; the last to arrive writes every per-env output
// and leaves the slot zero. Nothing waits for anything: a part adds its word and leaves.
//
// gca_helicopter_rollout: K of those steps with the caller's (K, E) actions (or the random policy) in ONE launch,
// helicopter_rollout_kernel: a workgroup per env keeps both grid planes in LDS (4-byte pitch, EMPTY padding) and the
// env's scalars in registers for the K steps, the CA pass in the strip's SWAR form on LDS dwords for any W; one barrier
// per step, no atomics, no `meet`. Grids whose planes do not fit in 64 KiB run K launches of the step kernel instead.
//
// gca_helicopter_policy_rollout: the same resident rollout with the agent inside (heli_rollout_body<true>): every step
// takes its action from a small policy network evaluated on that step's observation (gca_policy_dev.h), four more
// barriers per step; gca_helicopter_policy_act is that network alone, one workgroup per env, on a given observation.
#include "gca_common.h"
#include "gca_policy_dev.h"

namespace {

constexpr int HELI_SH = 16;       // rows per strip of the dword path
constexpr int HELI_THREADS = 256;

__device__ __forceinline__ uint32_t heli_shr1(uint32_t v) {  // lane l <- lane l-1, lane 0 <- 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t heli_shl1(uint32_t v) {  // lane l <- lane l+1, lane 63 <- 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true);
}

// ceil(thr * 2^53) clamped to [0, 2^53]: v < it  <=>  (double)v * 2^-53 < thr for every 53-bit v (NaN: never)
__device__ __forceinline__ uint64_t heli_int_threshold(double thr) {
    if (!(thr > 0.0)) return 0ull;
    if (thr >= 1.0) return 1ull << 53;
    return (uint64_t)ceil(thr * 0x1.0p53);
}

struct HeliRow {
    uint32_t x;  // the row's 4 cells of this lane
    uint32_t f;  // FIRE flags (0x01 per byte), 0 for a row outside the grid (padding = EMPTY)
    uint32_t h;  // f of (c-1) | c | (c+1) per byte
};

// raw loads of row R (clamped into the grid; a row outside is discarded by heli_classify): the lane's dword and, when
// the row continues beyond this 256-column chunk, the one byte to the left of lane 0 / right of lane 63
struct HeliRaw {
    uint32_t x, halo;
};
__device__ __forceinline__ HeliRaw heli_load(const uint8_t* __restrict__ S, int R, int H, int W, int col0, int lane,
                                             bool has_left, bool has_right) {
    const int Rc = min(max(R, 0), H - 1);
    const uint8_t* p = S + (uint32_t)Rc * (uint32_t)W + (uint32_t)col0;
    HeliRaw r;
    r.x = *reinterpret_cast<const uint32_t*>(p);
    r.halo = 0u;
    if (has_left && lane == 0) r.halo = p[-1];
    if (has_right && lane == 63) r.halo = p[4];
    return r;
}
__device__ __forceinline__ HeliRow heli_classify(const HeliRaw& raw, bool valid, uint32_t Fp, int lane, bool has_left,
                                                 bool has_right) {
    HeliRow o;
    o.x = raw.x;
    o.f = valid ? bytes_eq01(raw.x, Fp) : 0u;
    uint32_t prev = heli_shr1(o.f), next = heli_shl1(o.f);
    const uint32_t hf = (valid && raw.halo == (Fp & 0xFFu)) ? 1u : 0u;
    if (has_left && lane == 0) prev = hf << 24;
    if (has_right && lane == 63) next = hf;
    const uint32_t fl = __builtin_amdgcn_alignbyte(o.f, prev, 3);  // byte i = flag of column c-1
    const uint32_t fr = __builtin_amdgcn_alignbyte(next, o.f, 1);  // byte i = flag of column c+1
    o.h = o.f | fl | fr;
    return o;
}

struct HeliCtx {
    uint32_t Ep, Tp, Fp;       // replicated codes
    uint32_t k0, k1, env_id, step;
    uint64_t it_fire, it_tree;
    int prow, pcol;            // the helicopter's (moved) position
};

// one draw: Philox((cell, env, step, DSCE)) -> 53 bits < threshold (gca_ds_step's u01_f64(x.x, x.y) < thr)
__device__ __forceinline__ bool heli_draw(const HeliCtx& c, uint32_t cell, bool is_tree) {
    const u32x4 rx = philox4x32_10(u32x4{cell, c.env_id, c.step, GCA_TAG_DS_CELL}, c.k0, c.k1);
    const uint64_t v = (((uint64_t)rx.x << 32) | rx.y) >> 11;
    return v < (is_tree ? c.it_fire : c.it_tree);
}

// the codes, the key and the env id of a context; the caller adds the two thresholds and, per CA pass, step, prow, pcol
__device__ __forceinline__ HeliCtx heli_ctx(int empty, int tree, int fire, uint64_t seed, uint32_t env_id) {
    HeliCtx c;
    c.Ep = rep4((uint32_t)empty);
    c.Tp = rep4((uint32_t)tree);
    c.Fp = rep4((uint32_t)fire);
    c.k0 = (uint32_t)seed;
    c.k1 = (uint32_t)(seed >> 32);
    c.env_id = env_id;
    return c;
}

// column 0 of gca_random_actions
__device__ __forceinline__ int32_t heli_random_action(uint32_t env_id, uint32_t rs, uint64_t action_seed) {
    const u32x4 x = philox4x32_10(u32x4{0u, env_id, rs, GCA_TAG_ACTION}, (uint32_t)action_seed,
                                  (uint32_t)(action_seed >> 32));
    return randint_ms(x.x, 0, 9);
}

// helicopter.py:120-135: dot([0, 1, -1], counts / ncells) = cT / n - cF / n (0 * x and the first add are exact)
__device__ __forceinline__ double heli_reward(int32_t cT, int32_t cF, double n) {
    return __dsub_rn(__ddiv_rn((double)cT, n), __ddiv_rn((double)cF, n));
}

// The next state of the dword x at (row r, columns col0 .. col0 + 3) from its byte masks: fB FIRE, em EMPTY, ign TREE
// with a burning neighbour, dT the other TREE, win the winning draws. Modify is folded in: the helicopter's cell, if it
// would be FIRE, becomes EMPTY (hit). Cells of no known code keep their byte.
struct HeliNext {
    uint32_t out;        // the four new cell codes
    int32_t nE, nT, nF;  // how many of them are EMPTY / TREE / FIRE
    uint32_t hit;        // 1 when Modify put a fire out here
};
__device__ __forceinline__ HeliNext heli_next4(const HeliCtx& c, uint32_t x, uint32_t fB, uint32_t em, uint32_t ign,
                                               uint32_t dT, uint32_t win, int r, int col0) {
    uint32_t nF = ign | (dT & win);
    const uint32_t nT = (dT & ~win) | (em & win);
    uint32_t nE = (em & ~win) | fB;
    const uint32_t dc = (uint32_t)(c.pcol - col0);
    const uint32_t mk = (r == c.prow && dc < 4u) ? (1u << (8 * dc)) : 0u;
    const uint32_t hw = nF & mk;
    nF ^= hw;
    nE |= hw;
    const uint32_t known = nE | nT | nF;  // 0x01 where the cell holds one of the three codes
    HeliNext n;
    n.out = nE * (c.Ep & 0xFFu) + nT * (c.Tp & 0xFFu) + nF * (c.Fp & 0xFFu) + (x & ~(known * 0xFFu));
    n.nE = __popc(nE);
    n.nT = __popc(nT);
    n.nF = __popc(nF);
    n.hit = hw != 0u ? 1u : 0u;
    return n;
}

// rows [r0, min(r0 + HELI_SH, H)) x columns [256 ch, 256 ch + 256) of one env, by one wave
__device__ __forceinline__ void heli_strip(const uint8_t* __restrict__ S, uint8_t* __restrict__ D, int r0, int ch,
                                           int nch, int H, int W, int lane, const HeliCtx& c, int32_t& cE, int32_t& cT,
                                           int32_t& cF, int32_t& hit) {
    const int col0 = 256 * ch + 4 * lane;
    const bool hl = ch > 0, hr = ch < nch - 1;
    HeliRow A = heli_classify(heli_load(S, r0 - 1, H, W, col0, lane, hl, hr), r0 >= 1, c.Fp, lane, hl, hr);
    HeliRow B = heli_classify(heli_load(S, r0, H, W, col0, lane, hl, hr), true, c.Fp, lane, hl, hr);
    HeliRaw ahead = heli_load(S, r0 + 1, H, W, col0, lane, hl, hr);
    const int rows = min(HELI_SH, H - r0);
    for (int t = 0; t < rows; ++t) {
        const int R = r0 + t;
        const HeliRow C = heli_classify(ahead, R + 1 < H, c.Fp, lane, hl, hr);
        if (t + 1 < rows) ahead = heli_load(S, R + 2, H, W, col0, lane, hl, hr);
        const uint32_t nb = A.h | B.h | C.h;  // a burning Moore neighbour (the centre itself only matters for TREE)
        const uint32_t tr = bytes_eq01(B.x, c.Tp), em = bytes_eq01(B.x, c.Ep);
        const uint32_t ign = tr & nb;         // TREE -> FIRE, no draw
        const uint32_t dT = tr ^ ign;         // TREE that draws
        const uint32_t dr = dT | em;          // cells that draw
        uint32_t win = 0u;
        const uint32_t cell0 = (uint32_t)R * (uint32_t)W + (uint32_t)col0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool d = (dr >> (8 * j)) & 1u;
            if (__ballot(d) != 0ull) {  // wave-uniform: no Philox call for a wave whose cells draw nothing
                const bool w = heli_draw(c, cell0 + j, (dT >> (8 * j)) & 1u);
                win |= (d && w) ? (1u << (8 * j)) : 0u;
            }
        }
        const HeliNext n = heli_next4(c, B.x, B.f, em, ign, dT, win, R, col0);
        *reinterpret_cast<uint32_t*>(D + cell0) = n.out;
        cE += n.nE;
        cT += n.nT;
        cF += n.nF;
        hit += (int32_t)n.hit;
        A = B;
        B = C;
    }
}

// cells [begin, end) of one env, a cell per thread (any W)
__device__ __forceinline__ void heli_cells(const uint8_t* __restrict__ S, uint8_t* __restrict__ D, int begin, int end,
                                           int H, int W, int tid, const HeliCtx& c, int32_t& cE, int32_t& cT,
                                           int32_t& cF, int32_t& hit) {
    const int empty = (int)(c.Ep & 0xFFu), tree = (int)(c.Tp & 0xFFu), fire = (int)(c.Fp & 0xFFu);
    for (int cell = begin + tid; cell < end; cell += HELI_THREADS) {
        const int r = cell / W, col = cell - r * W;
        const int x = S[cell];
        int nx = x;
        if (x == fire) {
            nx = empty;
        } else if (x == tree || x == empty) {
            bool nbf = false;
            if (x == tree) {
#pragma unroll
                for (int dr = -1; dr <= 1; ++dr) {
#pragma unroll
                    for (int dc = -1; dc <= 1; ++dc) {
                        const int rr = r + dr, cc = col + dc;
                        if ((dr | dc) != 0 && rr >= 0 && rr < H && cc >= 0 && cc < W && S[rr * W + cc] == fire)
                            nbf = true;
                    }
                }
            }
            if (nbf) nx = fire;
            else if (heli_draw(c, (uint32_t)cell, x == tree)) nx = x == tree ? fire : tree;
        }
        if (r == c.prow && col == c.pcol && nx == fire) {  // Modify folded into the store
            nx = empty;
            hit += 1;
        }
        D[cell] = (uint8_t)nx;
        cE += nx == empty;
        cT += nx == tree;
        cF += nx == fire;
    }
}

struct HeliArgs {
    int empty, tree, fire, max_freeze;
    uint64_t seed, action_seed;
    int env_offset;
    const int32_t* action;
    int32_t* action_out;
    const double* thr;
    int32_t* freeze;
    uint32_t* rng_step;
    uint8_t* parity;
    uint8_t* buf0;
    uint8_t* buf1;
    int H, W;
    int32_t* pos;
    int32_t* counts;
    uint8_t* hit;
    double* reward;
    int64_t* steps_elapsed;
    unsigned long long* meet;
    int P;
    double* rec_reward;  // gca_helicopter_rollout's records of this step (nullable; action_out is the third)
    uint8_t* rec_hit;
};

// FAST: W % 256 == 0 and 4-byte aligned grids. Block = (env, part), 4 waves. Every wave of every block reaches the one
// barrier (it stands outside every condition), whatever its share of the rows.
template <bool FAST>
__global__ __launch_bounds__(HELI_THREADS) void helicopter_step_kernel(HeliArgs a) {
    __shared__ int32_t wave_cnt[HELI_THREADS / 64][4];
    const int P = a.P;
    const int e = blockIdx.x / P, part = blockIdx.x - e * P;
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W;
    // ---- every per-env input, read before anything of this env is written by anyone (the last part to arrive at
    //      `meet` writes, and it arrives after every part's reads: each part's word depends on them)
    const uint32_t rs = a.rng_step[e];
    const uint32_t env_id = (uint32_t)(a.env_offset + e);
    int32_t act;
    if (a.action) act = a.action[e];
    else act = heli_random_action(env_id, rs, a.action_seed);
    const int32_t fz = a.freeze[e];
    const bool odd = a.parity[e] != 0;
    const int32_t prow0 = a.pos[2 * e], pcol0 = a.pos[2 * e + 1];
    const int32_t c0 = a.counts[3 * e + 0], c1 = a.counts[3 * e + 1], c2 = a.counts[3 * e + 2];
    const int64_t se = a.steps_elapsed[e];
    const double thr_fire = a.thr[2 * e], thr_tree = a.thr[2 * e + 1];
    // ---- Move (helicopter.py:56-62 action sets): up {0,1,2}, down {6,7,8}, left {0,3,6}, right {2,5,8}
    const int a0 = clampi_dev(act, 0, 8);
    int row = prow0, col = pcol0;
    move_pos(a0, row, col, H, W, 0x007, 0x1C0, 0x049, 0x124);
    const bool do_ca = fz == 0;
    const int64_t HW = (int64_t)H * W;
    uint8_t* cur = (odd ? a.buf1 : a.buf0) + e * HW;
    uint8_t* nxt = (odd ? a.buf0 : a.buf1) + e * HW;
    int32_t cE = 0, cT = 0, cF = 0, hitc = 0;
    if (do_ca) {
        HeliCtx c = heli_ctx(a.empty, a.tree, a.fire, a.seed, env_id);
        c.step = rs;
        c.it_fire = heli_int_threshold(thr_fire);
        c.it_tree = heli_int_threshold(thr_tree);
        c.prow = row;
        c.pcol = col;
        if constexpr (FAST) {
            const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
            const int nch = W >> 8;
            const int strips = (H + HELI_SH - 1) / HELI_SH, spp = (strips + P - 1) / P;
            const int s_begin = part * spp, s_end = min(strips, s_begin + spp);
            const int items = max(s_end - s_begin, 0) * nch;
            for (int i = wave; i < items; i += HELI_THREADS / 64) {
                const int s = s_begin + i / nch, ch = i - (i / nch) * nch;
                heli_strip(cur, nxt, s * HELI_SH, ch, nch, H, W, lane, c, cE, cT, cF, hitc);
            }
        } else {
            const int rpp = (H + P - 1) / P;
            const int r_begin = min(part * rpp, H), r_end = min(H, r_begin + rpp);
            heli_cells(cur, nxt, r_begin * W, r_end * W, H, W, tid, c, cE, cT, cF, hitc);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cE += __shfl_xor(cE, off);
            cT += __shfl_xor(cT, off);
            cF += __shfl_xor(cF, off);
            hitc += __shfl_xor(hitc, off);
        }
    }
    if ((tid & 63) == 0) {
        wave_cnt[tid >> 6][0] = cE;
        wave_cnt[tid >> 6][1] = cT;
        wave_cnt[tid >> 6][2] = cF;
        wave_cnt[tid >> 6][3] = hitc;
    }
    __syncthreads();
    if (tid != 0) return;
    int32_t pE = 0, pT = 0, pF = 0;
    uint32_t h = 0;
#pragma unroll
    for (int w = 0; w < HELI_THREADS / 64; ++w) {
        pE += wave_cnt[w][0];
        pT += wave_cnt[w][1];
        pF += wave_cnt[w][2];
        h |= wave_cnt[w][3] != 0;
    }
    if (!do_ca && part == 0 && row >= 0 && row < H && col >= 0 && col < W) {
        // no CA pass: Modify patches the one byte in place (a caller's own position outside the grid writes nothing)
        uint8_t* g = cur + (int64_t)row * W + col;
        if (*g == (uint8_t)a.fire) {
            *g = (uint8_t)a.empty;
            h = 1;
        }
    }
    unsigned long long tot = (unsigned long long)(uint32_t)pE | ((unsigned long long)(uint32_t)pT << 20) |
                             ((unsigned long long)(uint32_t)pF << 40) | ((unsigned long long)h << 60);
    if (a.meet) {
        const unsigned long long pk = tot | (1ull << 61);
        const unsigned long long old = atomicAdd(&a.meet[e], pk);
        if ((int)(old >> 61) != P - 1) return;  // not the last part to arrive
        tot = old + pk;
        a.meet[e] = 0ull;
    }
    int32_t nE, nT, nF;
    const uint8_t hh = (uint8_t)((tot >> 60) & 1u);
    if (do_ca) {
        nE = (int32_t)(tot & 0xFFFFFu);
        nT = (int32_t)((tot >> 20) & 0xFFFFFu);
        nF = (int32_t)((tot >> 40) & 0xFFFFFu);
        a.parity[e] = odd ? 0 : 1;
    } else {
        nE = c0 + hh;
        nT = c1;
        nF = c2 - hh;
    }
    if (a.action_out) a.action_out[e] = act;
    a.pos[2 * e] = row;
    a.pos[2 * e + 1] = col;
    a.freeze[e] = do_ca ? a.max_freeze : fz - 1;
    a.counts[3 * e + 0] = nE;
    a.counts[3 * e + 1] = nT;
    a.counts[3 * e + 2] = nF;
    a.hit[e] = hh;
    const double rw = heli_reward(nT, nF, (double)HW);
    a.reward[e] = rw;
    if (a.rec_reward) a.rec_reward[e] = rw;
    if (a.rec_hit) a.rec_hit[e] = hh;
    a.rng_step[e] = rs + 1u;
    a.steps_elapsed[e] = se + 1;
}

// ---------------------------------------------------------------- K env steps in one launch, the grid resident in LDS
struct HeliRollArgs {
    int empty, tree, fire, max_freeze;
    uint64_t seed, action_seed;
    int env_offset, K, E;
    const int32_t* actions;  // (K, E) or null
    int32_t* action_out;     // (K, E) records, each nullable
    double* reward_out;
    uint8_t* hit_out;
    const double* thr;
    int32_t* freeze;
    uint32_t* rng_step;
    uint8_t* parity;
    uint8_t* buf0;
    uint8_t* buf1;
    int H, W;
    int D;            // dwords per row, ceil(W / 4)
    int plane_words;  // dwords per LDS plane, a multiple of 4
    int dwords;       // W % 4 == 0 and 4-byte aligned grids: dword loads / stores of the planes, else bytes
    int32_t* pos;
    int32_t* counts;
    uint8_t* hit;
    double* reward;
    int64_t* steps_elapsed;
};

// the cells of row r, dword d (columns 4d .. 4d+3) of an env's grid in global memory; columns >= W read as EMPTY
__device__ __forceinline__ uint32_t heli_g2r(const uint8_t* __restrict__ g, int r, int d, int W, bool dwords,
                                             uint32_t Ep) {
    const uint32_t cell0 = (uint32_t)r * (uint32_t)W + 4u * (uint32_t)d;
    if (dwords) return *reinterpret_cast<const uint32_t*>(g + cell0);
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) v |= (4 * d + j < W ? (uint32_t)g[cell0 + j] : (Ep & 0xFFu)) << (8 * j);
    return v;
}
__device__ __forceinline__ void heli_r2g(uint8_t* __restrict__ g, int r, int d, int W, bool dwords, uint32_t v) {
    const uint32_t cell0 = (uint32_t)r * (uint32_t)W + 4u * (uint32_t)d;
    if (dwords) {
        *reinterpret_cast<uint32_t*>(g + cell0) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * d + j < W) g[cell0 + j] = (uint8_t)(v >> (8 * j));
}

// ---- the policy of gca_helicopter_policy_rollout: the network and the (K, E, ...) records only that rollout has
struct HeliPolArgs {
    PolicyW w;
    int radius, lgB, Hc, Wc;
    float inv;  // 1 / block^2
    float* logits_out;
    float* value_out;
    uint8_t* local_out;
    float* coarse_out;
};

// Step k's action of env e in the resident rollout: gca_policy_observation's window and coarse map taken from the
// current LDS plane at the position BEFORE the move, then the network (policy_outputs, three barriers). The window's
// classes are read where they are needed and never staged; the coarse map goes to LDS (it is shared by all hidden
// units). Rows -1 / H, the dword after a row and the columns >= W hold EMPTY, which is neither TREE nor FIRE, but the
// loops below stay inside the grid's own rows and dwords anyway. Every thread returns the same action.
__device__ __forceinline__ int32_t heli_rollout_policy_act(const HeliRollArgs& a, const HeliPolArgs& q,
                                                           uint32_t* heli_lds, int p, int k, int e, int tid, int row,
                                                           int col, uint32_t env_id, uint32_t rs, uint32_t Tp,
                                                           uint32_t Fp) {
    const int H = a.H, W = a.W, D = a.D, PD = D + 1, NP = a.plane_words;
    const uint32_t* S = heli_lds + p * NP;
    const uint8_t* Sb = reinterpret_cast<const uint8_t*>(S);
    float* cs = reinterpret_cast<float*>(heli_lds + 2 * NP + 16);
    float* part = cs + ((q.w.C + 3) & ~3);
    float* hs = part + POL_PART;
    float* outs = hs + POL_VT;
    const size_t rec = (size_t)k * (size_t)a.E + (size_t)e;
    const uint32_t tree = Tp & 0xFFu, fire = Fp & 0xFFu;
    const int B = 1 << q.lgB, tiles = q.Hc * q.Wc;
    for (int t = tid; t < tiles; t += HELI_THREADS) {
        const int bi = t / q.Wc, bj = t - bi * q.Wc;
        const int r0 = bi << q.lgB, r1 = min(H, r0 + B), c0 = bj << q.lgB;
        int32_t cT = 0, cF = 0;
        if (q.lgB >= 2) {  // a tile's columns are whole dwords of the plane
            const int d0 = c0 >> 2, d1 = min(D, (c0 + B) >> 2);
            for (int r = r0; r < r1; ++r)
                for (int d = d0; d < d1; ++d) {
                    const uint32_t x = S[1 + (r + 1) * PD + d];
                    cT += __popc(bytes_eq01(x, Tp));
                    cF += __popc(bytes_eq01(x, Fp));
                }
        } else {
            const int c1 = min(W, c0 + B);
            for (int r = r0; r < r1; ++r)
                for (int cc = c0; cc < c1; ++cc) {
                    const uint32_t v = Sb[4 * (1 + (r + 1) * PD) + cc];
                    cT += v == tree;
                    cF += v == fire;
                }
        }
        const float fT = (float)cT * q.inv, fF = (float)cF * q.inv;
        cs[t] = fT;
        cs[tiles + t] = fF;
        if (q.coarse_out) {
            float* o = q.coarse_out + rec * (size_t)(2 * tiles);
            o[t] = fT;
            o[tiles + t] = fF;
        }
    }
    const uint32_t wr0 = (uint32_t)row - (uint32_t)q.radius, wc0 = (uint32_t)col - (uint32_t)q.radius;
    auto class_at = [&](int, int wi, int wj) -> uint32_t {
        const uint32_t r = wr0 + (uint32_t)wi, cc = wc0 + (uint32_t)wj;
        const bool in = r < (uint32_t)H && cc < (uint32_t)W;
        const uint32_t v = Sb[in ? 4u * (1u + (r + 1u) * (uint32_t)PD) + cc : 0u];
        return !in ? 3u : (v == tree ? 1u : (v == fire ? 2u : 0u));
    };
    if (q.local_out) {
        uint8_t* o = q.local_out + rec * (size_t)q.w.SS;
        for (int n = tid; n < q.w.SS; n += HELI_THREADS) {
            const int wi = n / q.w.S;
            o[n] = (uint8_t)class_at(n, wi, n - wi * q.w.S);
        }
    }
    float o[HELI_POL_NOUT];
    policy_outputs<HELI_POL_NOUT, POL_VT>(q.w, cs, part, hs, outs, tid, POL_VT,
                                          q.logits_out ? q.logits_out + rec * 9 : nullptr,
                                          q.value_out ? q.value_out + rec : nullptr, class_at, [] {}, o);
    // lane i < 9 also holds l_i on its own
    return __builtin_amdgcn_readfirstlane(heli_policy_sample(o, outs[min(tid & 63, 8)], q.w, env_id, rs));
}

// One workgroup (4 waves) per env, K steps. LDS: two planes of PD = D + 1 dwords per row, rows -1 .. H, one leading
// dword; cell (r, c) is byte c of dword 1 + (r + 1) * PD of its plane, and the dword after a row's D, rows -1 and H
// and the columns >= W of a row's last dword hold EMPTY for the whole launch (never FIRE, never stored to), so every
// neighbour outside the grid reads as not-FIRE with no bounds test. LDS plane p mirrors buf[p] of the env.
// Every thread carries the env's scalars. freeze, position, rng_step and the plane index follow from uniform loads and
// the actions alone, so they are the same in all 256 threads in every step; that makes `do_ca` uniform. The counts and
// the hit are exact in wave 0, which writes the records and the exit state: after a CA pass every thread reads the
// waves' words back, on a countdown step only thread 0 knows the hit and wave 0 takes it by readfirstlane.
// The K loop, the item loop inside a CA pass and the one barrier per step have the same trip count in every thread
// (K, `iters`, K): the barrier stands outside every condition, no thread leaves early, nothing waits for another
// workgroup.
template <bool POLICY>
__device__ __forceinline__ void heli_rollout_body(const HeliRollArgs a, const HeliPolArgs* pa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t heli_lds[];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H, W = a.W, D = a.D, PD = D + 1, NP = a.plane_words, K = a.K;
    const int64_t HW = (int64_t)H * W;
    const bool dwords = a.dwords != 0;
    uint32_t* const wave_cnt = heli_lds + 2 * NP;  // [step & 1][wave][2]
    uint32_t rs = a.rng_step[e];
    const uint32_t env_id = (uint32_t)(a.env_offset + e);
    int32_t fz = a.freeze[e];
    int p = a.parity[e] != 0;
    int row = a.pos[2 * e], col = a.pos[2 * e + 1];
    int32_t c0 = a.counts[3 * e + 0], c1 = a.counts[3 * e + 1], c2 = a.counts[3 * e + 2];
    HeliCtx c = heli_ctx(a.empty, a.tree, a.fire, a.seed, env_id);
    c.it_fire = heli_int_threshold(a.thr[2 * e]);
    c.it_tree = heli_int_threshold(a.thr[2 * e + 1]);
    const uint32_t fire = (uint32_t)a.fire;
    // ---- entry: the current plane from buf[p][e], everything else of both planes EMPTY
    {
        const uint8_t* g = (p ? a.buf1 : a.buf0) + e * HW;
        uint32_t* cur = heli_lds + p * NP;
        uint32_t* oth = heli_lds + (p ^ 1) * NP;
        for (int idx = tid; idx < NP; idx += HELI_THREADS) {
            const int t = idx - 1, rr = t / PD, d = t - rr * PD, r = rr - 1;
            uint32_t v = c.Ep;
            if (idx >= 1 && r >= 0 && r < H && d < D) v = heli_g2r(g, r, d, W, dwords, c.Ep);
            cur[idx] = v;
            oth[idx] = c.Ep;
        }
    }
    __syncthreads();
    // a thread's items of a CA pass: (row, dword) number tid + 256 * it, it < iters, walked without a division
    const int iters = (H * D + HELI_THREADS - 1) / HELI_THREADS;
    const int r_first = tid / D, d_first = tid - r_first * D;
    const int r_step = HELI_THREADS / D, d_step = HELI_THREADS - r_step * D;
    const uint32_t tail = 0x01010101u >> (8 * (4 * D - W));  // the last dword's columns < W
    int nca = 0;
    uint32_t hh = 0u;
    int32_t chunk = 0, rec_t = 0, rec_f = 0;
    uint32_t rec_h = 0u;
    for (int k = 0; k < K; ++k) {
        int32_t act;
        if constexpr (POLICY) {
            act = heli_rollout_policy_act(a, *pa, heli_lds, p, k, e, tid, row, col, env_id, rs, c.Tp, c.Fp);
        } else if (a.actions) {  // 64 steps' actions per load: lane l holds step (k & ~63) + l
            if ((k & 63) == 0) chunk = k + lane < K ? a.actions[(size_t)(k + lane) * a.E + e] : 0;
            act = __builtin_amdgcn_readlane(chunk, k & 63);
        } else {
            act = heli_random_action(env_id, rs, a.action_seed);
        }
        move_pos(clampi_dev(act, 0, 8), row, col, H, W, 0x007, 0x1C0, 0x049, 0x124);
        const bool do_ca = fz == 0;
        uint32_t* S = heli_lds + p * NP;
        uint32_t w0 = 0u, w1 = 0u;  // cE | cT << 16, cF | hit << 16 (the plane fits LDS: H * W < 2^15)
        uint32_t patched = 0u;
        if (do_ca) {
            uint32_t* Dst = heli_lds + (p ^ 1) * NP;
            const uint8_t* Sb = reinterpret_cast<const uint8_t*>(S);
            c.step = rs;
            c.prow = row;
            c.pcol = col;
            int r = r_first, d = d_first;
            for (int it = 0; it < iters; ++it) {
                const bool active = r < H;
                const int idx = 1 + (r + 1) * PD + d;
                uint32_t x = 0u, fB = 0u, em = 0u, ign = 0u, dT = 0u;
                if (active) {
                    x = S[idx];
                    const int bl = 4 * idx - 1, br = 4 * idx + 4, pb = 4 * PD;
                    const uint32_t lf = (Sb[bl - pb] == fire) | (Sb[bl] == fire) | (Sb[bl + pb] == fire);
                    const uint32_t rf = (Sb[br - pb] == fire) | (Sb[br] == fire) | (Sb[br + pb] == fire);
                    const uint32_t fx = bytes_eq01(x, c.Fp);
                    const uint32_t V = bytes_eq01(S[idx - PD], c.Fp) | fx | bytes_eq01(S[idx + PD], c.Fp);
                    const uint32_t nb = V | (V << 8) | lf | (V >> 8) | (rf << 24);  // a burning Moore neighbour
                    const uint32_t vm = d == D - 1 ? tail : 0x01010101u;
                    const uint32_t tr = bytes_eq01(x, c.Tp) & vm;
                    em = bytes_eq01(x, c.Ep) & vm;
                    fB = fx & vm;
                    ign = tr & nb;   // TREE -> FIRE, no draw
                    dT = tr ^ ign;   // TREE that draws
                }
                const uint32_t dr = dT | em;
                const uint32_t cell0 = (uint32_t)r * (uint32_t)W + 4u * (uint32_t)d;
                uint32_t win = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool dj = (dr >> (8 * j)) & 1u;
                    if (__ballot(dj) != 0ull) {  // wave-uniform: no Philox call for a wave whose cells draw nothing
                        const bool w = heli_draw(c, cell0 + j, (dT >> (8 * j)) & 1u);
                        win |= (dj && w) ? (1u << (8 * j)) : 0u;
                    }
                }
                if (active) {
                    const HeliNext n = heli_next4(c, x, fB, em, ign, dT, win, r, 4 * d);
                    Dst[idx] = n.out;
                    w0 += (uint32_t)n.nE + ((uint32_t)n.nT << 16);
                    w1 += (uint32_t)n.nF + (n.hit << 16);
                }
                d += d_step;
                r += r_step;
                if (d >= D) {
                    d -= D;
                    r += 1;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                w0 += __shfl_xor(w0, off);
                w1 += __shfl_xor(w1, off);
            }
            if (lane == 0) {  // double-buffered by step parity (below)
                uint32_t* wc = wave_cnt + (k & 1) * 8;
                wc[2 * wave] = w0;
                wc[2 * wave + 1] = w1;
            }
            p ^= 1;
            nca += 1;
        } else if (tid == 0 && row >= 0 && row < H && col >= 0 && col < W) {
            // no CA pass: Modify patches the one LDS byte in place
            uint8_t* b = reinterpret_cast<uint8_t*>(S) + 4 * (1 + (row + 1) * PD) + col;
            if (*b == (uint8_t)a.fire) {
                *b = (uint8_t)a.empty;
                patched = 1u;
            }
        }
        // The step's only barrier, outside every condition. It orders (1) the pass's stores / the byte patch before the
        // next step's reads of that plane, (2) this step's reads of plane p before the next pass's stores into it,
        // (3) after a pass, the waves' words before everyone's read of them. The words are double-buffered by step
        // parity: slot k & 1 is written again in step k + 2 at the earliest, which a wave reaches only through step
        // k + 1's barrier, i.e. after every wave's read here.
        __syncthreads();
        if (do_ca) {
            const uint32_t* wc = wave_cnt + (k & 1) * 8;
            const uint32_t t0 = wc[0] + wc[2] + wc[4] + wc[6], t1 = wc[1] + wc[3] + wc[5] + wc[7];
            hh = (t1 >> 16) != 0u ? 1u : 0u;
            c0 = (int32_t)(t0 & 0xFFFFu);
            c1 = (int32_t)(t0 >> 16);
            c2 = (int32_t)(t1 & 0xFFFFu);
            fz = a.max_freeze;
        } else {
            // a countdown step's hit is thread 0's alone and only wave 0 uses it (records, exit): nothing is published.
            // Waves 1-3 read 0 here, so their c0 / c2 / hh are right only from a CA step until the next hit; they are
            // never used.
            hh = (uint32_t)__builtin_amdgcn_readfirstlane((int)patched);
            c0 += (int32_t)hh;
            c2 -= (int32_t)hh;
            fz -= 1;
        }
        rs += 1u;
        // records: lane k & 63 keeps step k's action, TREE and FIRE counts and hit; wave 0 writes the 64 rows of a
        // chunk at its end, a lane per row, so the two f64 divisions of a reward are done 64 at a time instead of by
        // one lane in every step (no barrier inside: the other waves just pass)
        if (lane == (k & 63)) {
            chunk = act;
            rec_t = c1;
            rec_f = c2;
            rec_h = hh;
        }
        if (((k & 63) == 63 || k == K - 1) && wave == 0 && lane <= (k & 63)) {
            const size_t o = (size_t)((k & ~63) + lane) * a.E + e;
            if (a.action_out) a.action_out[o] = chunk;
            if (a.hit_out) a.hit_out[o] = (uint8_t)rec_h;
            if (a.reward_out) a.reward_out[o] = heli_reward(rec_t, rec_f, (double)HW);
        }
    }
    // ---- exit (the last step's barrier stands between every LDS store and these reads): the current plane, and after
    //      at least one CA pass the other one too -- the grid before the last pass with the patches made on it, which
    //      is what K step calls leave in buf[parity ^ 1]
    for (int q = 0; q < 2; ++q) {
        if (q == 1 && nca == 0) break;
        const int pl = p ^ q;
        uint8_t* g = (pl ? a.buf1 : a.buf0) + e * HW;
        const uint32_t* L = heli_lds + pl * NP;
        int r = r_first, d = d_first;
        for (int it = 0; it < iters; ++it) {
            if (r < H) heli_r2g(g, r, d, W, dwords, L[1 + (r + 1) * PD + d]);
            d += d_step;
            r += r_step;
            if (d >= D) {
                d -= D;
                r += 1;
            }
        }
    }
    if (tid != 0) return;
    a.parity[e] = (uint8_t)p;
    a.freeze[e] = fz;
    a.pos[2 * e] = row;
    a.pos[2 * e + 1] = col;
    a.counts[3 * e + 0] = c0;
    a.counts[3 * e + 1] = c1;
    a.counts[3 * e + 2] = c2;
    a.hit[e] = (uint8_t)hh;
    a.reward[e] = heli_reward(c1, c2, (double)HW);
    a.rng_step[e] = rs;
    a.steps_elapsed[e] += K;
}

// gca_helicopter_rollout's kernel: the caller's actions or the random policy
__global__ __launch_bounds__(HELI_THREADS) void helicopter_rollout_kernel(HeliRollArgs a) {
    heli_rollout_body<false>(a, nullptr);
}
// gca_helicopter_policy_rollout's: the same steps, the action of each from the policy network (a.actions is not read).
// LDS after the planes and the waves' words: policy_lds_words(C) words of the network.
__global__ __launch_bounds__(HELI_THREADS) void helicopter_policy_rollout_kernel(HeliRollArgs a, HeliPolArgs pa) {
    heli_rollout_body<true>(a, &pa);
}

// gca_helicopter_policy_act: one workgroup per env on the observation the caller hands over. A class above 3 (never
// written by gca_policy_observation) is taken modulo 4, so no weight row outside w_local is ever read.
__global__ __launch_bounds__(POL_VT) void helicopter_policy_act_kernel(
    PolicyW w, const uint8_t* __restrict__ local, const float* __restrict__ coarse,
    const uint32_t* __restrict__ rng_step, int env_offset, int32_t* __restrict__ action, float* __restrict__ logits,
    float* __restrict__ value) {
    extern __shared__ __attribute__((aligned(16))) uint32_t heli_lds[];
    const int e = blockIdx.x, tid = threadIdx.x;
    float* cs = reinterpret_cast<float*>(heli_lds);
    float* part = cs + ((w.C + 3) & ~3);
    float* hs = part + POL_PART;
    float* outs = hs + POL_VT;
    for (int c = tid; c < w.C; c += POL_VT) cs[c] = coarse[(size_t)e * (size_t)w.C + c];
    const uint8_t* __restrict__ loc = local + (size_t)e * (size_t)w.SS;
    float o[HELI_POL_NOUT];
    policy_outputs<HELI_POL_NOUT, POL_VT>(
        w, cs, part, hs, outs, tid, POL_VT, logits ? logits + (size_t)e * 9 : nullptr, value ? value + e : nullptr,
        [&](int n, int, int) -> uint32_t { return (uint32_t)loc[n] & 3u; }, [] {}, o);
    // lane i < 9 also holds l_i on its own
    const int32_t act = heli_policy_sample(o, outs[min(tid & 63, 8)], w, (uint32_t)(env_offset + e), rng_step[e]);
    if (tid == 0) action[e] = act;
}

// ---------------------------------------------------------------- host side
// The entry points that step the envs put their arguments into a HeliArgs `a` first (one workgroup per env, no `meet`);
// this hands its fields to their shared argument checks, `who` heading the message.
int heli_check_env(const char* who, const HeliArgs& a, int E) {
    return gca_check_heli_env(who, a.empty, a.tree, a.fire, a.max_freeze, a.thr, a.freeze, a.rng_step, a.parity, a.buf0,
                              a.buf1, a.H, a.W, a.pos, a.counts, a.hit, a.reward, a.steps_elapsed, E);
}

bool heli_aligned(const HeliArgs& a) { return (((uintptr_t)a.buf0 | (uintptr_t)a.buf1) & 3u) == 0; }
// whether the step kernel can run in its FAST form
bool heli_fast(const HeliArgs& a) { return a.W % 256 == 0 && heli_aligned(a); }

void launch_heli_step(bool fast, dim3 grid, void* stream, const HeliArgs& a) {
    const dim3 block(HELI_THREADS);
    if (fast) hipLaunchKernelGGL(helicopter_step_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(helicopter_step_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
}

// The resident rollout's arguments (the fields the two structs share from `s`) and its LDS bytes: two planes and the
// waves' words. False when those exceed the 64 KiB a launch gets by default.
bool heli_roll_args(const HeliArgs& s, int K, int E, const int32_t* actions, int32_t* action_out, double* reward_out,
                    uint8_t* hit_out, HeliRollArgs* a, size_t* lds_bytes) {
    const int64_t d = ((int64_t)s.W + 3) / 4;
    const int64_t words = (1 + ((int64_t)s.H + 2) * (d + 1) + 3) & ~(int64_t)3;
    const int64_t bytes = 2 * words * 4 + 16 * 4;
    if (bytes > 65536) return false;
    a->empty = s.empty; a->tree = s.tree; a->fire = s.fire; a->max_freeze = s.max_freeze;
    a->seed = s.seed; a->action_seed = s.action_seed; a->env_offset = s.env_offset; a->K = K; a->E = E;
    a->actions = actions; a->action_out = action_out; a->reward_out = reward_out; a->hit_out = hit_out;
    a->thr = s.thr; a->freeze = s.freeze; a->rng_step = s.rng_step; a->parity = s.parity;
    a->buf0 = s.buf0; a->buf1 = s.buf1; a->H = s.H; a->W = s.W; a->D = (int)d; a->plane_words = (int)words;
    a->dwords = (s.W % 4 == 0 && heli_aligned(s)) ? 1 : 0;
    a->pos = s.pos; a->counts = s.counts; a->hit = s.hit; a->reward = s.reward; a->steps_elapsed = s.steps_elapsed;
    *lds_bytes = (size_t)bytes;
    return true;
}

}  // namespace

extern "C" int gca_helicopter_step(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                                   const int32_t* action, uint64_t action_seed, int32_t* action_out,
                                   const double* thresholds, int32_t* freeze, uint32_t* rng_step, uint8_t* parity,
                                   uint8_t* buf0, uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts,
                                   uint8_t* hit, double* reward, int64_t* steps_elapsed, uint64_t* meet, int E,
                                   void* stream) {
    HeliArgs a{empty,  tree,     fire,   max_freeze, seed, action_seed, env_offset, action, action_out, thresholds,
               freeze, rng_step, parity, buf0,       buf1, H,           W,          pos,    counts,     hit,
               reward, steps_elapsed, nullptr, 1, nullptr, nullptr};
    if (const int st = heli_check_env("helicopter_step", a, E)) return st;
    const int64_t HW = (int64_t)H * W;
    const bool fast = heli_fast(a);
    // the parts' word packs 20-bit counts: larger grids (and every grid without `meet`) run one workgroup per env;
    // parts only while the launch is small (E * P < 1024 workgroups) and every part keeps at least two strips / rows
    const int units = fast ? (H + HELI_SH - 1) / HELI_SH : H;
    int P = 1;
    if (meet && HW + 1 < (1 << 20))
        while (P < 8 && (int64_t)E * P < 1024 && 2 * P <= units) P *= 2;
    // the launch's 32-bit workgroup count: the host build launches nothing
    GCA_CHECK_ARG((int64_t)E * P < (1ll << 31), "helicopter_step: too many workgroups");
    a.meet = P > 1 ? (unsigned long long*)meet : nullptr;
    a.P = P;
    launch_heli_step(fast, dim3((unsigned)((int64_t)E * P)), stream, a);
    GCA_CHECK_LAUNCH("helicopter_step");
    return GCA_OK;
}

extern "C" int gca_helicopter_rollout(int empty, int tree, int fire, int max_freeze, uint64_t seed, int env_offset,
                                      const int32_t* actions, uint64_t action_seed, int K, int32_t* action_out,
                                      double* reward_out, uint8_t* hit_out, const double* thresholds, int32_t* freeze,
                                      uint32_t* rng_step, uint8_t* parity, uint8_t* buf0, uint8_t* buf1, int H, int W,
                                      int32_t* pos, int32_t* counts, uint8_t* hit, double* reward,
                                      int64_t* steps_elapsed, int E, void* stream) {
    HeliArgs a{empty,  tree,     fire,   max_freeze, seed, action_seed, env_offset, nullptr, nullptr, thresholds,
               freeze, rng_step, parity, buf0,       buf1, H,           W,          pos,     counts,  hit,
               reward, steps_elapsed, nullptr, 1, nullptr, nullptr};
    if (const int st = heli_check_env("helicopter_rollout", a, E)) return st;
    if (const int st = gca_check_k("helicopter_rollout", K)) return st;
    if (K == 0) return GCA_OK;
    const dim3 grid((unsigned)E);
    HeliRollArgs ra;
    size_t lds_bytes = 0;
    if (heli_roll_args(a, K, E, actions, action_out, reward_out, hit_out, &ra, &lds_bytes)) {
        hipLaunchKernelGGL(helicopter_rollout_kernel, grid, dim3(HELI_THREADS), lds_bytes, (hipStream_t)stream, ra);
        GCA_CHECK_LAUNCH("helicopter_rollout");
        return GCA_OK;
    }
    // the planes do not fit in LDS: K launches of the step kernel, one workgroup per env, each writing its record row
    const bool fast = heli_fast(a);
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * (size_t)E;
        a.action = actions ? actions + o : nullptr;
        a.action_out = action_out ? action_out + o : nullptr;
        a.rec_reward = reward_out ? reward_out + o : nullptr;
        a.rec_hit = hit_out ? hit_out + o : nullptr;
        launch_heli_step(fast, grid, stream, a);
        GCA_CHECK_LAUNCH("helicopter_rollout");
    }
    return GCA_OK;
}

// ---------------------------------------------------------------- the helicopter policy (gca.h "helicopter policy")
// The network, its LDS words and the device's view of the weights are gca_policy_dev.h's.
extern "C" int gca_helicopter_policy_act(const gca_heli_policy* p, int C, const uint8_t* local, const float* coarse,
                                         const uint32_t* rng_step, int env_offset, uint64_t policy_seed, int greedy,
                                         int32_t* action, float* logits, float* value, int E, void* stream) {
    if (const int st = gca_check_policy_act(p, C, local, coarse, rng_step, action, E)) return st;
    PolicyW w;
    if (const int st = policy_view(nullptr, p, C, policy_seed, greedy, &w)) return st;
    hipLaunchKernelGGL(helicopter_policy_act_kernel, dim3((unsigned)E), dim3(POL_VT),
                       (size_t)policy_lds_words(C) * 4, (hipStream_t)stream, w, local, coarse, rng_step,
                       env_offset, action, logits, value);
    GCA_CHECK_LAUNCH("helicopter_policy_act");
    return GCA_OK;
}

extern "C" int gca_helicopter_policy_rollout(int empty, int tree, int fire, int max_freeze, uint64_t seed,
                                             int env_offset, const gca_heli_policy* p, uint64_t policy_seed, int greedy,
                                             int K, int32_t* action_out, float* logits_out, float* value_out,
                                             double* reward_out, uint8_t* hit_out, uint8_t* local_out,
                                             float* coarse_out, void* scratch, const double* thresholds,
                                             int32_t* freeze, uint32_t* rng_step, uint8_t* parity, uint8_t* buf0,
                                             uint8_t* buf1, int H, int W, int32_t* pos, int32_t* counts, uint8_t* hit,
                                             double* reward, int64_t* steps_elapsed, int E, void* stream) {
    HeliArgs a{empty,  tree,     fire,   max_freeze, seed, 0, env_offset, nullptr, nullptr, thresholds,
               freeze, rng_step, parity, buf0,       buf1, H, W,          pos,     counts,  hit,
               reward, steps_elapsed, nullptr, 1, nullptr, nullptr};
    if (const int st = gca_check_policy_rollout(empty, tree, fire, max_freeze, p, K, thresholds, freeze, rng_step, parity,
                                                buf0, buf1, H, W, pos, counts, hit, reward, steps_elapsed, E))
        return st;
    const int Hc = (H + p->block - 1) / p->block, Wc = (W + p->block - 1) / p->block, C = 2 * Hc * Wc;
    HeliPolArgs q;
    if (const int st = policy_view(nullptr, p, C, policy_seed, greedy, &q.w)) return st;
    if (K == 0) return GCA_OK;
    const dim3 grid((unsigned)E);
    HeliRollArgs ra;
    size_t lds_bytes = 0;
    if (heli_roll_args(a, K, E, nullptr, action_out, reward_out, hit_out, &ra, &lds_bytes) &&
        lds_bytes + (size_t)policy_lds_words(C) * 4 <= 65536) {
        q.radius = p->radius;
        q.lgB = 0;
        while ((1 << q.lgB) < p->block) ++q.lgB;
        q.Hc = Hc; q.Wc = Wc;
        q.inv = 1.0f / (float)(p->block * p->block);
        q.logits_out = logits_out; q.value_out = value_out; q.local_out = local_out; q.coarse_out = coarse_out;
        hipLaunchKernelGGL(helicopter_policy_rollout_kernel, grid, dim3(HELI_THREADS),
                           lds_bytes + (size_t)policy_lds_words(C) * 4, (hipStream_t)stream, ra, q);
        GCA_CHECK_LAUNCH("helicopter_policy_rollout");
        return GCA_OK;
    }
    // The planes and the network's words do not fit in LDS: K x (observation, act, step) launches. A step's action, window
    // and coarse map go to their record rows, or to `scratch` where the caller keeps no such record.
    const size_t SS = (size_t)q.w.SS;
    // only the device build has this path: the host build keeps its own buffers
    GCA_CHECK_ARG(scratch || (action_out && local_out && coarse_out),
                  "helicopter_policy_rollout: this shape runs K x 3 launches and needs `scratch` for the records not kept");
    // the act kernel's LDS: met only here, on the way to its launch (K > 0, after the `scratch` test)
    if (const int st = gca_check_rollout_coarse(C, GCA_POLICY_C_MAX)) return st;
    int32_t* s_act = (int32_t*)scratch;
    float* s_coarse = (float*)scratch + E;
    uint8_t* s_local = (uint8_t*)(s_coarse + (size_t)E * C);
    const bool fast = heli_fast(a);
    for (int k = 0; k < K; ++k) {
        const size_t o = (size_t)k * (size_t)E;
        int32_t* act_k = action_out ? action_out + o : s_act;
        uint8_t* loc_k = local_out ? local_out + o * SS : s_local;
        float* coa_k = coarse_out ? coarse_out + o * (size_t)C : s_coarse;
        if (const int st = gca_policy_observation(buf0, buf1, parity, pos, E, H, W, empty, tree, fire, p->radius,
                                                  p->block, 0, loc_k, coa_k, stream))
            return st;
        hipLaunchKernelGGL(helicopter_policy_act_kernel, grid, dim3(POL_VT), (size_t)policy_lds_words(C) * 4,
                           (hipStream_t)stream, q.w, loc_k, coa_k, rng_step, env_offset, act_k,
                           logits_out ? logits_out + o * 9 : nullptr, value_out ? value_out + o : nullptr);
        GCA_CHECK_LAUNCH("helicopter_policy_rollout");
        a.action = act_k;
        a.rec_reward = reward_out ? reward_out + o : nullptr;
        a.rec_hit = hit_out ? hit_out + o : nullptr;
        launch_heli_step(fast, grid, stream, a);
        GCA_CHECK_LAUNCH("helicopter_policy_rollout");
    }
    return GCA_OK;
}
