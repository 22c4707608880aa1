// gca_opt.hip — the optimizer's side of the PPO update (include/gca.h "optimizer"): gca_adam_step, the global-norm clip
// and the Adam step of up to eight tensors in two launches, and gca_permutation, the minibatch shuffle in one.
//
// gca_adam_step: the tensors are cut into chunks of CH elements (gca_opt_plan.h), one workgroup per chunk in both
// launches; a workgroup finds its tensor through the chunk prefix table in the kernel arguments.
//   norm    every workgroup writes its chunk's sum of squares (double) to the workspace; workgroup 0 also reads the
//           state block and writes the next count, pows and learning rate to the block's pending slot.
//   update  every workgroup re-adds the partials in gca.h's order (at most 2056 of them), reads the pending slot and
//           updates its chunk of w, m and v; workgroup 0 copies the pending slot into the state with the norm.
// No workgroup reads a word that another workgroup of the same launch writes, and nothing is accumulated with atomics.
// The f32 divide and square root are the correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt, the
// compiler's default, named in the Makefile); the build runs with -ffp-contract=off.
#include "gca_common.h"
#include "gca_opt_plan.h"

struct AdamArgs {
    float* w[GCA_ADAM_MAX_TENSORS];
    const float* g[GCA_ADAM_MAX_TENSORS];
    float* m[GCA_ADAM_MAX_TENSORS];
    float* v[GCA_ADAM_MAX_TENSORS];
    int64_t len[GCA_ADAM_MAX_TENSORS];
    int32_t first[GCA_ADAM_MAX_TENSORS];  // the first chunk of tensor t; from tensor n on the chunk count, which no
                                          // workgroup reaches
    uint32_t vec_mask;                        // bit t: the tensor's four pointers are 16-B aligned
    int64_t CH;
};

// the chunk of this workgroup: its tensor's arrays advanced to the chunk, and its element count
struct AdamChunk {
    float* w;
    const float* g;
    float* m;
    float* v;
    int cnt;
    bool vec;
};

__device__ __forceinline__ AdamChunk adam_find(const AdamArgs& a, int blk) {
    float *w = a.w[0], *m = a.m[0], *v = a.v[0];
    const float* g = a.g[0];
    int64_t len = a.len[0];
    int first = 0, t = 0;
#pragma unroll
    for (int i = 1; i < GCA_ADAM_MAX_TENSORS; ++i) {  // static indices and selects: the table stays in scalar registers
        const bool hit = blk >= a.first[i];
        w = hit ? a.w[i] : w;
        g = hit ? a.g[i] : g;
        m = hit ? a.m[i] : m;
        v = hit ? a.v[i] : v;
        len = hit ? a.len[i] : len;
        first = hit ? a.first[i] : first;
        t = hit ? i : t;
    }
    const int64_t base = (int64_t)(blk - first) * a.CH;
    const int64_t left = len - base;
    return AdamChunk{w + base, g + base, m + base, v + base, (int)(left < a.CH ? left : a.CH),
                     ((a.vec_mask >> t) & 1u) != 0};
}

// s[l] = s[l] + s[l + h], h = 128 .. 1: gca.h's tree
__device__ __forceinline__ double adam_tree(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int h = ADAM_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double adam_sq(double s, float x) { return s + (double)x * (double)x; }

__global__ __launch_bounds__(ADAM_THREADS) void adam_norm_kernel(AdamArgs a, int32_t* __restrict__ state, float lr0,
                                                                 float b1, float b2, int64_t steps_per_iteration,
                                                                 int64_t num_iterations, double* __restrict__ part) {
    __shared__ double red[ADAM_THREADS];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const AdamChunk c = adam_find(a, blk);
    double s = 0.0;
    for (int q = tid; 4 * q < c.cnt; q += ADAM_THREADS) {
        const int e = 4 * q;
        if (c.vec && e + 3 < c.cnt) {
            const float4 x = reinterpret_cast<const float4*>(c.g)[q];
            s = adam_sq(adam_sq(adam_sq(adam_sq(s, x.x), x.y), x.z), x.w);
        } else {
            for (int j = 0; j < 4; ++j)
                if (e + j < c.cnt) s = adam_sq(s, c.g[e + j]);
        }
    }
    s = adam_tree(s, red, tid);
    if (tid == 0) {
        part[blk] = s;
        if (blk == 0) {
            const int32_t count = state[ADAM_COUNT];
            state[ADAM_PENDING + ADAM_COUNT] = count + 1;
            state[ADAM_PENDING + ADAM_B1POW] = __float_as_int(__int_as_float(state[ADAM_B1POW]) * b1);
            state[ADAM_PENDING + ADAM_B2POW] = __float_as_int(__int_as_float(state[ADAM_B2POW]) * b2);
            state[ADAM_PENDING + ADAM_LR] = __float_as_int(adam_lr(lr0, count, steps_per_iteration, num_iterations));
        }
    }
}

struct AdamCoef {
    float b1, b2, omb1, omb2, c1, c2, lr, eps, norm, max_norm;
    bool clip;
};

// one element, gca.h's order
__device__ __forceinline__ void adam_elem(const AdamCoef& k, float& w, float g, float& m, float& v) {
    const float gc = k.clip ? (g / k.norm) * k.max_norm : g;
    m = (k.b1 * m) + (k.omb1 * gc);
    v = (k.b2 * v) + ((k.omb2 * gc) * gc);
    const float mhat = m / k.c1, vhat = v / k.c2;
    w = w - (k.lr * (mhat / (sqrtf(vhat) + k.eps)));
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_update_kernel(AdamArgs a, int32_t* __restrict__ state, float b1,
                                                                   float b2, float eps, float max_norm,
                                                                   const double* __restrict__ part, int nparts,
                                                                   float* __restrict__ info_out) {
    __shared__ double red[ADAM_THREADS];
    const int tid = threadIdx.x, blk = blockIdx.x;
    double s = 0.0;
    for (int p = tid; p < nparts; p += ADAM_THREADS) s = s + part[p];
    const float norm = sqrtf((float)adam_tree(s, red, tid));
    // workgroup 0 writes words 0..4 of the state below; everyone reads the pending slot only
    const int32_t count = state[ADAM_PENDING + ADAM_COUNT];
    const float b1p = __int_as_float(state[ADAM_PENDING + ADAM_B1POW]);
    const float b2p = __int_as_float(state[ADAM_PENDING + ADAM_B2POW]);
    const float lr = __int_as_float(state[ADAM_PENDING + ADAM_LR]);
    AdamCoef k;
    k.b1 = b1, k.b2 = b2, k.omb1 = 1.0f - b1, k.omb2 = 1.0f - b2, k.c1 = 1.0f - b1p, k.c2 = 1.0f - b2p;
    k.lr = lr, k.eps = eps, k.norm = norm, k.max_norm = max_norm;
    k.clip = max_norm > 0.0f && !(norm < max_norm);
    const AdamChunk c = adam_find(a, blk);
    for (int q = tid; 4 * q < c.cnt; q += ADAM_THREADS) {
        const int e = 4 * q;
        if (c.vec && e + 3 < c.cnt) {
            float4 w = reinterpret_cast<float4*>(c.w)[q], m = reinterpret_cast<float4*>(c.m)[q];
            float4 v = reinterpret_cast<float4*>(c.v)[q];
            const float4 g = reinterpret_cast<const float4*>(c.g)[q];
            adam_elem(k, w.x, g.x, m.x, v.x);
            adam_elem(k, w.y, g.y, m.y, v.y);
            adam_elem(k, w.z, g.z, m.z, v.z);
            adam_elem(k, w.w, g.w, m.w, v.w);
            reinterpret_cast<float4*>(c.w)[q] = w;
            reinterpret_cast<float4*>(c.m)[q] = m;
            reinterpret_cast<float4*>(c.v)[q] = v;
        } else {
            for (int j = 0; j < 4; ++j) {
                if (e + j < c.cnt) {
                    float w = c.w[e + j], m = c.m[e + j], v = c.v[e + j];
                    adam_elem(k, w, c.g[e + j], m, v);
                    c.w[e + j] = w;
                    c.m[e + j] = m;
                    c.v[e + j] = v;
                }
            }
        }
    }
    if (blk == 0 && tid == 0) {
        state[ADAM_COUNT] = count;
        state[ADAM_B1POW] = __float_as_int(b1p);
        state[ADAM_B2POW] = __float_as_int(b2p);
        state[ADAM_NORM] = __float_as_int(norm);
        state[ADAM_LR] = __float_as_int(lr);
        if (info_out) {
            info_out[0] = norm;
            info_out[1] = lr;
        }
    }
}

extern "C" int64_t gca_adam_step_workspace(int64_t total_elements) {
    if (gca_check_adam_step_workspace(total_elements)) return -1;
    return adam_workspace_bytes(total_elements);
}

extern "C" int gca_adam_step(const gca_adam_tensors* t, void* state, float lr0, float b1, float b2, float eps,
                             float max_norm, int64_t steps_per_iteration, int64_t num_iterations, float* info_out,
                             void* workspace, int64_t workspace_bytes, void* stream) {
    int64_t total;
    if (const int st = gca_check_adam_step(t, state, b1, b2, eps, steps_per_iteration, num_iterations, info_out,
                                           workspace, workspace_bytes, &total))
        return st;
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    a.CH = adam_chunk(total);
    int nb = 0;
    for (int i = 0; i < GCA_ADAM_MAX_TENSORS; ++i) {
        a.first[i] = nb;
        if (i >= t->n) continue;
        a.w[i] = t->w[i], a.g[i] = t->g[i], a.m[i] = t->m[i], a.v[i] = t->v[i], a.len[i] = t->len[i];
        const uintptr_t al = (uintptr_t)t->w[i] | (uintptr_t)t->g[i] | (uintptr_t)t->m[i] | (uintptr_t)t->v[i];
        if ((al & 15u) == 0) a.vec_mask |= 1u << i;
        nb += (int)((t->len[i] + a.CH - 1) / a.CH);
    }
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    int32_t* sw = reinterpret_cast<int32_t*>(state);
    hipLaunchKernelGGL(adam_norm_kernel, dim3((unsigned)nb), dim3(ADAM_THREADS), 0, st, a, sw, lr0, b1, b2,
                       steps_per_iteration, num_iterations, part);
    hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)nb), dim3(ADAM_THREADS), 0, st, a, sw, b1, b2, eps, max_norm,
                       part, nb, info_out);
    GCA_CHECK_LAUNCH("adam_step");
    return GCA_OK;
}

// ------------------------------------------------------------------ the permutation
struct PermRound {
    uint32_t k0, k1;
    __device__ __forceinline__ uint32_t operator()(uint32_t right, uint32_t round, uint32_t row_key) const {
        return philox4x32_10(u32x4{right, round, row_key, GCA_TAG_PERM}, k0, k1).x;
    }
};

__global__ __launch_bounds__(256) void permutation_kernel(uint32_t k0, uint32_t k1, uint32_t epoch0,
                                                          const int32_t* __restrict__ counter, uint32_t T, int h,
                                                          int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= T) return;
    const uint32_t row_key = epoch0 + blockIdx.y + (counter ? (uint32_t)counter[0] : 0u);
    bool capped = false;
    out[(size_t)blockIdx.y * T + i] = (int32_t)perm_walk(i, T, h, row_key, PermRound{k0, k1}, &capped);
}

extern "C" int gca_permutation(uint64_t seed, uint32_t epoch0, const int32_t* counter, int64_t T, int rows,
                               int32_t* out, void* stream) {
    if (const int st = gca_check_permutation(counter, T, rows, out)) return st;
    hipLaunchKernelGGL(permutation_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)rows), dim3(256), 0,
                       (hipStream_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32), epoch0, counter, (uint32_t)T,
                       perm_half_bits(T), out);
    GCA_CHECK_LAUNCH("permutation");
    return GCA_OK;
}
