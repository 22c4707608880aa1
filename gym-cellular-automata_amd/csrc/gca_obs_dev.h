// gca_obs_dev.h — the cell transforms and the display selection of the Advanced env's observation (gca_obs.hip's header
// comment states them; include/gca.h "Advanced env observations") as device functions, written once: gca_obs.hip colours
// the displayed value, gca_adv_policy.hip (gca_advanced_display, gca_advanced_policy_act_display) hands it to the agent.
//   blur(g)[r,c] = floor((2 S + 9) / 18), S the 3x3 sum with edge padding; vis(v) = (v == 3 && !is_night) ? 0 : v (the
//   reference's literal 3); the selection: the first ROW holding a positive extension value, its index clamped and used
//   as the CHANNEL index, the base channel when there is none.
#pragma once
#include "gca_common.h"

// blur of cell (r, c) from global memory, edge padding
__device__ __forceinline__ int blur_at(const uint8_t* __restrict__ g, int H, int W, int r, int c) {
    int s = 0;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr) {
        const int rr = min(max(r + dr, 0), H - 1);
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) s += g[(int64_t)rr * W + min(max(c + dc, 0), W - 1)];
    }
    return (2 * s + 9) / 18;
}

__device__ __forceinline__ int transform(int raw, int blurred, bool night, int skip_vis, int skip_blur) {
    int v = skip_blur ? raw : blurred;
    if (!skip_vis && v == 3 && !night) v = 0;
    return v;
}

struct ObsCfg {
    bool need_blur;  // some channel in use blurs
    uint32_t on;     // active extension channels
    bool night;      // pre-step day/night
};

// base channel + active extension channels of one cell from its raw value and blur
__device__ __forceinline__ int ext_value(const gca_obs_params& p, const ObsCfg& k, int i, int raw, int bl) {
    return ((k.on >> i) & 1u) ? transform(raw, bl, k.night, p.ext_skip_visibility[i], p.ext_skip_blur[i]) : 0;
}

// the PRE-step day/night of env e: the env step toggled is_night when time_step % day_length == 0 (time_step NULL:
// is_night as it is)
__device__ __forceinline__ bool obs_night(const gca_obs_params& p, const int32_t* __restrict__ is_night,
                                          const int32_t* __restrict__ time_step, int e) {
    bool night = is_night[e] != 0;
    if (time_step && p.day_length > 0 && time_step[e] % p.day_length == 0) night = !night;
    return night;
}

// the active extension channels of extension choice `choice` (clamped to the lookup's rows)
__device__ __forceinline__ uint32_t obs_channels_on(const gca_obs_params& p, int choice) {
    uint32_t on = 0u;
    choice = min(max(choice, 0), min(p.n_choices, 8) - 1);
    for (int i = 0; i < p.n_ext; ++i) on |= (p.ext_lookup[choice][i] != 0 ? 1u : 0u) << i;
    return on;
}

// The display selection of the step observation by one wave (all 64 lanes active; every wave of a workgroup may run it
// on its own: the result is a function of the grid alone, so all agree and no workgroup barrier is needed per scanned
// row): -1 = the base channel, else the extension channel shown everywhere. The scan normally stops at row 0.
__device__ __forceinline__ int obs_display_select(const gca_obs_params& p, const ObsCfg& k,
                                                  const uint8_t* __restrict__ g, int H, int W, int lane) {
    int sel = -1;
    bool scan_blur = false;
    for (int i = 0; i < p.n_ext; ++i) scan_blur |= ((k.on >> i) & 1u) && !p.ext_skip_blur[i];
    int fv = -1;
    for (int r = 0; r < H && fv < 0; ++r) {
        int any = 0;
        if ((W & 3) == 0) {
            for (int c4 = 4 * lane; c4 < W; c4 += 256) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(g + (int64_t)r * W + c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int raw = (int)((w >> (8 * j)) & 0xFFu);
                    const int bl = scan_blur ? blur_at(g, H, W, r, c4 + j) : raw;
                    for (int i = 0; i < p.n_ext; ++i) any |= ext_value(p, k, i, raw, bl) > 0;
                }
            }
        } else {
            for (int c = lane; c < W; c += 64) {
                const int raw = g[(int64_t)r * W + c];
                const int bl = scan_blur ? blur_at(g, H, W, r, c) : raw;
                for (int i = 0; i < p.n_ext; ++i) any |= ext_value(p, k, i, raw, bl) > 0;
            }
        }
        if (__ballot(any) != 0ull) fv = r;
    }
    if (fv >= 0) sel = min(fv, p.n_ext - 1);
    return sel;
}

// What the displayed plane of an env is, once its selection is known: all zeros (a switched-off channel), the raw grid
// or the blurred grid, each with or without visibility's rule on the literal 3.
enum { OBS_SHOW_ZERO = 0, OBS_SHOW_RAW = 1, OBS_SHOW_BLUR = 2 };
struct ObsShow {
    int kind;   // OBS_SHOW_*
    bool vis3;  // a value of 3 is shown as 0 (visibility applies and it is day)
};

__device__ __forceinline__ ObsShow obs_display_show(const gca_obs_params& p, const ObsCfg& k, int sel) {
    ObsShow s;
    if (sel < 0) {  // the base channel: the transformed grid, or the grid itself
        s.kind = p.should_transform ? OBS_SHOW_BLUR : OBS_SHOW_RAW;
        s.vis3 = p.should_transform && !k.night;
    } else if (!((k.on >> sel) & 1u)) {
        s.kind = OBS_SHOW_ZERO;
        s.vis3 = false;
    } else {
        s.kind = p.ext_skip_blur[sel] ? OBS_SHOW_RAW : OBS_SHOW_BLUR;
        s.vis3 = !p.ext_skip_visibility[sel] && !k.night;
    }
    return s;
}

// the displayed value of a cell from the value of its kind (raw or blurred; ignored for OBS_SHOW_ZERO)
__device__ __forceinline__ int obs_display_value(const ObsShow& s, int v) {
    if (s.kind == OBS_SHOW_ZERO) return 0;
    return (s.vis3 && v == 3) ? 0 : v;
}
