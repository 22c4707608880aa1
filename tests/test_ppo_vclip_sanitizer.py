"""CPU: the host build's gca_*_policy_grad_vclip under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone:
gca_cpu.cpp is compiled together with a small main that calls both entries on a tiny case (S = 3, C = 2, Hd = 32, T = 5,
N = 7 with repeated idx), and that program runs on its own. Nothing sanitized is loaded into Python. No GPU."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-cellular-automata_amd", "csrc")

MAIN = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "gca.h"

// exactly-sized heap arrays, so that any access past an end is reported
template <class T>
static T* fill(size_t n, unsigned& s, double lo, double hi) {
    T* a = (T*)malloc(n * sizeof(T));
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        a[i] = (T)(lo + (hi - lo) * ((s >> 8) / 16777216.0));
    }
    return a;
}

template <class F>
static int run(F entry, int64_t (*query)(const gca_policy*, int, int), int nh, int nout, const char* name) {
    const int radius = 1, S = 3, SS = S * S, C = 2, Hd = 32, T = 5, N = 7, NL = nout - 1;
    unsigned s = 12345u + nout;
    float* w_local; float* w_coarse; float* b1;
    if (posix_memalign((void**)&w_local, 16, (size_t)SS * 4 * Hd * 4) || posix_memalign((void**)&w_coarse, 16, C * Hd * 4) ||
        posix_memalign((void**)&b1, 16, Hd * 4))
        return 2;
    for (int i = 0; i < SS * 4 * Hd; ++i) { s = s * 1664525u + 1013904223u; w_local[i] = ((s >> 8) / 16777216.0f - 0.5f) * 0.6f; }
    for (int i = 0; i < C * Hd; ++i) { s = s * 1664525u + 1013904223u; w_coarse[i] = ((s >> 8) / 16777216.0f - 0.5f) * 0.6f; }
    for (int i = 0; i < Hd; ++i) { s = s * 1664525u + 1013904223u; b1[i] = ((s >> 8) / 16777216.0f - 0.5f) * 0.6f; }
    float* w_out = fill<float>((size_t)Hd * nout, s, -0.4, 0.4);
    float* b2 = fill<float>(nout, s, -0.5, 0.5);
    gca_policy p = {radius, 8, Hd, 0, w_local, w_coarse, b1, w_out, b2};
    uint8_t* local = fill<uint8_t>((size_t)T * SS, s, 0, 8);
    float* coarse = fill<float>((size_t)T * C, s, 0, 1);
    int32_t* action = fill<int32_t>((size_t)T * nh, s, 0, 2);
    float* old_logits = fill<float>((size_t)T * NL, s, -1, 1);
    float* old_value = fill<float>(T, s, -1, 1);
    float* advantage = fill<float>(T, s, -1, 1);
    float* returns = fill<float>(T, s, -1, 1);
    int32_t* idx = (int32_t*)malloc(N * sizeof(int32_t));
    const int32_t rows[N] = {4, 0, 4, 2, 1, 0, 3};
    for (int i = 0; i < N; ++i) idx[i] = rows[i];
    float* g_w_local = fill<float>((size_t)SS * 4 * Hd, s, 0, 0);
    float* g_w_coarse = fill<float>((size_t)C * Hd, s, 0, 0);
    float* g_b1 = fill<float>(Hd, s, 0, 0);
    float* g_w_out = fill<float>((size_t)Hd * nout, s, 0, 0);
    float* g_b2 = fill<float>(nout, s, 0, 0);
    float* stats = fill<float>(8, s, 0, 0);
    float* vstats = fill<float>(3, s, 0, 0);
    const int64_t need = query(&p, C, N);
    if (need <= 0) return 3;
    void* ws;
    if (posix_memalign(&ws, 16, (size_t)need)) return 2;
    int bad = 0;
    for (int pass = 0; pass < 3 && !bad; ++pass) {  // idx with repeats; idx = NULL (rows 0 .. T - 1); a null vstats
        const int st = entry(&p, C, local, coarse, action, old_logits, old_value, advantage, returns, T,
                             pass == 1 ? NULL : idx, pass == 1 ? T : N, 0.2f, 0.01f, 0.5f, 1, g_w_local, g_w_coarse,
                             g_b1, g_w_out, g_b2, stats, pass == 2 ? NULL : vstats, ws, need, NULL);
        if (st != 0) { printf("%s: status %d: %s\n", name, st, gca_last_error()); bad = 1; }
        for (int i = 0; i < 8; ++i) bad |= !isfinite(stats[i]);
        for (int i = 0; i < 3; ++i) bad |= !(vstats[i] >= 0.0f && (i == 0 || vstats[i] <= 1.0f));
        for (int i = 0; i < Hd * nout; ++i) bad |= !isfinite(g_w_out[i]);
    }
    // an index outside [0, T) is refused before anything is read
    idx[3] = T;
    if (entry(&p, C, local, coarse, action, old_logits, old_value, advantage, returns, T, idx, N, 0.2f, 0.01f, 0.5f, 1,
              g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats, vstats, ws, need, NULL) != 1)
        bad = 1;
    void* all[] = {w_local, w_coarse, b1, w_out, b2, local, coarse, action, old_logits, old_value, advantage, returns, idx,
                   g_w_local, g_w_coarse, g_b1, g_w_out, g_b2, stats, vstats, ws};
    for (void* a : all) free(a);
    printf("%s: %s\n", name, bad ? "BAD" : "ok");
    return bad;
}

int main() {
    int bad = run(gca_helicopter_policy_grad_vclip, gca_helicopter_policy_grad_workspace, 1, 10, "helicopter");
    bad |= run(gca_bulldozer_policy_grad_vclip, gca_bulldozer_policy_grad_workspace, 2, 12, "bulldozer");
    return bad;
}
"""


def test_host_vclip_entries_run_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host library"
    src = tmp_path / "vclip_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "vclip_san"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(CSRC, "gca_cpu.cpp"), str(src), "-o", str(exe)], check=True)
    # the sanitizers' runtimes are linked statically: the program needs nothing from the environment it starts in
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert "helicopter: ok" in out.stdout and "bulldozer: ok" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert "LeakSanitizer" not in out.stderr
