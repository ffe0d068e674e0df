// ac_ppo_plan_check.cpp -- the PPO trainer's HIP-free plan unit under the host sanitizers (CPU only):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/micro/ac_ppo_plan_check.cpp \
//       bc_mpc_amd/csrc/ac_ppo_plan.cpp bc_mpc_amd/csrc/ac_fit_plan.cpp -o tools/micro/ac_ppo_plan_check && \
//   tools/micro/ac_ppo_plan_check
// Every accepted pair at the limits builds its work list; every refusal returns its code; the run checks walk
// their index arrays to the end.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bc_mpc_amd/csrc/ac_ppo_plan.h"

using namespace bcmpc;

static int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, bcmpc_acppo_last_error()); ++failures; } \
    } while (0)

static bcmpc_acfit_config cfg(int head, int S, int out, int h, int L, int dev = 0) {
    bcmpc_acfit_config c{};
    c.state_dim = S; c.out_dim = out; c.hidden = h; c.n_layers = L; c.head = head; c.batch_size = 128; c.device = dev;
    c.beta1 = 0.9f; c.beta2 = 0.999f; c.epsilon = 1e-8f;
    return c;
}

int main() {
    const bcmpc_acppo_config adam{0.9f, 0.999f, 1e-8f};
    for (int h : {1, 7, 16, 17, 128, 129, 256})
        for (int L : {1, 2, 4})
            for (int S : {1, 20, 32})
                for (int A : {1, 6, 16}) {
                    const bcmpc_acfit_config p = cfg(BCMPC_ACFIT_POLICY, S, A, h, L), v = cfg(BCMPC_ACFIT_VALUE, S, 1, h, L);
                    acppo::Plan plan;
                    EXPECT(acppo::make_plan(&adam, &p, &v, &plan) == BCMPC_OK);
                    size_t tiles = 0;
                    for (int s = 0; s < 2; ++s)
                        for (int l = 0; l <= L; ++l) {
                            const int in = l == 0 ? S : h, o = l == L ? (s == 0 ? A : 1) : h;
                            tiles += (size_t)(in / 16 + 1) * ((o + 15) / 16);
                        }
                    EXPECT(plan.tasks.size() == tiles + 2);
                    EXPECT(plan.tasks[tiles].kind == 2 && plan.tasks[tiles + 1].kind == 3);
                    for (const acppo::Task& t : plan.tasks) {
                        if (t.kind != 0) continue;
                        const int in = t.layer == 0 ? S : h, o = t.layer == L ? (t.stack == 0 ? A : 1) : h;
                        EXPECT(t.stack >= 0 && t.stack < 2 && t.layer >= 0 && t.layer <= L);
                        EXPECT(t.k0 % 16 == 0 && t.k0 <= in && t.n0 % 16 == 0 && t.n0 < o);
                    }
                    EXPECT((int64_t)plan.lds_words == bcmpc_acppo_lds_words(h, L, S, A));
                    EXPECT(plan.lds_words <= acfit::kLdsMaxWords);
                }
    const bcmpc_acfit_config p = cfg(BCMPC_ACFIT_POLICY, 20, 6, 128, 2), v = cfg(BCMPC_ACFIT_VALUE, 20, 1, 128, 2);
    bcmpc_acfit_config q;
    EXPECT(bcmpc_acppo_check_pair(&adam, &v, &v) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_pair(&adam, &p, &p) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_pair(nullptr, &p, &v) == BCMPC_ERR_ARG);
    q = v; q.state_dim = 19; EXPECT(bcmpc_acppo_check_pair(&adam, &p, &q) == BCMPC_ERR_ARG);
    q = v; q.hidden = 64; EXPECT(bcmpc_acppo_check_pair(&adam, &p, &q) == BCMPC_ERR_ARG);
    q = v; q.n_layers = 1; EXPECT(bcmpc_acppo_check_pair(&adam, &p, &q) == BCMPC_ERR_ARG);
    q = v; q.device = 3; EXPECT(bcmpc_acppo_check_pair(&adam, &p, &q) == BCMPC_ERR_ARG);
    q = p; q.out_dim = 17; EXPECT(bcmpc_acppo_check_pair(&adam, &q, &v) == BCMPC_ERR_UNSUPPORTED);
    const bcmpc_acppo_config bad{1.0f, 0.999f, 1e-8f};
    EXPECT(bcmpc_acppo_check_pair(&bad, &p, &v) == BCMPC_ERR_ARG);

    std::vector<int64_t> idx(3 * 128);
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int64_t)(i * 7 % 600);
    const int32_t sizes[3] = {128, 123, 128};
    EXPECT(bcmpc_acppo_check_run(idx.data(), sizes, 3, 600, 1e-3f, 0.2f, 0.f) == BCMPC_OK);
    EXPECT(bcmpc_acppo_check_run(idx.data(), sizes, 3, 599, 1e-3f, 0.2f, 0.f) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_run(idx.data(), sizes, 3, 600, NAN, 0.2f, 0.f) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_run(idx.data(), sizes, 3, 600, 1e-3f, -0.1f, 0.f) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_run(idx.data(), sizes, 3, 600, 1e-3f, INFINITY, 0.f) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_run(idx.data(), sizes, 3, 600, 1e-3f, 0.2f, NAN) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_run(nullptr, sizes, 3, 600, 1e-3f, 0.2f, 0.f) == BCMPC_ERR_ARG);
    EXPECT(bcmpc_acppo_check_run(nullptr, nullptr, 0, 600, 1e-3f, 0.2f, 0.f) == BCMPC_OK);
    EXPECT(acppo::check_state(true, true, true, true, true, true) == BCMPC_OK);
    EXPECT(acppo::check_state(false, true, true, true, true, true) == BCMPC_ERR_STATE);
    EXPECT(acppo::check_state(true, false, true, true, true, true) == BCMPC_ERR_STATE);
    EXPECT(acppo::check_state(true, true, false, true, true, true) == BCMPC_ERR_STATE);
    const float f[3] = {0.f, 1.f, INFINITY};
    EXPECT(acppo::check_finite(f, 2, "x") == BCMPC_OK && acppo::check_finite(f, 3, "x") == BCMPC_ERR_ARG);
    EXPECT(std::strstr(bcmpc_acppo_last_error(), "x must be finite") != nullptr);
    // the filter's device image [2][32] at the smallest and the largest state: mean / std up to S, 0 / 1 beyond
    // (the sources hold exactly S floats: a read past them is the sanitizer's to catch)
    for (int S : {1, 32}) {
        std::vector<float> mean(S), sd(S);
        for (int i = 0; i < S; ++i) { mean[i] = 0.5f + (float)i; sd[i] = 2.0f + (float)i; }
        EXPECT(acfit::check_filter(mean.data(), sd.data(), S) == BCMPC_OK);
        float img[64];
        for (float& x : img) x = NAN;
        acfit::filter_image(mean.data(), sd.data(), S, img);
        for (int i = 0; i < 32; ++i) {
            EXPECT(img[i] == (i < S ? mean[i] : 0.f));
            EXPECT(img[32 + i] == (i < S ? sd[i] : 1.f));
        }
    }
    std::printf(failures ? "%d failures\n" : "ac_ppo_plan_check ok\n", failures);
    return failures ? 1 : 0;
}
