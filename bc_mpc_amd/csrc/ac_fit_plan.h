// ac_fit_plan.h -- what bcmpc_acfit_create decides before it touches the device: the checked config, the flat
// parameter layout, the row kernel's LDS and the parameter kernel's work list.  Pure host arithmetic (no HIP).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/bcmpc.h"

#pragma GCC visibility push(hidden)
namespace bcmpc::acfit {

constexpr int kRows = 16;                   // batch rows per row-block workgroup (one MFMA row tile)
constexpr int kWaves = 16;                  // waves of the row-block workgroup
constexpr int kTgtLd = 16;                  // stride of the target rows in LDS (out_dim <= 16)
constexpr size_t kLdsMaxWords = 160 * 1024 / 4;

struct Tile {                               // one workgroup of acfit_params_kernel
    int32_t kind;                           // 0: weight tile (+ bias row), 3: loss and step counter
    int32_t layer;
    int32_t k0, n0;                         // tile origin
};

struct Plan {
    bcmpc_acfit_config cfg{};
    int S = 0, N = 0, h = 0, L = 0;
    int ld = 0;                             // row stride of the LDS row buffers (f32 words)
    size_t lds_words = 0;                   // acfit_rows_kernel's dynamic LDS
    size_t n_params = 0;
    int32_t w_off[BCMPC_ACFIT_MAX_LAYERS + 1]{}, b_off[BCMPC_ACFIT_MAX_LAYERS + 1]{};
    int32_t lin[BCMPC_ACFIT_MAX_LAYERS + 1]{}, lout[BCMPC_ACFIT_MAX_LAYERS + 1]{};
    std::vector<Tile> tiles;
};

int fail(int code, const std::string& msg);               // bcmpc_acfit_last_error() text
// the shape checks alone (bcmpc_acfit_lds_words); a refusal sets the error text and returns its code
int check_shape(int head, int state_dim, int out_dim, int hidden, int n_layers);
// LDS words of the row kernel: two row buffers and one activation buffer per hidden layer, [kRows][ld] each,
// the targets [kRows][kTgtLd], the loss partials [kWaves], the K-split partials [kWaves][256]
size_t lds_words(int hidden, int n_layers, int state_dim, int out_dim);
int make_plan(const bcmpc_acfit_config* c, Plan* out);    // every check of bcmpc_acfit_create
// bcmpc_acfit_run's checks: sizes >= 1, indices inside [0, n_data); *total, *bmax: the rows and the largest batch
int check_run(const int64_t* indices, const int32_t* batch_sizes, int32_t iterations, float lr, int64_t n_data,
              int64_t* total, int32_t* bmax);
int check_filter(const float* mean, const float* std, int S);
// the device image of a checked filter, [2][32]: mean then std, 0 / 1 beyond S
void filter_image(const float* mean, const float* std, int S, float* out);

}  // namespace bcmpc::acfit
#pragma GCC visibility pop
