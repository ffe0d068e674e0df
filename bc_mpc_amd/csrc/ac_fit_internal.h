// ac_fit_internal.h -- the actor-critic fitter's state and the parts of a run, for the units that enqueue its
// steps into a chain of their own (ac_ppo.hip interleaves the policy fitter's BC step with its PPO step).  Host
// declarations only; the kernels stay in ac_fit.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "ac_fit_plan.h"
#include "train_run.h"

struct bcmpc_acfit {
    bcmpc::acfit::Plan plan;
    hipStream_t stream = nullptr;
    float *d_w = nullptr, *d_wt = nullptr, *d_m = nullptr, *d_v = nullptr;
    float *d_x0 = nullptr, *d_dp = nullptr, *d_act = nullptr, *d_dzs = nullptr, *d_lpart = nullptr;
    int32_t bcap = 0;                             // rows the activation buffers hold
    float* d_filt = nullptr;                      // [2][32] ob_mean, ob_std: one address for the fitter's life
    float* d_state = nullptr;                     // [beta1_power, beta2_power, learning rate]
    float h_state[3] = {0.f, 0.f, 0.f};           // their host mirror, the upload's source
    int32_t* d_iter = nullptr;
    bcmpc::acfit::Tile* d_tiles = nullptr;
    double *d_obs = nullptr, *d_tgt = nullptr;
    int64_t n_data = 0, data_cap = 0;
    int64_t* d_idx = nullptr; int64_t idx_cap = 0;
    float* d_loss = nullptr; int32_t loss_cap = 0;
    // one captured graph of a whole uniform-batch run, reused while everything it holds by address or by value
    // stands: the step count and batch size, the index and loss buffers (the key below); the data and activation
    // buffers (graph.drop() where they are reallocated).  The filter and the learning rate are read from
    // device memory at fixed addresses: new values need no new graph.
    bcmpc::train::GraphRun graph;
    bool last_graph = false;
    bool has_weights = false, has_filter = false;
};

#pragma GCC visibility push(hidden)
namespace bcmpc::acfit {

// activation buffers for batches of up to `rows` rows (no run is in flight); a growth drops the fitter's graph
bool acfit_reserve(bcmpc_acfit* f, int32_t rows);
// A run in three parts, all on `stream`.  prepare: the activation, index and loss buffers for `total` indices in
// `iterations` steps of at most `bmax` rows, the indices' upload, the step counter at 0, the beta powers and the
// learning rate.  The caller has run check_run and the state checks.
int acfit_prepare(bcmpc_acfit* f, hipStream_t stream, const int64_t* indices, int64_t total, int32_t bmax,
                  int32_t iterations, float learning_rate);
// one Adam step: 2 launches; rows d_idx[iter * stride ..] (the device step counter), B of them
int acfit_step(bcmpc_acfit* f, hipStream_t stream, const int64_t* d_idx, int stride, int B);
// finish: the losses' download (optional), the stream's synchronisation, the host mirror of the beta powers
int acfit_finish(bcmpc_acfit* f, hipStream_t stream, int32_t iterations, float* losses);

}  // namespace bcmpc::acfit
#pragma GCC visibility pop
