// train_run.h -- the host side the three trainers share (fit.hip, ac_fit.hip, ac_ppo.hip): grow-only device
// buffers, and a whole run of N steps replayed as one captured graph.  Header only; nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <initializer_list>
#include <string>

#include "../../include/bcmpc.h"

#pragma GCC visibility push(hidden)
namespace bcmpc::train {

struct Buf {                                // one device buffer of a group; bytes == 0: freed, not allocated
    void** p; size_t bytes;
    template <class T> Buf(T** q, size_t n) : p((void**)q), bytes(n) {}
};

// Buffers that share one capacity grow together and never shrink.  Freed, nulled and the capacity zeroed before
// the first allocation, so a failed one (false) leaves the trainer consistent: the next call starts over.
template <class Cap>
inline bool grow(Cap* cap, Cap need, std::initializer_list<Buf> bufs) {
    if (need <= *cap) return true;
    for (const Buf& b : bufs)
        if (*b.p) { (void)hipFree(*b.p); *b.p = nullptr; }
    *cap = 0;
    for (const Buf& b : bufs)
        if (b.bytes && hipMalloc(b.p, b.bytes) != hipSuccess) return false;
    *cap = need;
    return true;
}

// One captured graph of a whole run (a single chain of kernel nodes on one stream), reused while its key stands:
// everything the graph holds by value or by address that no drop() at a reallocation covers.
struct GraphRun {
    static constexpr int kKey = 16;
    hipGraphExec_t exec = nullptr;
    intptr_t key[kKey] = {};
    int32_t captures = 0;

    void drop() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
    // Replays the graph when `k` is its key; otherwise captures what enqueue() (-> BCMPC_OK or its own failure)
    // puts on `stream`, instantiates, keys, counts and launches.  fail: the trainer's error function.
    template <class Enqueue>
    int run(hipStream_t stream, const intptr_t (&k)[kKey], int (*fail)(int, const std::string&), Enqueue&& enqueue) {
        if (!(exec && std::memcmp(k, key, sizeof(key)) == 0)) {
            drop();
            if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess)
                return fail(BCMPC_ERR_HIP, "graph capture failed to start");
            const int rc = enqueue();
            hipGraph_t g = nullptr;
            const hipError_t ec = hipStreamEndCapture(stream, &g);
            if (rc != BCMPC_OK || ec != hipSuccess) {
                if (g) (void)hipGraphDestroy(g);
                return rc != BCMPC_OK ? rc : fail(BCMPC_ERR_HIP, "graph capture failed");
            }
            const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess) { exec = nullptr; return fail(BCMPC_ERR_HIP, "graph instantiation failed"); }
            std::memcpy(key, k, sizeof(key));
            ++captures;
        }
        if (hipGraphLaunch(exec, stream) != hipSuccess) return fail(BCMPC_ERR_HIP, "graph launch failed");
        return BCMPC_OK;
    }
};

}  // namespace bcmpc::train
#pragma GCC visibility pop
