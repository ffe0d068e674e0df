// mt_draw.cpp -- NumPy's MT19937 action stream: the device draw, the pre-draw worker, the speculative draw,
// bcmpc_get_action_mt19937 and the bcmpc_mt19937_* entry points.
#include "host_internal.h"

using namespace bcmpc::host;

// a host thread of the split NumPy-stream draw gets at least this many generator words
// (BCMPC_MT_MIN_WORDS overrides): below it the jump-ahead (~0.1 ms per thread) does not pay
static int64_t mt_min_words() {
    const char* v = std::getenv("BCMPC_MT_MIN_WORDS");
    return (v && *v) ? std::max<int64_t>(1, std::atoll(v)) : int64_t(1) << 20;
}

extern "C" {

// ---- NumPy-stream draw on the device -------------------------------------------------------
// Generator words per chunk (one workgroup each; BCMPC_MT_CHUNK_WORDS overrides) and coefficient
// slices per jump polynomial (BCMPC_MT_SPLITS): chunks trade jump work (one 624 x 19937 GF(2)
// correlation each, ~0.35 us of the whole chip, VALU-bound) against serial generation (~0.9 words
// per ns per workgroup).  cfg3 (15.7M words): 2^16 words -> 240 chunks x 17 slices, draw ~0.18 ms
// (tools/mt_device_sweep.py, profiles/r02_mt_device_sweep.txt).  Smaller draws want smaller chunks (the
// serial generation of one chunk is the draw's critical path once the chip has spare workgroups): ~60
// chunks per draw, as a power of two in [2^12, 2^16] words -- cfg2 (983k words) 0.366 -> 0.322 ms and a
// K = 1000 x 15 draw 0.262 -> 0.223 ms per drop-in get_action at 2^14 (profiles/r02c_mt_chunk_sweep.txt);
// round 4 (the team kernel 30% faster): the K = 1000 x 15 draw at 2^12-word chunks, back to back 0.162 ->
// 0.153 ms, with host work between calls 0.111 -> 0.105 (profiles/r04_cfg1_chunk_ab.jsonl; 2^13 0.155, 2^15 0.173).
static int64_t mt_chunk_words(int64_t shard_words) {
    const char* v = std::getenv("BCMPC_MT_CHUNK_WORDS");
    if (v && *v) return std::max<int64_t>(2, std::atoll(v)) & ~int64_t(1);
    int64_t w = int64_t(1) << 12;
    while (w < (int64_t(1) << 16) && 2 * w <= shard_words / 60) w *= 2;
    return w;
}
static int mt_splits(int cj) {
    const char* v = std::getenv("BCMPC_MT_SPLITS");
    if (v && *v) return std::max(1, std::min(64, std::atoi(v)));
    return std::max(2, std::min(32, (4096 + cj - 1) / std::max(1, cj)));
}
// NumPy-stream draws of at most this many generator words (2 A H k_global; BCMPC_MT_ZC_WORDS overrides)
// are drawn on the host straight into pinned memory that the rollout kernel reads over the bus
// (zero copy): there the device draw is a few chunks whose serial generation chains (one workgroup,
// 227 words per LDS-synchronised step) and copies cost more than the host's ~0.5 ns per word.  2^16:
// the reference's K = 400 steps (33.6k words at H = 7); a K = 1000 x 15 draw (180k) is faster on the
// device with 2^14-word chunks (0.223 vs 0.250 ms per drop-in get_action)
// ---- pre-draw worker (small NumPy-stream draws) ----
static bool mt_predraw_enabled() {
    static const bool on = [] {
        const char* v = std::getenv("BCMPC_MT_PREDRAW");
        return !(v && v[0] == '0');
    }();
    return on;
}

static bool mt_predraw_late() {
    static const bool on = [] {
        const char* v = std::getenv("BCMPC_MT_PREDRAW_LATE");
        return !(v && v[0] == '0');
    }();
    return on;
}

static bool mt_predraw_dev() {
    static const bool on = [] {
        const char* v = std::getenv("BCMPC_MT_PREDRAW_DEV");
        return !(v && v[0] == '0');
    }();
    return on;
}

// The worker and the control thread hand jobs over by spinning first (BCMPC_MT_PREDRAW_SPIN_US, default
// 200 us) and only then blocking on the condition variable: a futex wake of either side costs several
// microseconds on a loaded host, the same order as the K = 400 draw itself
static int64_t predraw_spin_ns() {
    static const int64_t ns = [] {
        const char* v = std::getenv("BCMPC_MT_PREDRAW_SPIN_US");
        return (v && *v) ? std::max<int64_t>(0, std::atoll(v)) * 1000 : int64_t(200000);
    }();
    return ns;
}

// spin until *a == want or (b and *b), at most predraw_spin_ns()
static void spin_until(const std::atomic<bool>* a, bool want, const std::atomic<bool>* b = nullptr) {
    const int64_t lim = predraw_spin_ns();
    if (lim <= 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&] {
        return a->load(std::memory_order_acquire) == want || (b && b->load(std::memory_order_acquire));
    };
    for (uint32_t i = 1; !done(); ++i) {
        if ((i & 255) == 0 && std::chrono::duration_cast<std::chrono::nanoseconds>(
                                  std::chrono::steady_clock::now() - t0).count() > lim)
            return;
        __builtin_ia32_pause();
    }
}

// wait until the worker is idle (its buffer complete); returns the buffer index it last filled
static int predraw_wait(bcmpc_engine* e) {
    spin_until(&e->pre.inflight, false);
    std::unique_lock<std::mutex> lk(e->pre.mu);
    e->pre.cv.wait(lk, [&] { return !e->pre.pending && !e->pre.busy; });
    return e->pre.buf;
}

// rows [H][shard] of the draw that starts at NumPy state `from`, into the buffer the last call did not read
static void predraw_post(bcmpc_engine* e, const Mt19937& from, const double* low, const double* high, int A,
                         int64_t k_global, int64_t cand_offset, bool rows) {
    auto& p = e->pre;
    {
        std::lock_guard<std::mutex> lk(p.mu);
        p.rows = rows;
        p.from = from;
        p.low.assign(low, low + A);
        p.high.assign(high, high + A);
        p.kg = k_global;
        p.off = cand_offset;
        p.buf = e->zc_last ^ 1;
        p.ready = false;
        p.pending = true;
        p.job = p.job + 1 == 0 ? 1 : p.job + 1;       // (0 is "no wait")
        p.claimed.store(false, std::memory_order_relaxed);
        p.inflight.store(true, std::memory_order_release);
    }
    if (!p.th.joinable()) {
        p.th = std::thread([e] {
            auto& q = e->pre;
            const bcmpc_config& c = e->cfg;
            std::unique_lock<std::mutex> lk(q.mu);
            for (;;) {
                if (!q.quit && !q.pending) {              // spin for the next job before sleeping
                    lk.unlock();
                    spin_until(&q.inflight, true, &q.quit_a);
                    lk.lock();
                }
                q.cv.wait(lk, [&] { return q.quit || q.pending; });
                if (q.quit) return;
                q.pending = false;
                q.busy = true;
                Mt19937 g = q.from;
                const std::vector<double> lo = q.low, hi = q.high;
                const int64_t kg = q.kg, off = q.off;
                const bool rows = q.rows;
                const uint32_t job = q.job;
                double* dst = e->h_zc[q.buf];
                lk.unlock();
                // (tests: BCMPC_MT_PREDRAW_DELAY_US holds every job back, so calls find it in flight)
                if (const char* dv = std::getenv("BCMPC_MT_PREDRAW_DELAY_US"))
                    std::this_thread::sleep_for(std::chrono::microseconds(std::atoll(dv)));
                const int64_t K = c.num_paths;
                const size_t row = (size_t)K * c.action_dim;
                if (rows && off == 0 && K == kg)          // the whole draw: one pass over [H * K] rows
                    mt_uniform_rows(g, lo.data(), hi.data(), c.action_dim, (int64_t)c.horizon * kg, 0,
                                    (int64_t)c.horizon * kg, dst);
                else if (rows)
                    for (int h = 0; h < c.horizon; ++h)
                        mt_uniform_rows(g, lo.data(), hi.data(), c.action_dim, kg, off, off + K, dst + h * row);
                else
                    g.advance(2 * (int64_t)c.action_dim * c.horizon * kg);
                if (rows && e->h_rows_seq)                // (x86 stores are ordered: the rows before the word)
                    __atomic_store_n(e->h_rows_seq, job, __ATOMIC_RELEASE);
                bool copied = false;
                const int qb = (int)(dst == e->h_zc[0] ? 0 : 1);
                // the rows into HBM while the caller's env step runs (not when a call already reads them
                // from the pinned buffer: the copy would only share the bus with that kernel)
                if (rows && e->copy_st && e->d_rows[qb] && !q.claimed.load(std::memory_order_acquire)) {
                    (void)hipSetDevice(c.device);
                    copied = hipMemcpyAsync(e->d_rows[qb], dst, (size_t)c.horizon * row * sizeof(double),
                                            hipMemcpyHostToDevice, e->copy_st) == hipSuccess &&
                             hipEventRecord(e->copy_ev[qb], e->copy_st) == hipSuccess;
                }
                lk.lock();
                e->copy_valid[qb] = copied;
                q.to = g;
                q.ready = true;
                q.busy = false;
                q.inflight.store(false, std::memory_order_release);
                q.cv.notify_all();
            }
        });
    }
    p.cv.notify_all();
}

// (2^18 with the pre-draw worker measured worse at cfg1's 180k words back to back: the kernel's own reads of
// 720 KB of rows over the bus, +30 us -- profiles/r03_dropin_zc_bound_ab.txt; draws whose rows are not read,
// the stochastic policy's, take the host path at any size: only NumPy's state advances)
// (round 4: the next call's rows are drawn from the moment this call's rollout is launched.  Taking cfg1's
//  180k-word draw on the host that way measured worse back to back than the device draw -- 0.234 vs 0.197 ms,
//  the host draw outlasts the 0.14-ms rollout it overlaps -- and equal with host work between calls:
//  profiles/r04_dropin_zc_ab.jsonl; the bound stays 2^16)
static int64_t mt_zero_copy_words(const bcmpc_engine*) {
    const char* v = std::getenv("BCMPC_MT_ZC_WORDS");
    if (v && *v) return std::max<int64_t>(0, std::atoll(v));
    return int64_t(1) << 16;
}

static bool mt_device_path() {
    const char* v = std::getenv("BCMPC_MT_PATH");
    return !(v && std::strcmp(v, "host") == 0);
}

// The draw's chunks for this engine's shard of [H, k_global, A]: the shard's rows of step h are the
// draw words [2A (h kg + off), 2A (h kg + off + K)) (one run; all steps merge into one when the shard
// is the whole draw), each run cut into pieces of <= mt_chunk_words(..) words; the chunk that draws
// the draw's last word also leaves NumPy's final state, else one extra chunk draws that word alone.
static int mt_plan(bcmpc_engine* e, int64_t kg, int64_t off) {
    if (e->mt_kg == kg && e->mt_off == off) return BCMPC_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));         // (a queued speculative draw may still read the old plan)
    if (e->spec_st) HIP_TRY(hipStreamSynchronize(e->spec_st));
    if (e->d_spec_part) (void)hipFree(e->d_spec_part);
    e->d_spec_part = nullptr;
    const int64_t K = e->cfg.num_paths, A = e->cfg.action_dim, H = e->cfg.horizon;
    const int64_t N = 2 * A * H * kg;
    struct Run { int64_t s, len, out0; };
    std::vector<Run> runs;
    if (off == 0 && K == kg) runs.push_back({0, N, 0});
    else
        for (int64_t h = 0; h < H; ++h) runs.push_back({2 * A * (h * kg + off), 2 * A * K, h * K * A});
    const int64_t target = mt_chunk_words(2 * A * H * K);
    std::vector<MtChunk> ch;
    bool has_final = false;
    for (const Run& r : runs) {
        const int64_t R = r.len / 2, P = std::max<int64_t>(1, (r.len + target - 1) / target);
        for (int64_t p = 0; p < P; ++p) {
            const int64_t d0 = R * p / P, d1 = R * (p + 1) / P;
            if (d1 <= d0) continue;
            MtChunk c{};
            c.s = r.s + 2 * d0;
            c.n = 2 * (d1 - d0);
            c.out0 = r.out0 + d0;
            c.f = (int32_t)(c.s / kMtN);
            c.j0 = (int32_t)((c.s / 2) % A);
            c.final_ = c.s + c.n == N;
            has_final |= c.final_ != 0;
            ch.push_back(c);
        }
    }
    if (!has_final) {
        MtChunk c{};
        c.s = N - 2; c.n = 2; c.out0 = -1; c.f = (int32_t)((N - 2) / kMtN); c.final_ = 1;
        ch.push_back(c);
    }
    std::vector<int64_t> fs;
    for (MtChunk& c : ch) {
        c.jidx = -1;
        if (c.f >= 2) { c.jidx = (int32_t)fs.size(); fs.push_back(c.f); }
    }
    const int cj = (int)fs.size(), S = mt_splits(cj);
    std::vector<uint32_t> polys((size_t)std::max(1, cj) * kMtPolyWords, 0);
    if (cj) mt_block_polys(fs, polys.data());
    for (void* p : {(void*)e->d_mt_polys, (void*)e->d_mt_chunks, (void*)e->d_mt_part})
        if (p) (void)hipFree(p);
    e->d_mt_polys = nullptr; e->d_mt_chunks = nullptr; e->d_mt_part = nullptr;
    e->mt_kg = e->mt_off = -1;
    if (!e->d_mt_io) {
        HIP_TRY(hipMalloc(&e->d_mt_io, 1280 * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&e->d_mt_bounds, 2 * BCMPC_MAX_ACTION * sizeof(double)));
        HIP_TRY(hipMalloc(&e->d_mt_xs, (size_t)kMtStream * sizeof(uint32_t)));
        HIP_TRY(hipHostMalloc(&e->h_mt_io, 1280 * sizeof(uint32_t) + 2 * BCMPC_MAX_ACTION * sizeof(double),
                              hipHostMallocDefault));
    }
    HIP_TRY(hipMalloc(&e->d_mt_polys, polys.size() * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&e->d_mt_chunks, ch.size() * sizeof(MtChunk)));
    HIP_TRY(hipMalloc(&e->d_mt_part, (size_t)std::max(1, cj) * S * kMtN * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&e->d_spec_part, (size_t)std::max(1, cj) * S * kMtN * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(e->d_mt_polys, polys.data(), polys.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_mt_chunks, ch.data(), ch.size() * sizeof(MtChunk), hipMemcpyHostToDevice));
    e->mt_nchunks = (int32_t)ch.size();
    e->mt_cj = cj;
    e->mt_s = S;
    e->mt_kg = kg;
    e->mt_off = off;
    return BCMPC_OK;
}

// enqueue the draw of this shard's [H, K, A] from NumPy's state (key, pos) into e->d_actions and the
// final state into d_mt_io[640..1265) (copied back by the caller after its sync)
static int mt_draw_enqueue(bcmpc_engine* e, const uint32_t* mt_key, int32_t pos, const double* low,
                           const double* high, int64_t kg, int64_t off) {
    int rc = mt_plan(e, kg, off);
    if (rc != BCMPC_OK) return rc;
    rc = actions_buffer(e);
    if (rc != BCMPC_OK) return rc;
    const int A = e->cfg.action_dim;
    std::memcpy(e->h_mt_io, mt_key, kMtN * sizeof(uint32_t));
    e->h_mt_io[kMtN] = (uint32_t)pos;
    double* hb = reinterpret_cast<double*>(e->h_mt_io + 1280);
    for (int j = 0; j < A; ++j) { hb[j] = low[j]; hb[A + j] = high[j]; }
    HIP_TRY(hipMemcpyAsync(e->d_mt_io, e->h_mt_io, (kMtN + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_mt_bounds, hb, 2 * A * sizeof(double), hipMemcpyHostToDevice, e->stream));
    MtDrawArgs a{};
    a.in = e->d_mt_io;
    a.bounds = e->d_mt_bounds;
    a.xs = e->d_mt_xs;
    a.polys = e->d_mt_polys;
    a.chunks = e->d_mt_chunks;
    a.part = e->d_mt_part;
    a.final_state = e->d_mt_io + 640;
    a.out = e->d_actions;
    a.nchunks = e->mt_nchunks; a.Cj = e->mt_cj; a.S = e->mt_s; a.A = A;
    HIP_TRY(launch_mt_draw(a, e->stream));
    HIP_TRY(hipMemcpyAsync(e->h_mt_io + 640, e->d_mt_io + 640, (kMtN + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           e->stream));
    return BCMPC_OK;
}

static bool mt_speculate() {
    static const bool on = [] {
        const char* v = std::getenv("BCMPC_MT_SPECULATE");
        return !(v && v[0] == '0');
    }();
    return on;
}
constexpr int kSpecPause = 32;

// the main stream waits for a speculative draw still running beside it (its slots, its input -- the final
// state of the draw before it -- and the MT scratch are read or rewritten by what follows)
static int spec_join(bcmpc_engine* e) {
    if (!e->spec_side_pending) return BCMPC_OK;
    HIP_TRY(hipStreamWaitEvent(e->stream, e->spec_done_ev, 0));
    e->spec_side_pending = false;
    return BCMPC_OK;
}

// enqueue the speculative draw of the next call's rows into spec slot `slot`: from the device-resident
// final state `in` of the draw just enqueued, same bounds and shard (mt_plan is the current one)
static int mt_spec_enqueue(bcmpc_engine* e, const uint32_t* in, int slot, const double* low, const double* high,
                           bool side) {
    const bcmpc_config& c = e->cfg;
    const int A = c.action_dim;
    const size_t n = (size_t)c.horizon * (size_t)c.num_paths * (size_t)A;
    if (n > e->spec_cap) {
        for (auto& sp : e->spec) {
            if (sp.d_act) (void)hipFree(sp.d_act);
            sp.d_act = nullptr;
        }
        e->spec_cap = 0;
        for (auto& sp : e->spec) HIP_TRY(hipMalloc(&sp.d_act, n * sizeof(double)));
        e->spec_cap = n;
    }
    auto& sp = e->spec[slot];
    const size_t io_bytes = 640 * sizeof(uint32_t) + 2 * BCMPC_MAX_ACTION * sizeof(double);
    if (!sp.d_io) {
        HIP_TRY(hipMalloc(&sp.d_io, io_bytes));
        HIP_TRY(hipHostMalloc(&sp.h_io, io_bytes, hipHostMallocDefault));
    }
    hipStream_t st = e->stream;
    if (side) {                                   // beside this call's rollout, after its draw
        if (!e->spec_st) {
            HIP_TRY(hipStreamCreateWithFlags(&e->spec_st, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&e->spec_in_ev, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&e->spec_done_ev, hipEventDisableTiming));
        }
        if (!e->d_spec_xs) HIP_TRY(hipMalloc(&e->d_spec_xs, (size_t)kMtStream * sizeof(uint32_t)));
        HIP_TRY(hipEventRecord(e->spec_in_ev, e->stream));
        HIP_TRY(hipStreamWaitEvent(e->spec_st, e->spec_in_ev, 0));
        st = e->spec_st;
    }
    // (the slot's staging is rewritten two calls later at the earliest: its copy has run by then)
    double* hb = reinterpret_cast<double*>(sp.h_io + 640);
    for (int j = 0; j < A; ++j) { hb[j] = low[j]; hb[A + j] = high[j]; }
    HIP_TRY(hipMemcpyAsync(sp.d_io + 640, hb, 2 * A * sizeof(double), hipMemcpyHostToDevice, st));
    MtDrawArgs a{};
    a.in = in;
    a.bounds = reinterpret_cast<const double*>(sp.d_io + 640);
    a.xs = side ? e->d_spec_xs : e->d_mt_xs;
    a.polys = e->d_mt_polys;
    a.chunks = e->d_mt_chunks;
    a.part = side ? e->d_spec_part : e->d_mt_part;
    a.final_state = sp.d_io;
    a.out = sp.d_act;
    a.nchunks = e->mt_nchunks; a.Cj = e->mt_cj; a.S = e->mt_s; a.A = A;
    HIP_TRY(launch_mt_draw(a, st));
    HIP_TRY(hipMemcpyAsync(sp.h_io, sp.d_io, (kMtN + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (side) {
        HIP_TRY(hipEventRecord(e->spec_done_ev, st));
        e->spec_side_pending = true;
    }
    return BCMPC_OK;
}

int bcmpc_get_action_mt19937(bcmpc_engine* e, const double* state, uint32_t* mt_key, int32_t* mt_pos,
                             const double* low, const double* high, int64_t k_global, int64_t cand_offset,
                             uint64_t seed, bcmpc_result* out, double* costs_out) {
    if (!e || !state || !mt_key || !mt_pos || !low || !high || !out) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (c.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "get_action needs a fused objective (cheetah cost or learned reward)");
    if (c.cost == BCMPC_COST_TERMS)
        return fail(BCMPC_ERR_UNSUPPORTED, "the NumPy-stream draw does not cover cost-term engines: draw on the host "
                                           "and pass the array to bcmpc_get_action");
    if (e->has_value)
        return fail(BCMPC_ERR_UNSUPPORTED, "the NumPy-stream draw does not cover engines with a terminal value: draw on "
                                           "the host and pass the array to bcmpc_get_action");
    if (k_global < c.num_paths || cand_offset < 0 || cand_offset + c.num_paths > k_global)
        return fail(BCMPC_ERR_ARG, "this engine's candidates must lie inside [0, k_global)");
    if (*mt_pos < 0 || *mt_pos > 624) return fail(BCMPC_ERR_ARG, "MT19937 position out of range");
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(e);
    const int64_t draw_words = 2 * (int64_t)c.action_dim * c.horizon * k_global;
    // MPCcontrollerPolicyNet with self_exp=True draws its exploration array (controllers.py:191) but rolls out
    // the policy's own samples (:202-203): only NumPy's state has to advance, no row is read
    const bool rows_needed = !(e->PL > 0 && c.policy_mode == BCMPC_POLICY_STOCHASTIC);
    if ((draw_words <= mt_zero_copy_words(e) || !rows_needed) && mt_device_path()) {
        // small draw: the host generates the shard's rows of every step into pinned memory (the
        // reference's own draw order), the kernel reads them in place; state in the kernel
        // arguments, result into mapped memory, one spin -- no copy either way
        const int64_t K = c.num_paths;
        const int A = c.action_dim, H = c.horizon;
        const size_t row = (size_t)K * A, n = (size_t)H * row;
        const bool predraw = mt_predraw_enabled();
        Mt19937 g;
        std::memcpy(g.key, mt_key, sizeof(g.key));
        g.pos = *mt_pos;
        auto same_job = [&] {                         // the posted job draws exactly this call's rows
            const auto& p = e->pre;
            return p.rows == rows_needed && p.kg == k_global && p.off == cand_offset && g.pos == p.from.pos &&
                   std::memcmp(g.key, p.from.key, sizeof(g.key)) == 0 &&
                   std::memcmp(low, p.low.data(), sizeof(double) * A) == 0 &&
                   std::memcmp(high, p.high.data(), sizeof(double) * A) == 0;
        };
        // late hit (team kernel): the worker is still drawing this call's rows (a caller with no host work
        // between calls) -- launch now, the kernel waits for the rows' sequence word instead of the host
        // waiting for the worker (the job's parameters are written only by this thread, in predraw_post)
        // (not with a communicator attached: a kernel that gave up waiting would have run the exchange on
        //  unpublished rows, and the ranks cannot rerun one step alone -- the host waits for the worker)
        const bool late = predraw && mt_predraw_late() && e->kernel == BCMPC_KERNEL_TEAM && e->h_rows_seq && !e->comm &&
                          n <= e->zc_cap && e->pre.inflight.load(std::memory_order_acquire) && same_job();
        if (late) e->pre.claimed.store(true, std::memory_order_release);
        // (otherwise no pre-draw is running past this point: the worker finishes its job before the buffers
        //  change)
        int b = late ? e->pre.buf : predraw_wait(e);
        if (!late && n > e->zc_cap) {
            // fine-grained host memory: no GPU cache keeps an earlier call's rows (the rows change every call)
            for (int i = 0; i < 2; ++i) {
                if (e->h_zc[i]) (void)hipHostFree(e->h_zc[i]);
                e->h_zc[i] = nullptr;
                e->d_zc[i] = nullptr;
            }
            e->zc_cap = 0;
            e->pre.ready = false;
            for (int i = 0; i < 2; ++i) {
                HIP_TRY(hipHostMalloc(&e->h_zc[i], n * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
                HIP_TRY(hipHostGetDevicePointer((void**)&e->d_zc[i], e->h_zc[i], 0));
            }
            if (mt_predraw_dev()) {
                if (!e->copy_st) {
                    HIP_TRY(hipStreamCreateWithFlags(&e->copy_st, hipStreamNonBlocking));
                    for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&e->copy_ev[i], hipEventDisableTiming));
                }
                for (int i = 0; i < 2; ++i) {
                    if (e->d_rows[i]) (void)hipFree(e->d_rows[i]);
                    e->d_rows[i] = nullptr;
                    e->copy_valid[i] = false;
                    HIP_TRY(hipMalloc(&e->d_rows[i], n * sizeof(double)));
                }
            }
            if (!e->h_rows_seq) {
                HIP_TRY(hipHostMalloc(&e->h_rows_seq, sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
                HIP_TRY(hipHostGetDevicePointer((void**)&e->d_rows_seq, e->h_rows_seq, 0));
                __atomic_store_n(e->h_rows_seq, 0u, __ATOMIC_RELEASE);
            }
            e->zc_cap = n;
        }
        const bool hit = !late && predraw && e->pre.ready && same_job();
        if (!late) e->pre.ready = false;
        const double* rows_ptr = nullptr;
        if (late) {                                   // the kernel reads the pinned rows once published
            if (rows_needed) {
                rows_ptr = e->d_zc[b];
                e->rows_wait_seq = e->pre.job;
            }
            ++e->pre.hits;
            ++e->pre.late;
        } else if (hit) {                                    // NumPy's stream is exactly where the worker drew from
            b = e->pre.buf;
            g = e->pre.to;
            ++e->pre.hits;
            // (its device copy, when it has landed: the kernel then reads HBM instead of the bus)
            // (the stream wait orders and publishes the copy for the kernel; it has already completed)
            if (rows_needed && e->copy_valid[b] && hipEventQuery(e->copy_ev[b]) == hipSuccess &&
                hipStreamWaitEvent(e->stream, e->copy_ev[b], 0) == hipSuccess)
                rows_ptr = e->d_rows[b];
        } else {
            b = e->zc_last ^ 1;
            if (predraw) ++e->pre.misses;
            if (rows_needed && cand_offset == 0 && K == k_global)   // the whole draw: one pass
                mt_uniform_rows(g, low, high, A, (int64_t)H * k_global, 0, (int64_t)H * k_global, e->h_zc[b]);
            else if (rows_needed)
                for (int h = 0; h < H; ++h)
                    mt_uniform_rows(g, low, high, A, k_global, cand_offset, cand_offset + K, e->h_zc[b] + h * row);
            else
                g.advance(draw_words);
        }
        const bool lean = e->comm == nullptr;
        if (!lean)
            HIP_TRY(hipMemcpyAsync(e->d_state, state, sizeof(double) * c.state_dim, hipMemcpyHostToDevice, e->stream));
        e->want_done = lean && !costs_out;
        if (!rows_ptr && rows_needed) rows_ptr = e->d_zc[b];
        if (!late) e->copy_valid[b] = false;          // (the next fill of this buffer replaces it)
        RolloutLaunch r;
        if (lean) r.state_inline = state; else r.state = e->d_state;
        r.actions = rows_ptr; r.seed = seed; r.cand_offset = cand_offset; r.costs = e->d_costs;
        r.result = lean ? e->d_result_map : e->d_result; r.stream = e->stream;
        int rc = rollout_impl(e, r);
        e->rows_wait_seq = 0;
        // the next call's rows start at once, while this call's rollout runs (round 4; the worker is idle
        // here unless this call claimed its in-flight job late).  They start from NumPy's state after this
        // call's draw: a rerun on the fallback engine consumes the same draw, and a call that fails leaves
        // NumPy's state unadvanced, so the next call misses them (same_job) and draws afresh
        const bool posted_early = predraw && !late && rc == BCMPC_OK;
        if (posted_early) {
            e->zc_last = b;
            predraw_post(e, g, low, high, A, k_global, cand_offset, rows_needed);
        }
        const bool spin = e->want_done && rc == BCMPC_OK;
        e->want_done = false;
        if (rc == BCMPC_OK && !lean &&
            hipMemcpyAsync(e->h_result, e->d_result, sizeof(bcmpc_result), hipMemcpyDeviceToHost, e->stream) != hipSuccess)
            rc = fail(BCMPC_ERR_HIP, "result copy failed");
        if (rc == BCMPC_OK && costs_out &&
            hipMemcpyAsync(costs_out, e->d_costs, sizeof(double) * c.num_paths, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
            rc = fail(BCMPC_ERR_HIP, "costs copy failed");
        if (spin) {
            if (const int wr = wait_done(e, e->seq)) return wr;
        } else {
            if (e->comm && rc == BCMPC_OK) {                // (bounded: the exchange's peers)
                if (const int sr = sync_step(e, e->stream)) return sr;
            } else {
                const hipError_t se = hipStreamSynchronize(e->stream);   // (also on error: the kernel reads h_zc)
                if (rc != BCMPC_OK) return rc;
                if (se != hipSuccess) return fail(BCMPC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
            }
        }
        if (late) {                                   // (the job is finished: the kernel has read its rows)
            predraw_wait(e);
            g = e->pre.to;
            e->pre.ready = false;
        }
        if (step_failed(e)) {                         // (NumPy's state not yet advanced)
            bcmpc_engine* re = nullptr;
            if (const int fr = rerun_engine(e, &re)) return fr;
            return bcmpc_get_action_mt19937(re, state, mt_key, mt_pos, low, high, k_global, cand_offset, seed,
                                            out, costs_out);
        }
        std::memcpy(mt_key, g.key, sizeof(g.key));
        *mt_pos = g.pos;
        *out = lean ? *e->h_result_map : *e->h_result;
        e->zc_last = b;
        if (predraw && !posted_early) predraw_post(e, g, low, high, A, k_global, cand_offset, rows_needed);
        return BCMPC_OK;
    }
    if (mt_device_path()) {
        // the draw on the device: state + (key, pos) up, draw, rollout, argmin, result + final state down,
        // one synchronisation.  NumPy's state is handed back only when the whole call succeeded.
        const bool lean = e->comm == nullptr;         // (as bcmpc_get_action)
        if (!lean)
            HIP_TRY(hipMemcpyAsync(e->d_state, state, sizeof(double) * c.state_dim, hipMemcpyHostToDevice, e->stream));
        const int A = c.action_dim;
        // the previous call's speculative draw, when it starts exactly where NumPy's stream is
        const bool shit = e->spec_armed && e->spec_kg == k_global && e->spec_off == cand_offset &&
                          e->spec_pos == *mt_pos && std::memcmp(e->spec_key, mt_key, sizeof(e->spec_key)) == 0 &&
                          std::memcmp(e->spec_low, low, sizeof(double) * A) == 0 &&
                          std::memcmp(e->spec_high, high, sizeof(double) * A) == 0;
        if (e->spec_armed) {
            if (shit) {
                ++e->spec_hits;
                e->spec_miss_run = 0;
            } else {
                ++e->spec_misses;
                if (++e->spec_miss_run >= 2) {
                    e->spec_pause = kSpecPause;
                    e->spec_miss_run = 0;
                }
            }
        }
        e->spec_armed = false;
        const int cur = e->spec_slot;
        if (const int jr = spec_join(e)) return jr;
        int rc = shit ? BCMPC_OK : mt_draw_enqueue(e, mt_key, *mt_pos, low, high, k_global, cand_offset);
        // (the final-state copy was enqueued before the rollout: the argmin's done word implies it)
        const uint32_t* fin_d = shit ? e->spec[cur].d_io : e->d_mt_io + 640;
        const uint32_t* fin_h = shit ? e->spec[cur].h_io : e->h_mt_io + 640;
        e->want_done = lean && !costs_out;
        // the next call's draw: slab-kernel engines whose grid leaves CUs free (K <= 32 per CU: cfg2's 4096)
        // draw it beside this rollout (on spec_st, from this draw's final state); the others behind the argmin
        // -- a team's grid needs every CU it was given, and at cfg3 (1024 workgroups) a draw beside the
        // rollout delays it by more than it hides (profiles/r03_spec2_ab.txt)
        int nslot = -1;
        const bool speculate = rc == BCMPC_OK && e->want_done && mt_speculate();
        const bool side = e->kernel != BCMPC_KERNEL_TEAM && e->ncu > 0 && c.num_paths <= 32 * (int64_t)e->ncu;
        bool paused = false;
        if (speculate && e->spec_pause > 0) {
            --e->spec_pause;
            paused = true;
        } else if (speculate && side) {
            nslot = shit ? cur ^ 1 : 0;
            if (mt_plan(e, k_global, cand_offset) != BCMPC_OK || mt_spec_enqueue(e, fin_d, nslot, low, high, true) != BCMPC_OK)
                nslot = -1;
        }
        RolloutLaunch r;
        if (lean) r.state_inline = state; else r.state = e->d_state;
        r.actions = shit ? e->spec[cur].d_act : e->d_actions; r.seed = seed; r.cand_offset = cand_offset;
        r.costs = e->d_costs; r.result = lean ? e->d_result_map : e->d_result; r.stream = e->stream;
        if (rc == BCMPC_OK) rc = rollout_impl(e, r);
        const bool spin = e->want_done && rc == BCMPC_OK;
        e->want_done = false;
        // team engines: the next call's draw behind this call's argmin (a spinning call returns at the done
        // word, so the draw runs while the caller steps its env); not when the call synchronises the stream
        // (a hit skipped mt_plan: another shard / size drawn in between may have replaced the plan)
        if (spin && speculate && !side && !paused) {
            nslot = shit ? cur ^ 1 : 0;
            if (mt_plan(e, k_global, cand_offset) != BCMPC_OK ||
                mt_spec_enqueue(e, fin_d, nslot, low, high, false) != BCMPC_OK)
                nslot = -1;
        }
        if (!spin) nslot = -1;
        if (rc == BCMPC_OK && !lean &&
            hipMemcpyAsync(e->h_result, e->d_result, sizeof(bcmpc_result), hipMemcpyDeviceToHost, e->stream) != hipSuccess)
            rc = fail(BCMPC_ERR_HIP, "result copy failed");
        if (rc == BCMPC_OK && costs_out &&
            hipMemcpyAsync(costs_out, e->d_costs, sizeof(double) * c.num_paths, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
            rc = fail(BCMPC_ERR_HIP, "costs copy failed");
        if (spin) {
            if (const int wr = wait_done(e, e->seq)) return wr;
        } else {
            if (e->comm && rc == BCMPC_OK) {                // (bounded: the exchange's peers)
                if (const int sr = sync_step(e, e->stream)) return sr;
            } else {
                const hipError_t se = hipStreamSynchronize(e->stream);   // (also on error: nothing left in flight)
                if (rc != BCMPC_OK) return rc;
                if (se != hipSuccess) return fail(BCMPC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
            }
        }
        if (step_failed(e)) {                         // (NumPy's state not yet advanced)
            bcmpc_engine* re = nullptr;
            if (const int fr = rerun_engine(e, &re)) return fr;
            return bcmpc_get_action_mt19937(re, state, mt_key, mt_pos, low, high, k_global, cand_offset, seed,
                                            out, costs_out);
        }
        std::memcpy(mt_key, fin_h, kMtN * sizeof(uint32_t));
        *mt_pos = (int32_t)fin_h[kMtN];
        *out = lean ? *e->h_result_map : *e->h_result;
        if (nslot >= 0) {                             // armed: it starts where this call leaves NumPy
            e->spec_armed = true;
            e->spec_slot = nslot;
            std::memcpy(e->spec_key, mt_key, sizeof(e->spec_key));
            e->spec_pos = *mt_pos;
            e->spec_kg = k_global;
            e->spec_off = cand_offset;
            std::memcpy(e->spec_low, low, sizeof(double) * A);
            std::memcpy(e->spec_high, high, sizeof(double) * A);
        }
        return BCMPC_OK;
    }
    const int64_t K = c.num_paths;
    const int A = c.action_dim, H = c.horizon;
    const size_t row = (size_t)K * A, n = (size_t)H * row;
    if (const int br = actions_buffer(e)) return br;
    if (n > e->stage_cap) {                      // pinned staging: the generator writes, the DMA reads
        if (e->h_stage) (void)hipHostFree(e->h_stage);
        e->h_stage = nullptr;
        e->stage_cap = 0;
        HIP_TRY(hipHostMalloc(&e->h_stage, n * sizeof(double), hipHostMallocDefault));
        e->stage_cap = n;
    }
    HIP_TRY(hipMemcpyAsync(e->d_state, state, sizeof(double) * c.state_dim, hipMemcpyHostToDevice, e->stream));
    Mt19937 g;
    std::memcpy(g.key, mt_key, sizeof(g.key));
    g.pos = *mt_pos;
    // Large draws: the stream split over host threads by jump-ahead (mt_jump.cpp); each thread
    // copies its own slice as soon as it is drawn.  Otherwise [H, k_global, A] in C order, one
    // step at a time, the drawn steps copied while the next ones are drawn.
    int chunk_rc = 0;
    auto copy_chunk = [&](int64_t o_lo, int64_t o_hi) -> int {
        return hipMemcpyAsync(e->d_actions + o_lo, e->h_stage + o_lo, (size_t)(o_hi - o_lo) * sizeof(double),
                              hipMemcpyHostToDevice, e->stream) == hipSuccess ? 0 : 1;
    };
    if (mt_uniform_rows_par(g, low, high, A, (int64_t)H * k_global, k_global, cand_offset, cand_offset + K,
                            e->h_stage, mt_default_threads(), mt_min_words(), copy_chunk, &chunk_rc) > 0) {
        if (chunk_rc) {
            (void)hipStreamSynchronize(e->stream);     // slices already enqueued still read the staging buffer
            return fail(BCMPC_ERR_HIP, "hipMemcpyAsync of a drawn action slice failed");
        }
    } else {
        // copies go out in pieces of >= 2 MiB (one per call for small draws: each copy costs ~5-10 us
        // of runtime overhead)
        constexpr size_t kPiece = size_t(1) << 18;   // doubles
        int h_sent = 0;
        for (int h = 0; h < H; ++h) {
            mt_uniform_rows(g, low, high, A, k_global, cand_offset, cand_offset + K, e->h_stage + h * row);
            if ((size_t)(h + 1 - h_sent) * row >= kPiece || h + 1 == H) {
                const hipError_t ce = hipMemcpyAsync(e->d_actions + h_sent * row, e->h_stage + h_sent * row,
                                                     (size_t)(h + 1 - h_sent) * row * sizeof(double),
                                                     hipMemcpyHostToDevice, e->stream);
                if (ce != hipSuccess) {
                    (void)hipStreamSynchronize(e->stream);   // (earlier pieces still read the staging buffer)
                    return fail(BCMPC_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(ce));
                }
                h_sent = h + 1;
            }
        }
    }
    RolloutLaunch r;
    r.state = e->d_state; r.actions = e->d_actions; r.seed = seed; r.cand_offset = cand_offset;
    r.costs = e->d_costs; r.result = e->d_result; r.stream = e->stream;
    int rc = rollout_impl(e, r);
    if (rc == BCMPC_OK &&
        hipMemcpyAsync(e->h_result, e->d_result, sizeof(bcmpc_result), hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        rc = fail(BCMPC_ERR_HIP, "result copy failed");
    if (rc == BCMPC_OK && costs_out &&
        hipMemcpyAsync(costs_out, e->d_costs, sizeof(double) * K, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        rc = fail(BCMPC_ERR_HIP, "costs copy failed");
    // (also on error: the staging buffer's copies are done before it can be reused)
    if (e->comm && rc == BCMPC_OK) {                // (bounded: the exchange's peers)
        if (const int sr = sync_step(e, e->stream)) return sr;
    } else {
        const hipError_t se = hipStreamSynchronize(e->stream);
        if (rc != BCMPC_OK) return rc;
        if (se != hipSuccess) return fail(BCMPC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    }
    if (step_failed(e)) {
        bcmpc_engine* re = nullptr;
        if (const int fr = rerun_engine(e, &re)) return fr;
        return bcmpc_get_action_mt19937(re, state, mt_key, mt_pos, low, high, k_global, cand_offset, seed, out,
                                        costs_out);
    }
    std::memcpy(mt_key, g.key, sizeof(g.key));      // NumPy's state advances only when the call succeeded
    *mt_pos = g.pos;
    *out = *e->h_result;
    return BCMPC_OK;
}

int bcmpc_mt19937_uniform_device(bcmpc_engine* e, uint32_t* mt_key, int32_t* mt_pos, const double* low,
                                 const double* high, int64_t k_global, int64_t cand_offset, double* out) {
    if (!e || !mt_key || !mt_pos || !low || !high || !out) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (c.num_paths < 1 || k_global < c.num_paths || cand_offset < 0 || cand_offset + c.num_paths > k_global)
        return fail(BCMPC_ERR_ARG, "this engine's candidates must lie inside [0, k_global)");
    if (*mt_pos < 0 || *mt_pos > 624) return fail(BCMPC_ERR_ARG, "MT19937 position out of range");
    HIP_TRY(hipSetDevice(c.device));
    if (const int jr = spec_join(e)) return jr;
    int rc = mt_draw_enqueue(e, mt_key, *mt_pos, low, high, k_global, cand_offset);
    const size_t n = (size_t)c.horizon * c.num_paths * c.action_dim;
    if (rc == BCMPC_OK &&
        hipMemcpyAsync(out, e->d_actions, n * sizeof(double), hipMemcpyDeviceToHost, e->stream) != hipSuccess)
        rc = fail(BCMPC_ERR_HIP, "action copy failed");
    if (e->comm && rc == BCMPC_OK) {                // (bounded: the exchange's peers)
        if (const int sr = sync_step(e, e->stream)) return sr;
    } else {
        const hipError_t se = hipStreamSynchronize(e->stream);
        if (rc != BCMPC_OK) return rc;
        if (se != hipSuccess) return fail(BCMPC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    }
    std::memcpy(mt_key, e->h_mt_io + 640, kMtN * sizeof(uint32_t));
    *mt_pos = (int32_t)e->h_mt_io[640 + kMtN];
    return BCMPC_OK;
}

int bcmpc_mt19937_uniform(uint32_t* mt_key, int32_t* mt_pos, const double* low, const double* high,
                          int32_t action_dim, int64_t n_rows, double* out) {
    if (!mt_key || !mt_pos || !low || !high || !out || action_dim < 1 || n_rows < 0)
        return fail(BCMPC_ERR_ARG, "bad argument");
    if (*mt_pos < 0 || *mt_pos > 624) return fail(BCMPC_ERR_ARG, "MT19937 position out of range");
    Mt19937 g;
    std::memcpy(g.key, mt_key, sizeof(g.key));
    g.pos = *mt_pos;
    mt_uniform_rows(g, low, high, action_dim, n_rows, 0, n_rows, out);
    std::memcpy(mt_key, g.key, sizeof(g.key));
    *mt_pos = g.pos;
    return BCMPC_OK;
}

int bcmpc_mt19937_uniform_par(uint32_t* mt_key, int32_t* mt_pos, const double* low, const double* high,
                              int32_t action_dim, int64_t n_rows, int64_t period, int64_t keep_lo, int64_t keep_hi,
                              double* out, int32_t threads, int64_t min_words_per_thread, int32_t* used_threads) {
    if (!mt_key || !mt_pos || !low || !high || !out || action_dim < 1 || n_rows < 0 ||
        period < 1 || keep_lo < 0 || keep_hi > period || keep_lo >= keep_hi || n_rows % period)
        return fail(BCMPC_ERR_ARG, "bad argument");
    if (*mt_pos < 0 || *mt_pos > 624) return fail(BCMPC_ERR_ARG, "MT19937 position out of range");
    Mt19937 g;
    std::memcpy(g.key, mt_key, sizeof(g.key));
    g.pos = *mt_pos;
    if (threads <= 0) threads = mt_default_threads();
    if (min_words_per_thread < 0) min_words_per_thread = mt_min_words();
    const int used = mt_uniform_rows_par(g, low, high, action_dim, n_rows, period, keep_lo, keep_hi, out, threads,
                                         min_words_per_thread, nullptr, nullptr);
    const bool par = used > 0;
    if (!par) {
        const int64_t kw = keep_hi - keep_lo;
        for (int64_t p = 0; p < n_rows / period; ++p)
            mt_uniform_rows(g, low, high, action_dim, period, keep_lo, keep_hi, out + p * kw * action_dim);
    }
    if (used_threads) *used_threads = par ? used : 1;
    std::memcpy(mt_key, g.key, sizeof(g.key));
    *mt_pos = g.pos;
    return BCMPC_OK;
}

}  // extern "C"
