// bnpc_mhbatch.cpp - the parameter batch with the device screen in front
// (bnpc_mh_batch_dev and the calls that fuse it with the counts), and the
// walker that takes a batch's draws ahead on the aside thread.  The pinned
// block (MHPin, bnpc_ctx.h) is read and written in place by k_mh_screen,
// launched by mh_screen_launch in bnpc_kernels.hip.

#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <functional>
#include <vector>
#include <algorithm>

#include "bnpc_ctx.h"

static size_t mh_pin_offsets(size_t E, size_t off[6])
{
    const size_t Ea = (E + 15) & ~(size_t)15;
    off[0] = 0;
    off[1] = off[0] + Ea * 8;
    off[2] = off[1] + Ea * 8;
    off[3] = off[2] + Ea * 4;
    off[4] = off[3] + Ea * 4;
    off[5] = off[4] + Ea * 4;
    return off[5] + Ea;
}

// ---- draws taken AHEAD ------------------------------
// The draws of a parameter batch - choice(sd, M), M uniforms, M uniforms per
// cluster, cluster by cluster (libs/CRP.py:328-335) - depend on nothing but
// the position of the stream, and rank 0's walk through them paces a large
// batch (0.5 ms of config 5's 0.9 ms parameter phase) while the same thread
// idles 0.9 ms in front of the sweep's kernel.  So the step posts a WALKER on
// the aside thread as soon as the stream's way to the batch is known (after a
// sweep's permutation: one uniform per cell, the alpha test; in a move: after
// its last variable draw): on a private COPY of the stream it goes that way
// (`prelude`), notes the state it arrives with (`start`) and draws rows
// straight into the pinned block, publishing row after row.  The batch adopts
// them iff the live stream stands exactly at `start` when it begins - any
// birth, any other draw, any difference makes the two states differ, and the
// walker's work is dropped (the live stream was never touched).  Same bits
// by construction: the same generator from the same state.  A batch with
// more rows than the walker took draws the rest itself, one with fewer
// continues from the state kept after its last row.
struct MhAhead {
    // set by the thread that posts the walker
    bnpc_mt19937 rng;               // the walker's private stream
    bnpc_legacy_gauss gauss;
    std::function<bool(bnpc_mt19937 *, bnpc_legacy_gauss *)> prelude;
    int64_t rows = 0, M = 0, n_sd = 0;
    MHPin h;
    bool active = false;            // posted and not yet taken or dropped
    // written by the walker
    std::atomic<int> start_known{0};    // 1: `start` holds; -1: no way known
    bnpc_mt19937 start;
    std::atomic<int64_t> rows_ready{0};
    std::vector<bnpc_mt19937> after_row;
    std::atomic<int> cancel{0};
};

static inline void mt_canonical(bnpc_mt19937 &s)
{
    if (s.pos >= 624) mt_refill(&s);
}

static bool mt_same_position(const bnpc_mt19937 &a, const bnpc_mt19937 &b)
{
    bnpc_mt19937 x = a, y = b;
    mt_canonical(x);
    mt_canonical(y);
    return x.pos == y.pos && memcmp(x.key, y.key, sizeof x.key) == 0;
}

// the walker is stopped and forgotten (its draws were not wanted)
static void mh_ahead_drop(bnpc_ctx *c)
{
    MhAhead *ah = c->ahead;
    if (!ah || !ah->active) return;
    ah->cancel.store(1, std::memory_order_release);
    bnpc_aside_wait();
    ah->active = false;
}

// A batch of G rows claims a walker's rows: they are kept iff the batch fits
// them (`fits`: the caller's conditions, then stream, M and n_sd) and the live
// stream stands exactly where the walker's stood when it began to draw.
// Returns the number adopted (counted on the context); 0: the walker is
// dropped.
static int64_t mh_ahead_claim(bnpc_ctx *c, bool fits, const bnpc_mt19937 *rng,
                              int64_t G, int64_t M, int64_t n_sd)
{
    MhAhead *ah = c->ahead;
    if (!ah || !ah->active) return 0;
    bool ok = fits && rng && ah->M == M && ah->n_sd == n_sd
        && c->tun.mh_ahead != 3;
    if (ok) {
        int known = 0;
        bnpc_spin_until([&] {
            return (known = ah->start_known.load(std::memory_order_acquire))
                != 0;
        });
        ok = known == 1 && mt_same_position(ah->start, *rng);
    }
    if (!ok) {
        mh_ahead_drop(c);
        return 0;
    }
    const int64_t rows = std::min<int64_t>(ah->rows, G);
    c->ahead_taken++;
    c->ahead_rows_taken += rows;
    return rows;
}

// returns when the walker has published its rows up to n
static void mh_ahead_wait_rows(const MhAhead *ah, int64_t n)
{
    bnpc_spin_until([&] {
        return ah->rows_ready.load(std::memory_order_acquire) >= n;
    });
}

// A small batch (the rows of a restricted scan) takes a walker's rows whole:
// the number adopted (the live stream then stands behind them), 0 if there is
// no walker or the live stream stands elsewhere.
static int64_t mh_ahead_adopt(bnpc_ctx *c, bnpc_mt19937 *rng, int64_t G,
                              int64_t M, int64_t n_sd)
{
    const int64_t rows = mh_ahead_claim(c, true, rng, G, M, n_sd);
    if (rows) {
        mh_ahead_wait_rows(c->ahead, rows);
        *rng = c->ahead->after_row[(size_t)(rows - 1)];
        mh_ahead_drop(c);
    }
    return rows;
}

void mh_ahead_destroy(bnpc_ctx *c)
{
    mh_ahead_drop(c);
    delete c->ahead;
    c->ahead = nullptr;
}

static int mh_pin_get(bnpc_ctx *c, size_t E, MHPin &host, MHPin &dev,
                      bool keep_ahead = false)
{
    // (whoever else wants the block ends a walker that writes into it)
    if (!keep_ahead) mh_ahead_drop(c);
    size_t off[6];
    // the block is laid out for its CAPACITY in entries, not for this batch:
    // rows the walker drew for K + 1 clusters lie where a batch of K finds them
    size_t need = mh_pin_offsets(E, off);
    if (E <= c->mh_capE) need = mh_pin_offsets(c->mh_capE, off);
    if (need > c->mh_cap || E > c->mh_capE) {
        mh_ahead_drop(c);
        // the screen of a batch in flight reads this block: nothing is in
        // flight here (every screened call ends with a synchronisation)
        if (c->mh_pin) HIPCHK(hipHostFree(c->mh_pin));
        c->mh_pin = nullptr;
        c->mh_dev = nullptr;
        c->mh_cap = 0;
        // (no head room for the largest blocks: a slice of a batch beyond the
        // budget never grows)
        const size_t capE = E + (need < c->tun.mh_pin_max ? E / 4 : 0) + 64;
        const size_t cap = mh_pin_offsets(capE, off) + 4096;
        c->mh_capE = 0;
        const hipError_t e = hipHostMalloc(&c->mh_pin, cap,
                                           hipHostMallocDefault);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            // the caller evaluates the batch without the screen
            (void)hipGetLastError();
            c->mh_pin = nullptr;
            bnpc_set_error("no pinned memory for the screen of a parameter "
                           "batch (%zu bytes)", cap);
            return MH_PIN_NO_MEMORY;
        }
        HIPCHK(e);
        void *d = nullptr;
        HIPCHK(hipHostGetDevicePointer(&d, c->mh_pin, 0));
        c->mh_dev = (char *)d;
        c->mh_cap = cap;
        c->mh_capE = capE;
    }
    char *h = (char *)c->mh_pin, *d = c->mh_dev;
    host = {(double *)(h + off[0]), (double *)(h + off[1]),
            (int32_t *)(h + off[2]), (float *)(h + off[3]),
            (float *)(h + off[4]), (uint8_t *)(h + off[5])};
    dev = {(double *)(d + off[0]), (double *)(d + off[1]),
           (int32_t *)(d + off[2]), (float *)(d + off[3]),
           (float *)(d + off[4]), (uint8_t *)(d + off[5])};
    return 0;
}

// Post the walker (bnpc_internal.h).  Returns 0 whether or not one was posted
// (*posted says): no walker is never an error.
int bnpc_mh_ahead_begin(bnpc_ctx *c, const bnpc_mt19937 *rng,
                        const bnpc_legacy_gauss *g,
                        const std::function<bool(bnpc_mt19937 *,
                                                 bnpc_legacy_gauss *)> &prelude,
                        int64_t rows, int64_t M, int64_t n_sd, bool *posted,
                        int64_t min_entries)
{
    if (posted) *posted = false;
    if (!c || !rng || !g || rows < 1 || M != c->M || n_sd < 1 || n_sd > 8)
        return 0;
    const int mode = c->tun.mh_ahead;
    const int64_t E = rows * M;
    size_t off[6];
    if (min_entries < 0) min_entries = MH_AHEAD_MIN;
    if (mode == 0 || !c->tun.mh_screen || rows > MH_AHEAD_MAX_ROWS
        || E < (mode >= 2 ? MH_SCREEN_MIN : min_entries)
        || mh_pin_offsets((size_t)E, off) > c->tun.mh_pin_max
        || c->any_tile_pending())
        return 0;
    if (hipSetDevice(c->device) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (!c->ahead) c->ahead = new MhAhead();
    MHPin h, d;
    if (mh_pin_get(c, (size_t)E, h, d)) return 0;   // (drops a walker at work)
    MhAhead *ah = c->ahead;
    ah->rng = *rng;
    ah->gauss = *g;
    ah->prelude = prelude;
    ah->rows = rows;
    ah->M = M;
    ah->n_sd = n_sd;
    ah->h = h;
    ah->start_known.store(0, std::memory_order_relaxed);
    ah->rows_ready.store(0, std::memory_order_relaxed);
    ah->cancel.store(0, std::memory_order_relaxed);
    ah->after_row.resize((size_t)rows);
    const bool ok = bnpc_aside_start([ah]() {
        if (ah->prelude && !ah->prelude(&ah->rng, &ah->gauss)) {
            ah->start_known.store(-1, std::memory_order_release);
            return;
        }
        mt_canonical(ah->rng);
        ah->start = ah->rng;
        ah->start_known.store(1, std::memory_order_release);
        const int64_t M = ah->M;
        for (int64_t r = 0; r < ah->rows; r++) {
            if (ah->cancel.load(std::memory_order_acquire)) break;
            // (non-temporal stores, fenced before the row is published)
            if (bnpc_mt_mh_draws_to(&ah->rng, 1, M, ah->n_sd,
                                    ah->h.sd_idx + r * M, ah->h.U + r * M,
                                    ah->h.u + r * M, true))
                break;
            ah->after_row[(size_t)r] = ah->rng;
            ah->rows_ready.store(r + 1, std::memory_order_release);
        }
    });
    if (!ok) return 0;
    ah->active = true;
    c->ahead_begun++;
    if (posted) *posted = true;
    return 0;
}

void bnpc_mh_ahead_drop(bnpc_ctx *c)
{
    if (c) mh_ahead_drop(c);
}

// The rows of a restricted scan's parameter batch (bnpc_rg_counts_and_batch)
// taken ahead: posted by the scan when its visiting order is drawn - exactly
// `uniforms` uniforms (one per cell) lie between there and the batch.
void bnpc_mh_ahead_scan(bnpc_ctx *c, const bnpc_mt19937 *rng, int64_t uniforms,
                        int64_t rows, int64_t M, int64_t n_sd)
{
    static const bnpc_legacy_gauss no_gauss = {};
    const auto way = [uniforms](bnpc_mt19937 *r, bnpc_legacy_gauss *) {
        for (int64_t left = 2 * uniforms; left > 0;) {
            if (r->pos >= 624) mt_refill(r);
            const int64_t take = std::min<int64_t>(624 - r->pos, left);
            r->pos += (int32_t)take;
            left -= take;
        }
        return true;
    };
    bool posted = false;
    (void)bnpc_mh_ahead_begin(c, rng, &no_gauss, way, rows, M, n_sd, &posted,
                              MH_AHEAD_SCAN_MIN);
}

extern "C" int bnpc_mh_ahead_stats(bnpc_ctx *c, int64_t *begun, int64_t *taken,
                                   int64_t *rows)
{
    ARGCHK(c && begun && taken && rows, "NULL argument");
    *begun = c->ahead_begun;
    *taken = c->ahead_taken;
    *rows = c->ahead_rows_taken;
    return 0;
}
static int mh_screen_argchk(const bnpc_ctx *c, const bnpc_mh_args *a)
{
    ARGCHK(c && a, "NULL argument");
    ARGCHK(a->G > 0 && a->M == c->M, "batch shape does not match the context");
    ARGCHK(a->old_theta && a->sd && a->n_sd >= 1 && a->n_sd <= 8 && a->sd_idx
           && a->U && a->u, "NULL argument");
    ARGCHK(a->FP > 0.0 && a->FP < 1.0 && a->FN > 0.0 && a->FN < 1.0,
           "error rates must lie in (0, 1)");
    return 0;
}

extern "C" int bnpc_mh_screen(bnpc_ctx *c, int counts_src,
                              const bnpc_mh_args *a, uint8_t *flags,
                              float *new32)
{
    if (int rc = mh_screen_argchk(c, a)) return rc;
    ARGCHK(flags, "flags is NULL");
    HIPCHK(hipSetDevice(c->device));
    const size_t E = (size_t)a->G * a->M;
    MHPin h, d;
    if (mh_pin_get(c, E, h, d)) return 1;
    memcpy(h.U, a->U, E * 8);
    memcpy(h.u, a->u, E * 8);
    memcpy(h.sd_idx, a->sd_idx, E * 4);
    memcpy(h.theta, a->old_theta, E * 4);
    if (int rc = mh_screen_launch(c, counts_src, a, d)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(flags, h.flags, E);
    // (defined where the flag is 3)
    if (new32) memcpy(new32, h.new32, E * sizeof(float));
    return 0;
}

// bnpc_mh_batch with the device screen in front (include/bnpc_hip.h).
// `pending`: counts the device is still writing into pinned memory behind the
// stream (n1 rows then n0 rows, a->G x M each): copied into a->n1 / a->n0
// once the first screen has been waited for - before the host reads any.
static bool mh_screen_applies(const bnpc_ctx *c, const bnpc_mh_args *a)
{
    return !(a->trans_prob || !c->tun.mh_screen || a->screen
             || a->G * a->M < MH_SCREEN_MIN);
}

// The counts a fused launch is still writing behind the stream, taken now
// (a batch that will not wait for its first screen before the host reads them)
static int mh_take_pending(bnpc_ctx *c, const bnpc_mh_args *a,
                           const int **pending)
{
    if (!*pending) return 0;
    const size_t E = (size_t)a->G * a->M;
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy((void *)a->n1, *pending, E * sizeof(int32_t));
    memcpy((void *)a->n0, *pending + E, E * sizeof(int32_t));
    *pending = nullptr;
    return 0;
}

static int mh_batch_dev_impl(bnpc_ctx *c, const bnpc_host_kernels *k,
                             bnpc_mt19937 *rng, const bnpc_mh_args *a,
                             int counts_src, int *status, const int *pending,
                             int64_t row0 = 0, int64_t G_all = -1)
{
    ARGCHK(c && a && status, "NULL argument");
    if (!mh_screen_applies(c, a)) {
        ARGCHK(!pending, "counts still pending");
        // (the step's parameter batch without its screen: a walker's draws
        // are not wanted - the scored batch of a move, counts_src 1, runs
        // WHILE one walks and leaves it alone)
        if (counts_src == 0) mh_ahead_drop(c);
        return bnpc_mh_batch(k, rng, a, status);
    }
    if (int rc = mh_screen_argchk(c, a)) return rc;
    HIPCHK(hipSetDevice(c->device));
    {
        // The pinned block has a budget (a first step that is a
        // move at config 5 brings a batch of K0 x M = 158 M entries - 5.7 GB
        // pinned per chain without one).  A larger batch is screened in
        // slices of whole rows that reuse the block: the draws are taken row
        // by row in the reference's order either way, and nothing of a row
        // depends on another.
        size_t off[6];
        const size_t per_row = mh_pin_offsets((size_t)a->M, off);
        const int64_t rows_max = std::max<int64_t>(
            1, (int64_t)(c->tun.mh_pin_max / per_row));
        if (a->G > rows_max && counts_src == 0 && row0 == 0 && G_all < 0) {
            if (int rc = mh_take_pending(c, a, &pending)) return rc;
            *status = 0;
            for (int64_t g0 = 0; g0 < a->G; g0 += rows_max) {
                const int64_t Gs = std::min<int64_t>(rows_max, a->G - g0);
                const size_t at = (size_t)g0 * a->M;
                bnpc_mh_args b = *a;
                b.G = Gs;
                b.old_theta += at;
                b.n1 += at;
                b.n0 += at;
                if (b.known_theta) {
                    b.known_theta += at;
                    b.known_prior += at;
                }
                b.sd_idx += at;
                b.U += at;
                b.u += at;
                b.new_theta += at;
                if (b.prior_out) b.prior_out += at;
                b.A += at;
                b.log_prob += g0;
                b.declined += g0;
                int st = 0;
                if (int rc = mh_batch_dev_impl(c, k, rng, &b, 0, &st, nullptr,
                                               g0, a->G))
                    return rc;
                // (an element left to SciPy: the caller evaluates the whole
                // batch from its draws - no point in going on.  Status 1
                // promises ALL the draws and the stream behind them: the
                // rows of the slices not reached are drawn here, straight
                // into the caller's arrays)
                if (st) {
                    *status = 1;
                    const int64_t done = g0 + Gs;
                    if (rng && done < a->G) {
                        const size_t rest = (size_t)done * a->M;
                        if (int rc = bnpc_mt_mh_draws(rng, a->G - done, a->M,
                                a->n_sd, a->sd_idx + rest, a->U + rest,
                                a->u + rest))
                            return rc;
                    }
                    return 0;
                }
                // (a last slice below the screen's minimum went to the plain
                // batch, which keeps no sum of the densities: continued here,
                // one accumulator, index order)
                if (b.prior_seq_sum && b.prior_out && !a->uniform_prior
                    && !mh_screen_applies(c, &b)) {
                    const size_t n = (size_t)Gs * a->M;
                    double s = *b.prior_seq_sum;
                    size_t i = 0;
                    if (s != s) s = b.prior_out[i++];
                    for (; i < n; i++) s += b.prior_out[i];
                    *b.prior_seq_sum = s;
                }
            }
            return 0;
        }
    }
    static const bool trace = [] {      // BNPC_TIMING=mh
        const char *e = getenv("BNPC_TIMING");
        return e && strstr(e, "mh");
    }();
    timespec ts0, ts1;
    if (trace) clock_gettime(CLOCK_MONOTONIC, &ts0);
    const int64_t G = a->G, M = a->M;
    const size_t E = (size_t)G * M;
    MHPin h, d;
    if (const int prc = mh_pin_get(c, E, h, d, true)) {
        if (prc != MH_PIN_NO_MEMORY) return 1;
        // no pinned block: the batch without its screen (the exact arithmetic
        // of every entry on the team) instead of a failed step
        if (int rc = mh_take_pending(c, a, &pending)) return rc;
        return bnpc_mh_batch(k, rng, a, status);
    }
    // Parts in a pipeline (batches of 4 rows and more): the draws of part
    // p + 1 are taken while the device screens part p, and the host evaluates
    // what a screen left while the next one runs.  Two halves for the batches
    // of a config-3 step; a LARGE batch (configs 4 and 5: 65 000 - 250 000
    // entries, 0.2 ms of draws) is cut into up to 8 parts, two of them
    // issued up front; while the team evaluates what the screen left of part
    // p, its rank 0 - this thread, the only one that touches the stream -
    // first takes the draws of part p + 2, stages them and launches their
    // screen (bnpc_mh_rank0_hook), then joins the evaluation.  (A helper
    // std::thread did the issuing earlier in round 4: a thread started per
    // batch on whatever core is free took 80-120 us for the draws of a part
    // that this thread, warm, takes in 27 - tools/draws_bench.py.)
    // Draws taken ahead (MhAhead above): adopted iff the live stream stands
    // where the walker's stood when it began to draw.
    MhAhead *ah = c->ahead;
    const int64_t ahead_rows = mh_ahead_claim(
        c, row0 == 0 && G_all < 0 && counts_src == 0, rng, G, M, a->n_sd);
    // the walker's part of the batch is over: the live stream continues from
    // the state kept after the last row taken from it
    auto ahead_close = [&]() {
        if (!ahead_rows || !ah->active) return;
        mh_ahead_wait_rows(ah, ahead_rows);
        *rng = ah->after_row[(size_t)(ahead_rows - 1)];
        mh_ahead_drop(c);
    };
    const bool threaded = rng && c->tun.done_words && G >= 4 && counts_src == 0
        && E >= MH_THREADED_MIN;     // "pipelined on rank 0"
    int parts = (G >= 4 && counts_src == 0) ? 2 : 1;
    if (threaded)
        parts = (int)std::max<int64_t>(2, std::min<int64_t>(
            std::min<int64_t>(8, G), (int64_t)(E / (MH_THREADED_MIN / 2))));
    int64_t cut[9];
    for (int p = 0; p <= parts; p++) cut[p] = G * p / parts;
    // ONE team job for the whole batch (round 6; below): its ranks wait for a
    // part's verdicts at the first row of it they touch
    const bool one_job = c->tun.done_words && parts >= 2;
    for (int p = 0; p < 2; p++)
        if (!c->mh_ev[p])
            HIPCHK(hipEventCreateWithFlags(&c->mh_ev[p],
                                           hipEventDisableTiming));
    SideLane lane(c);
    unsigned done_seq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double t_draws_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // draws + staging + launch of one part (either thread)
    auto issue_part = [&](int p) -> int {
        const int64_t g0 = cut[p], Gp = cut[p + 1] - cut[p];
        const size_t at = (size_t)g0 * M, n = (size_t)Gp * M;
        timespec tq0, tq1;
        if (trace) clock_gettime(CLOCK_MONOTONIC, &tq0);
        if (rng) {
            int64_t lo = g0;
            const int64_t hi = g0 + Gp;
            if (lo < ahead_rows) {      // rows the walker took (or is taking)
                const int64_t upto = std::min(hi, ahead_rows);
                mh_ahead_wait_rows(ah, upto);
                lo = upto;
            }
            if (lo < hi) {              // rows this thread draws
                ahead_close();
                const size_t lat = (size_t)lo * M;
                if (int rc = bnpc_mt_mh_draws_to(rng, hi - lo, M, a->n_sd,
                                                 h.sd_idx + lat, h.U + lat,
                                                 h.u + lat, threaded))
                    return rc;
            }
            if (trace) {
                clock_gettime(CLOCK_MONOTONIC, &tq1);
                t_draws_us[p] = (tq1.tv_sec - tq0.tv_sec) * 1e6
                    + (tq1.tv_nsec - tq0.tv_nsec) / 1e3;
            }
        } else {
            memcpy(h.U + at, a->U + at, n * 8);
            memcpy(h.u + at, a->u + at, n * 8);
            memcpy(h.sd_idx + at, a->sd_idx + at, n * 4);
        }
        memcpy(h.theta + at, a->old_theta + at, n * 4);
        // (one word for all parts: the launches of a stream finish in order)
        const DoneSignal sig = make_signal(c, threaded || one_job ? 0 : p,
                                           &done_seq[p]);
        if (int rc = mh_screen_launch(c, counts_src, a, d, g0, Gp, sig, row0,
                                      G_all))
            return rc;
        if (!done_seq[p]) HIPCHK(hipEventRecord(c->mh_ev[p & 1], c->stream));
        return 0;
    };
    timespec t_issued[8], t_got[8], t_waited[8], t_hosted[8];
    // issue one part, keep its time for the trace
    auto issue_timed = [&](int p) -> int {
        const int rc = issue_part(p);
        if (trace) clock_gettime(CLOCK_MONOTONIC, &t_issued[p]);
        return rc;
    };
    int next_issue = 0;
    {
        // (parts whose draws are there cost this thread a copy and a launch:
        // all of them up front)
        int up_front = threaded ? std::min(2, parts) : parts;
        while (up_front < parts && ahead_rows >= cut[up_front + 1]
               && ah->rows_ready.load(std::memory_order_acquire)
                   >= cut[up_front + 1])
            up_front++;
        for (; next_issue < up_front; next_issue++)
            if (int rc = issue_timed(next_issue)) return rc;
    }
    if (trace) clock_gettime(CLOCK_MONOTONIC, &ts1);
    int64_t kept = 0;
    double weighted_per_row = 0.0;      // flagged entries of the parts so far
    *status = 0;
    bool all_signalled = one_job;
    for (int p = 0; p < next_issue; p++)
        all_signalled = all_signalled && done_seq[p] != 0;
    if (all_signalled) {
        // ---- the batch as ONE team job ---------------------------------
        // Round 5 evaluated part after part: a team job per part, its rank 0
        // issuing the next part but one before it joined - seven wake-ups,
        // seven barriers and seven tails per config-5 batch, 60-70 us a part
        // even with the draws taken ahead.  Now the team is started once:
        // rank 0 (this thread) first issues what is left to issue - a copy
        // and a launch per part when a walker took the draws, else the draws
        // too -, copies the counts a fused launch wrote, and joins; every
        // rank, before it touches a row, waits until the part the row lies
        // in has been launched and the device's completion word has reached
        // that launch's number (the parts finish in order on one stream).
        std::atomic<int> issued(next_issue), ready(0), failed(0);
        const volatile unsigned *word = c->done_pin;    // slot 0
        const std::function<bool(int64_t)> gate = [&](int64_t g) -> bool {
            int p = 0;
            while (p + 1 < parts && g >= cut[p + 1]) p++;
            if (ready.load(std::memory_order_acquire) > p) return true;
            bnpc_spin_until([&] {
                return failed.load(std::memory_order_relaxed)
                    || (issued.load(std::memory_order_acquire) > p
                        && (int)(*word - done_seq[p]) >= 0);
            }, 4000);
            if (failed.load(std::memory_order_relaxed)) return false;
            std::atomic_thread_fence(std::memory_order_acquire);
            int seen = ready.load(std::memory_order_relaxed);
            while (seen < p + 1
                   && !ready.compare_exchange_weak(seen, p + 1,
                                                   std::memory_order_release))
            {}
            return true;
        };
        int hook_rc = 0;
        const int *counts_dev = pending;
        const std::function<void()> hook = [&]() {
            while (next_issue < parts && !hook_rc) {
                hook_rc = issue_timed(next_issue);
                if (!hook_rc && !done_seq[next_issue]) hook_rc = 1;
                next_issue++;
                issued.store(next_issue, std::memory_order_release);
            }
            if (hook_rc) {
                failed.store(1, std::memory_order_relaxed);
                return;
            }
            if (counts_dev) {   // behind the first screen: the counts are there
                if (!gate(0)) return;
                memcpy((void *)a->n1, counts_dev, E * sizeof(int32_t));
                memcpy((void *)a->n0, counts_dev + E, E * sizeof(int32_t));
            }
        };
        bnpc_mh_args b = *a;
        b.sd_idx = h.sd_idx;
        b.U = h.U;
        b.u = h.u;
        b.screen = h.flags;
        b.screen_theta = h.new32;
        if (pending) {          // the evaluation reads them where they are
            b.n1 = pending;
            b.n0 = pending + E;
        }
        int64_t counts[3] = {0, 0, 0};
        b.flag_counts = counts;
        b.flagged_estimate = std::max<int64_t>(
            1, (int64_t)(c->mh_flagged_share * (double)E));
        int st = 0;
        bnpc_mh_rank0_hook(&hook);
        bnpc_mh_row_gate(&gate);
        int rc = bnpc_mh_batch(k, nullptr, &b, &st);
        bnpc_mh_rank0_hook(nullptr);
        bnpc_mh_row_gate(nullptr);
        pending = nullptr;
        if (rc == 0 && hook_rc) {
            bnpc_set_error("a part of a screened parameter batch could not "
                           "be issued");
            rc = hook_rc == 2 ? 2 : 1;
        }
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        if (st) *status = 1;
        kept = counts[0] + counts[1] + counts[2];
        c->mh_flagged_share = ((double)(counts[0] + counts[1])
            + 0.5 * (double)counts[2]) / (double)E;
        if (trace)
            for (int p = 0; p < parts; p++) t_got[p] = t_waited[p] =
                t_hosted[p] = t_issued[p];
    } else
    for (int p = 0; p < parts; p++) {
        const int64_t g0 = cut[p], Gp = cut[p + 1] - cut[p];
        const size_t at = (size_t)g0 * M;
        if (trace) clock_gettime(CLOCK_MONOTONIC, &t_got[p]);
        if (done_seq[p]) {
            if (int rc = wait_done(c, threaded || one_job ? 0 : p, done_seq[p]))
                return rc;
        } else {
            HIPCHK(hipEventSynchronize(c->mh_ev[p & 1]));
        }
        if (trace) clock_gettime(CLOCK_MONOTONIC, &t_waited[p]);
        if (pending) {          // the counts were written before the screen
            memcpy((void *)a->n1, pending, E * sizeof(int32_t));
            memcpy((void *)a->n0, pending + E, E * sizeof(int32_t));
            pending = nullptr;
        }
        bnpc_mh_args b = *a;
        b.G = Gp;
        b.old_theta += at;
        b.n1 += at;
        b.n0 += at;
        if (b.known_theta) {
            b.known_theta += at;
            b.known_prior += at;
        }
        b.sd_idx = h.sd_idx + at;
        b.U = h.U + at;
        b.u = h.u + at;
        b.new_theta += at;
        if (b.prior_out) b.prior_out += at;
        b.A += at;
        b.log_prob += g0;
        b.declined += g0;
        b.screen = h.flags + at;
        b.screen_theta = h.new32 + at;
        // (the flags sit in memory the device has just written: a pass over
        // them - to size the team, to count what was left - is 10-15 us of
        // misses per part on the calling thread; the team counts while it
        // works, and the parts of one batch leave about the same share)
        int64_t counts[3] = {0, 0, 0};
        b.flag_counts = counts;
        b.flagged_estimate = p == 0 ? 0
            : std::max<int64_t>(1, (int64_t)(weighted_per_row * (double)Gp));
        int st = 0;
        // rank 0 of this part's evaluation issues the next part but one first
        int hook_rc = 0;
        const std::function<void()> hook = [&]() {
            hook_rc = issue_timed(next_issue++);
        };
        if (next_issue < parts) bnpc_mh_rank0_hook(&hook);
        int rc = bnpc_mh_batch(k, nullptr, &b, &st);
        bnpc_mh_rank0_hook(nullptr);
        if (rc == 0) rc = hook_rc;
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        if (st) *status = 1;
        kept += counts[0] + counts[1] + counts[2];
        weighted_per_row = ((double)(counts[0] + counts[1])
            + 0.5 * (double)counts[2]) / (double)Gp;
        if (trace) clock_gettime(CLOCK_MONOTONIC, &t_hosted[p]);
    }
    ahead_close();
    c->screened += (int64_t)E;
    c->screen_kept += kept;
    if (trace) {
        timespec ts3;
        clock_gettime(CLOCK_MONOTONIC, &ts3);
        auto us = [](const timespec &x, const timespec &y) {
            return (y.tv_sec - x.tv_sec) * 1e6 + (y.tv_nsec - x.tv_nsec) / 1e3;
        };
        fprintf(stderr, "[mh_batch_dev] %lld x %lld in %d part(s): draws + "
                "staging + launches %.1f us, waits + host %.1f us (%lld left)\n",
                (long long)G, (long long)M, parts, us(ts0, ts1), us(ts1, ts3),
                (long long)kept);
        if (threaded)
            for (int p = 0; p < parts; p++)
                fprintf(stderr, "[mh_batch_dev]   part %d: issued at %.1f "
                        "(its draws %.1f), picked up at %.1f, screened at "
                        "%.1f, evaluated at %.1f us\n", p,
                        us(ts0, t_issued[p]), t_draws_us[p], us(ts0, t_got[p]),
                        us(ts0, t_waited[p]), us(ts0, t_hosted[p]));
    }
    if (*status != 0 || (rng && G_all >= 0)) {
        // the caller's view of the draws (the SciPy-level twin evaluates the
        // batch from them when the library hands an element back; a slice's
        // are taken out before the next slice reuses the block - a later one
        // may be the one that hands the batch back)
        memcpy(a->sd_idx, h.sd_idx, E * 4);
        memcpy(a->U, h.U, E * 8);
        memcpy(a->u, h.u, E * 8);
    }
    return 0;
}

// The second half of a restricted-Gibbs scan (bnpc_rg_scan_step,
// bnpc_sweeps.cpp) on ONE stream synchronisation: the column counts of the two
// launch clusters for the new assignment (labels: one per slot of the view),
// the draws of the parameter batch, its device screen - queued behind the
// counts it reads - then the counts are copied out and the host evaluates what
// the screen left.  Scored batches and contexts without the screen take the
// two calls one after the other.
int bnpc_rg_counts_and_batch(bnpc_ctx *c, const bnpc_host_kernels *k,
                             bnpc_mt19937 *rng, int view,
                             const int64_t *labels, const bnpc_mh_args *a,
                             int32_t *n1, int32_t *n0, int *status)
{
    ARGCHK(c && a && labels && n1 && n0 && status && rng, "NULL argument");
    const int64_t M = a->M;
    auto finish_rows = [&]() {
        if (a->G == 3)
            for (int64_t m = 0; m < M; m++) {       // the merged cluster
                n1[2 * M + m] = n1[m] + n1[M + m];
                n0[2 * M + m] = n0[m] + n0[M + m];
            }
    };
    const bool fused = !a->trans_prob && c->tun.mh_screen
        && a->G * M >= MH_SCREEN_MIN && !c->any_tile_pending();
    if (!fused) {
        if (int rc = bnpc_view_counts(c, view, labels, 2, n1, n0)) return rc;
        finish_rows();
        return bnpc_mh_batch_dev(c, k, rng, a, 1, status);
    }
    if (int rc = mh_screen_argchk(c, a)) return rc;
    ARGCHK(view >= 0 && view < BNPC_MAX_VIEWS, "view out of range");
    HIPCHK(hipSetDevice(c->device));
    c->cnt_rows = 0;
    const int *pending = nullptr;
    if (int rc = view_label_counts(c, view, labels, 2, n1, n0, &pending))
        return rc;
    c->cnt_rows = 2;
    const size_t E = (size_t)a->G * M;
    MHPin h, d;
    if (mh_pin_get(c, E, h, d, true)) return 1;
    {
        // the rows a walker took under the scan's sums and loop (posted when
        // the scan had drawn its visiting order: one uniform per cell lay
        // between there and here), the rest by this thread
        const int64_t got = mh_ahead_adopt(c, rng, a->G, M, a->n_sd);
        if (got < a->G) {
            const size_t at = (size_t)got * M;
            if (int rc = bnpc_mt_mh_draws(rng, a->G - got, M, a->n_sd,
                                          h.sd_idx + at, h.U + at, h.u + at))
                return rc;
        }
    }
    memcpy(h.theta, a->old_theta, E * 4);
    unsigned done_seq = 0;
    const DoneSignal sig = make_signal(c, 0, &done_seq);
    if (int rc = mh_screen_launch(c, 1, a, d, 0, -1, sig)) return rc;
    if (int rc = wait_done(c, 0, done_seq)) return rc;
    if (pending) {
        const size_t half = (size_t)2 * M * sizeof(int32_t);
        memcpy(n1, pending, half);
        memcpy(n0, pending + (size_t)2 * M, half);
    }
    finish_rows();
    bnpc_mh_args b = *a;
    b.sd_idx = h.sd_idx;
    b.U = h.U;
    b.u = h.u;
    b.screen = h.flags;
    b.screen_theta = h.new32;
    int64_t counts[3] = {0, 0, 0};
    b.flag_counts = counts;
    if (int rc = bnpc_mh_batch(k, nullptr, &b, status)) return rc;
    c->screened += (int64_t)E;
    c->screen_kept += counts[0] + counts[1] + counts[2];
    if (*status != 0) {
        memcpy(a->sd_idx, h.sd_idx, E * 4);
        memcpy(a->U, h.U, E * 8);
        memcpy(a->u, h.u, E * 8);
    }
    return 0;
}

extern "C" int bnpc_mh_batch_dev(bnpc_ctx *c, const bnpc_host_kernels *k,
                                 bnpc_mt19937 *rng, const bnpc_mh_args *a,
                                 int counts_src, int *status)
{
    return mh_batch_dev_impl(c, k, rng, a, counts_src, status, nullptr);
}

// update_parameters in one call (libs/CRP.py:302-311): the per-cluster
// column counts for `assignment` (bnpc_colcounts_by_label; they stay resident
// for bnpc_ll_total) and the screened parameter batch on them, the screens
// queued behind the counts kernel - the counts reach a->n1 / a->n0 (the
// caller's arrays, K x M each) with the first screen's results.
extern "C" int bnpc_label_counts_and_batch(bnpc_ctx *c,
                                           const bnpc_host_kernels *k,
                                           bnpc_mt19937 *rng,
                                           const int64_t *assignment,
                                           const int64_t *ids,
                                           const bnpc_mh_args *a, int *status)
{
    ARGCHK(c && a && status && a->n1 && a->n0, "NULL argument");
    const bool fused = mh_screen_applies(c, a) && !c->any_tile_pending();
    const int *pending = nullptr;
    if (int rc = colcounts_by_label_impl(c, assignment, ids, a->G,
            (int32_t *)a->n1, (int32_t *)a->n0, fused ? &pending : nullptr))
        return rc;
    return mh_batch_dev_impl(c, k, rng, a, 0, status, pending);
}

extern "C" int bnpc_mh_screen_stats(bnpc_ctx *c, int64_t *screened,
                                    int64_t *kept)
{
    ARGCHK(c && screened && kept, "NULL argument");
    *screened = c->screened;
    *kept = c->screen_kept;
    return 0;
}

