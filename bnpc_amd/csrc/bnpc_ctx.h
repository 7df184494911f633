// bnpc_ctx.h - private to libbnpc_hip.so: the context behind a bnpc_ctx
// handle and what its three translation units share.
//   bnpc_context.cpp   error state, switches, pinned memory and staging,
//                      completion words, create / destroy / views
//   bnpc_kernels.hip   the kernels and every function that launches one
//   bnpc_mhbatch.cpp   the screened parameter batch and its read-ahead walker
// The host units reach the device only through the HIP runtime and the
// launchers declared at the end of this file.
#ifndef BNPC_CTX_H
#define BNPC_CTX_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "bnpc_hip.h"
#include "bnpc_internal.h"

#define HIPCHK(expr)                                                         \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            bnpc_set_error("%s failed: %s (%s:%d)", #expr,                   \
                           hipGetErrorString(e_), __FILE__, __LINE__);       \
            return 1;                                                        \
        }                                                                    \
    } while (0)

#define ARGCHK(cond, msg)                                                    \
    do {                                                                     \
        if (!(cond)) {                                                       \
            bnpc_set_error("bad argument: %s", msg);                         \
            return 2;                                                        \
        }                                                                    \
    } while (0)

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct View {
    DevBuf masks;       // ulonglong2 [nblk][Mpad]
    int64_t n = 0;      // slots in use
    int64_t nblk = 0;
};

// Switches, read from the environment when a context is created and again
// by bnpc_reload_options (tests); never on the launch path.  README lists
// them; the tuning constants that used to be switches (chunking of split
// launches, zero-copy sizes, the screen's minimum batch ...) are the measured
// values below.
struct Tunables {
    int msplit = 1;                 // BNPC_MSPLIT: mutation-split small launches
    int force_kw = 0;               // BNPC_KW: force the cluster tile (tests)
    int zero_copy = 1;              // BNPC_ZERO_COPY: small payloads are read /
                                    // written in place in pinned host memory
    int mask_counts_max = 64;       // BNPC_MASK_COUNTS_MAX: segments for the
                                    // mask-popcount counts (tests lower it)
    int mh_screen = 1;              // BNPC_MH_SCREEN: device screen of the
                                    // parameter batches
    int done_words = 1;             // BNPC_DONE_WORDS: completion words written
                                    // by the kernels (0: stream synchronisation)
    int msplit_chunks = 0;          // BNPC_MSPLIT = N >= 2: force the chunk count
                                    // of split launches (tools/msplit_sweep.py)
    int screen_theta = 1;           // BNPC_MH_SCREEN = 2: verdicts only - not the
                                    // float32 bits of the proposals it accepts
    int mh_ahead = 1;               // BNPC_MH_AHEAD: the draws of the next
                                    // parameter batch taken ahead on the aside
                                    // thread (0: never; 2: for a batch of any
                                    // size - tests; 3: taken and then thrown
                                    // away - tests of the discard path)
    size_t mh_pin_max = (size_t)512 << 20;  // pinned block of a screened
                                    // parameter batch at most: twice
                                    // BNPC_SWEEP_BYTES, the host budget of a
                                    // sweep's matrix (default 256 MiB -> 512:
                                    // 37 bytes per entry, 14.5 M entries -
                                    // config 4's K0 x M batch fits, config 5's
                                    // 158 M are screened in slices of rows
                                    // that reuse the block)
};

#define MSPLIT_MAX 64               // chunks of a split launch at most
#define ASM2_MIN_WGS 448            // workgroups from which a wave takes 2 blocks
#define TABLES_FLAT_MAX (1 << 20)   // table elements up to which one thread
                                    // builds one element
#define ZC_IN_MAX ((int64_t)256 << 10)      // zero-copy inputs / results up to
#define ZC_OUT_MAX ((int64_t)512 << 10)
#define MH_SCREEN_MIN 512           // batch entries from which the screen pays
#define MH_THREADED_MIN 65536       // batch entries from which rank 0 issues
                                    // draws and launches ahead of the waits
                                    // (the pinned block of a screened batch
                                    // is at most Tunables::mh_pin_max bytes)
#define MH_PIN_NO_MEMORY 77         // mh_pin_get: the host refused the block
#define MH_AHEAD_MIN 8192           // batch entries from which its draws are
                                    // taken ahead (config 3's 10-16 thousand:
                                    // parameters 0.102 -> 0.090 ms, five
                                    // interleaved pairs, profiles/r06/
                                    // c3_walker_ab; config 2's 2000 cost less
                                    // than the hand-over)
#define MH_AHEAD_SCAN_MIN 2048      // ... of a restricted scan's batch (2-3 rows:
                                    // the walker has the scan's sums and loop,
                                    // 50 us and more, for 10-35 us of draws)
#define MH_AHEAD_MAX_ROWS 1024      // ... and rows up to which (a stream state
                                    // is kept per row: 2.5 KB)
#define HINT_COLS_MAX 32767         // columns of a hinted sweep (int16 in the
                                    // record)
#define HINT_THROUGH_MAX 1024       // ... up to which rows that will be scanned
                                    // are written through to the host
#define LDS_TABLE_MIN_M 3072        // k_ll8_lds: mutations (padded) from which,
#define LDS_TABLE_MIN_WGS 4096      // ... and workgroups from which it wins

#define DONE_SLOTS 3     // 0, 1: the launches of a call; 2: the deferred total
// what a kernel needs to tell the host that it is done (signal_done below)
struct DoneSignal {
    unsigned *count;    // device word, zero between launches
    unsigned *flag;     // pinned host word (device address)
    unsigned seq;
};

// the column priors of a hint launch of up to 64 columns (kernel argument)
struct Top2Prior {
    double v[64];
};

struct bnpc_ctx {
    Tunables tun;
    int device = 0;
    int64_t N = 0, M = 0;
    int W = 0;          // 64-bit words per row
    int Mpad = 0;       // W * 64
    int Mt = 0;         // table row count per group: M rounded up to 8
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ulonglong2 *rows = nullptr;           // [N][W]
    std::vector<ulonglong2> host_rows;    // the same words on the host: the
                                          // observations of ONE cell shape the
                                          // Beta draws of a cluster it opens
    std::vector<int32_t> cell_n1, cell_n0;
    View views[BNPC_MAX_VIEWS];
    // scratch
    DevBuf theta, tabs, tab_in, out, cells, chunks, cnt, partial, part;
    DevBuf theta_store, row_idx;    // resident parameter rows + selection
    int64_t store_rows = 0;
    const long long *use_rows = nullptr;    // non-null: tables from the store
    // resident per-cluster counts of the last bnpc_colcounts_by_label
    DevBuf lab_cnt;
    int64_t lab_K = 0;
    uint64_t lab_gen = 0;       // bumped by every bnpc_colcounts_by_label
    int64_t cnt_rows = 0;       // segments of the last bnpc_view_counts (c->cnt)
    // pinned host buffers: the sweep's ll matrix / small reductions
    void *pin = nullptr;
    size_t pin_cap = 0;
    void *pin_small = nullptr;
    // side lane: a second stream with its own scratch, used by the small
    // synchronous calls (one column for a cluster opened mid-sweep) while an
    // issued tile occupies the main stream - they must not queue behind it
    hipStream_t side_stream = nullptr;
    DevBuf side_theta, side_tabs, side_out, side_part;
    // pinned staging arena for small host <-> device payloads (parameter
    // rows, cell lists, counts): a copy from/to pinned memory is a plain DMA
    // enqueue, a copy from/to pageable memory is staged by the runtime at
    // ~10 us apiece.  Reset at the start of every call that uses it; every
    // such call ends with a stream synchronisation.
    void *stage = nullptr;
    char *stage_dev = nullptr;      // the arena as the device addresses it
    size_t stage_used = 0;
    // small results written by kernels straight into pinned host memory
    void *zc_out = nullptr;
    char *zc_out_dev = nullptr;
    void *hint_pin = nullptr;       // the sweep's per-cell hints (pinned)
    size_t hint_cap = 0;
    DevBuf hint_prior;              // priors of a hinted sweep with > 64 columns
    void *hint_prior_pin = nullptr; // ... staged here (pinned, HINT_COLS_MAX)
    // bnpc_ll_theta_pinned_sums_issue: a hinted sweep whose hint kernel is
    // launched later (bnpc_hints_in_order_issue), when the caller has drawn
    // its visiting order under the sums - what that launch needs
    struct {
        // 0: no sums issued; 1: issued, the hint kernel is to be launched;
        // 2: issued without a hint buffer (the matrix was copied instead)
        int state = 0;
        int64_t n = 0, K = 0, ldo = 0;
        size_t bytes = 0;
        Top2Prior prior;            // K <= 64 (more: c->hint_prior)
        void *hint_dev = nullptr;
        double *rows_dev = nullptr;
    } hint_later;
    void *order_pin = nullptr;      // the visiting order, pinned (N entries)
    DevBuf order_dev;               // ... and on the device
    // pinned block of a screened parameter batch (bnpc_mh_batch_dev): the
    // draws, the old parameter rows and the screen's verdicts, read / written
    // in place by k_mh_screen
    void *mh_pin = nullptr;
    char *mh_dev = nullptr;
    size_t mh_cap = 0;
    size_t mh_capE = 0;             // entries the block is laid out for
    struct MhAhead *ahead = nullptr;    // draws taken ahead (bnpc_mh_ahead_*)
    int64_t ahead_begun = 0, ahead_taken = 0, ahead_rows_taken = 0;
    double mh_flagged_share = 0.25; // host work the last screened batch left,
                                    // per entry (sizes the next one's team)
    hipEvent_t mh_ev[2] = {};
    int64_t screened = 0, screen_kept = 0;  // elements seen / left to the host
    size_t pin_lazy_bytes = 0;      // sweep matrix still on the device (c->out)
    // ... unless the previous hinted sweep had to fetch it: then the copy is
    // queued right behind the hint kernel and lands while the host prepares
    // the sweep (a running chain scans ~9 % of its cells: it always needs it;
    // a settled one never does)
    bool matrix_eager = false, lazy_fetched = false, pin_copy_queued = false;
    hipEvent_t ev_hints = nullptr;
    // completion words (DoneSignal): two slots, so that two launches of one
    // call may be in flight (the two halves of a screened batch)
    unsigned *done_count = nullptr;         // device, DONE_SLOTS words
    unsigned *done_pin = nullptr;           // pinned host, DONE_SLOTS x 16 words
    unsigned *done_dev = nullptr;           // ... as the device addresses it
    unsigned done_seq = 0;
    unsigned total_seq = 0;                 // of the pending bnpc_ll_total
    int total_slot = -1;
    DoneSignal sig_next = {nullptr, nullptr, 0};    // for the last kernel of
    bool sig_attached = false;                      // the next issue_ll
    // bnpc_ll_theta_begin / _end: an evaluation whose result is written in
    // place for the host and picked up later (the caller works in between)
    bool defer_next = false, defer_set = false;
    struct {
        void *zc_host;
        unsigned seq;
        double *out;
        size_t bytes;
        int64_t n, K, ldo;
    } defer = {nullptr, 0, nullptr, 0, 0, 0, 0};
    // bnpc_view_set's own pinned cell list (N entries) and the event that
    // says the last gather has read it
    void *view_cells_pin = nullptr;
    const long long *view_cells_dev = nullptr;
    hipEvent_t view_cells_read = nullptr;
    bool view_cells_busy = false;
    bool total_pending = false;     // a deferred bnpc_ll_total_issue
    int total_blocks = 0, total_E = 0;
    // where the kernels of the current call read their inputs from: device
    // scratch filled by a DMA copy, or the staging arena in place
    const float *theta_src = nullptr;
    const double *tab_src = nullptr;
    const long long *cells_src = nullptr;
    // Issued (asynchronous) tiles: up to BNPC_TILE_SLOTS in flight, each with
    // its own pinned result buffer.  The sums of consecutive tiles alternate
    // between two device buffers and the copy to the host runs on its own
    // stream, so the copy of one tile overlaps the sums of the next.
    void *tile_pin[BNPC_TILE_SLOTS] = {};
    size_t tile_cap[BNPC_TILE_SLOTS] = {};
    size_t tile_bytes[BNPC_TILE_SLOTS] = {};
    void *tile_rows[BNPC_TILE_SLOTS] = {};      // pinned staging of the ids
    size_t tile_rows_cap[BNPC_TILE_SLOTS] = {};
    void *tile_cells[BNPC_TILE_SLOTS] = {};     // ... and of the tile's cells
    size_t tile_cells_cap[BNPC_TILE_SLOTS] = {};
    void *tile_hint[BNPC_TILE_SLOTS] = {};      // pinned: the tile's hints
    size_t tile_hint_cap[BNPC_TILE_SLOTS] = {};
    void *tile_prior[BNPC_TILE_SLOTS] = {};     // pinned staging of the priors
    size_t tile_prior_cap[BNPC_TILE_SLOTS] = {};
    bool tile_hinted[BNPC_TILE_SLOTS] = {};
    DevBuf tile_prior_dev[2];                   // by parity, like tile_out
    hipEvent_t tile_done[BNPC_TILE_SLOTS] = {}; // copy landed in tile_pin
    bool tile_pending[BNPC_TILE_SLOTS] = {};
    DevBuf tile_out[2];                         // by parity of the issue count
    hipEvent_t tile_summed[2] = {};             // sums written to tile_out
    hipEvent_t tile_out_free[2] = {};           // its last copy has left
    uint64_t tile_seq = 0;
    hipStream_t copy_stream = nullptr;
    bool any_tile_pending() const
    {
        for (bool p : tile_pending)
            if (p) return true;
        return false;
    }
    // configuration of the last k_ll launch (bnpc_bench_ll re-issues it)
    int last_kw = 0, last_view = -1, last_ms = 1, last_mchunk = 0;
    int64_t last_K = 0, last_ldo = 0;
    double *last_out = nullptr;
    double *dst_override = nullptr; // device-addressable result buffer
    bool last_from_theta = false;
    double last_FP = 0.0, last_FN = 0.0;
    char last_name[96] = "";
};

static inline int ensure(DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) HIPCHK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    size_t cap = bytes + bytes / 4 + 256;
    HIPCHK(hipMalloc(&b.p, cap));
    b.cap = cap;
    return 0;
}

// A DoneSignal for the next launch on slot 0 / 1 (the words are made on first
// use; without them - or with BNPC_DONE_WORDS=0 - the signal is empty and the
// caller synchronises as before).  *seq receives the number to wait for.
static inline DoneSignal make_signal(bnpc_ctx *c, int slot,
                                     unsigned *seq)
{
    DoneSignal none = {nullptr, nullptr, 0};
    *seq = 0;
    if (!c->tun.done_words) return none;
    if (!c->done_count) {
        void *pin = nullptr, *dev = nullptr, *cnt = nullptr;
        if (hipHostMalloc(&pin, DONE_SLOTS * 64, hipHostMallocDefault) != hipSuccess
            || hipHostGetDevicePointer(&dev, pin, 0) != hipSuccess
            || hipMalloc(&cnt, DONE_SLOTS * sizeof(unsigned)) != hipSuccess
            || hipMemset(cnt, 0, DONE_SLOTS * sizeof(unsigned))
                != hipSuccess) {
            (void)hipGetLastError();
            if (pin) (void)hipHostFree(pin);
            if (cnt) (void)hipFree(cnt);
            return none;
        }
        memset(pin, 0, DONE_SLOTS * 64);
        c->done_pin = (unsigned *)pin;
        c->done_dev = (unsigned *)dev;
        c->done_count = (unsigned *)cnt;
    }
    if (++c->done_seq == 0) c->done_seq = 1;    // 0 = "no signal"
    *seq = c->done_seq;
    DoneSignal d = {c->done_count + slot, c->done_dev + 16 * slot, *seq};
    return d;
}

// device -> host, completed by the caller's stream synchronisation followed
// by d2h_finish (which moves the staged bytes to their destination)
struct D2H {
    void *dst, *slot;
    size_t bytes;
};

// While a tile is in flight, run a call on the side lane: swap the stream and
// the scratch buffers the likelihood path uses, restore on scope exit.
struct SideLane {
    bnpc_ctx *c;
    bool on;
    explicit SideLane(bnpc_ctx *ctx)
        : c(ctx), on(ctx->side_stream && ctx->any_tile_pending())
    {
        if (on) flip();
    }
    ~SideLane()
    {
        if (on) flip();
    }
    void flip()
    {
        std::swap(c->stream, c->side_stream);
        std::swap(c->theta, c->side_theta);
        std::swap(c->tabs, c->side_tabs);
        std::swap(c->out, c->side_out);
        std::swap(c->part, c->side_part);
    }
};

// ---- device screen of a parameter batch -----------------------------------
// layout of the pinned block for G x M = E elements (all 16-byte aligned):
//   U[E] f64 | u[E] f64 | sd_idx[E] i32 | theta[E] f32 | new32[E] f32 |
//   flags[E] u8
// (new32: the proposals whose float32 bits the screen vouches for, flag 3)
struct MHPin {
    double *U, *u;
    int32_t *sd_idx;
    float *theta;
    float *new32;
    uint8_t *flags;
};

// ---- shared by the translation units, not exported from the library -------
#pragma GCC visibility push(hidden)
// bnpc_context.cpp
void *stage_slot(bnpc_ctx *c, size_t bytes);
int arena_reset(bnpc_ctx *c);
int wait_done(bnpc_ctx *c, int slot, unsigned seq);
const void *stage_in_place(bnpc_ctx *c, const void *src, size_t bytes);
void *zc_result(bnpc_ctx *c, size_t bytes, void **dev);
int h2d(bnpc_ctx *c, void *dst, const void *src, size_t bytes);
int d2h_begin(bnpc_ctx *c, D2H &t, void *dst, const void *src, size_t bytes);
void d2h_finish(const D2H &t);
int ensure_pin(bnpc_ctx *c, size_t bytes);
int ensure_host(void **p, size_t *cap, size_t bytes);
int ensure_lanes(bnpc_ctx *c);
// bnpc_kernels.hip: the launchers the host units call
int build_view(bnpc_ctx *c, int view, const long long *d_cells, int64_t n);
int colcounts_by_label_impl(bnpc_ctx *c, const int64_t *assignment,
                            const int64_t *ids, int64_t K, int32_t *n1,
                            int32_t *n0, const int **defer);
int view_label_counts(bnpc_ctx *c, int view, const int64_t *labels,
                      int64_t G, int32_t *n1, int32_t *n0,
                      const int **defer);
int mh_screen_launch(bnpc_ctx *c, int src, const bnpc_mh_args *a,
                     const MHPin &dev, int64_t g0 = 0, int64_t Gp = -1,
                     DoneSignal sig = {nullptr, nullptr, 0},
                     int64_t row0 = 0, int64_t G_all = -1);
// bnpc_mhbatch.cpp
void mh_ahead_destroy(bnpc_ctx *c);
#pragma GCC visibility pop

#endif
