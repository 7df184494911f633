// bnpc_context.cpp - the host side of a context (bnpc_ctx.h): error state,
// the switches read from the environment, pinned host memory and the staging
// arena, completion words, and create / destroy / reload / shape / views.
// The kernels these drive are launched in bnpc_kernels.hip.

#include <hip/hip_runtime.h>
#include <atomic>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <mutex>
#include <vector>
#include <algorithm>

#include "bnpc_ctx.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void bnpc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *bnpc_last_error(void) { return g_err; }
extern "C" int bnpc_abi_version(void) { return 12; }

static int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

static void read_tunables(Tunables &t)
{
    t.msplit = env_int("BNPC_MSPLIT", 1);
    t.force_kw = env_int("BNPC_KW", 0);
    if (t.force_kw != 1 && t.force_kw != 2 && t.force_kw != 4
        && t.force_kw != 8)
        t.force_kw = 0;
    t.zero_copy = env_int("BNPC_ZERO_COPY", 1);
    t.mask_counts_max = env_int("BNPC_MASK_COUNTS_MAX", 64);
    t.mh_screen = env_int("BNPC_MH_SCREEN", 1);
    t.done_words = env_int("BNPC_DONE_WORDS", 1);
    t.screen_theta = t.mh_screen != 2;
    t.mh_ahead = env_int("BNPC_MH_AHEAD", 1);
    {
        const char *e = getenv("BNPC_SWEEP_BYTES");
        const long long b = e ? atoll(e) : 0;
        t.mh_pin_max = 2 * (size_t)(b > 0 ? b : (long long)256 << 20);
    }
    t.msplit_chunks = t.msplit >= 2 ? t.msplit : 0;
}

// Large pinned host buffers (result matrices, tiles: hundreds of MiB).
// hipHostMalloc pins 4 KiB pages - 45-48 ms per 300 MiB on the MI355X host,
// and a first sweep needs two or three of them.  Anonymous memory on
// transparent huge pages, touched and then registered, costs 17 + 1 ms for the
// same size and is the same DMA target (57 GB/s either way;
// tools/ubench/pin_probe.hip).  Falls back to hipHostMalloc when huge pages
// are switched off (4 KiB pages would make this route the slower one) or
// anything fails.  `cap` identifies the route at release time: huge-page
// buffers have a capacity that is a multiple of 2 MiB and are remembered.
#define PIN_HUGE_MIN ((size_t)16 << 20)
#define PIN_HUGE_ALIGN ((size_t)2 << 20)

static bool thp_available()
{
    static const bool ok = [] {
        FILE *f = fopen("/sys/kernel/mm/transparent_hugepage/enabled", "r");
        if (!f) return false;
        char line[128] = {0};
        const bool got = fgets(line, sizeof line, f) != nullptr;
        fclose(f);
        return got && !strstr(line, "[never]");
    }();
    return ok;
}

static std::vector<void *> &huge_pins()
{
    static std::vector<void *> v;
    return v;
}

static std::mutex &huge_pins_lock()         // contexts may live on threads
{
    static std::mutex m;
    return m;
}

static int pinned_alloc(void **out, size_t *cap, size_t bytes)
{
    *out = nullptr;
    *cap = 0;
    if (bytes >= PIN_HUGE_MIN && thp_available()) {
        const size_t len = (bytes + PIN_HUGE_ALIGN - 1) & ~(PIN_HUGE_ALIGN - 1);
        char *raw = (char *)mmap(nullptr, len + PIN_HUGE_ALIGN,
                                 PROT_READ | PROT_WRITE,
                                 MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (raw != (char *)MAP_FAILED) {
            char *p = (char *)(((uintptr_t)raw + PIN_HUGE_ALIGN - 1)
                               & ~(uintptr_t)(PIN_HUGE_ALIGN - 1));
            if (p > raw) munmap(raw, (size_t)(p - raw));
            const size_t tail = (size_t)(raw + len + PIN_HUGE_ALIGN - (p + len));
            if (tail) munmap(p + len, tail);
            (void)madvise(p, len, MADV_HUGEPAGE);
            // fault the huge pages in before pinning: one touch per 2 MiB
            // (the kernel zeroes them; anything left on small pages is
            // faulted in by the registration itself)
            for (size_t off = 0; off < len; off += PIN_HUGE_ALIGN)
                ((volatile char *)p)[off] = 0;
            if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> hold(huge_pins_lock());
                huge_pins().push_back(p);
                *out = p;
                *cap = len;
                return 0;
            }
            (void)hipGetLastError();
            munmap(p, len);
        }
    }
    HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    *cap = bytes;
    return 0;
}

static void pinned_free(void *p, size_t cap)
{
    if (!p) return;
    bool huge = false;
    {
        std::lock_guard<std::mutex> hold(huge_pins_lock());
        std::vector<void *> &v = huge_pins();
        auto it = std::find(v.begin(), v.end(), p);
        if (it != v.end()) {
            v.erase(it);
            huge = true;
        }
    }
    if (huge) {
        (void)hipHostUnregister(p);
        munmap(p, cap);
    } else {
        (void)hipHostFree(p);
    }
}

#define STAGE_BYTES ((size_t)4 << 20)
#define ZC_OUT_BYTES ((size_t)1 << 20)

// a slot of the staging arena, or nullptr when the payload is too large
void *stage_slot(bnpc_ctx *c, size_t bytes)
{
    if (!c->stage) {
        if (hipHostMalloc(&c->stage, STAGE_BYTES, hipHostMallocDefault)
                != hipSuccess) {
            c->stage = nullptr;
            return nullptr;
        }
        void *dev = nullptr;
        if (hipHostGetDevicePointer(&dev, c->stage, 0) == hipSuccess)
            c->stage_dev = (char *)dev;
    }
    const size_t at = (c->stage_used + 255) & ~(size_t)255;
    if (at + bytes > STAGE_BYTES) return nullptr;
    c->stage_used = at + bytes;
    return (char *)c->stage + at;
}

// Start of a call that stages inputs: the arena is free again - unless a
// deferred total (bnpc_ll_total_issue) may still be reading its parameters
// from it; then that kernel is waited for first (its result stays parked).
int arena_reset(bnpc_ctx *c)
{
    if (c->total_pending) HIPCHK(hipStreamSynchronize(c->stream));
    c->stage_used = 0;
    return 0;
}

// Wait for the word of a signalled launch; seq == 0 (no signal was attached)
// or a word that does not come within the spin: hipStreamSynchronize.
int wait_done(bnpc_ctx *c, int slot, unsigned seq)
{
    if (seq) {
        const volatile unsigned *f = c->done_pin + 16 * slot;
        for (int spins = 0; spins < 20000; spins++) {       // ~100-200 us
            // (launches of a stream finish in order and the numbers only
            // grow: a later number on the word says this one is done too)
            if ((int)(*f - seq) >= 0) {
                std::atomic_thread_fence(std::memory_order_acquire);
                return 0;
            }
            bnpc_cpu_relax();
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Zero-copy input: the payload is copied into the pinned arena and the
// kernels of this call read it there, over the host link, instead of from a
// device buffer filled by a DMA copy - for payloads of a few hundred KiB a
// copy engine launch costs more than the bytes.  Returns the DEVICE address,
// or nullptr (too large / switched off): then the caller copies.  Every call
// that uses the arena ends with a stream synchronisation.
const void *stage_in_place(bnpc_ctx *c, const void *src, size_t bytes)
{
    if (!c->tun.zero_copy || (int64_t)bytes > ZC_IN_MAX) return nullptr;
    void *slot = stage_slot(c, bytes);
    if (!slot || !c->stage_dev) return nullptr;
    memcpy(slot, src, bytes);
    return c->stage_dev + ((char *)slot - (char *)c->stage);
}

// Zero-copy output: `bytes` of pinned host memory the kernels of this call may
// write their (small) result to; *dev receives the device address.  nullptr:
// not available for this size.
void *zc_result(bnpc_ctx *c, size_t bytes, void **dev)
{
    if (!c->tun.zero_copy || (int64_t)bytes > ZC_OUT_MAX
        || bytes > ZC_OUT_BYTES)
        return nullptr;
    if (!c->zc_out) {
        if (hipHostMalloc(&c->zc_out, ZC_OUT_BYTES, hipHostMallocDefault)
                != hipSuccess) {
            c->zc_out = nullptr;
            return nullptr;
        }
        void *d = nullptr;
        if (hipHostGetDevicePointer(&d, c->zc_out, 0) != hipSuccess) {
            (void)hipHostFree(c->zc_out);
            c->zc_out = nullptr;
            return nullptr;
        }
        c->zc_out_dev = (char *)d;
    }
    *dev = c->zc_out_dev;
    return c->zc_out;
}

// host -> device on the context's stream; `src` may be released on return
// only if the caller synchronises the stream before it returns itself
int h2d(bnpc_ctx *c, void *dst, const void *src, size_t bytes)
{
    void *slot = stage_slot(c, bytes);
    if (slot) {
        memcpy(slot, src, bytes);
        src = slot;
    }
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

int d2h_begin(bnpc_ctx *c, D2H &t, void *dst, const void *src,
              size_t bytes)
{
    t.dst = dst;
    t.bytes = bytes;
    t.slot = stage_slot(c, bytes);
    HIPCHK(hipMemcpyAsync(t.slot ? t.slot : dst, src, bytes,
                          hipMemcpyDeviceToHost, c->stream));
    return 0;
}

void d2h_finish(const D2H &t)
{
    if (t.slot) memcpy(t.dst, t.slot, t.bytes);
}

int ensure_pin(bnpc_ctx *c, size_t bytes)
{
    if (c->pin_copy_queued) {   // a queued copy still targets the buffer
        HIPCHK(hipStreamSynchronize(c->stream));
        c->pin_copy_queued = false;
    }
    c->pin_lazy_bytes = 0;      // a new request supersedes a matrix not fetched
    if (bytes <= c->pin_cap) return 0;
    pinned_free(c->pin, c->pin_cap);
    c->pin = nullptr;
    c->pin_cap = 0;
    return pinned_alloc(&c->pin, &c->pin_cap, bytes + bytes / 4 + 4096);
}

// the side lane, created at the first tile of a context: calls made while
// tiles are in flight (a column for a cluster just opened, the columns of
// clusters born since a tile was issued) run beside 10 ms kernels that fill
// the chip; on a stream of the highest priority their few workgroups get the
// next free slots instead of waiting for a whole tile.  (Compute units of
// their own - the tile kernels on a CU-masked stream, the side lane on the
// rest - were tried in round 4: the masked stream ran the whole sweep 12 %
// slower, 0.53 against 0.475 s, for births that are bound by their host-side
// Beta draws anyway.)
int ensure_lanes(bnpc_ctx *c)
{
    if (c->side_stream) return 0;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess
        || hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking,
                                       greatest) != hipSuccess) {
        (void)hipGetLastError();        // no priorities here: a plain stream
        c->side_stream = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&c->side_stream,
                                        hipStreamNonBlocking));
    }
    return 0;
}

// ---------------------------------------------------------------------------
// host side of the C-ABI
// ---------------------------------------------------------------------------
extern "C" int bnpc_device_count(int *count)
{
    ARGCHK(count, "count is NULL");
    HIPCHK(hipGetDeviceCount(count));
    return 0;
}

extern "C" int bnpc_device_info(int device, char *name, int len, int *cus)
{
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (name && len > 0) {
        strncpy(name, prop.gcnArchName, len - 1);
        name[len - 1] = 0;
    }
    if (cus) *cus = prop.multiProcessorCount;
    return 0;
}

extern "C" int bnpc_device_pci_bus_id(int device, char *bus_id, int len)
{
    ARGCHK(bus_id && len >= 16, "bus_id buffer too small");
    HIPCHK(hipDeviceGetPCIBusId(bus_id, len, device));
    return 0;
}

// Context from ready bit planes: rows[N][W] of {ones, zeros} words (bits past
// M clear, no bit set in both planes - checked).
static int create_from_planes(int device, int64_t N, int64_t M,
                              const ulonglong2 *rows, bnpc_ctx **out)
{
    HIPCHK(hipSetDevice(device));
    bnpc_ctx *c = new bnpc_ctx();
    read_tunables(c->tun);
    c->device = device;
    c->N = N;
    c->M = M;
    c->W = (int)((M + 63) / 64);
    c->Mpad = c->W * 64;
    c->Mt = (int)((M + 7) / 8 * 8);
    c->cell_n1.assign(N, 0);
    c->cell_n0.assign(N, 0);
    const int tail_bits = (int)(M - (int64_t)(c->W - 1) * 64);  // 1..64
    const unsigned long long tail_mask =
        tail_bits == 64 ? ~0ull : ((1ull << tail_bits) - 1);
    for (int64_t i = 0; i < N; i++) {
        int32_t s1 = 0, s0 = 0;
        const ulonglong2 *r = rows + (size_t)i * c->W;
        for (int w = 0; w < c->W; w++) {
            const unsigned long long ok = (w == c->W - 1) ? tail_mask : ~0ull;
            if ((r[w].x & r[w].y) || ((r[w].x | r[w].y) & ~ok)) {
                delete c;
                bnpc_set_error("bit planes of row %lld are inconsistent",
                               (long long)i);
                return 2;
            }
            s1 += __builtin_popcountll(r[w].x);
            s0 += __builtin_popcountll(r[w].y);
        }
        c->cell_n1[i] = s1;
        c->cell_n0[i] = s0;
    }

#define CRCHK(expr)                                                          \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            bnpc_set_error("%s failed: %s", #expr, hipGetErrorString(e_));   \
            bnpc_destroy(c);                                                 \
            return 1;                                                        \
        }                                                                    \
    } while (0)
    const size_t bytes = (size_t)N * c->W * sizeof(ulonglong2);
    c->host_rows.assign(rows, rows + (size_t)N * c->W);
    CRCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CRCHK(hipEventCreate(&c->ev0));
    CRCHK(hipEventCreate(&c->ev1));
    CRCHK(hipMalloc((void **)&c->rows, bytes));
    CRCHK(hipMemcpyAsync(c->rows, rows, bytes, hipMemcpyHostToDevice,
                         c->stream));
    if (build_view(c, 0, nullptr, N)) {
        bnpc_destroy(c);
        return 1;
    }
    CRCHK(hipStreamSynchronize(c->stream));
#undef CRCHK
    *out = c;
    return 0;
}

template <typename GetCode>
static int create_impl(int device, int64_t N, int64_t M, GetCode code,
                       bnpc_ctx **out)
{
    ARGCHK(out, "out is NULL");
    ARGCHK(N > 0 && M > 0, "N and M must be positive");
    ARGCHK(M < (1ll << 30) && N < (1ll << 40), "matrix too large");
    *out = nullptr;
    const int W = (int)((M + 63) / 64);
    // pack on the host: 2 bits per entry
    std::vector<ulonglong2> rows((size_t)N * W);
    for (int64_t i = 0; i < N; i++) {
        for (int w = 0; w < W; w++) {
            unsigned long long o = 0, z = 0;
            const int64_t m0 = (int64_t)w * 64;
            const int64_t m1 = std::min<int64_t>(M, m0 + 64);
            for (int64_t m = m0; m < m1; m++) {
                const int v = code(i, m);
                if (v == 1) o |= 1ull << (m - m0);
                else if (v == 0) z |= 1ull << (m - m0);
                else if (v != 3) {
                    bnpc_set_error("data[%lld,%lld] is not 0, 1 or missing",
                                   (long long)i, (long long)m);
                    return 2;
                }
            }
            rows[(size_t)i * W + w] = make_ulonglong2(o, z);
        }
    }
    return create_from_planes(device, N, M, rows.data(), out);
}

extern "C" int bnpc_create_planes(int device, int64_t N, int64_t M,
                                  const uint64_t *planes, bnpc_ctx **out)
{
    ARGCHK(out && planes, "NULL argument");
    ARGCHK(N > 0 && M > 0, "N and M must be positive");
    ARGCHK(M < (1ll << 30) && N < (1ll << 40), "matrix too large");
    *out = nullptr;
    return create_from_planes(device, N, M, (const ulonglong2 *)planes, out);
}

extern "C" int bnpc_create(int device, int64_t N, int64_t M,
                           const double *data_nan, bnpc_ctx **out)
{
    ARGCHK(data_nan, "data is NULL");
    return create_impl(device, N, M, [=](int64_t i, int64_t m) -> int {
        const double v = data_nan[(size_t)i * M + m];
        if (v != v) return 3;
        if (v == 1.0) return 1;
        if (v == 0.0) return 0;
        return -1;
    }, out);
}

extern "C" int bnpc_create_codes(int device, int64_t N, int64_t M,
                                 const int8_t *codes, bnpc_ctx **out)
{
    ARGCHK(codes, "codes is NULL");
    return create_impl(device, N, M, [=](int64_t i, int64_t m) -> int {
        const int v = codes[(size_t)i * M + m];
        return v == 2 ? 1 : v;      // 2 (homozygous) -> 1, dpmmIO.py:93
    }, out);
}

extern "C" int bnpc_destroy(bnpc_ctx *c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->view_cells_pin) (void)hipHostFree(c->view_cells_pin);
    if (c->view_cells_read) (void)hipEventDestroy(c->view_cells_read);
    if (c->done_pin) (void)hipHostFree(c->done_pin);
    if (c->done_count) (void)hipFree(c->done_count);
    DevBuf *bufs[] = {&c->theta, &c->tabs, &c->tab_in, &c->out, &c->cells,
                      &c->tile_out[0], &c->tile_out[1],
                      &c->tile_prior_dev[0], &c->tile_prior_dev[1],
                      &c->chunks, &c->cnt, &c->partial, &c->part,
                      &c->lab_cnt, &c->theta_store, &c->row_idx,
                      &c->side_theta, &c->side_tabs, &c->side_out,
                      &c->side_part, &c->hint_prior, &c->order_dev};
    for (DevBuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (View &v : c->views)
        if (v.masks.p) (void)hipFree(v.masks.p);
    if (c->rows) (void)hipFree(c->rows);
    pinned_free(c->pin, c->pin_cap);
    if (c->pin_small) (void)hipHostFree(c->pin_small);
    if (c->stage) (void)hipHostFree(c->stage);
    if (c->zc_out) (void)hipHostFree(c->zc_out);
    if (c->hint_pin) (void)hipHostFree(c->hint_pin);
    if (c->hint_prior_pin) (void)hipHostFree(c->hint_prior_pin);
    if (c->order_pin) (void)hipHostFree(c->order_pin);
    mh_ahead_destroy(c);
    if (c->mh_pin) (void)hipHostFree(c->mh_pin);
    for (int p = 0; p < 2; p++)
        if (c->mh_ev[p]) (void)hipEventDestroy(c->mh_ev[p]);
    for (int s = 0; s < BNPC_TILE_SLOTS; s++) {
        pinned_free(c->tile_pin[s], c->tile_cap[s]);
        pinned_free(c->tile_rows[s], c->tile_rows_cap[s]);
        pinned_free(c->tile_cells[s], c->tile_cells_cap[s]);
        pinned_free(c->tile_hint[s], c->tile_hint_cap[s]);
        pinned_free(c->tile_prior[s], c->tile_prior_cap[s]);
        if (c->tile_done[s]) (void)hipEventDestroy(c->tile_done[s]);
    }
    for (int s = 0; s < 2; s++) {
        if (c->tile_summed[s]) (void)hipEventDestroy(c->tile_summed[s]);
        if (c->tile_out_free[s]) (void)hipEventDestroy(c->tile_out_free[s]);
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->ev_hints) (void)hipEventDestroy(c->ev_hints);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    delete c;
    return 0;
}

extern "C" int bnpc_reload_options(bnpc_ctx *c)
{
    ARGCHK(c, "ctx is NULL");
    read_tunables(c->tun);
    return 0;
}

extern "C" int bnpc_shape(const bnpc_ctx *c, int64_t *N, int64_t *M)
{
    ARGCHK(c, "ctx is NULL");
    if (N) *N = c->N;
    if (M) *M = c->M;
    return 0;
}

// the {ones, zeros} words of one cell's row (bnpc_sweeps.cpp: native births)
const unsigned long long *bnpc_ctx_row(const bnpc_ctx *c, int64_t cell,
                                       int64_t *M, int *W)
{
    if (!c || cell < 0 || cell >= c->N || c->host_rows.empty()) return nullptr;
    if (M) *M = c->M;
    if (W) *W = c->W;
    return (const unsigned long long *)(c->host_rows.data()
                                        + (size_t)cell * c->W);
}

extern "C" int bnpc_cell_counts(bnpc_ctx *c, int32_t *n1, int32_t *n0)
{
    ARGCHK(c && n1 && n0, "NULL argument");
    memcpy(n1, c->cell_n1.data(), c->N * sizeof(int32_t));
    memcpy(n0, c->cell_n0.data(), c->N * sizeof(int32_t));
    return 0;
}

extern "C" int bnpc_view_set(bnpc_ctx *c, int view, const int64_t *cells,
                             int64_t n)
{
    ARGCHK(c, "ctx is NULL");
    ARGCHK(view >= 1 && view < BNPC_MAX_VIEWS, "view out of range");
    ARGCHK(n >= 0 && (n == 0 || cells), "cells is NULL");
    for (int64_t i = 0; i < n; i++)
        ARGCHK(cells[i] >= 0 && cells[i] < c->N, "cell index out of range");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) {
        c->views[view].n = 0;
        c->views[view].nblk = 0;
        return 0;
    }
    // The cell list travels through a pinned buffer of its own (N entries,
    // read in place by the gather kernel), so the call returns without
    // waiting for the device: what uses the view is queued behind the gather
    // on the same stream, and the buffer is only written again once the
    // gather that read it last has finished (an event; it has, long since,
    // in a split / merge move: a 12 us wait per move otherwise).
    if (!c->view_cells_pin) {
        void *pin = nullptr, *dev = nullptr;
        if (hipHostMalloc(&pin, (size_t)c->N * sizeof(long long),
                          hipHostMallocDefault) == hipSuccess
            && hipHostGetDevicePointer(&dev, pin, 0) == hipSuccess
            && hipEventCreateWithFlags(&c->view_cells_read,
                                       hipEventDisableTiming) == hipSuccess) {
            c->view_cells_pin = pin;
            c->view_cells_dev = (const long long *)dev;
        } else {
            (void)hipGetLastError();
            if (pin) (void)hipHostFree(pin);
        }
    }
    if (c->view_cells_pin && n <= c->N && !c->any_tile_pending()) {
        if (c->view_cells_busy) {
            HIPCHK(hipEventSynchronize(c->view_cells_read));
            c->view_cells_busy = false;
        }
        memcpy(c->view_cells_pin, cells, n * sizeof(long long));
        if (build_view(c, view, c->view_cells_dev, n)) return 1;
        HIPCHK(hipEventRecord(c->view_cells_read, c->stream));
        c->view_cells_busy = true;
        return 0;
    }
    if (arena_reset(c)) return 1;
    const long long *d_cells = (const long long *)stage_in_place(
        c, cells, n * sizeof(long long));
    if (!d_cells) {
        if (ensure(c->cells, n * sizeof(long long))) return 1;
        if (h2d(c, c->cells.p, cells, n * sizeof(long long))) return 1;
        d_cells = (const long long *)c->cells.p;
    }
    if (build_view(c, view, d_cells, n)) return 1;
    // the caller's buffer is only borrowed: finish the copy before returning
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int ensure_host(void **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return 0;
    pinned_free(*p, *cap);
    *p = nullptr;
    *cap = 0;
    // tiles of a sweep are sized to a byte budget: little slack is needed
    return pinned_alloc(p, cap, bytes + bytes / 16 + 4096);
}

// bnpc_view_set for a tile of a tiled sweep: the cell list is staged in the
// tile slot's own pinned buffer (read in place by the gather kernel) and
// NOTHING is waited for - the stream may hold the sums of the tiles issued
// before, which a synchronisation here would serialise with the host.  The
// view is for work issued behind it on the context's stream
// (bnpc_ll_rows_issue on the same slot).
extern "C" int bnpc_view_set_slot(bnpc_ctx *c, int view, const int64_t *cells,
                                  int64_t n, int slot)
{
    ARGCHK(c, "ctx is NULL");
    ARGCHK(view >= 1 && view < BNPC_MAX_VIEWS, "view out of range");
    ARGCHK(slot >= 0 && slot < BNPC_TILE_SLOTS, "slot out of range");
    ARGCHK(n > 0 && cells, "empty cell list");
    ARGCHK(!c->tile_pending[slot], "slot has an unconsumed tile");
    for (int64_t i = 0; i < n; i++)
        ARGCHK(cells[i] >= 0 && cells[i] < c->N, "cell index out of range");
    HIPCHK(hipSetDevice(c->device));
    if (ensure_lanes(c)) return 1;
    // (for all N cells at once: tiles grow as the clusters die, and growing
    // a pinned buffer means hipHostFree - a device-wide synchronisation of
    // ~5 ms in the middle of the pipeline; measured: 33 of them, 0.17 s of a
    // config-5 first sweep)
    if (ensure_host(&c->tile_cells[slot], &c->tile_cells_cap[slot],
                    std::max<int64_t>(n, c->N) * sizeof(long long)))
        return 1;
    memcpy(c->tile_cells[slot], cells, n * sizeof(long long));
    void *d = nullptr;
    HIPCHK(hipHostGetDevicePointer(&d, c->tile_cells[slot], 0));
    // Tiles grow as the clusters die (1024 cells, then 1536, 2048, ...), and
    // growing a device buffer means hipFree - a device-wide synchronisation
    // in the middle of the pipeline.  Room for 4 x the first tile, at least
    // 16384 cells (all cells if there are fewer), is taken at once.
    View &v = c->views[view];
    int64_t room = std::max<int64_t>(4 * n, 16384);
    room = std::min<int64_t>(std::max<int64_t>(room, n), std::max(c->N, n));
    if (ensure(v.masks, ((size_t)((room + 63) / 64) * c->Mpad + 8)
                            * sizeof(ulonglong2)))
        return 1;
    return build_view(c, view, (const long long *)d, n);
}

extern "C" int bnpc_view_size(const bnpc_ctx *c, int view, int64_t *n)
{
    ARGCHK(c && n, "NULL argument");
    ARGCHK(view >= 0 && view < BNPC_MAX_VIEWS, "view out of range");
    *n = c->views[view].n;
    return 0;
}

