// bnpc_post.h - the posterior handle and the host-side pieces every posterior
// pass's driver is made of.  Internal to bnpc_codist.hip (the handle and the
// passes over the labels and the pair counts), bnpc_post_ward.hip (Ward's
// linkage of the pair counts) and bnpc_post_passes.hip (the passes over the
// parameter trace or the data).
//
// No kernel is declared here: a kernel is launched only from the translation
// unit that defines it, so the two helpers that launch one
// (post_check_distinct: k_cg_rank, post_build_masks: k_mf_masks) stand beside
// their kernels in bnpc_post_passes.hip.  What one file alone holds stays in
// that file too: the handle's owner while it is made (bnpc_codist.hip), the
// holder of Ward's stream and captured graph (bnpc_post_ward.hip).
//
// What every driver keeps, whatever it shares:
//   - the order of its checks: the arguments (code 2), the handle's labels,
//     the rates, the samples' cluster counts against the trace, the codes,
//     then memory (code 5);
//   - the order of its allocations in front of hipMemGetInfo: the default
//     slab is computed from what is free after them;
//   - every launch (grid, block, LDS bytes, arguments, stream 0) and its
//     place between the laps: the ms[] slots of the _times entry points mean
//     what their comments say.
#ifndef BNPC_POST_H
#define BNPC_POST_H
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "bnpc_hip.h"
#include "bnpc_internal.h"

struct bnpc_post {
    int device = 0;
    int64_t S = 0, N = 0;
    int *differ = nullptr;                  // condensed, device
    int *assign = nullptr;                  // the S x N samples, device
    bool labels_in_range = false;           // every sample label in [0, N)
    unsigned long long *sums = nullptr;     // device scratch
    long long ward_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // row scans / chain steps of the
                                            // last bnpc_post_ward
};

#define PCK(expr)                                                            \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            bnpc_set_error("%s failed: %s", #expr, hipGetErrorString(e_));   \
            return 1;                                                        \
        }                                                                    \
    } while (0)

#define GT_MIXED 0xfffeu        // no cluster / no row: labels and rows lie below
#define GT_GLOBAL_WG 512        // workgroups of a per-sample kernel on global slices

// 0, or 5 with "<pass>: out of device memory (...)", or 1 for any other error
inline int post_alloc_rc(const char *pass, hipError_t e)
{
    if (e == hipSuccess) return 0;
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        bnpc_set_error("%s: out of device memory (%s)", pass,
                       hipGetErrorString(e));
        return 5;
    }
    bnpc_set_error("%s: a device allocation failed: %s", pass,
                   hipGetErrorString(e));
    return 1;
}

// device buffers of one call of a pass, freed on every return
struct PostBuffers {
    std::vector<void *> p;
    PostBuffers() = default;
    PostBuffers(const PostBuffers &) = delete;
    PostBuffers &operator=(const PostBuffers &) = delete;
    template <class T> hipError_t alloc(T **out, size_t count)
    {
        *out = nullptr;
        p.reserve(p.size() + 1);            // (before there is anything to lose)
        hipError_t e = hipMalloc((void **)out, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p.push_back((void *)*out);
        return e;
    }
    template <class T> int alloc_or_oom(const char *pass, T **out, size_t count)
    {
        return post_alloc_rc(pass, alloc(out, count));
    }
    ~PostBuffers()
    {
        for (void *q : p) (void)hipFree(q);
    }
};

// inside a driver: buf.alloc_or_oom, or the driver returns its code
#define POST_ALLOC(buf, pass, out, count)                                    \
    do {                                                                     \
        if (int rc_ = (buf).alloc_or_oom(pass, out, count)) return rc_;      \
    } while (0)

// two device events, destroyed on every return
struct PostEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    PostEvents() = default;
    PostEvents(const PostEvents &) = delete;
    PostEvents &operator=(const PostEvents &) = delete;
    hipError_t create()
    {
        hipError_t e = hipEventCreate(&ev[0]);
        return e == hipSuccess ? hipEventCreate(&ev[1]) : e;
    }
    ~PostEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// the laps of the device's clock behind a _times entry point: begin(), the
// work, end(its slot of ms).  Inert where ms is NULL.
struct PostLaps {
    PostEvents evs;
    float *ms = nullptr;
    bool bad = false;
    // timing is on where ms_ is not NULL: ms_[0 .. n) start at zero
    hipError_t start(float *ms_, int n)
    {
        if (!ms_) return hipSuccess;
        for (int k = 0; k < n; k++) ms_[k] = 0.0f;
        ms = ms_;
        return evs.create();
    }
    void begin()
    {
        if (ms && hipEventRecord(evs.ev[0], 0) != hipSuccess) bad = true;
    }
    void end(int slot)
    {
        if (!ms) return;
        float t = 0.0f;
        if (hipEventRecord(evs.ev[1], 0) != hipSuccess
            || hipEventSynchronize(evs.ev[1]) != hipSuccess
            || hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]) != hipSuccess)
            bad = true;
        ms[slot] += t;
    }
    bool failed() const { return bad; }
    // a driver's last word: 0, or 1 where a lap failed
    int result(const char *pass) const
    {
        if (!failed()) return 0;
        bnpc_set_error("%s: the device events failed", pass);
        return 1;
    }
};

// where a per-sample kernel's working set of `words` goes: LDS while it fits
// lds_max (a workgroup per sample), else a global slice per workgroup.
// raise: the kernel whose dynamic-LDS limit is raised to lds_max (the genotype
// pass, past 64 KiB), or NULL where lds_max needs no raising (the rank pass).
struct PostArea {
    unsigned grid = 0;
    size_t lds = 0;
    unsigned *scratch = nullptr;
    long long stride = 0;
};
inline hipError_t post_rank_area(const void *raise, long long words,
                                 size_t lds_max, int64_t S, PostBuffers &buf,
                                 PostArea &a)
{
    if ((size_t)words * 4 <= lds_max) {
        a.grid = (unsigned)std::min<int64_t>(S, 65535);
        a.lds = (size_t)words * 4;
        return raise ? hipFuncSetAttribute(raise,
                           hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)lds_max)
                     : hipSuccess;
    }
    a.grid = (unsigned)std::min<int64_t>(S, GT_GLOBAL_WG);
    a.stride = words;
    return buf.alloc(&a.scratch, (size_t)a.grid * words);
}

// the handle holds its samples and their labels index a cell: 0 or 2
inline int post_check_handle(const char *pass, const bnpc_post *p)
{
    if (p->assign && p->labels_in_range) return 0;
    bnpc_set_error("%s: the sample labels must lie in [0, N = %lld)", pass,
                   (long long)p->N);
    return 2;
}

// every sample's error rates are probabilities strictly inside (0, 1): 0 or 2
inline int post_check_rates(const char *pass, const double *FN,
                            const double *FP, int64_t S)
{
    for (int64_t s = 0; s < S; s++) {
        if (!(FN[s] > 0.0 && FN[s] < 1.0 && FP[s] > 0.0 && FP[s] < 1.0)) {
            bnpc_set_error("%s: FN = %g, FP = %g of sample %lld are not both "
                           "inside (0, 1)", pass, FN[s], FP[s], (long long)s);
            return 2;
        }
    }
    return 0;
}

// the samples of a chunk of the trace: the caller's `chunk`, or where that is
// 0 what 512 MiB hold at bytes_per_sample; one at the least, S and what a
// launch takes as an int at the most
inline int64_t post_default_chunk(int64_t chunk, size_t bytes_per_sample,
                                  int64_t S)
{
    int64_t sc = chunk;
    if (sc == 0)
        sc = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20)
                                            / bytes_per_sample));
    return std::min<int64_t>(std::min(sc, S), INT_MAX);
}

// the cells of a slab of codes while the lane masks are built: whole blocks
// of 64 - 64 cells at the least, about 64 MB of codes and what a launch's
// second dimension takes at the most
inline int64_t post_mask_slab_cells(int64_t N, int64_t M)
{
    const int64_t nb = (N + 63) / 64;
    return 64 * std::min<int64_t>(std::min<int64_t>(nb, 65535),
        std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / ((size_t)M * 64))));
}

#endif
