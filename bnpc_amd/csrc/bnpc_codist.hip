// bnpc_codist.hip - posterior co-clustering distance.
//
//   differ[(i,j)] = #{ samples s : assignment[s][i] != assignment[s][j] },
//   i < j, condensed in scipy's pdist order
//   = the per-sample pdist(..., 'hamming') accumulation of
//     utils.get_dist (/root/reference/libs/utils.py:90-97); the mean distance
//     is differ / S.  Exact integers -> bit-exact parity.
//
// Work is S * N^2 / 2 label compares (4e10 at 3350 samples x 5000 cells): a
// workgroup owns a 64 x 64 tile of cell pairs, streams the samples through
// LDS 32 at a time (two 64-label rows per sample) and every thread keeps a
// 4 x 4 block of pair counters in registers.  int32 VALU, LDS-broadcast
// reads; only tiles on or above the diagonal do any work.
//
// This file holds what works on the labels and the pair counts alone: the
// handle, MPEAR, the support pass and the chain agreement.  Ward's linkage of
// the pair counts is in bnpc_post_ward.hip, the passes over the parameter
// trace or the data behind the same handle are in bnpc_post_passes.hip, the
// handle and the drivers' pieces in bnpc_post.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <vector>

#include "bnpc_hip.h"
#include "bnpc_internal.h"
#include "bnpc_post.h"

#define SC 32       // samples staged per LDS round

__global__ __launch_bounds__(256) void k_codist(
    const int *__restrict__ assign, long long S, long long N,
    int *__restrict__ differ)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ int A[SC][64];
    __shared__ int B[SC][64];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    int cnt[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) cnt[a][b] = 0;

    for (long long s0 = 0; s0 < S; s0 += SC) {
        // stage SC samples x (64 + 64) labels: 4096 ints by 256 threads
#pragma unroll
        for (int r = 0; r < (2 * SC * 64) / 256; r++) {
            const int e = r * 256 + tid;
            const int which = e / (SC * 64);
            const int rem = e - which * (SC * 64);
            const int sc = rem >> 6, col = rem & 63;
            const long long s = s0 + sc;
            const long long cell = (long long)(which ? tj : ti) * 64 + col;
            int v = -1 - col;       // padding never equals a real label
            if (s < S && cell < N) v = assign[s * N + cell];
            if (which) B[sc][col] = v; else A[sc][col] = v;
        }
        __syncthreads();
        const int lim = (S - s0 < SC) ? (int)(S - s0) : SC;
        for (int sc = 0; sc < lim; sc++) {
            const int4 av = *reinterpret_cast<const int4 *>(&A[sc][ty * 4]);
            const int4 bv = *reinterpret_cast<const int4 *>(&B[sc][tx * 4]);
            const int a4[4] = {av.x, av.y, av.z, av.w};
            const int b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) cnt[a][b] += (a4[a] != b4[b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const long long i = (long long)ti * 64 + ty * 4 + a;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const long long j = (long long)tj * 64 + tx * 4 + b;
            if (i < j && j < N) {
                const long long idx = i * (2 * N - i - 1) / 2 + (j - i - 1);
                differ[idx] = cnt[a][b];
            }
        }
    }
}

// a tile of 64 x 64 pairs per workgroup, the whole square of tiles
static void cd_launch(const int *d_assign, int64_t S, int64_t N, int *d_differ)
{
    const unsigned nt = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(k_codist, dim3(nt, nt), dim3(256), 0, 0, d_assign,
                       (long long)S, (long long)N, d_differ);
}

extern "C" int bnpc_codist(int device, const int32_t *assignments, int64_t S,
                           int64_t N, int32_t *differ)
{
    if (!assignments || !differ || S < 1 || N < 2) {
        bnpc_set_error("bad argument: need S >= 1 samples of N >= 2 cells");
        return 2;
    }
    const size_t pairs = (size_t)N * (N - 1) / 2;
    PCK(hipSetDevice(device));
    PostBuffers buf;
    int *d_a = nullptr, *d_d = nullptr;
    PCK(buf.alloc(&d_a, (size_t)S * N));
    PCK(buf.alloc(&d_d, pairs));
    PCK(hipMemcpy(d_a, assignments, (size_t)S * N * sizeof(int),
                  hipMemcpyHostToDevice));
    cd_launch(d_a, S, N, d_d);
    PCK(hipGetLastError());
    PCK(hipMemcpy(differ, d_d, pairs * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------
// The posterior estimator as a pipeline: the pair
// counts STAY on the device, the mean distance goes to the host once (SciPy's
// Ward linkage needs it there), and every candidate cut of the tree is scored
// on the device in one pass over the counts.
//
// MPEAR of a clustering c (Fritsch & Ickstadt 2009, eq. 13;
// /root/reference/libs/utils.py:133-145) needs, with pi = 1 - differ / S,
//     I_sum  = #{pairs with c_i == c_j}            (from the label counts)
//     pi_sum = P - sum(differ) / S                  (one sum, all candidates)
//     index  = sum_{c_i == c_j} pi = I_sum - D_c / S,
//     D_c    = sum_{i < j, c_i == c_j} differ_ij   <- k_mpear_sums, int64
// i.e. exact integers, order-free; the float64 `pi` (10 GB at 50 000 cells)
// and the reference's pass over it per candidate are never made.
//
// k_mpear_sums: persistent workgroups walk the 64 x 64 pair tiles on or above
// the diagonal; a tile's counts sit in LDS (pairs with i >= j as zeros), the
// labels of its 64 + 64 cells under CP candidates beside them, candidate
// fastest (conflict-free: the lanes of a wave read consecutive candidates of
// one cell, the count of one pair is a broadcast).  Thread = (candidate,
// row part): it adds the counts of its pairs whose two cells share the
// candidate's label into ONE register accumulator that lives across all its
// tiles - no reduction inside the loop; at the end the parts are added
// through LDS and each workgroup makes one 64-bit atomic add per candidate.
// ---------------------------------------------------------------------------
#define MP_MAXCP 128

__global__ __launch_bounds__(256) void k_mpear_sums(
    const int *__restrict__ differ, long long N,
    const unsigned short *__restrict__ labels,  // [C][N]
    int c0, int C, int CP, unsigned long long *__restrict__ out)
{
    __shared__ int D[64][64];
    __shared__ unsigned short LA[64][MP_MAXCP];
    __shared__ unsigned short LB[64][MP_MAXCP];
    __shared__ unsigned long long red[256];
    const int tid = threadIdx.x;
    const int c = tid % CP, part = tid / CP, parts = 256 / CP;
    const long long nt = (N + 63) / 64;
    const long long tiles = nt * (nt + 1) / 2;
    unsigned long long acc = 0;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        // tile index -> (ti <= tj), rows of the upper triangle in order
        long long ti = (long long)((2.0 * nt + 1.0
            - sqrt((2.0 * nt + 1.0) * (2.0 * nt + 1.0) - 8.0 * (double)t))
            * 0.5);
        while (ti > 0 && ti * (2 * nt - ti + 1) / 2 > t) ti--;
        while ((ti + 1) * (2 * nt - ti) / 2 <= t) ti++;
        const long long tj = ti + (t - ti * (2 * nt - ti + 1) / 2);
        __syncthreads();                        // the previous tile is done
        for (int e = tid; e < 4096; e += 256) {
            const int a = e >> 6, b = e & 63;
            const long long i = ti * 64 + a, j = tj * 64 + b;
            int v = 0;
            if (i < j && j < N)
                v = differ[i * (2 * N - i - 1) / 2 + (j - i - 1)];
            D[a][b] = v;
        }
        for (int e = tid; e < 64 * CP; e += 256) {
            const int cell = e / CP, cc = e - cell * CP;
            const long long i = ti * 64 + cell, j = tj * 64 + cell;
            const bool live = c0 + cc < C;
            // cells past N / candidates past C: labels that match nothing
            LA[cell][cc] = (live && i < N)
                ? labels[(size_t)(c0 + cc) * N + i] : (unsigned short)0xfffe;
            LB[cell][cc] = (live && j < N)
                ? labels[(size_t)(c0 + cc) * N + j] : (unsigned short)0xffff;
        }
        __syncthreads();
        for (int a = part; a < 64; a += parts) {
            const unsigned short la = LA[a][c];
            unsigned sum = 0;                   // 64 counts <= S each
#pragma unroll 8
            for (int b = 0; b < 64; b++)
                sum += (LB[b][c] == la) ? (unsigned)D[a][b] : 0u;
            acc += sum;
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (part == 0) {
        unsigned long long s = 0;
        for (int p = 0; p < parts; p++) s += red[p * CP + c];
        if (c0 + c < C && s) atomicAdd(&out[c0 + c], s);
    }
}

// sum of all pair counts (pi_sum), fixed grid, one atomic per workgroup
__global__ __launch_bounds__(256) void k_differ_sum(
    const int *__restrict__ differ, long long pairs,
    unsigned long long *__restrict__ out)
{
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs;
         i += (long long)gridDim.x * 256)
        acc += (unsigned long long)differ[i];
    __shared__ unsigned long long red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicAdd(out, red[0]);
}

// mean distance differ / S as float64 (what SciPy's linkage takes): the same
// IEEE division NumPy performs on the host, 16 bytes per lane coalesced
__global__ __launch_bounds__(256) void k_differ_to_dist(
    const int *__restrict__ differ, long long pairs, double S,
    double *__restrict__ dist)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs;
         i += (long long)gridDim.x * 256)
        dist[i] = (double)differ[i] / S;
}

// the sum of the handle's pair counts, added to p->sums[0]
static void ds_launch(const bnpc_post *p)
{
    const long long pairs = (long long)p->N * (p->N - 1) / 2;
    hipLaunchKernelGGL(k_differ_sum, dim3(1024), dim3(256), 0, 0, p->differ,
                       pairs, p->sums);
}

// candidates [c0, c0 + CP) of C, their sums added to p->sums[1 + candidate]
static void mp_launch(const bnpc_post *p, const unsigned short *d_lab, int c0,
                      int C, int CP)
{
    hipLaunchKernelGGL(k_mpear_sums, dim3(1024), dim3(256), 0, 0, p->differ,
                       (long long)p->N, d_lab, c0, C, CP, p->sums + 1);
}

extern "C" int bnpc_post_destroy(bnpc_post *p)
{
    if (!p) return 0;
    (void)hipSetDevice(p->device);
    if (p->differ) (void)hipFree(p->differ);
    if (p->assign) (void)hipFree(p->assign);
    if (p->sums) (void)hipFree(p->sums);
    delete p;
    return 0;
}

// a handle in the making: destroyed with what it holds unless released
struct PostDestroy {
    void operator()(bnpc_post *p) const { (void)bnpc_post_destroy(p); }
};

extern "C" int bnpc_post_create(int device, const int32_t *assignments,
                                int64_t S, int64_t N, bnpc_post **out,
                                int64_t *differ_sum)
{
    if (!assignments || !out || S < 1 || N < 2) {
        bnpc_set_error("bad argument: need S >= 1 samples of N >= 2 cells");
        return 2;
    }
    *out = nullptr;
    PCK(hipSetDevice(device));
    std::unique_ptr<bnpc_post, PostDestroy> owner(new bnpc_post());
    bnpc_post *const p = owner.get();
    p->device = device;
    p->S = S;
    p->N = N;
    const size_t pairs = (size_t)N * (N - 1) / 2;
    PCK(hipMalloc((void **)&p->assign, (size_t)S * N * sizeof(int)));
    PCK(hipMalloc((void **)&p->differ, pairs * sizeof(int)));
    PCK(hipMalloc((void **)&p->sums, (1024 + 1) * sizeof(unsigned long long)));
    PCK(hipMemcpy(p->assign, assignments, (size_t)S * N * sizeof(int),
                  hipMemcpyHostToDevice));
    cd_launch(p->assign, S, N, p->differ);
    PCK(hipGetLastError());
    PCK(hipMemsetAsync(p->sums, 0, sizeof(unsigned long long), 0));
    ds_launch(p);
    PCK(hipGetLastError());
    // the samples stay on the device for bnpc_post_genotypes, which indexes
    // with their labels: the range is checked here, on the host
    int lo = 0, hi = 0;
    const size_t total_labels = (size_t)S * N;
    if (total_labels) lo = hi = assignments[0];
    for (size_t i = 0; i < total_labels; i++) {
        lo = std::min(lo, assignments[i]);
        hi = std::max(hi, assignments[i]);
    }
    p->labels_in_range = lo >= 0 && (int64_t)hi < N;
    unsigned long long total = 0;
    PCK(hipMemcpy(&total, p->sums, sizeof total, hipMemcpyDeviceToHost));
    if (differ_sum) *differ_sum = (int64_t)total;
    *out = owner.release();
    return 0;
}

// condensed pair counts / mean distances to the host (either may be NULL)
extern "C" int bnpc_post_fetch(bnpc_post *p, int32_t *differ, double *dist)
{
    if (!p) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    PCK(hipSetDevice(p->device));
    const size_t pairs = (size_t)p->N * (p->N - 1) / 2;
    if (differ)
        PCK(hipMemcpy(differ, p->differ, pairs * sizeof(int),
                      hipMemcpyDeviceToHost));
    if (dist) {
        // in slabs: the float64 form is twice the counts (10 GB at 50 000)
        const size_t slab = (size_t)64 << 20;           // elements
        PostBuffers buf;
        double *d_slab = nullptr;
        PCK(buf.alloc(&d_slab, std::min(slab, pairs)));
        for (size_t at = 0; at < pairs; at += slab) {
            const size_t n = std::min(slab, pairs - at);
            hipLaunchKernelGGL(k_differ_to_dist, dim3(2048), dim3(256), 0, 0,
                               p->differ + at, (long long)n, (double)p->S,
                               d_slab);
            PCK(hipGetLastError());
            PCK(hipMemcpy(dist + at, d_slab, n * sizeof(double),
                          hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

// same_differ[c] = sum over pairs i < j with labels[c][i] == labels[c][j] of
// differ_ij, for C candidate clusterings (labels < 65534)
extern "C" int bnpc_post_mpear(bnpc_post *p, const uint16_t *labels, int64_t C,
                               int64_t *same_differ)
{
    if (!p || !labels || !same_differ || C < 1 || C > 1024) {
        bnpc_set_error("bad argument: mpear sums of 1..1024 candidates");
        return 2;
    }
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    unsigned short *d_lab = nullptr;
    const size_t count = (size_t)C * p->N;
    PCK(buf.alloc(&d_lab, count));
    PCK(hipMemcpy(d_lab, labels, count * sizeof(unsigned short),
                  hipMemcpyHostToDevice));
    PCK(hipMemset(p->sums, 0, 1025 * sizeof(unsigned long long)));
    const int CP = C <= 32 ? 32 : (C <= 64 ? 64 : 128);
    for (int c0 = 0; c0 < C; c0 += CP) {
        mp_launch(p, d_lab, c0, (int)C, CP);
        PCK(hipGetLastError());
    }
    unsigned long long host[1024];
    PCK(hipMemcpy(host, p->sums + 1, C * sizeof(unsigned long long),
                  hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < C; c++) same_differ[c] = (int64_t)host[c];
    return 0;
}

// ---------------------------------------------------------------------------
// Per-cell cluster support (what the reference shows as the N x N posterior
// similarity heat map, libs/dpmmIO.py:245-274 of the reference, reduced to
// tables that mean something at any size): for a clustering `labels`,
//   differ_to[i][k] = sum over cells j != i with labels[j] == k of differ_ij
// int64, exact; everything else (support, cluster similarity) is the host's.
//
// One workgroup owns a block of 64 cells and produces that block's finished
// rows: it walks all ceil(N / 64) tiles of its stripe through LDS - right of
// the diagonal as the row stripe (i in the block, j), left of it as the
// column stripe (i, j in the block: 256-byte runs per i), the diagonal tile
// once, mirrored - so that every tile is read twice in total, nothing is
// added to global memory by two workgroups, and every workgroup has the same
// work.  The condensed rows start at any 4-byte offset, so the loads are
// 4 bytes per lane, 256 contiguous bytes per wave.
//
// A tile sits in LDS as T[other cell][own cell] (rows padded to 65: the
// transposing stores of a row-stripe tile are conflict-free too).  Thread =
// (own cell a, a quarter of the other cells b): it adds T[b][a] into
// acc[labels[b]][a], a 64-bit accumulator in LDS (own cell fastest: the lanes
// of a wave hit consecutive addresses, the label is a broadcast).  The four
// waves may meet on one accumulator, so the add is an LDS atomic - integers:
// the result does not depend on the order.  The next two tiles' 16 counts
// per thread each are in flight while the current one is added up.
//
// K > BNPC_SUPPORT_KC runs in passes (blockIdx.y) of that many clusters;
// labels outside the pass are skipped.  The accumulators take what the
// clustering needs, min(K, KC) * 512 bytes: 4 workgroups per compute unit up
// to 40 clusters, 1 at 128.
// ---------------------------------------------------------------------------
#define PS_KC BNPC_SUPPORT_KC
#define PS_TILE_WORDS (64 * 65 + 64)    // T[64][65], labels of the other cells

static size_t ps_lds_bytes(int64_t K)
{
    return (size_t)std::min<int64_t>(K, PS_KC) * 64 * sizeof(unsigned long long)
        + PS_TILE_WORDS * sizeof(int);
}

__global__ __launch_bounds__(256) void k_post_support(
    const int *__restrict__ differ, long long N,
    const int *__restrict__ labels,         // padded to 64 * ceil(N / 64): -1
    int K, long long *__restrict__ out)     // [N][K]
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long ps_lds[];
    const int tid = threadIdx.x;
    const long long nb = (N + 63) / 64, own = blockIdx.x;
    const int k0 = (int)blockIdx.y * PS_KC;
    const int kc = K - k0 < PS_KC ? K - k0 : PS_KC;
    const int kc_lds = K < PS_KC ? K : PS_KC;
    unsigned long long *acc = ps_lds;                   // [kc][64]
    int *T = (int *)(ps_lds + (size_t)kc_lds * 64);     // [64][65]
    int *lab = T + 64 * 65;                             // [64]
    for (int e = tid; e < kc * 64; e += 256) acc[e] = 0;

    // element (r, c) of tile t: pair (R0 + r, C0 + c), thread -> c fastest;
    // left of the diagonal the tile's rows are the other cells.  The index of
    // pair (i, j) is off(i) + j, off(i) = i (2N - i - 1) / 2 - i - 1: one
    // 64-bit product per tile, then off(i + 4) = off(i) + 4 (N - i) - 14.
    // A pair outside the triangle reads element 0 and counts as zero: the
    // loads are unconditional and stay in flight together.
    const int c = tid & 63, rq = tid >> 6;
    auto fetch = [&](long long t, int (&v)[16], int &lv) {
        const int j = (int)(t < own ? own : t) * 64 + c;
        int i = (int)(t < own ? t : own) * 64 + rq;
        long long off = (long long)i * (2 * N - i - 1) / 2 - i - 1;
        const bool inside = j < N;
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const bool pair = inside && i < j;
            const int x = differ[pair ? off + j : 0];
            v[u] = pair ? x : 0;
            off += 4 * (N - i) - 14;
            i += 4;
        }
        lv = labels[t * 64 + c];
    };
    // tile t from its registers into LDS, tile t + 2 into the registers,
    // tile t added up
    auto step = [&](long long t, int (&v)[16], int &lv) {
        __syncthreads();                    // the previous tile is added up
        if (t < own) {                      // other = r, own = c
#pragma unroll
            for (int u = 0; u < 16; u++) T[(u * 4 + rq) * 65 + c] = v[u];
        } else if (t > own) {               // other = c, own = r
#pragma unroll
            for (int u = 0; u < 16; u++) T[c * 65 + u * 4 + rq] = v[u];
        } else {                            // the diagonal tile, mirrored
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int r = u * 4 + rq;
                if (r < c) T[c * 65 + r] = T[r * 65 + c] = v[u];
                if (r == c) T[r * 65 + r] = 0;
            }
        }
        if (rq == 0) lab[c] = lv;
        __syncthreads();
        if (t + 2 < nb) fetch(t + 2, v, lv);
        // own cell a = c, other cells b = 16 rq .. 16 rq + 15; a tile's count
        // is at most S, the sums over a stripe need the 64 bits
#pragma unroll 4
        for (int bb = 0; bb < 16; bb++) {
            const int b = rq * 16 + bb;
            const unsigned k = (unsigned)(lab[b] - k0);
            if (k < (unsigned)kc)
                atomicAdd(&acc[k * 64 + c],
                          (unsigned long long)(unsigned)T[b * 65 + c]);
        }
    };
    // two tiles of 16 counts per thread in flight: a workgroup alone on its
    // compute unit still covers most of the memory latency
    int va[16], vb[16], la = -1, lb = -1;
    fetch(0, va, la);
    if (nb > 1) fetch(1, vb, lb);
    for (long long t = 0; t < nb; t += 2) {
        step(t, va, la);
        if (t + 1 < nb) step(t + 1, vb, lb);
    }
    __syncthreads();
    for (int e = tid; e < 64 * kc; e += 256) {
        const int a = e / kc, k = e - a * kc;
        const long long i = own * 64 + a;
        if (i < N) out[i * K + k0 + k] = (long long)acc[k * 64 + a];
    }
}

// the clustering as the kernel takes it: compact in [0, K), none empty,
// padded to whole blocks with -1; 0 or the return code
static int ps_labels(const bnpc_post *p, const int32_t *labels, int64_t K,
                     std::vector<int> &lab)
{
    const int64_t N = p->N;
    lab.assign((size_t)((N + 63) / 64) * 64, -1);
    std::vector<int64_t> size(K, 0);
    for (int64_t i = 0; i < N; i++) {
        if (labels[i] < 0 || labels[i] >= K) {
            bnpc_set_error("support: cluster label %d of cell %lld is not in "
                           "[0, %lld)", labels[i], (long long)i, (long long)K);
            return 2;
        }
        lab[i] = labels[i];
        size[labels[i]]++;
    }
    for (int64_t k = 0; k < K; k++) {
        if (size[k] == 0) {
            bnpc_set_error("support: cluster %lld has no cells (labels must "
                           "be compact)", (long long)k);
            return 2;
        }
    }
    return 0;
}

// device copies of the labels and the N x K table; 0, 1 or 5 (the table does
// not fit the device's free memory: the return code of bnpc_post_ward)
static int ps_buffers(const bnpc_post *p, const std::vector<int> &lab,
                      int64_t K, PostBuffers &buf, int **d_lab,
                      long long **d_out)
{
    const int64_t N = p->N;
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    const size_t need = (size_t)N * K * sizeof(long long)
        + lab.size() * sizeof(int) + ((size_t)1 << 20);
    if (need > free_b) {
        bnpc_set_error("support: the %lld x %lld table needs %.1f GB, %.1f GB "
                       "of device memory are free", (long long)N, (long long)K,
                       need / 1e9, free_b / 1e9);
        return 5;
    }
    POST_ALLOC(buf, "support", d_lab, lab.size());
    POST_ALLOC(buf, "support", d_out, (size_t)N * K);
    PCK(hipMemcpy(*d_lab, lab.data(), lab.size() * sizeof(int),
                  hipMemcpyHostToDevice));
    PCK(hipFuncSetAttribute((const void *)k_post_support,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)ps_lds_bytes(PS_KC)));
    return 0;
}

static void ps_launch(const bnpc_post *p, const int *d_lab, int64_t K,
                      long long *d_out)
{
    const unsigned nb = (unsigned)((p->N + 63) / 64);
    const unsigned passes = (unsigned)((K + PS_KC - 1) / PS_KC);
    hipLaunchKernelGGL(k_post_support, dim3(nb, passes), dim3(256),
                       ps_lds_bytes(K), 0, p->differ, (long long)p->N, d_lab,
                       (int)K, d_out);
}

extern "C" int bnpc_post_support(bnpc_post *p, const int32_t *labels,
                                 int64_t K, int64_t *differ_to)
{
    if (!p || !labels || !differ_to || K < 1 || K >= (int64_t)GT_MIXED) {
        bnpc_set_error("bad argument: support needs labels, 1 <= K < 65534 "
                       "clusters and the output");
        return 2;
    }
    std::vector<int> lab;
    if (int rc = ps_labels(p, labels, K, lab)) return rc;
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    int *d_lab = nullptr;
    long long *d_out = nullptr;
    if (int rc = ps_buffers(p, lab, K, buf, &d_lab, &d_out)) return rc;
    ps_launch(p, d_lab, K, d_out);
    PCK(hipGetLastError());
    PCK(hipMemcpy(differ_to, d_out, (size_t)p->N * K * sizeof(long long),
                  hipMemcpyDeviceToHost));
    return 0;
}

// diagnostic (tools/posterior_bench.py): the three passes that read the whole
// matrix of pair counts, one launch each by device events, the fastest of
// `reps`: ms[0] k_differ_sum, ms[1] k_mpear_sums for the one clustering,
// ms[2] k_post_support
extern "C" int bnpc_post_pass_times(bnpc_post *p, const int32_t *labels,
                                    int64_t K, int reps, float *ms)
{
    if (!p || !labels || !ms || K < 1 || K >= (int64_t)GT_MIXED || reps < 1) {
        bnpc_set_error("bad argument: pass times need labels, 1 <= K < 65534 "
                       "clusters, reps >= 1 and the output");
        return 2;
    }
    std::vector<int> lab;
    if (int rc = ps_labels(p, labels, K, lab)) return rc;
    const int64_t N = p->N;
    std::vector<unsigned short> lab16(N);
    for (int64_t i = 0; i < N; i++) lab16[i] = (unsigned short)labels[i];
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    int *d_lab = nullptr;
    long long *d_out = nullptr;
    unsigned short *d_lab16 = nullptr;
    if (int rc = ps_buffers(p, lab, K, buf, &d_lab, &d_out)) return rc;
    PCK(buf.alloc(&d_lab16, N));
    PCK(hipMemcpy(d_lab16, lab16.data(), N * sizeof(unsigned short),
                  hipMemcpyHostToDevice));
    PostEvents evs;
    PCK(evs.create());
    for (int which = 0; which < 3; which++) {
        for (int r = 0; r < reps; r++) {
            // (the sums of the first two land in scratch nobody reads)
            PCK(hipMemsetAsync(p->sums, 0, 2 * sizeof(unsigned long long), 0));
            PCK(hipEventRecord(evs.ev[0], 0));
            if (which == 0)
                ds_launch(p);
            else if (which == 1)
                mp_launch(p, d_lab16, 0, 1, 32);
            else
                ps_launch(p, d_lab, K, d_out);
            PCK(hipGetLastError());
            float t = 0.0f;
            PCK(hipEventRecord(evs.ev[1], 0));
            PCK(hipEventSynchronize(evs.ev[1]));
            PCK(hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]));
            if (r == 0 || t < ms[which]) ms[which] = t;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Between-chain agreement of the clustering (-pc; not a reference output): do
// the chains of a pooled posterior hold the same co-clustering?  The pooled
// samples sit on the device chain after chain; bounds (C + 1 integers, 0 = b_0
// < ... < b_C = S) say where.  With S_c = b_{c+1} - b_c, R_c = S - S_c and,
// for a pair i != j, d_c the samples of chain c in which the two differ and
// d = sum_c d_c the pooled count (p->differ),
//   same_c = S_c - d_c,  same_r = (S - d) - same_c,
//   x      = same_c R_c - same_r S_c          (x / (S_c R_c): the pair's
//            co-clustering probability in chain c minus that in the rest)
//   flip   = [2 same_c > S_c] != [2 same_r > R_c]
//   abs_sum[c][i] = sum_{j != i} |x|, max_abs[c][i] = max_{j != i} |x|,
//   flips[c][i]   = sum_{j != i} flip.
// postproc.host_chain_agreement is the definition.  Integers only, so the
// tables do not depend on the order of the adds or on the launch: equal bits.
//
// k_chain_agree is k_codist's tile loop run chain by chain: a workgroup owns a
// 64 x 64 tile of pairs on or above the diagonal, a thread 4 x 4 counters, the
// samples go through LDS 32 at a time and a staging round ends at the chain's
// last sample.  The pooled counts of the tile are loaded once, into LDS (-1:
// not a pair i < j < N; 16 more registers a thread would cost a wave per SIMD,
// and the waves are what hides the LDS reads of the compare loop: measured
// 1.49 x k_codist with them in registers, 1.21 x from LDS).  At a chain's end
// the thread forms x, |x| and flip of its pairs - counts below 2^31 as 32-bit
// operands, their products and x in 64-bit integers - and zeroes its counters:
// the per-chain pair counts never reach memory (5 GB each at 50 000 cells).  A
// pair adds to the row of cell i and to the column of cell j: the rows are
// reduced over the 16 lanes that share them by shuffles, the columns over the
// 4 rows of a wave by shuffles and over the 4 waves through LDS, and then 64 +
// 64 consecutive threads add the tile's 128 cells into the three tables with
// 64-bit atomics - 512 contiguous bytes per wave instruction.  One tile per
// workgroup, as k_codist: 384 atomics per tile and chain, 9.4e8 of 8 bytes at
// 50 000 cells x 8 chains, beside 16 compares per thread and sample.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chain_agree(
    const int *__restrict__ assign, long long S, long long N,
    const int *__restrict__ differ, const long long *__restrict__ bounds,
    int C, unsigned long long *__restrict__ abs_sum,
    unsigned long long *__restrict__ max_abs,
    unsigned long long *__restrict__ flips)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ int A[SC][64];
    __shared__ int B[SC][64];
    __shared__ int PL[64][64];      // the tile's pooled counts
    __shared__ unsigned long long rowres[3][64];
    __shared__ unsigned long long colpart[4][3][64];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int wave = tid >> 6;
    int cnt[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const long long i = (long long)ti * 64 + ty * 4 + a;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const long long j = (long long)tj * 64 + tx * 4 + b;
            cnt[a][b] = 0;
            int pv = -1;
            if (i < j && j < N)
                pv = differ[i * (2 * N - i - 1) / 2 + (j - i - 1)];
            PL[ty * 4 + a][tx * 4 + b] = pv;    // read back by this thread only
        }
    }

    for (int c = 0; c < C; c++) {
        const long long s_lo = bounds[c], s_hi = bounds[c + 1];
        for (long long s0 = s_lo; s0 < s_hi; s0 += SC) {
#pragma unroll
            for (int r = 0; r < (2 * SC * 64) / 256; r++) {
                const int e = r * 256 + tid;
                const int which = e / (SC * 64);
                const int rem = e - which * (SC * 64);
                const int sc = rem >> 6, col = rem & 63;
                const long long s = s0 + sc;
                const long long cell = (long long)(which ? tj : ti) * 64 + col;
                int v = -1 - col;       // padding never equals a real label
                if (s < s_hi && cell < N) v = assign[s * N + cell];
                if (which) B[sc][col] = v; else A[sc][col] = v;
            }
            __syncthreads();
            const int lim = (s_hi - s0 < SC) ? (int)(s_hi - s0) : SC;
            for (int sc = 0; sc < lim; sc++) {
                const int4 av = *reinterpret_cast<const int4 *>(&A[sc][ty * 4]);
                const int4 bv = *reinterpret_cast<const int4 *>(&B[sc][tx * 4]);
                const int a4[4] = {av.x, av.y, av.z, av.w};
                const int b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        cnt[a][b] += (a4[a] != b4[b]);
            }
            __syncthreads();
        }

        // the chain against the rest, pair by pair
        const unsigned St = (unsigned)S, Sc = (unsigned)(s_hi - s_lo);
        const unsigned Rc = St - Sc;
        // (a row at a time: its sums are reduced over the 16 lanes of one
        // ty and stored before the next row's are formed - few live registers)
        unsigned long long cs[4], cm[4];
        unsigned cf[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cs[k] = cm[k] = 0;
            cf[k] = 0;
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            unsigned long long rs = 0, rm = 0;
            unsigned rf = 0;
            const int4 pv
                = *reinterpret_cast<const int4 *>(&PL[ty * 4 + a][tx * 4]);
            const int pooled[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (pooled[b] >= 0) {
                    // every count is below 2^31: 32-bit operands, 64-bit
                    // products.  same_c R_c - same_r S_c with same_r =
                    // same - same_c is same_c S - same S_c
                    const unsigned same_c = Sc - (unsigned)cnt[a][b];
                    const unsigned same = St - (unsigned)pooled[b];
                    const unsigned same_r = same - same_c;
                    const long long x
                        = (long long)((unsigned long long)same_c * St)
                        - (long long)((unsigned long long)same * Sc);
                    const unsigned long long ax
                        = (unsigned long long)(x < 0 ? -x : x);
                    const unsigned flip
                        = (2u * same_c > Sc) != (2u * same_r > Rc);
                    rs += ax;
                    cs[b] += ax;
                    rm = ax > rm ? ax : rm;
                    cm[b] = ax > cm[b] ? ax : cm[b];
                    rf += flip;
                    cf[b] += flip;
                }
                cnt[a][b] = 0;
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const unsigned long long m = __shfl_xor(rm, off);
                rs += __shfl_xor(rs, off);
                rf += __shfl_xor(rf, off);
                rm = m > rm ? m : rm;
            }
            if (tx == 0) {
                rowres[0][ty * 4 + a] = rs;
                rowres[1][ty * 4 + a] = rm;
                rowres[2][ty * 4 + a] = rf;
            }
        }
        // columns: over the 4 ty of a wave here, over the waves below
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const unsigned long long m = __shfl_xor(cm[k], off);
                cs[k] += __shfl_xor(cs[k], off);
                cf[k] += __shfl_xor(cf[k], off);
                cm[k] = m > cm[k] ? m : cm[k];
            }
        }
        if ((tid & 63) < 16) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                colpart[wave][0][tx * 4 + k] = cs[k];
                colpart[wave][1][tx * 4 + k] = cm[k];
                colpart[wave][2][tx * 4 + k] = cf[k];
            }
        }
        __syncthreads();
        // (the next chain's staging rounds put two barriers between these
        // reads and the next epilogue's writes: every chain has a sample)
        if (tid < 128) {
            const int t = tid & 63;
            unsigned long long vs, vm, vf;
            long long cell;
            if (tid < 64) {
                cell = (long long)ti * 64 + t;
                vs = rowres[0][t];
                vm = rowres[1][t];
                vf = rowres[2][t];
            } else {
                cell = (long long)tj * 64 + t;
                vs = vm = vf = 0;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const unsigned long long m = colpart[w][1][t];
                    vs += colpart[w][0][t];
                    vm = m > vm ? m : vm;
                    vf += colpart[w][2][t];
                }
            }
            if (cell < N) {
                const size_t at = (size_t)c * N + cell;
                if (vs) atomicAdd(&abs_sum[at], vs);
                if (vm) atomicMax(&max_abs[at], vm);
                if (vf) atomicAdd(&flips[at], vf);
            }
        }
    }
}

// reps == 0: the pass, its tables to the host.  reps >= 1 (ms: 2 floats): no
// output; ms[0] the fastest of reps passes (the tables' zeroing and
// k_chain_agree), ms[1] the fastest of reps k_codist launches over the same
// samples, which rewrite the handle's pair counts with the values they hold
static int ca_run(bnpc_post *p, const int64_t *bounds, int64_t C,
                  int64_t *abs_sum, int64_t *max_abs, int64_t *flips,
                  int reps, float *ms)
{
    if (!p || !bounds || C < 2 || C > (int64_t)INT_MAX) {
        bnpc_set_error("bad argument: the chain agreement needs the bounds of "
                       "C >= 2 chains");
        return 2;
    }
    const int64_t S = p->S, N = p->N;
    if (S > (int64_t)INT_MAX) {
        bnpc_set_error("chain agreement: %lld samples do not fit the 32-bit "
                       "pair counts", (long long)S);
        return 2;
    }
    if (bounds[0] != 0 || bounds[C] != S) {
        bnpc_set_error("chain agreement: the bounds run from %lld to %lld, "
                       "not from 0 to the %lld samples",
                       (long long)bounds[0], (long long)bounds[C],
                       (long long)S);
        return 2;
    }
    for (int64_t c = 0; c < C; c++) {
        const int64_t Sc = bounds[c + 1] - bounds[c];
        if (Sc < 1) {
            bnpc_set_error("chain agreement: chain %lld is empty (bounds "
                           "%lld, %lld)", (long long)c, (long long)bounds[c],
                           (long long)bounds[c + 1]);
            return 2;
        }
    }
    // (rising bounds from 0 to S: every chain lies inside the samples)
    for (int64_t c = 0; c < C; c++) {
        const int64_t Sc = bounds[c + 1] - bounds[c];
        const unsigned __int128 span = (unsigned __int128)Sc * (S - Sc)
            * (unsigned __int128)N * (N - 1);
        if (span >> 63) {
            bnpc_set_error("chain agreement: S_c R_c N (N - 1) of chain %lld "
                           "does not fit 63 bits", (long long)c);
            return 2;
        }
    }
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    PostEvents evs;
    const size_t cells = (size_t)C * N;
    unsigned long long *d_tab = nullptr;
    long long *d_bounds = nullptr;
    hipError_t e = buf.alloc(&d_tab, 3 * cells);
    if (e == hipSuccess) e = buf.alloc(&d_bounds, (size_t)C + 1);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        bnpc_set_error("chain agreement: the tables of %lld chains x %lld "
                       "cells need %.1f GB of device memory (%s)",
                       (long long)C, (long long)N, 24.0 * cells / 1e9,
                       hipGetErrorString(e));
        return 5;
    }
    PCK(e);
    std::vector<long long> hb(bounds, bounds + C + 1);
    PCK(hipMemcpy(d_bounds, hb.data(), hb.size() * sizeof(long long),
                  hipMemcpyHostToDevice));
    if (reps) PCK(evs.create());
    const unsigned nt = (unsigned)((N + 63) / 64);
    for (int which = 0; which < (reps ? 2 : 1); which++) {
        for (int r = 0; r < (reps ? reps : 1); r++) {
            if (reps) PCK(hipEventRecord(evs.ev[0], 0));
            if (which == 0) {
                PCK(hipMemsetAsync(d_tab, 0,
                                   3 * cells * sizeof(unsigned long long), 0));
                hipLaunchKernelGGL(k_chain_agree, dim3(nt, nt), dim3(256), 0,
                                   0, p->assign, (long long)S, (long long)N,
                                   p->differ, d_bounds, (int)C, d_tab,
                                   d_tab + cells, d_tab + 2 * cells);
            } else {
                cd_launch(p->assign, S, N, p->differ);
            }
            PCK(hipGetLastError());
            if (reps) {
                float t = 0.0f;
                PCK(hipEventRecord(evs.ev[1], 0));
                PCK(hipEventSynchronize(evs.ev[1]));
                PCK(hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]));
                if (r == 0 || t < ms[which]) ms[which] = t;
            }
        }
    }
    if (reps) {
        PCK(hipDeviceSynchronize());
        return 0;
    }
    // through a host copy: the outputs are written only when all is well
    std::vector<unsigned long long> host(3 * cells);
    PCK(hipMemcpy(host.data(), d_tab, host.size() * sizeof(unsigned long long),
                  hipMemcpyDeviceToHost));
    memcpy(abs_sum, host.data(), cells * sizeof(int64_t));
    memcpy(max_abs, host.data() + cells, cells * sizeof(int64_t));
    memcpy(flips, host.data() + 2 * cells, cells * sizeof(int64_t));
    return 0;
}

extern "C" int bnpc_post_chain_agreement(bnpc_post *p, const int64_t *bounds,
                                         int64_t C, int64_t *abs_sum,
                                         int64_t *max_abs, int64_t *flips)
{
    if (!abs_sum || !max_abs || !flips) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    return ca_run(p, bounds, C, abs_sum, max_abs, flips, 0, nullptr);
}

// diagnostic (tools/posterior_bench.py): see ca_run
extern "C" int bnpc_post_chain_agreement_times(bnpc_post *p,
                                               const int64_t *bounds,
                                               int64_t C, int reps, float *ms)
{
    if (!ms || reps < 1) {
        bnpc_set_error("bad argument: the times need reps >= 1 and the output");
        return 2;
    }
    return ca_run(p, bounds, C, nullptr, nullptr, nullptr, reps, ms);
}
