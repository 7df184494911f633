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
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "bnpc_hip.h"
#include "bnpc_internal.h"

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

extern "C" int bnpc_codist(int device, const int32_t *assignments, int64_t S,
                           int64_t N, int32_t *differ)
{
    if (!assignments || !differ || S < 1 || N < 2) {
        bnpc_set_error("bad argument: need S >= 1 samples of N >= 2 cells");
        return 2;
    }
#define CK(expr)                                                             \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            bnpc_set_error("%s failed: %s", #expr, hipGetErrorString(e_));   \
            if (d_a) (void)hipFree(d_a);                                     \
            if (d_d) (void)hipFree(d_d);                                     \
            return 1;                                                        \
        }                                                                    \
    } while (0)
    int *d_a = nullptr, *d_d = nullptr;
    const size_t pairs = (size_t)N * (N - 1) / 2;
    CK(hipSetDevice(device));
    CK(hipMalloc((void **)&d_a, (size_t)S * N * sizeof(int)));
    CK(hipMalloc((void **)&d_d, pairs * sizeof(int)));
    CK(hipMemcpy(d_a, assignments, (size_t)S * N * sizeof(int),
                 hipMemcpyHostToDevice));
    const unsigned nt = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(k_codist, dim3(nt, nt), dim3(256), 0, 0, d_a,
                       (long long)S, (long long)N, d_d);
    CK(hipGetLastError());
    CK(hipMemcpy(differ, d_d, pairs * sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(d_a);
    (void)hipFree(d_d);
#undef CK
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

// row scans and chain steps of the last bnpc_post_ward (diagnostic)
extern "C" int bnpc_post_ward_stats(const bnpc_post *p, int64_t *scans,
                                    int64_t *steps)
{
    if (!p || !scans || !steps) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    *scans = p->ward_stats[0];
    *steps = p->ward_stats[1];
    return 0;
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
    bnpc_post *p = new bnpc_post();
    p->device = device;
    p->S = S;
    p->N = N;
    const size_t pairs = (size_t)N * (N - 1) / 2;
    int *d_a = nullptr;
    auto fail = [&]() {
        if (d_a) (void)hipFree(d_a);
        bnpc_post_destroy(p);
        return 1;
    };
#define PF(expr)                                                             \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            bnpc_set_error("%s failed: %s", #expr, hipGetErrorString(e_));   \
            return fail();                                                   \
        }                                                                    \
    } while (0)
    PF(hipMalloc((void **)&d_a, (size_t)S * N * sizeof(int)));
    PF(hipMalloc((void **)&p->differ, pairs * sizeof(int)));
    PF(hipMalloc((void **)&p->sums, (1024 + 1) * sizeof(unsigned long long)));
    PF(hipMemcpy(d_a, assignments, (size_t)S * N * sizeof(int),
                 hipMemcpyHostToDevice));
    const unsigned nt = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(k_codist, dim3(nt, nt), dim3(256), 0, 0, d_a,
                       (long long)S, (long long)N, p->differ);
    PF(hipGetLastError());
    PF(hipMemsetAsync(p->sums, 0, sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_differ_sum, dim3(1024), dim3(256), 0, 0, p->differ,
                       (long long)pairs, p->sums);
    PF(hipGetLastError());
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
    PF(hipMemcpy(&total, p->sums, sizeof total, hipMemcpyDeviceToHost));
    p->assign = d_a;
    d_a = nullptr;
#undef PF
    if (differ_sum) *differ_sum = (int64_t)total;
    *out = p;
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
        double *d_slab = nullptr;
        PCK(hipMalloc((void **)&d_slab, std::min(slab, pairs) * sizeof(double)));
        for (size_t at = 0; at < pairs; at += slab) {
            const size_t n = std::min(slab, pairs - at);
            hipLaunchKernelGGL(k_differ_to_dist, dim3(2048), dim3(256), 0, 0,
                               p->differ + at, (long long)n, (double)p->S,
                               d_slab);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess)
                e = hipMemcpy(dist + at, d_slab, n * sizeof(double),
                              hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                bnpc_set_error("mean distance: %s", hipGetErrorString(e));
                (void)hipFree(d_slab);
                return 1;
            }
        }
        (void)hipFree(d_slab);
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
    unsigned short *d_lab = nullptr;
    const size_t bytes = (size_t)C * p->N * sizeof(unsigned short);
    PCK(hipMalloc((void **)&d_lab, bytes));
    hipError_t e = hipMemcpy(d_lab, labels, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemset(p->sums, 0, 1025 * sizeof(unsigned long long));
    const int CP = C <= 32 ? 32 : (C <= 64 ? 64 : 128);
    for (int c0 = 0; e == hipSuccess && c0 < C; c0 += CP) {
        hipLaunchKernelGGL(k_mpear_sums, dim3(1024), dim3(256), 0, 0,
                           p->differ, (long long)p->N, d_lab, c0, (int)C, CP,
                           p->sums + 1);
        e = hipGetLastError();
    }
    unsigned long long host[1024];
    if (e == hipSuccess)
        e = hipMemcpy(host, p->sums + 1, C * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost);
    (void)hipFree(d_lab);
    if (e != hipSuccess) {
        bnpc_set_error("mpear sums: %s", hipGetErrorString(e));
        return 1;
    }
    for (int64_t c = 0; c < C; c++) same_differ[c] = (int64_t)host[c];
    return 0;
}

// ---------------------------------------------------------------------------
// Ward linkage of the mean distances on the device (the `linkage(dist,
// method='ward')` of /root/reference/libs/utils.py:104; SciPy is a pinned
// third-party dependency of the reference - scipy==1.10.1, requirements.txt:4
// - and what is restated here is its published algorithm for this call:
// scipy/cluster/_hierarchy.pyx `nn_chain` - the nearest-neighbour chain of
// Murtagh / Müllner with the Lance-Williams update `_ward`).
//
// At 50 000 cells the condensed distance vector is 10 GB and SciPy spends 62 s
// walking it row by row on one core; here the distances never leave the device
// (float64 from the resident pair counts, the same IEEE division, kept as a
// full symmetric matrix so that a row is contiguous).
//
// The chain is sequential - every step needs the previous one's result - but
// the work inside a step is not, and ONE workgroup (round 3) cannot carry it:
// measured at 50 000 cells, 1.2 s of row scans and 4.2 s of Lance-Williams
// passes - a pass scatters an 8-byte store per cluster down a column of the
// matrix, and one compute unit hands the L2 one cache line per clock.  Round 4
// splits a step in two kernels that alternate on one stream (captured once as
// a graph of 128 pairs and replayed; the kernel boundary is the hand-off, all
// state lives in device memory, so there is no inter-workgroup protocol
// inside a launch to get wrong):
//
//   k_ward_chain   ONE wave takes in what the last piece of work left (the
//                  partial minima), walks the chain - a handful of dependent
//                  loads per step - until it needs work, posts it and ends:
//                  a merge, or the nearest neighbour of a stale row;
//   k_ward_work    the whole chip does it: ceil(N / 256) workgroups the
//                  Lance-Williams pass of the merge (row y contiguous,
//                  columns x and y scattered over every CU's path to the L2),
//                  ~N / 1500 workgroups a slice each of the row to be scanned
//                  - with a merge, the row the chain returns to (its
//                  neighbour was one of the two merged clusters, always), as
//                  the merge leaves it: column x gone, column y at the new
//                  distance, computed from values the chain kernel read
//                  beforehand, so the scan does not race with the pass.
//
// Work per step is cut as well:
//  * a row scan is a pure (minimum, smallest index) reduction: the diagonal,
//    the padding and the columns of merged-away clusters hold +inf, so there
//    is no activity test, 16-byte loads;
//  * every row keeps its nearest neighbour (nn_d, nn_i) = (minimum, smallest
//    index among equals) of its CURRENT entries, initialised for all rows by
//    one chip-wide pass (k_ward_init).  The Lance-Williams pass keeps that
//    exact - a row whose neighbour was one of the two merged clusters is
//    marked stale, any other row takes the merged cluster as its neighbour
//    iff (new distance, its index) is lexicographically smaller - and
//    computes the merged row's own neighbour on the way.  A chain step whose
//    top row has a valid neighbour needs no scan; a stale row is scanned when
//    (and only if) it reaches the top.  (With the many exact ties of
//    co-clustering distances the neighbours of a cluster's rows all point at
//    its smallest index, and its merges make them stale over and over: 2.6
//    scans per merge remain, 1 of them riding on the merge's own launch.
//    Keeping the k nearest per row instead was simulated: k = 8 still needs
//    1.3 scans per merge - not worth its bookkeeping.)
//
// N = 50 000: 4.2 s (round 3) -> 1.5 s; what is left is latency - 130 000
// launches of each kernel, ~5 us of dependent loads apiece.
//
// The sequential scan's choices are kept exactly: the nearest neighbour is
// the first index of the row's minimum, unless the chain's previous element
// is as near (`dist < current_min` is strict: the previous element wins
// ties); the distance to the previous element is the one recorded when it
// pushed the current top (neither has been merged since, so the entry is
// unchanged).  Same merges, same heights bit for bit (sqrt, mul, add, div are
// IEEE on both sides, compiled without contraction); the final stable sort by
// height and the relabelling are done by the binding as SciPy does them.
// ---------------------------------------------------------------------------
#define WARD_NONE 0x7fffffff

// the mean distances as a FULL symmetric matrix, rows `pitch` doubles apart
// (pitch even: rows are 16-byte aligned; 20 GB at 50 000 cells), from the
// pair counts; +inf on the diagonal and in the padding
__global__ __launch_bounds__(256) void k_differ_to_square(
    const int *__restrict__ differ, long long n, long long pitch, double S,
    double *__restrict__ F)
{
    const long long total = n * pitch;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total;
         e += (long long)gridDim.x * 256) {
        const long long i = e / pitch, j = e - i * pitch;
        double v = INFINITY;
        if (i != j && j < n) {
            const long long a = i < j ? i : j, b = i < j ? j : i;
            v = (double)differ[a * (2 * n - a - 1) / 2 + (b - a - 1)] / S;
        }
        F[e] = v;
    }
}

// (d, i) < (bd, bi) lexicographically
__device__ __forceinline__ void ward_take(double d, int i, double &bd, int &bi)
{
    if (d < bd || (d == bd && i < bi)) {
        bd = d;
        bi = i;
    }
}

// scipy's _ward: the distance of cluster i (ni cells) to the union of x and y
__device__ __forceinline__ double ward_lw(int ni, int nx, int ny, double dxi,
                                          double dyi, double dxy)
{
    const double t = 1.0 / (double)(nx + ny + ni);
    return sqrt((double)(ni + nx) * t * dxi * dxi
                + (double)(ni + ny) * t * dyi * dyi
                - (double)ni * t * dxy * dxy);
}

// state of the chain between launches (device memory)
struct WardState {
    long long merges, steps, scans, first_alive;
    int len, err, done;
    // the work k_ward_chain posted for k_ward_work: 1 = the merge (x, y) -> y,
    // x < y, plus - if b >= 0 - the nearest neighbour of row b AS THE MERGE
    // LEAVES IT (column x gone, column y at the new distance, computed from
    // nb, dxb, dyb); 2 = the nearest neighbour of row b as it stands
    int cmd, x, y, nx, ny, b, nb, pad_;
    double dxy, dxb, dyb;
};

#define WARD_B 256          // threads of a k_ward_work / k_ward_init workgroup
#define WARD_SCAN_U 4       // 16-byte loads per thread of a row-scan slice

__device__ __forceinline__ void ward_reduce_b(double &bd, int &bi, double *r_d,
                                              int *r_i)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_down(bd, off);
        const int oi = __shfl_down(bi, off);
        ward_take(od, oi, bd, bi);
    }
    if (lane == 0) {
        r_d[wave] = bd;
        r_i[wave] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < (int)(blockDim.x >> 6); w++)
            ward_take(r_d[w], r_i[w], bd, bi);
}

// (minimum, first index) of columns [2 * j0, 2 * j1) of one row: inactive
// columns, the diagonal and the padding hold +inf; columns skip_x / sub_y (or
// -1) are taken as +inf / sub_v instead of what memory holds
__device__ __forceinline__ void ward_scan_slice(
    const double *F, long long pitch, long long r, long long j0, long long j1,
    int skip_x, int sub_y, double sub_v, double &bd, int &bi)
{
    const double2 *row = (const double2 *)(F + (size_t)r * pitch);
    const double2 inf2 = {INFINITY, INFINITY};
    bd = INFINITY;
    bi = WARD_NONE;
    for (long long base = j0; base < j1;
         base += (long long)WARD_SCAN_U * blockDim.x) {
        double2 v[WARD_SCAN_U];
#pragma unroll
        for (int u = 0; u < WARD_SCAN_U; u++) {
            const long long j = base + (long long)u * blockDim.x + threadIdx.x;
            v[u] = j < j1 ? row[j] : inf2;
        }
#pragma unroll
        for (int u = 0; u < WARD_SCAN_U; u++) {
            const long long j = base + (long long)u * blockDim.x + threadIdx.x;
            const int c0 = (int)(2 * j), c1 = c0 + 1;
            double a0 = v[u].x, a1 = v[u].y;
            if (c0 == skip_x) a0 = INFINITY;
            if (c1 == skip_x) a1 = INFINITY;
            if (c0 == sub_y) a0 = sub_v;
            if (c1 == sub_y) a1 = sub_v;
            // (this thread's indices ascend: strict < keeps the first)
            if (a0 < bd) {
                bd = a0;
                bi = c0;
            }
            if (a1 < bd) {
                bd = a1;
                bi = c1;
            }
        }
    }
}

// every row's nearest neighbour, every cluster's size: one workgroup per row
__global__ __launch_bounds__(WARD_B) void k_ward_init(
    const double *__restrict__ F, long long n, long long pitch,
    int *__restrict__ size, double *__restrict__ nn_d, int *__restrict__ nn_i)
{
    __shared__ double r_d[WARD_B / 64];
    __shared__ int r_i[WARD_B / 64];
    for (long long r = blockIdx.x; r < n; r += gridDim.x) {
        double bd;
        int bi;
        ward_scan_slice(F, pitch, r, 0, pitch >> 1, -1, -1, 0.0, bd, bi);
        ward_reduce_b(bd, bi, r_d, r_i);
        if (threadIdx.x == 0) {
            size[r] = 1;
            nn_d[r] = bd;
            nn_i[r] = bi == WARD_NONE ? -1 : bi;
        }
        __syncthreads();
    }
}

// ONE wave: take in what the last k_ward_work left, then walk the chain until
// the next piece of work is known (a merge, or the scan of a stale row)
__global__ __launch_bounds__(64) void k_ward_chain(
    const double *__restrict__ F, long long n, long long pitch,
    int *__restrict__ size, int *__restrict__ chain,
    double *__restrict__ chain_d, double *__restrict__ nn_d,
    int *__restrict__ nn_i, double *__restrict__ Z,
    const double *__restrict__ pm_d, const int *__restrict__ pm_i, int Gm,
    const double *__restrict__ ps_d, const int *__restrict__ ps_i, int Gs,
    WardState *__restrict__ ws)
{
    const int lane = threadIdx.x;
    if (ws->err || ws->done) return;
    const int last = ws->cmd;
    if (last) {
        // the minima of the partial minima the workgroups left
        double md = INFINITY, sd = INFINITY;
        int mi = WARD_NONE, si = WARD_NONE;
        if (last == 1)
            for (int q = lane; q < Gm; q += 64) ward_take(pm_d[q], pm_i[q], md, mi);
        const int row = ws->b;
        if (row >= 0)
            for (int q = lane; q < Gs; q += 64) ward_take(ps_d[q], ps_i[q], sd, si);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_down(md, off), pd = __shfl_down(sd, off);
            const int oi = __shfl_down(mi, off), pi = __shfl_down(si, off);
            ward_take(od, oi, md, mi);
            ward_take(pd, pi, sd, si);
        }
        if (lane == 0) {
            if (last == 1) {
                nn_d[ws->y] = md;
                nn_i[ws->y] = mi == WARD_NONE ? -1 : mi;
            }
            if (row >= 0) {
                nn_d[row] = sd;
                nn_i[row] = si == WARD_NONE ? -2 : si;
                if (si == WARD_NONE) ws->err = 1;   // nothing to merge with
            }
        }
    }
    if (lane != 0) return;
    if (ws->err) return;
    long long first_alive = ws->first_alive, steps = ws->steps,
        merges = ws->merges;
    int len = ws->len, cmd = 0;
    while (cmd == 0) {
        if (merges == n - 1) {
            ws->done = 1;
            break;
        }
        if (len == 0) {
            while (first_alive < n && size[first_alive] == 0) first_alive++;
            chain[0] = (int)first_alive;
            len = 1;
        }
        // (independent loads side by side: every one of them is an L2 round
        // trip, and the walk is nothing but their latencies)
        const int x = chain[len - 1];
        const int prev = chain[len > 1 ? len - 2 : 0];
        const int under = chain[len > 2 ? len - 3 : 0];
        const double dprev = chain_d[len - 1];
        const int cand = nn_i[x];
        const double dc = nn_d[x];
        if (cand < 0) {             // stale: scanned chip-wide
            ws->b = x;
            ws->scans++;
            cmd = 2;
            break;
        }
        int y = cand;
        double dmin = dc;
        if (len > 1 && !(dc < dprev)) {     // the previous element wins ties
            y = prev;
            dmin = dprev;
        }
        if (++steps > 8 * n + 64 || y < 0 || y >= n) {
            ws->err = 1;            // cannot happen
            break;
        }
        if (len > 1 && y == prev) {
            len -= 2;
            int a = x, b = y;
            if (a > b) {
                const int t = a;
                a = b;
                b = t;
            }
            const bool back = len > 0 && merges + 1 < n - 1;
            const int na = size[a], nb = size[b];
            const int top_n = back ? size[under] : 0;
            const double top_dx = back ? F[(size_t)a * pitch + under] : 0.0;
            const double top_dy = back ? F[(size_t)b * pitch + under] : 0.0;
            Z[merges * 4 + 0] = (double)a;
            Z[merges * 4 + 1] = (double)b;
            Z[merges * 4 + 2] = dmin;
            Z[merges * 4 + 3] = (double)(na + nb);
            size[a] = 0;
            size[b] = na + nb;
            merges++;
            ws->x = a;
            ws->y = b;
            ws->nx = na;
            ws->ny = nb;
            ws->dxy = dmin;
            // the row the chain returns to: its neighbour was one of the two
            ws->b = -1;
            if (back) {
                ws->b = under;
                ws->nb = top_n;
                ws->dxb = top_dx;
                ws->dyb = top_dy;
                ws->scans++;
            }
            cmd = 1;
            break;
        }
        chain[len] = y;
        chain_d[len] = dmin;
        len++;
    }
    ws->cmd = cmd;
    ws->first_alive = first_alive;
    ws->steps = steps;
    ws->merges = merges;
    ws->len = len;
}

// The posted work, on the whole chip.  Workgroups [0, Gm): the Lance-Williams
// pass of the merge (x, y) -> y, one cluster i per thread - rows x and y are
// read and row y written contiguously, columns x (now +inf) and y (the
// symmetric entries) are scattered over every compute unit's path to the L2;
// every row's nearest neighbour is kept exact on the way.  Workgroups
// [Gm, Gm + Gs): a slice each of the row whose neighbour is asked for.
__global__ __launch_bounds__(WARD_B) void k_ward_work(
    double *__restrict__ F, long long n, long long pitch,
    const int *__restrict__ size, double *__restrict__ nn_d,
    int *__restrict__ nn_i, double *__restrict__ pm_d,
    int *__restrict__ pm_i, int Gm, double *__restrict__ ps_d,
    int *__restrict__ ps_i, int Gs, const WardState *__restrict__ ws)
{
    __shared__ double r_d[WARD_B / 64];
    __shared__ int r_i[WARD_B / 64];
    const int cmd = ws->cmd;
    if (!cmd || ws->err || ws->done) return;
    const int x = ws->x, y = ws->y, nx = ws->nx, ny = ws->ny, rb = ws->b;
    const double dxy = ws->dxy;
    double bd = INFINITY;
    int bi = WARD_NONE;
    if ((int)blockIdx.x >= Gm) {
        if (rb < 0) return;
        const int s = (int)blockIdx.x - Gm;
        const long long n2 = pitch >> 1;
        const long long per = (n2 + Gs - 1) / Gs;
        const long long j0 = s * per, j1 = j0 + per < n2 ? j0 + per : n2;
        double vb = 0.0;
        if (cmd == 1) vb = ward_lw(ws->nb, nx, ny, ws->dxb, ws->dyb, dxy);
        ward_scan_slice(F, pitch, rb, j0, j1, cmd == 1 ? x : -1,
                        cmd == 1 ? y : -1, vb, bd, bi);
        ward_reduce_b(bd, bi, r_d, r_i);
        if (threadIdx.x == 0) {
            ps_d[s] = bd;
            ps_i[s] = bi;
        }
        return;
    }
    if (cmd != 1) return;
    const double *__restrict__ rx = F + (size_t)x * pitch;
    double *__restrict__ ry = F + (size_t)y * pitch;
    for (long long i = (long long)blockIdx.x * WARD_B + threadIdx.x; i < n;
         i += (long long)Gm * WARD_B) {
        if (i == x) {
            ry[i] = INFINITY;           // x is gone
            continue;
        }
        const int ni = size[i];
        if (ni == 0 || i == y) continue;
        const double v = ward_lw(ni, nx, ny, rx[i], ry[i], dxy);
        ry[i] = v;
        double *__restrict__ ri = F + (size_t)i * pitch;
        ri[y] = v;
        ri[x] = INFINITY;
        ward_take(v, (int)i, bd, bi);
        if (i == rb) continue;          // its neighbour is being recomputed
        // row i's nearest neighbour, kept exact
        const int ci = nn_i[i];
        if (ci == x || ci == y) {
            // its minimum was one of the merged entries: still the minimum
            // only if the new entry is no larger
            if (ci == y && v <= nn_d[i])
                nn_d[i] = v;
            else
                nn_i[i] = -1;
        } else if (ci >= 0) {
            const double cd = nn_d[i];
            if (v < cd || (v == cd && y < ci)) {
                nn_d[i] = v;
                nn_i[i] = y;
            }
        }
    }
    ward_reduce_b(bd, bi, r_d, r_i);
    if (threadIdx.x == 0) {
        pm_d[blockIdx.x] = bd;
        pm_i[blockIdx.x] = bi;
    }
}

// Z_raw[(N - 1) x 4]: the merges in the order the chain makes them (x < y:
// indices of the two clusters' slots, height, size) - what scipy's nn_chain
// holds before its final sort and relabelling.
extern "C" int bnpc_post_ward(bnpc_post *p, double *Z_raw)
{
    if (!p || !Z_raw) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    PCK(hipSetDevice(p->device));
    const long long n = p->N;
    if (n < 2) return 0;
    const long long pitch = (n + 1) & ~1ll;
    const int Gm = (int)std::min<long long>((n + WARD_B - 1) / WARD_B, 1024);
    const int Gs = (int)std::max<long long>(1, std::min<long long>(
        ((pitch >> 1) + WARD_B * 3 - 1) / (WARD_B * 3), 256));
    // the full symmetric matrix: 8 N^2 bytes (20 GB at 50 000 cells).  Not
    // fitting is the ONE failure the caller may answer with SciPy's routine
    // on the condensed vector: it gets a return code of its own (5).
    {
        size_t free_b = 0, total_b = 0;
        PCK(hipMemGetInfo(&free_b, &total_b));
        const size_t need = (size_t)n * pitch * sizeof(double)
            + (size_t)n * 72 + ((size_t)1 << 20);
        if (need > free_b) {
            bnpc_set_error("ward linkage: the %lld x %lld distance matrix "
                           "needs %.1f GB, %.1f GB of device memory are free",
                           n, n, need / 1e9, free_b / 1e9);
            return 5;
        }
    }
    double *d_D = nullptr, *d_Z = nullptr, *d_cd = nullptr, *d_nd = nullptr,
        *d_pd = nullptr;
    int *d_size = nullptr, *d_chain = nullptr, *d_ni = nullptr,
        *d_pi = nullptr;
    WardState *d_ws = nullptr;
    hipStream_t st = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    const int G = Gm + Gs;
    hipError_t e = hipMalloc((void **)&d_D, (size_t)n * pitch * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_Z, (size_t)(n - 1) * 4 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_size, (size_t)n * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&d_chain, (size_t)(n + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&d_cd, (size_t)(n + 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_nd, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_ni, (size_t)n * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&d_pd, (size_t)G * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_pi, (size_t)G * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&d_ws, sizeof(WardState));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemsetAsync(d_ws, 0, sizeof(WardState), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_differ_to_square, dim3(4096), dim3(256), 0, st,
                           p->differ, n, pitch, (double)p->S, d_D);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_ward_init,
                           dim3((unsigned)std::min<long long>(n, 4096)),
                           dim3(WARD_B), 0, st, d_D, n, pitch, d_size, d_nd,
                           d_ni);
        e = hipGetLastError();
    }
    // chain, work, chain, work ... on one stream: a graph of WARD_BATCH such
    // pairs, replayed until the chain reports that everything is merged (a
    // launch that finds nothing to do returns at once)
    const int WARD_BATCH = 128;
    auto pair = [&](hipStream_t s) {
        hipLaunchKernelGGL(k_ward_chain, dim3(1), dim3(64), 0, s, d_D, n,
                           pitch, d_size, d_chain, d_cd, d_nd, d_ni, d_Z,
                           d_pd, d_pi, Gm, d_pd + Gm, d_pi + Gm, Gs, d_ws);
        hipLaunchKernelGGL(k_ward_work, dim3((unsigned)G), dim3(WARD_B), 0, s,
                           d_D, n, pitch, d_size, d_nd, d_ni, d_pd, d_pi, Gm,
                           d_pd + Gm, d_pi + Gm, Gs, d_ws);
    };
    bool graphed = false;
    // (BNPC_WARD_DEVICE=plain: plain launches - rocprofv3's kernel trace does
    // not survive the replay of a captured graph on this stack)
    const char *wg = getenv("BNPC_WARD_DEVICE");
    if (e == hipSuccess && !(wg && !strcmp(wg, "plain"))
        && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal)
            == hipSuccess) {
        for (int k = 0; k < WARD_BATCH; k++) pair(st);
        if (hipStreamEndCapture(st, &graph) == hipSuccess && graph
            && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)
                == hipSuccess)
            graphed = true;
    }
    (void)hipGetLastError();
    WardState ws;
    memset(&ws, 0, sizeof ws);
    // about 2.6 pieces of work per merge (measured: the merge itself and 1.6
    // scans of stale rows); the state is looked at after every `look` batches
    long long batches = 0;
    const long long look = std::max<long long>(1, (n / WARD_BATCH) / 8);
    const long long cap = 16 * (n / WARD_BATCH + 2) + 64;
    while (e == hipSuccess && !ws.done && !ws.err && batches < cap) {
        const long long burst = batches == 0
            ? std::max<long long>(1, 2 * n / WARD_BATCH) : look;
        for (long long q = 0; q < burst && e == hipSuccess; q++) {
            if (graphed) {
                e = hipGraphLaunch(exec, st);
            } else {
                for (int k = 0; k < WARD_BATCH; k++) pair(st);
                e = hipGetLastError();
            }
        }
        batches += burst;
        if (e == hipSuccess)
            e = hipMemcpyAsync(&ws, d_ws, sizeof ws, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e == hipSuccess)
        e = hipMemcpy(Z_raw, d_Z, (size_t)(n - 1) * 4 * sizeof(double),
                      hipMemcpyDeviceToHost);
    p->ward_stats[0] = ws.scans;
    p->ward_stats[1] = ws.steps;
    const int err = ws.err || (e == hipSuccess && ws.merges != n - 1);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    if (st) (void)hipStreamDestroy(st);
    if (d_D) (void)hipFree(d_D);
    if (d_Z) (void)hipFree(d_Z);
    if (d_size) (void)hipFree(d_size);
    if (d_chain) (void)hipFree(d_chain);
    if (d_cd) (void)hipFree(d_cd);
    if (d_nd) (void)hipFree(d_nd);
    if (d_ni) (void)hipFree(d_ni);
    if (d_pd) (void)hipFree(d_pd);
    if (d_pi) (void)hipFree(d_pi);
    if (d_ws) (void)hipFree(d_ws);
    if (e == hipErrorOutOfMemory) {
        // an allocation that failed although the pre-check saw room
        // (fragmentation, other chains on the same GPU): the announced
        // out-of-memory code, so that the caller's host fallback applies
        (void)hipGetLastError();
        bnpc_set_error("ward linkage: out of device memory (%s)",
                       hipGetErrorString(e));
        return 5;
    }
    if (e != hipSuccess) {
        bnpc_set_error("ward linkage: %s", hipGetErrorString(e));
        return 1;
    }
    if (err) {
        bnpc_set_error("ward linkage: the neighbour chain did not close "
                       "(non-finite distances?)");
        return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Posterior genotypes (utils.py:148-192): per MPEAR cluster k, the mean of
// the sampled parameter rows of the samples in which k's cells sit together
// (and alone, if such samples exist); a cluster that is never together takes
// the count-weighted rows of the labels its cells carry, over every sample.
//
// Read closely, the reference's loop needs, per (cluster, sample):
//   together  all of k's labels equal (the `bincount` argmax is then that
//             common label c; where k is not together it is never used)
//   alone     no cell outside k carries c
//   rank      the row of c in params_full[s]: the distinct labels of sample s
//             below c
// Pass 1 (k_gt_flags, one workgroup per sample) reads the sample row once:
// a presence bitmap of its labels with per-word prefix popcounts (rank), a
// label -> owning cluster map written twice with plain stores (any member's
// cluster, then MIXED wherever a member disagrees), and per cluster one
// member's label, marked bad wherever another member disagrees.  Nothing is
// ordered, so nothing needs an atomic but the bitmap's OR.
// Pass 1b (k_gt_hist, only for clusters never together): per sample the
// (rank, count) histogram of the cluster's labels, in rank order.
// Pass 2 (k_gt_accum, one thread per (cluster, mutation)) walks the chosen
// samples in increasing s with a float64 accumulator, exactly the
// reference's `params[row] += params_full[s][rank]`; for a never-together
// cluster each sample's term is summed in rank order from 0 (`np.dot` of
// integer counts: every product is exact) and then added.  The parameter
// trace is streamed in sample chunks; the accumulators stay on the device.
// The divisions are the host's.
//
// The pass-1 working set (2.25 N bytes + 8 K) sits in LDS while it fits
// (about 70 000 cells); past that each workgroup takes a slice of global
// memory and the same code runs on it through flat pointers.
// ---------------------------------------------------------------------------
#define GT_MIXED 0xfffeu
#define GT_LDS_MAX 163840
#define GT_GLOBAL_WG 512

// exclusive prefix popcount of nw bitmap words (all threads call); the
// distinct labels in total are returned to every thread
__device__ static unsigned gt_scan(const unsigned *bm, unsigned *pf,
                                   long long nw, unsigned *part)
{
    const int tid = threadIdx.x;
    const long long per = (nw + 255) / 256;
    const long long w0 = std::min(nw, tid * per), w1 = std::min(nw, w0 + per);
    unsigned sum = 0;
    for (long long w = w0; w < w1; w++) sum += __popc(bm[w]);
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0;
        for (int t = 0; t < 256; t++) {
            const unsigned v = part[t];
            part[t] = run;
            run += v;
        }
        part[256] = run;
    }
    __syncthreads();
    unsigned run = part[tid];
    for (long long w = w0; w < w1; w++) {
        pf[w] = run;
        run += __popc(bm[w]);
    }
    const unsigned total = part[256];
    __syncthreads();                        // part is reused by the next scan
    return total;
}

__device__ static inline unsigned gt_rank(const unsigned *bm,
                                          const unsigned *pf, int L)
{
    return pf[L >> 5] + __popc(bm[L >> 5] & ((1u << (L & 31)) - 1u));
}

// pass-1 working set in 32-bit words: part[260] bm[nw] pf[nw] own[N] (uint16)
// rep[K] bad[K]
static long long gt_flags_words(long long N, long long K)
{
    const long long nw = (N + 31) / 32;
    return 260 + 2 * nw + (N + 1) / 2 + 2 * K;
}

__global__ __launch_bounds__(256) void k_gt_flags(
    const int *__restrict__ a, long long S, long long N,
    const unsigned short *__restrict__ cl, int K,
    unsigned *gscratch, long long stride,
    unsigned char *__restrict__ flags,      // [K][S]: 1 together, 2 alone
    int *__restrict__ rank,                 // [K][S]
    int *__restrict__ distinct)             // [S]
{
    extern __shared__ __attribute__((aligned(16))) unsigned gt_lds[];
    unsigned *area = gscratch ? gscratch + blockIdx.x * stride : gt_lds;
    const long long nw = (N + 31) / 32;
    unsigned *part = area;
    unsigned *bm = area + 260;
    unsigned *pf = bm + nw;
    unsigned short *own = (unsigned short *)(pf + nw);
    int *rep = (int *)(pf + nw + (N + 1) / 2);
    unsigned *bad = (unsigned *)(rep + K);
    const int tid = threadIdx.x;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int *row = a + s * N;
        for (long long w = tid; w < nw; w += 256) bm[w] = 0;
        for (int k = tid; k < K; k += 256) bad[k] = 0;
        __syncthreads();
        for (long long i = tid; i < N; i += 256) {
            const int L = row[i];
            const unsigned short k = cl[i];
            atomicOr(&bm[L >> 5], 1u << (L & 31));
            own[L] = k;
            rep[k] = L;
        }
        __syncthreads();
        for (long long i = tid; i < N; i += 256) {
            const int L = row[i];
            const unsigned short k = cl[i];
            if (own[L] != k) own[L] = (unsigned short)GT_MIXED;
            if (rep[k] != L) bad[k] = 1;
        }
        __syncthreads();
        const unsigned total = gt_scan(bm, pf, nw, part);
        for (int k = tid; k < K; k += 256) {
            const int c = rep[k];
            const bool together = bad[k] == 0;
            const bool alone = together && own[c] == (unsigned short)k;
            flags[(size_t)k * S + s] =
                (unsigned char)((together ? 1 : 0) | (alone ? 2 : 0));
            rank[(size_t)k * S + s] = (int)gt_rank(bm, pf, c);
        }
        if (tid == 0) distinct[s] = (int)total;
        __syncthreads();                    // the area is reused
    }
}

// pass-1b working set in 32-bit words: part[260] bm[nw] pf[nw] lb[nw] lp[nw]
static long long gt_hist_words(long long N)
{
    return 260 + 4 * ((N + 31) / 32);
}

// per sample and never-together cluster j (cells members[mstart[j] ..
// + msize[j]]): hd[j][s] distinct labels, then hcnt / hrank[hbase[j] +
// s * msize[j] + q] the count and the sample rank of its q-th smallest label
__global__ __launch_bounds__(256) void k_gt_hist(
    const int *__restrict__ a, long long S, long long N,
    const int *__restrict__ members, const long long *__restrict__ mstart,
    const int *__restrict__ msize, const long long *__restrict__ hbase,
    int NT, unsigned *gscratch, long long stride,
    int *__restrict__ hcnt, int *__restrict__ hrank, int *__restrict__ hd)
{
    extern __shared__ __attribute__((aligned(16))) unsigned gt_lds[];
    unsigned *area = gscratch ? gscratch + blockIdx.x * stride : gt_lds;
    const long long nw = (N + 31) / 32;
    unsigned *part = area;
    unsigned *bm = area + 260;
    unsigned *pf = bm + nw;
    unsigned *lb = pf + nw;
    unsigned *lp = lb + nw;
    const int tid = threadIdx.x;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int *row = a + s * N;
        for (long long w = tid; w < nw; w += 256) bm[w] = 0;
        __syncthreads();
        for (long long i = tid; i < N; i += 256) {
            const int L = row[i];
            atomicOr(&bm[L >> 5], 1u << (L & 31));
        }
        __syncthreads();
        gt_scan(bm, pf, nw, part);
        for (int j = 0; j < NT; j++) {
            const int *cells = members + mstart[j];
            const int n = msize[j];
            for (long long w = tid; w < nw; w += 256) lb[w] = 0;
            __syncthreads();
            for (int q = tid; q < n; q += 256) {
                const int L = row[cells[q]];
                atomicOr(&lb[L >> 5], 1u << (L & 31));
            }
            __syncthreads();
            const unsigned d = gt_scan(lb, lp, nw, part);
            const long long base = hbase[j] + s * n;
            for (int q = tid; q < n; q += 256) {
                const int L = row[cells[q]];
                const unsigned at = gt_rank(lb, lp, L);
                atomicAdd(&hcnt[base + at], 1);
                hrank[base + at] = (int)gt_rank(bm, pf, L);
            }
            if (tid == 0) hd[(size_t)j * S + s] = (int)d;
            __syncthreads();
        }
    }
}

// one chunk of samples [s0, s0 + sc): P is its [sc][W][M] float32 trace.
// Cluster k = blockIdx.y adds the rows rows[lo[k] .. hi[k]) (sample-major
// global row indices s * W + rank, increasing s), or, never together
// (ntj[k] >= 0), its histogram terms of every sample in the chunk.
__global__ __launch_bounds__(256) void k_gt_accum(
    const float *__restrict__ P, long long s0, int sc, long long S, int W,
    long long M, const long long *__restrict__ rows,
    const long long *__restrict__ lo, const long long *__restrict__ hi,
    const int *__restrict__ ntj, const int *__restrict__ msize,
    const long long *__restrict__ hbase, const int *__restrict__ hcnt,
    const int *__restrict__ hrank, const int *__restrict__ hd,
    double *__restrict__ acc)
{
    const int k = blockIdx.y;
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double v = acc[(size_t)k * M + m];
    const long long base = s0 * W;
    const int j = ntj[k];
    if (j < 0) {
        const long long e = hi[k];
#pragma unroll 8
        for (long long q = lo[k]; q < e; q++)
            v += (double)P[(size_t)(rows[q] - base) * M + m];
    } else {
        const int n = msize[j];
        for (int i = 0; i < sc; i++) {
            const long long s = s0 + i;
            const int *hc = hcnt + hbase[j] + s * n;
            const int *hr = hrank + hbase[j] + s * n;
            const int d = hd[(size_t)j * S + s];
            double t = 0.0;
            for (int q = 0; q < d; q++)
                t += (double)hc[q] * (double)P[((size_t)i * W + hr[q]) * M + m];
            v += t;
        }
    }
    acc[(size_t)k * M + m] = v;
}

namespace {
// device buffers of one bnpc_post_genotypes call, freed on every return
struct GtBuffers {
    void *p[32] = {};
    int n = 0;
    template <class T> hipError_t alloc(T **out, size_t count)
    {
        *out = nullptr;
        hipError_t e = hipMalloc((void **)out, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) p[n++] = (void *)*out;
        return e;
    }
    ~GtBuffers()
    {
        for (int i = 0; i < n; i++) (void)hipFree(p[i]);
    }
};

// where a per-sample kernel's working set of `words` goes: LDS while it fits
// (a workgroup per sample), else a global slice per workgroup
struct GtArea {
    unsigned grid = 0;
    size_t lds = 0;
    unsigned *scratch = nullptr;
    long long stride = 0;
};
hipError_t gt_area(const void *kernel, long long words, int64_t S,
                   GtBuffers &buf, GtArea &a)
{
    if ((size_t)words * 4 <= GT_LDS_MAX) {
        a.grid = (unsigned)std::min<int64_t>(S, 65535);
        a.lds = (size_t)words * 4;
        return hipFuncSetAttribute(kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GT_LDS_MAX);
    }
    a.grid = (unsigned)std::min<int64_t>(S, GT_GLOBAL_WG);
    a.stride = words;
    return buf.alloc(&a.scratch, (size_t)a.grid * words);
}
}  // namespace

extern "C" int bnpc_post_genotypes(bnpc_post *p, const int32_t *labels,
                                   int64_t K, const float *params, int64_t W,
                                   int64_t M, int64_t chunk, double *geno)
{
    if (!p || !labels || !params || !geno || K < 1 || K >= (int64_t)GT_MIXED
        || W < 1 || M < 1 || chunk < 0) {
        bnpc_set_error("bad argument: genotypes need labels, 1 <= K < 65534 "
                       "clusters, a W >= 1 x M >= 1 trace and the output");
        return 2;
    }
    if (!p->assign || !p->labels_in_range) {
        bnpc_set_error("genotypes: the sample labels must lie in [0, N = %lld)",
                       (long long)p->N);
        return 2;
    }
    const int64_t S = p->S, N = p->N;
    // the clusters: compact in [0, K), none empty; members grouped by cluster
    std::vector<int64_t> start(K + 1, 0);
    for (int64_t i = 0; i < N; i++) {
        if (labels[i] < 0 || labels[i] >= K) {
            bnpc_set_error("genotypes: cluster label %d of cell %lld is not in "
                           "[0, %lld)", labels[i], (long long)i, (long long)K);
            return 2;
        }
        start[labels[i] + 1]++;
    }
    for (int64_t k = 0; k < K; k++) {
        if (start[k + 1] == 0) {
            bnpc_set_error("genotypes: cluster %lld has no cells (labels must "
                           "be compact)", (long long)k);
            return 2;
        }
        start[k + 1] += start[k];
    }
    std::vector<int> members(N);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < N; i++) members[at[labels[i]]++] = (int)i;
    }
    std::vector<unsigned short> cl(N);
    for (int64_t i = 0; i < N; i++) cl[i] = (unsigned short)labels[i];

    PCK(hipSetDevice(p->device));
    GtBuffers buf;
    unsigned short *d_cl;
    unsigned char *d_flags;
    int *d_rank, *d_distinct;
    PCK(buf.alloc(&d_cl, N));
    PCK(buf.alloc(&d_flags, (size_t)K * S));
    PCK(buf.alloc(&d_rank, (size_t)K * S));
    PCK(buf.alloc(&d_distinct, S));
    PCK(hipMemcpy(d_cl, cl.data(), N * sizeof(unsigned short),
                  hipMemcpyHostToDevice));

    // pass 1
    {
        GtArea area;
        PCK(gt_area((const void *)k_gt_flags, gt_flags_words(N, K), S, buf,
                    area));
        hipLaunchKernelGGL(k_gt_flags, dim3(area.grid), dim3(256), area.lds,
                           0, p->assign, (long long)S, (long long)N, d_cl,
                           (int)K, area.scratch, area.stride, d_flags, d_rank,
                           d_distinct);
        PCK(hipGetLastError());
    }
    std::vector<unsigned char> flags((size_t)K * S);
    std::vector<int> rank((size_t)K * S), distinct(S);
    PCK(hipMemcpy(flags.data(), d_flags, flags.size(), hipMemcpyDeviceToHost));
    PCK(hipMemcpy(rank.data(), d_rank, rank.size() * sizeof(int),
                  hipMemcpyDeviceToHost));
    PCK(hipMemcpy(distinct.data(), d_distinct, S * sizeof(int),
                  hipMemcpyDeviceToHost));

    // the chosen samples of every cluster: together and alone, else
    // together; a cluster never together goes to the histogram path
    std::vector<long long> rows, lo0(K), hi0(K);
    std::vector<double> den(K);
    std::vector<int> ntj(K, -1), nt_cells;
    std::vector<long long> nt_start, nt_base;
    std::vector<int> nt_size;
    long long hist_total = 0;
    for (int64_t k = 0; k < K; k++) {
        const unsigned char *f = flags.data() + (size_t)k * S;
        bool any_alone = false, any_together = false;
        for (int64_t s = 0; s < S; s++) {
            any_together |= (f[s] & 1) != 0;
            any_alone |= f[s] == 3;
        }
        lo0[k] = (long long)rows.size();
        if (any_together) {
            const unsigned char need = any_alone ? 3 : 1;
            for (int64_t s = 0; s < S; s++) {
                if ((f[s] & need) != need) continue;
                const int r = rank[(size_t)k * S + s];
                if (r >= W) {
                    bnpc_set_error("genotypes: sample %lld needs row %d of a "
                                   "trace %lld rows wide", (long long)s, r,
                                   (long long)W);
                    return 2;
                }
                rows.push_back((long long)s * W + r);
            }
            den[k] = (double)(rows.size() - lo0[k]);
        } else {
            const int64_t n = start[k + 1] - start[k];
            for (int64_t s = 0; s < S; s++) {
                if (distinct[s] > W) {
                    bnpc_set_error("genotypes: sample %lld has %d clusters, "
                                   "the trace %lld rows", (long long)s,
                                   distinct[s], (long long)W);
                    return 2;
                }
            }
            ntj[k] = (int)nt_size.size();
            nt_start.push_back(start[k]);
            nt_size.push_back((int)n);
            nt_base.push_back(hist_total);
            hist_total += (long long)S * n;
            den[k] = (double)(S * n);
        }
        hi0[k] = (long long)rows.size();
    }
    const int NT = (int)nt_size.size();

    int *d_members = nullptr, *d_msize = nullptr, *d_hcnt = nullptr,
        *d_hrank = nullptr, *d_hd = nullptr, *d_ntj;
    long long *d_mstart = nullptr, *d_hbase = nullptr, *d_rows, *d_lo, *d_hi;
    PCK(buf.alloc(&d_ntj, K));
    PCK(hipMemcpy(d_ntj, ntj.data(), K * sizeof(int), hipMemcpyHostToDevice));
    if (NT) {
        // pass 1b
        PCK(buf.alloc(&d_members, N));
        PCK(buf.alloc(&d_mstart, NT));
        PCK(buf.alloc(&d_msize, NT));
        PCK(buf.alloc(&d_hbase, NT));
        PCK(buf.alloc(&d_hcnt, hist_total));
        PCK(buf.alloc(&d_hrank, hist_total));
        PCK(buf.alloc(&d_hd, (size_t)NT * S));
        PCK(hipMemcpy(d_members, members.data(), N * sizeof(int),
                      hipMemcpyHostToDevice));
        PCK(hipMemcpy(d_mstart, nt_start.data(), NT * sizeof(long long),
                      hipMemcpyHostToDevice));
        PCK(hipMemcpy(d_msize, nt_size.data(), NT * sizeof(int),
                      hipMemcpyHostToDevice));
        PCK(hipMemcpy(d_hbase, nt_base.data(), NT * sizeof(long long),
                      hipMemcpyHostToDevice));
        PCK(hipMemset(d_hcnt, 0, (size_t)hist_total * sizeof(int)));
        GtArea area;
        PCK(gt_area((const void *)k_gt_hist, gt_hist_words(N), S, buf, area));
        hipLaunchKernelGGL(k_gt_hist, dim3(area.grid), dim3(256), area.lds, 0,
                           p->assign, (long long)S, (long long)N, d_members,
                           d_mstart, d_msize, d_hbase, NT, area.scratch,
                           area.stride, d_hcnt, d_hrank, d_hd);
        PCK(hipGetLastError());
    }

    // pass 2, the trace in chunks of samples
    const size_t sample_floats = (size_t)W * M;
    int64_t sc = chunk;
    if (sc == 0)
        sc = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20)
                                            / (sample_floats * sizeof(float))));
    sc = std::min(sc, S);
    float *d_P;
    double *d_acc;
    PCK(buf.alloc(&d_rows, rows.size()));
    PCK(buf.alloc(&d_lo, K));
    PCK(buf.alloc(&d_hi, K));
    PCK(buf.alloc(&d_P, (size_t)sc * sample_floats));
    PCK(buf.alloc(&d_acc, (size_t)K * M));
    if (!rows.empty())
        PCK(hipMemcpy(d_rows, rows.data(), rows.size() * sizeof(long long),
                      hipMemcpyHostToDevice));
    PCK(hipMemset(d_acc, 0, (size_t)K * M * sizeof(double)));
    std::vector<long long> lo(K), hi(K), cursor(lo0);
    for (int64_t s0 = 0; s0 < S; s0 += sc) {
        const int64_t n = std::min(sc, S - s0);
        const long long end = (long long)(s0 + n) * W;
        for (int64_t k = 0; k < K; k++) {
            lo[k] = cursor[k];
            while (cursor[k] < hi0[k] && rows[cursor[k]] < end) cursor[k]++;
            hi[k] = cursor[k];
        }
        PCK(hipMemcpy(d_lo, lo.data(), K * sizeof(long long),
                      hipMemcpyHostToDevice));
        PCK(hipMemcpy(d_hi, hi.data(), K * sizeof(long long),
                      hipMemcpyHostToDevice));
        PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                      (size_t)n * sample_floats * sizeof(float),
                      hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_gt_accum,
                           dim3((unsigned)((M + 255) / 256), (unsigned)K),
                           dim3(256), 0, 0, d_P, (long long)s0, (int)n,
                           (long long)S, (int)W, (long long)M, d_rows, d_lo,
                           d_hi, d_ntj, d_msize, d_hbase, d_hcnt, d_hrank,
                           d_hd, d_acc);
        PCK(hipGetLastError());
    }
    PCK(hipMemcpy(geno, d_acc, (size_t)K * M * sizeof(double),
                  hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < K; k++)
        for (int64_t m = 0; m < M; m++) geno[(size_t)k * M + m] /= den[k];
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
                      int64_t K, GtBuffers &buf, int **d_lab,
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
    hipError_t e = buf.alloc(d_lab, lab.size());
    if (e == hipSuccess) e = buf.alloc(d_out, (size_t)N * K);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        bnpc_set_error("support: out of device memory (%s)",
                       hipGetErrorString(e));
        return 5;
    }
    PCK(e);
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
    GtBuffers buf;
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
    GtBuffers buf;
    int *d_lab = nullptr;
    long long *d_out = nullptr;
    unsigned short *d_lab16 = nullptr;
    if (int rc = ps_buffers(p, lab, K, buf, &d_lab, &d_out)) return rc;
    PCK(buf.alloc(&d_lab16, N));
    PCK(hipMemcpy(d_lab16, lab16.data(), N * sizeof(unsigned short),
                  hipMemcpyHostToDevice));
    hipEvent_t ev[2] = {nullptr, nullptr};
    PCK(hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    const long long pairs = (long long)N * (N - 1) / 2;
    for (int which = 0; which < 3 && e == hipSuccess; which++) {
        ms[which] = 0.0f;
        for (int r = 0; r < reps && e == hipSuccess; r++) {
            // (the sums of the first two land in scratch nobody reads)
            e = hipMemsetAsync(p->sums, 0, 2 * sizeof(unsigned long long), 0);
            if (e == hipSuccess) e = hipEventRecord(ev[0], 0);
            if (which == 0)
                hipLaunchKernelGGL(k_differ_sum, dim3(1024), dim3(256), 0, 0,
                                   p->differ, pairs, p->sums);
            else if (which == 1)
                hipLaunchKernelGGL(k_mpear_sums, dim3(1024), dim3(256), 0, 0,
                                   p->differ, (long long)N, d_lab16, 0, 1, 32,
                                   p->sums + 1);
            else
                ps_launch(p, d_lab, K, d_out);
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
            if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
            float t = 0.0f;
            if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[0], ev[1]);
            if (r == 0 || t < ms[which]) ms[which] = t;
        }
    }
    (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    if (e != hipSuccess) {
        bnpc_set_error("pass times: %s", hipGetErrorString(e));
        return 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Per-cell posterior genotypes (-pg): the model-averaged parameter of every
// (cell, mutation).  With r_s(i) the row of cell i's cluster in sample s (the
// distinct labels of the sample below the cell's: gt_rank) and
// v = (double)P[s][r_s(i)][m],
//   sum1[i][m] = sum of v, sum2[i][m] = sum of v * v  (float64, one sample at
//   a time in increasing s from 0.0), ones[i][m] = samples with v > 0.5.
// postproc.host_cell_genotypes is the host loop this is pinned to, bit for
// bit: no atomics on the sums, no tree over the samples.
//
// Per chunk of the trace and slab of cells, two launches:
// k_cg_rank   a workgroup per sample: the presence bitmap of its labels and
//             the prefix popcounts (gt_scan) in LDS, then rank[s][i] as
//             uint16 for the slab's cells.  Working set 8 ceil(N / 32) + 1040
//             bytes; past CG_LDS_MAX a global slice per workgroup, as the
//             genotype pass does.  (Without a rank table it only counts the
//             sample's clusters: the argument check.)
// k_cg_accum  thread = (mutation m, CG_CELLS consecutive cells): the lanes of
//             a wave run along the mutations (256 contiguous bytes of one
//             parameter row per load), the cells' ranks are the same for the
//             whole workgroup (one 16-byte load per sample), and the
//             3 x CG_CELLS accumulators stay in registers over the chunk -
//             CG_CELLS independent add chains per thread.  Workgroups that
//             follow each other share the mutation tile, so a cluster's row
//             is served from cache to all its cells.  Between chunks the
//             accumulators live in the slab's tables on the device.
// ---------------------------------------------------------------------------
#define CG_CELLS 8
#define CG_LDS_MAX 65536            // two workgroups per compute unit at least

static long long cg_rank_words(long long N)
{
    return 260 + 2 * ((N + 31) / 32);
}

// samples [s0, s0 + sc) of a; cells [i0, i0 + nc) of each into rank[q][pitch]
// (q = s - s0), the sample's distinct labels into distinct[q]; either output
// may be NULL
__global__ __launch_bounds__(256) void k_cg_rank(
    const int *__restrict__ a, long long s0, int sc, long long N,
    long long i0, long long nc, long long pitch,
    unsigned *gscratch, long long stride,
    unsigned short *__restrict__ rank, int *__restrict__ distinct)
{
    extern __shared__ __attribute__((aligned(16))) unsigned gt_lds[];
    unsigned *area = gscratch ? gscratch + blockIdx.x * stride : gt_lds;
    const long long nw = (N + 31) / 32;
    unsigned *part = area;
    unsigned *bm = area + 260;
    unsigned *pf = bm + nw;
    const int tid = threadIdx.x;
    for (int q = blockIdx.x; q < sc; q += gridDim.x) {
        const int *row = a + (s0 + q) * N;
        for (long long w = tid; w < nw; w += 256) bm[w] = 0;
        __syncthreads();
        for (long long i = tid; i < N; i += 256) {
            const int L = row[i];
            atomicOr(&bm[L >> 5], 1u << (L & 31));
        }
        __syncthreads();
        const unsigned total = gt_scan(bm, pf, nw, part);
        if (rank) {
            unsigned short *out = rank + (size_t)q * pitch;
            for (long long i = tid; i < nc; i += 256)
                out[i] = (unsigned short)gt_rank(bm, pf, row[i0 + i]);
        }
        if (distinct && tid == 0) distinct[q] = (int)total;
        __syncthreads();                    // the area is reused
    }
}

// one chunk of sc samples: P is its [sc][W][M] float32 trace, rank its
// [sc][pitch] rows (pitch a multiple of CG_CELLS, the padding cells rank 0);
// the tables are the slab's [nc][M]
__global__ __launch_bounds__(256) void k_cg_accum(
    const float *__restrict__ P, int sc, int W, long long M,
    const unsigned short *__restrict__ rank, long long pitch, long long nc,
    double *__restrict__ sum1, double *__restrict__ sum2,
    unsigned *__restrict__ ones)
{
    const long long m = (long long)blockIdx.y * 256 + threadIdx.x;
    if (m >= M) return;
    const long long c0 = (long long)blockIdx.x * CG_CELLS;
    double a1[CG_CELLS], a2[CG_CELLS];
    unsigned n1[CG_CELLS];
#pragma unroll
    for (int c = 0; c < CG_CELLS; c++) {
        const bool in = c0 + c < nc;
        const size_t at = (size_t)(in ? c0 + c : c0) * M + m;
        a1[c] = in ? sum1[at] : 0.0;
        a2[c] = in ? sum2[at] : 0.0;
        n1[c] = in ? ones[at] : 0u;
    }
    const unsigned short *rk = rank + c0;
    const size_t sample = (size_t)W * M;
    const float *Ps = P + m;
#pragma unroll 2
    for (int q = 0; q < sc; q++) {
        // the workgroup's CG_CELLS ranks: 16 aligned bytes, the same address
        // in every lane
        const uint4 packed = *(const uint4 *)rk;
        const unsigned r2[4] = {packed.x, packed.y, packed.z, packed.w};
        float f[CG_CELLS];
#pragma unroll
        for (int c = 0; c < CG_CELLS; c++) {
            const unsigned r = (r2[c >> 1] >> (16 * (c & 1))) & 0xffffu;
            f[c] = Ps[(size_t)r * M];
        }
#pragma unroll
        for (int c = 0; c < CG_CELLS; c++) {
            const double v = (double)f[c];
            a1[c] += v;
            a2[c] += v * v;     // exact product: FMA or not, the same bits
            n1[c] += v > 0.5 ? 1u : 0u;
        }
        rk += pitch;
        Ps += sample;
    }
#pragma unroll
    for (int c = 0; c < CG_CELLS; c++) {
        if (c0 + c < nc) {
            const size_t at = (size_t)(c0 + c) * M + m;
            sum1[at] = a1[c];
            sum2[at] = a2[c];
            ones[at] = n1[c];
        }
    }
}

namespace {
struct CgEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~CgEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
}  // namespace

// ms (NULL, or 3 floats): device-event milliseconds summed over the call -
// ms[0] the trace uploads, ms[1] k_cg_rank, ms[2] k_cg_accum
static int cg_run(bnpc_post *p, const float *params, int64_t W, int64_t M,
                  int64_t chunk, int64_t slab, double *sum1, double *sum2,
                  uint32_t *ones, float *ms)
{
    if (!p || !params || W < 1 || W >= (int64_t)GT_MIXED || M < 1
        || M > (int64_t)65535 * 256 || chunk < 0 || slab < 0) {
        bnpc_set_error("bad argument: cell genotypes need a 1 <= W < 65534 x "
                       "M >= 1 trace, chunk >= 0 and slab >= 0");
        return 2;
    }
    if (!p->assign || !p->labels_in_range) {
        bnpc_set_error("cell genotypes: the sample labels must lie in "
                       "[0, N = %lld)", (long long)p->N);
        return 2;
    }
    const int64_t S = p->S, N = p->N;
    PCK(hipSetDevice(p->device));
    GtBuffers buf;
    CgEvents evs;
    auto oom = [](hipError_t e) {
        (void)hipGetLastError();
        bnpc_set_error("cell genotypes: out of device memory (%s)",
                       hipGetErrorString(e));
        return 5;
    };
#define CGA(expr)                                                            \
    do {                                                                     \
        hipError_t a_ = (expr);                                              \
        if (a_ == hipErrorOutOfMemory) return oom(a_);                       \
        PCK(a_);                                                             \
    } while (0)

    // every sample's cluster count against the trace's rows, before anything
    // is added up
    GtArea area;
    int *d_distinct;
    CGA(buf.alloc(&d_distinct, S));
    if ((size_t)cg_rank_words(N) * 4 <= CG_LDS_MAX) {
        area.grid = (unsigned)std::min<int64_t>(S, 65535);
        area.lds = (size_t)cg_rank_words(N) * 4;
    } else {
        area.grid = (unsigned)std::min<int64_t>(S, GT_GLOBAL_WG);
        area.stride = cg_rank_words(N);
        CGA(buf.alloc(&area.scratch, (size_t)area.grid * area.stride));
    }
    std::vector<int> distinct(S);
    for (int64_t s0 = 0; s0 < S; s0 += INT_MAX) {
        const int64_t n = std::min<int64_t>(INT_MAX, S - s0);
        hipLaunchKernelGGL(k_cg_rank, dim3(area.grid), dim3(256), area.lds, 0,
                           p->assign, (long long)s0, (int)n, (long long)N, 0LL,
                           0LL, 0LL, area.scratch, area.stride,
                           (unsigned short *)nullptr, d_distinct + s0);
        PCK(hipGetLastError());
    }
    PCK(hipMemcpy(distinct.data(), d_distinct, S * sizeof(int),
                  hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < S; s++) {
        if (distinct[s] > W) {
            bnpc_set_error("cell genotypes: sample %lld has %d clusters, the "
                           "trace %lld rows", (long long)s, distinct[s],
                           (long long)W);
            return 2;
        }
    }

    // the chunk of the trace, then as many cells as fit beside it
    const size_t sample_floats = (size_t)W * M;
    int64_t sc = chunk;
    if (sc == 0)
        sc = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20)
                                            / (sample_floats * sizeof(float))));
    sc = std::min<int64_t>(std::min(sc, S), INT_MAX);
    float *d_P;
    CGA(buf.alloc(&d_P, (size_t)sc * sample_floats));
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    // per cell: the three table rows and its ranks (the pitch rounds up)
    const size_t per_cell = (size_t)M * 20 + (size_t)sc * 2;
    const size_t margin = ((size_t)64 << 20) + (size_t)sc * 2 * CG_CELLS;
    const size_t room = free_b > margin ? (free_b - margin) / per_cell : 0;
    int64_t nc = slab ? std::min(slab, N)
                      : (int64_t)std::min<size_t>((size_t)N, room);
    if (nc < 1 || (size_t)nc > room) {
        bnpc_set_error("cell genotypes: a slab of %lld cells x %lld mutations "
                       "needs %.1f GB, %.1f GB of device memory are free",
                       (long long)std::max<int64_t>(nc, 1), (long long)M,
                       (double)std::max<int64_t>(nc, 1) * per_cell / 1e9,
                       free_b / 1e9);
        return 5;
    }
    const int64_t pitch = (nc + CG_CELLS - 1) / CG_CELLS * CG_CELLS;
    unsigned short *d_rank;
    double *d_sum1, *d_sum2;
    unsigned *d_ones;
    CGA(buf.alloc(&d_rank, (size_t)sc * pitch));
    CGA(buf.alloc(&d_sum1, (size_t)nc * M));
    CGA(buf.alloc(&d_sum2, (size_t)nc * M));
    CGA(buf.alloc(&d_ones, (size_t)nc * M));
#undef CGA
    // (the padding cells of a row keep rank 0: a row every trace has)
    PCK(hipMemset(d_rank, 0, (size_t)sc * pitch * sizeof(unsigned short)));
    if (ms) {
        ms[0] = ms[1] = ms[2] = 0.0f;
        PCK(hipEventCreate(&evs.ev[0]));
        PCK(hipEventCreate(&evs.ev[1]));
    }
    // a lap of the device's clock: begin(), the work, end(its slot of ms)
    int lap_rc = 0;
    auto begin = [&]() {
        if (ms && hipEventRecord(evs.ev[0], 0) != hipSuccess) lap_rc = 1;
    };
    auto end = [&](int which) {
        if (!ms) return;
        float t = 0.0f;
        if (hipEventRecord(evs.ev[1], 0) != hipSuccess
            || hipEventSynchronize(evs.ev[1]) != hipSuccess
            || hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]) != hipSuccess)
            lap_rc = 1;
        ms[which] += t;
    };
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t cells = std::min(nc, N - i0);
        PCK(hipMemset(d_sum1, 0, (size_t)cells * M * sizeof(double)));
        PCK(hipMemset(d_sum2, 0, (size_t)cells * M * sizeof(double)));
        PCK(hipMemset(d_ones, 0, (size_t)cells * M * sizeof(unsigned)));
        for (int64_t s0 = 0; s0 < S; s0 += sc) {
            const int64_t n = std::min(sc, S - s0);
            begin();
            PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                          (size_t)n * sample_floats * sizeof(float),
                          hipMemcpyHostToDevice));
            end(0);
            begin();
            hipLaunchKernelGGL(k_cg_rank,
                               dim3((unsigned)std::min<int64_t>(n, area.grid)),
                               dim3(256), area.lds, 0, p->assign,
                               (long long)s0, (int)n, (long long)N,
                               (long long)i0, (long long)cells,
                               (long long)pitch, area.scratch, area.stride,
                               d_rank, (int *)nullptr);
            PCK(hipGetLastError());
            end(1);
            begin();
            hipLaunchKernelGGL(k_cg_accum,
                               dim3((unsigned)((cells + CG_CELLS - 1) / CG_CELLS),
                                    (unsigned)((M + 255) / 256)),
                               dim3(256), 0, 0, d_P, (int)n, (int)W,
                               (long long)M, d_rank, (long long)pitch,
                               (long long)cells, d_sum1, d_sum2, d_ones);
            PCK(hipGetLastError());
            end(2);
        }
        const size_t at = (size_t)i0 * M, count = (size_t)cells * M;
        if (sum1)
            PCK(hipMemcpy(sum1 + at, d_sum1, count * sizeof(double),
                          hipMemcpyDeviceToHost));
        if (sum2)
            PCK(hipMemcpy(sum2 + at, d_sum2, count * sizeof(double),
                          hipMemcpyDeviceToHost));
        if (ones)
            PCK(hipMemcpy(ones + at, d_ones, count * sizeof(unsigned),
                          hipMemcpyDeviceToHost));
    }
    PCK(hipDeviceSynchronize());
    if (lap_rc) {
        bnpc_set_error("cell genotypes: the device events failed");
        return 1;
    }
    return 0;
}

extern "C" int bnpc_post_cell_genotypes(bnpc_post *p, const float *params,
                                        int64_t W, int64_t M, int64_t chunk,
                                        int64_t slab, double *sum1,
                                        double *sum2, uint32_t *ones)
{
    return cg_run(p, params, W, M, chunk, slab, sum1, sum2, ones, nullptr);
}

// diagnostic (tools/posterior_bench.py): one bnpc_post_cell_genotypes call
// without its tables' way back, by device events (see cg_run)
extern "C" int bnpc_post_cell_genotypes_times(bnpc_post *p,
                                              const float *params, int64_t W,
                                              int64_t M, int64_t chunk,
                                              int64_t slab, float *ms)
{
    if (!ms) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    return cg_run(p, params, W, M, chunk, slab, nullptr, nullptr, nullptr, ms);
}

// ---------------------------------------------------------------------------
// Per-cell posterior fit (-pf): the pointwise log-likelihood of every cell in
// every posterior sample and its per-cell reductions.  With r_s(i) the row of
// cell i's cluster in sample s (k_cg_rank), th = P[s][r][m] (float32),
// t = (double)th and o = (double)(1.0f - th),
//   L1 = log(t * (1 - FN[s]) + o * FP[s])   L0 = log(t * FN[s] + o * (1 - FP[s]))
// (the expressions of k_tables_theta, every operation rounded on its own),
//   ll[s][i] = sum over m of L1[s][r][m] where the cell shows a 1, L0 where
//              it shows a 0, nothing where the entry is missing
// and per cell, over its column of ll one sample at a time in increasing s:
// mean = (sum from 0.0) / S, m2 = sum of (ll - mean)^2,
// lme = mx + log(sum of exp(ll - mx)) - log(S) with mx the column's maximum.
// postproc.host_cell_fit is the host loop this is pinned to: mean and m2 bit
// for bit on the returned ll; ll itself to the rounding of a sum over the
// mutations in another order (no atomics: the same bits on every call).
//
// Per slab of cells the data go up once as two bit planes (is-1, is-0), 32
// mutations to a word pair; per chunk of the trace, three launches:
// k_cg_rank    the slab's ranks of the chunk's samples (as for -pg)
// k_cf_tables  thread = one (sample, row, mutation) of the chunk: L1 and L0 as
//              float64 [sc][W][M], the rows below the sample's cluster count
// k_cf_sums    workgroup = (CG_CELLS consecutive cells, sample): the lanes run
//              along the mutations (512 contiguous bytes of one table row per
//              wave and load, which all cells of the cluster share from
//              cache), a lane adds the elements m = lane, lane + 256, ... of
//              each of its cells into an accumulator of its own, then a fixed
//              tree over the workgroup (shuffles in the wave, the four waves
//              in order) and LL[s][cell] of the slab, which stays on the
//              device over all chunks
// and after the last chunk
// k_cf_reduce  thread = cell: two walks down its S values of LL.
// LL resident (S x slab x 8 bytes) is what makes the reductions independent
// of the chunking: mean is needed before m2 and the maximum before the
// exp-sum, over all the samples.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cf_tables(
    const float *__restrict__ P, int sc, int W, long long M,
    const int *__restrict__ distinct, const double *__restrict__ FN,
    const double *__restrict__ FP, double *__restrict__ L1,
    double *__restrict__ L0)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int q = blockIdx.y; q < sc; q += gridDim.y) {
        if (idx >= (long long)distinct[q] * M) continue;
        const size_t at = (size_t)q * W * M + idx;
        const double fn = FN[q], fp = FP[q];
        const float th = P[at];
        const double th64 = (double)th;
        const double om64 = (double)(1.0f - th);
        L1[at] = log(th64 * (1.0 - fn) + om64 * fp);
        L0[at] = log(th64 * fn + om64 * (1.0 - fp));
    }
}

// one chunk of sc samples, the first of them sample s0: L1 / L0 its tables,
// rank its [sc][pitch] rows (pitch a multiple of CG_CELLS, the padding cells
// rank 0), planes the slab's [pitch][nwm] word pairs (x: is-1, y: is-0; the
// padding cells and the bits past M zero), LL the slab's [S][pitch]
__global__ __launch_bounds__(256) void k_cf_sums(
    const double *__restrict__ L1, const double *__restrict__ L0, int sc,
    int W, long long M, const unsigned short *__restrict__ rank,
    long long pitch, long long nc, const uint2 *__restrict__ planes,
    long long nwm, long long s0, double *__restrict__ LL)
{
    __shared__ double part[4][CG_CELLS];
    const int tid = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * CG_CELLS;
    const uint2 *pl = planes + (size_t)c0 * nwm;
    for (int q = blockIdx.y; q < sc; q += gridDim.y) {
        // the workgroup's CG_CELLS ranks: 16 aligned bytes, the same address
        // in every lane
        const uint4 packed = *(const uint4 *)(rank + (size_t)q * pitch + c0);
        const unsigned r2[4] = {packed.x, packed.y, packed.z, packed.w};
        const double *t1[CG_CELLS], *t0[CG_CELLS];
        double acc[CG_CELLS];
#pragma unroll
        for (int c = 0; c < CG_CELLS; c++) {
            const unsigned r = (r2[c >> 1] >> (16 * (c & 1))) & 0xffffu;
            const size_t row = ((size_t)q * W + r) * M;
            t1[c] = L1 + row;
            t0[c] = L0 + row;
            acc[c] = 0.0;
        }
        for (long long m = tid; m < M; m += 256) {
            const unsigned bit = 1u << (m & 31);
            double v[CG_CELLS];
#pragma unroll
            for (int c = 0; c < CG_CELLS; c++) {
                const uint2 w = pl[(size_t)c * nwm + (m >> 5)];
                const double *src = (w.x & bit) ? t1[c] : t0[c];
                v[c] = ((w.x | w.y) & bit) ? src[m] : 0.0;
            }
#pragma unroll
            for (int c = 0; c < CG_CELLS; c++) acc[c] += v[c];
        }
#pragma unroll
        for (int c = 0; c < CG_CELLS; c++) {
            double v = acc[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((tid & 63) == 0) part[tid >> 6][c] = v;
        }
        __syncthreads();
        if (tid < CG_CELLS && c0 + tid < nc)
            LL[(size_t)(s0 + q) * pitch + c0 + tid] =
                ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        __syncthreads();                    // part is reused
    }
}

// cell i of the slab: its column LL[0 .. S)[i] in increasing s
__global__ __launch_bounds__(256) void k_cf_reduce(
    const double *__restrict__ LL, long long S, long long pitch, long long nc,
    double *__restrict__ mean, double *__restrict__ m2,
    double *__restrict__ lme)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const double *col = LL + i;
    double mx = col[0], acc = 0.0;
    for (long long s = 0; s < S; s++) {
        const double v = col[(size_t)s * pitch];
        mx = v > mx ? v : mx;
        acc += v;
    }
    const double mu = acc / (double)S;
    double dev = 0.0, es = 0.0;
    for (long long s = 0; s < S; s++) {
        const double v = col[(size_t)s * pitch];
        dev += (v - mu) * (v - mu);
        es += exp(v - mx);
    }
    mean[i] = mu;
    m2[i] = dev;
    lme[i] = (mx + log(es)) - log((double)S);
}

// ms (NULL, or 5 floats): device-event milliseconds summed over the call -
// ms[0] the uploads (bit planes and trace), ms[1] k_cg_rank, ms[2]
// k_cf_tables, ms[3] k_cf_sums, ms[4] k_cf_reduce
static int cf_run(bnpc_post *p, const uint8_t *codes, const float *params,
                  int64_t W, int64_t M, const double *FN, const double *FP,
                  int64_t chunk, int64_t slab, double *mean, double *m2,
                  double *lme, double *ll, float *ms)
{
    if (!p || !codes || !params || !FN || !FP || W < 1
        || W >= (int64_t)GT_MIXED || M < 1
        || (W * M + 255) / 256 > (int64_t)INT_MAX || chunk < 0 || slab < 0) {
        bnpc_set_error("bad argument: the cell fit needs the data's codes, a "
                       "1 <= W < 65534 x M >= 1 trace, FN, FP, chunk >= 0 and "
                       "slab >= 0");
        return 2;
    }
    if (!p->assign || !p->labels_in_range) {
        bnpc_set_error("cell fit: the sample labels must lie in [0, N = %lld)",
                       (long long)p->N);
        return 2;
    }
    const int64_t S = p->S, N = p->N;
    for (int64_t s = 0; s < S; s++) {
        if (!(FN[s] > 0.0 && FN[s] < 1.0 && FP[s] > 0.0 && FP[s] < 1.0)) {
            bnpc_set_error("cell fit: FN = %g, FP = %g of sample %lld are not "
                           "both inside (0, 1)", FN[s], FP[s], (long long)s);
            return 2;
        }
    }
    // the two bit planes of every cell, 32 mutations to a word pair
    const int64_t nwm = (M + 31) / 32;
    std::vector<uint2> planes((size_t)N * nwm, make_uint2(0u, 0u));
    for (int64_t i = 0; i < N; i++) {
        const uint8_t *row = codes + (size_t)i * M;
        uint2 *out = planes.data() + (size_t)i * nwm;
        for (int64_t m = 0; m < M; m++) {
            const uint8_t c = row[m];
            if (c == 1) {
                out[m >> 5].x |= 1u << (m & 31);
            } else if (c == 0) {
                out[m >> 5].y |= 1u << (m & 31);
            } else if (c != 3) {
                bnpc_set_error("cell fit: code %d of cell %lld at mutation "
                               "%lld is not 0, 1 or 3", (int)c, (long long)i,
                               (long long)m);
                return 2;
            }
        }
    }
    PCK(hipSetDevice(p->device));
    GtBuffers buf;
    CgEvents evs;
    auto oom = [](hipError_t e) {
        (void)hipGetLastError();
        bnpc_set_error("cell fit: out of device memory (%s)",
                       hipGetErrorString(e));
        return 5;
    };
#define CFA(expr)                                                            \
    do {                                                                     \
        hipError_t a_ = (expr);                                              \
        if (a_ == hipErrorOutOfMemory) return oom(a_);                       \
        PCK(a_);                                                             \
    } while (0)

    // every sample's cluster count against the trace's rows, before anything
    // is added up; the table kernel reads the counts too
    GtArea area;
    int *d_distinct;
    CFA(buf.alloc(&d_distinct, S));
    if ((size_t)cg_rank_words(N) * 4 <= CG_LDS_MAX) {
        area.grid = (unsigned)std::min<int64_t>(S, 65535);
        area.lds = (size_t)cg_rank_words(N) * 4;
    } else {
        area.grid = (unsigned)std::min<int64_t>(S, GT_GLOBAL_WG);
        area.stride = cg_rank_words(N);
        CFA(buf.alloc(&area.scratch, (size_t)area.grid * area.stride));
    }
    std::vector<int> distinct(S);
    for (int64_t s0 = 0; s0 < S; s0 += INT_MAX) {
        const int64_t n = std::min<int64_t>(INT_MAX, S - s0);
        hipLaunchKernelGGL(k_cg_rank, dim3(area.grid), dim3(256), area.lds, 0,
                           p->assign, (long long)s0, (int)n, (long long)N, 0LL,
                           0LL, 0LL, area.scratch, area.stride,
                           (unsigned short *)nullptr, d_distinct + s0);
        PCK(hipGetLastError());
    }
    PCK(hipMemcpy(distinct.data(), d_distinct, S * sizeof(int),
                  hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < S; s++) {
        if (distinct[s] > W) {
            bnpc_set_error("cell fit: sample %lld has %d clusters, the trace "
                           "%lld rows", (long long)s, distinct[s],
                           (long long)W);
            return 2;
        }
    }

    // the chunk of the trace and its two tables (20 bytes per parameter),
    // then as many cells as fit beside them
    const size_t sample_floats = (size_t)W * M;
    int64_t sc = chunk;
    if (sc == 0)
        sc = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20)
                                            / (sample_floats * 20)));
    sc = std::min<int64_t>(std::min(sc, S), INT_MAX);
    float *d_P;
    double *d_L1, *d_L0, *d_FN, *d_FP;
    CFA(buf.alloc(&d_P, (size_t)sc * sample_floats));
    CFA(buf.alloc(&d_L1, (size_t)sc * sample_floats));
    CFA(buf.alloc(&d_L0, (size_t)sc * sample_floats));
    CFA(buf.alloc(&d_FN, (size_t)S));
    CFA(buf.alloc(&d_FP, (size_t)S));
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    // per cell: its column of LL, its bit planes, its ranks and the three
    // results (the pitch rounds up)
    const size_t per_cell = (size_t)S * 8 + (size_t)nwm * 8 + (size_t)sc * 2
        + 24;
    const size_t margin = ((size_t)64 << 20) + per_cell * CG_CELLS;
    const size_t room = free_b > margin ? (free_b - margin) / per_cell : 0;
    int64_t nc = slab ? std::min(slab, N)
                      : (int64_t)std::min<size_t>((size_t)N, room);
    if (nc < 1 || (size_t)nc > room) {
        bnpc_set_error("cell fit: a slab of %lld cells x %lld samples needs "
                       "%.1f GB, %.1f GB of device memory are free",
                       (long long)std::max<int64_t>(nc, 1), (long long)S,
                       (double)std::max<int64_t>(nc, 1) * per_cell / 1e9,
                       free_b / 1e9);
        return 5;
    }
    const int64_t pitch = (nc + CG_CELLS - 1) / CG_CELLS * CG_CELLS;
    unsigned short *d_rank;
    uint2 *d_planes;
    double *d_LL, *d_out;
    CFA(buf.alloc(&d_rank, (size_t)sc * pitch));
    CFA(buf.alloc(&d_planes, (size_t)pitch * nwm));
    CFA(buf.alloc(&d_LL, (size_t)S * pitch));
    CFA(buf.alloc(&d_out, (size_t)3 * nc));
#undef CFA
    // (the padding cells of a row keep rank 0, a row every trace has, and
    // empty planes)
    PCK(hipMemset(d_rank, 0, (size_t)sc * pitch * sizeof(unsigned short)));
    PCK(hipMemset(d_planes, 0, (size_t)pitch * nwm * sizeof(uint2)));
    PCK(hipMemcpy(d_FN, FN, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_FP, FP, S * sizeof(double), hipMemcpyHostToDevice));
    if (ms) {
        for (int k = 0; k < 5; k++) ms[k] = 0.0f;
        PCK(hipEventCreate(&evs.ev[0]));
        PCK(hipEventCreate(&evs.ev[1]));
    }
    // a lap of the device's clock: begin(), the work, end(its slot of ms)
    int lap_rc = 0;
    auto begin = [&]() {
        if (ms && hipEventRecord(evs.ev[0], 0) != hipSuccess) lap_rc = 1;
    };
    auto end = [&](int which) {
        if (!ms) return;
        float t = 0.0f;
        if (hipEventRecord(evs.ev[1], 0) != hipSuccess
            || hipEventSynchronize(evs.ev[1]) != hipSuccess
            || hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]) != hipSuccess)
            lap_rc = 1;
        ms[which] += t;
    };
    const unsigned table_blocks = (unsigned)((W * M + 255) / 256);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t cells = std::min(nc, N - i0);
        const unsigned tiles = (unsigned)((cells + CG_CELLS - 1) / CG_CELLS);
        begin();
        PCK(hipMemcpy(d_planes, planes.data() + (size_t)i0 * nwm,
                      (size_t)cells * nwm * sizeof(uint2),
                      hipMemcpyHostToDevice));
        // (a last, shorter slab: its tile's padding cells are empty too)
        if (cells < pitch)
            PCK(hipMemset(d_planes + (size_t)cells * nwm, 0,
                          (size_t)(pitch - cells) * nwm * sizeof(uint2)));
        end(0);
        for (int64_t s0 = 0; s0 < S; s0 += sc) {
            const int64_t n = std::min(sc, S - s0);
            const unsigned rows = (unsigned)std::min<int64_t>(n, 65535);
            begin();
            PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                          (size_t)n * sample_floats * sizeof(float),
                          hipMemcpyHostToDevice));
            end(0);
            begin();
            hipLaunchKernelGGL(k_cg_rank,
                               dim3((unsigned)std::min<int64_t>(n, area.grid)),
                               dim3(256), area.lds, 0, p->assign,
                               (long long)s0, (int)n, (long long)N,
                               (long long)i0, (long long)cells,
                               (long long)pitch, area.scratch, area.stride,
                               d_rank, (int *)nullptr);
            PCK(hipGetLastError());
            end(1);
            begin();
            hipLaunchKernelGGL(k_cf_tables, dim3(table_blocks, rows),
                               dim3(256), 0, 0, d_P, (int)n, (int)W,
                               (long long)M, d_distinct + s0, d_FN + s0,
                               d_FP + s0, d_L1, d_L0);
            PCK(hipGetLastError());
            end(2);
            begin();
            hipLaunchKernelGGL(k_cf_sums, dim3(tiles, rows), dim3(256), 0, 0,
                               d_L1, d_L0, (int)n, (int)W, (long long)M,
                               d_rank, (long long)pitch, (long long)cells,
                               d_planes, (long long)nwm, (long long)s0, d_LL);
            PCK(hipGetLastError());
            end(3);
        }
        begin();
        hipLaunchKernelGGL(k_cf_reduce, dim3((unsigned)((cells + 255) / 256)),
                           dim3(256), 0, 0, d_LL, (long long)S,
                           (long long)pitch, (long long)cells, d_out,
                           d_out + nc, d_out + 2 * nc);
        PCK(hipGetLastError());
        end(4);
        double *host[3] = {mean, m2, lme};
        for (int k = 0; k < 3; k++)
            if (host[k])
                PCK(hipMemcpy(host[k] + i0, d_out + (size_t)k * nc,
                              cells * sizeof(double), hipMemcpyDeviceToHost));
        if (ll)
            PCK(hipMemcpy2D(ll + i0, (size_t)N * sizeof(double), d_LL,
                            (size_t)pitch * sizeof(double),
                            (size_t)cells * sizeof(double), (size_t)S,
                            hipMemcpyDeviceToHost));
    }
    PCK(hipDeviceSynchronize());
    if (lap_rc) {
        bnpc_set_error("cell fit: the device events failed");
        return 1;
    }
    return 0;
}

extern "C" int bnpc_post_cell_fit(bnpc_post *p, const uint8_t *codes,
                                  const float *params, int64_t W, int64_t M,
                                  const double *FN, const double *FP,
                                  int64_t chunk, int64_t slab, double *mean,
                                  double *m2, double *lme, double *ll)
{
    return cf_run(p, codes, params, W, M, FN, FP, chunk, slab, mean, m2, lme,
                  ll, nullptr);
}

// diagnostic (tools/posterior_bench.py): one bnpc_post_cell_fit call without
// its results' way back, by device events (see cf_run)
extern "C" int bnpc_post_cell_fit_times(bnpc_post *p, const uint8_t *codes,
                                        const float *params, int64_t W,
                                        int64_t M, const double *FN,
                                        const double *FP, int64_t chunk,
                                        int64_t slab, float *ms)
{
    if (!ms) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    return cf_run(p, codes, params, W, M, FN, FP, chunk, slab, nullptr,
                  nullptr, nullptr, nullptr, ms);
}

// ---------------------------------------------------------------------------
// Per-mutation posterior fit and error rates (-pm): how well the model
// explains every column of the data, and the error rates the column implies.
// Within one sample all cells of a cluster share their parameter row, so
// everything per mutation follows from the exact column counts
//   c1[s][r][m], c0[s][r][m] = cells of row r in sample s that show a 1 / a 0
// and a float64 walk down the sample's rows.  With th = P[s][r][m] (float32),
// t = (double)th, o = (double)(1.0f - th) and the expressions of k_cf_tables,
//   a1 = t * (1 - FN[s])  b1 = o * FP[s]        d1 = a1 + b1  L1 = log(d1)
//   a0 = t * FN[s]        b0 = o * (1 - FP[s])  d0 = a0 + b0  L0 = log(d0)
//   qfp = b1 / d1   qfn = a0 / d0
// per (s, m), over r = 0 .. D_s - 1 in increasing r from 0.0:
//   ll  += (double)c1 * L1 + (double)c0 * L0      efn += (double)c0 * qfn
//   efp += (double)c1 * qfp      eg1 += (double)c1 * (a1 / d1) + (double)c0 * qfn
//   call1_obs1 += c1, call1_obs0 += c0 where th > 0.5f
// and per mutation, over the samples in increasing s: the sums of ll, ll * ll,
// efn, efp, eg1 and the two integers.  postproc.host_mutation_fit is the host
// loop this is pinned to: everything but log bit for bit.
//
// The counts do not depend on the order of the cells, so once per call the
// cells are sorted by a hint clustering and the data become 64-cell lane masks
// {ones, zeros}[block of 64 cells][mutation] (k_mf_masks).  Per chunk of the
// trace:
// k_cg_rank   every cell's rank in the chunk's samples (as for -pg)
// k_mf_count  wave = (sample, 64 mutations), lane = mutation.  Per block of
//             cells the wave turns the block's 64 ranks (lane = cell for this
//             one load) into wave-uniform (row, member mask) pairs - the first
//             remaining lane's rank, the ballot of the equal ones, repeat -
//             and per pair adds popcount(ones & mask), popcount(zeros & mask)
//             to counts[row][lane] in LDS.  The wave owns its tile: no
//             atomics, no barrier.  A tile holds MF_ROWS rows; a sample with
//             more takes its rows in passes of MF_ROWS, the subtotals carried
//             in registers, so the order over r is the same.  After a pass
//             lane m walks the pass's rows and forms the subtotals of (s, m).
// k_mf_reduce thread = mutation: the chunk's subtotals in sample order into
//             the seven accumulators, which stay on the device between chunks.
// ---------------------------------------------------------------------------
#define MF_ROWS 32                  // rows of a wave's LDS tile: 16 KB

// cells [0, cells) of a slab in sorted order, codes their [cells][M] bytes;
// block b of the slab into masks[b][Mp] (x: ones, y: zeros; the cells past
// `cells` and the columns past M empty).  bad: the smallest slab index of a
// code other than 0 / 1 / 3.
__global__ __launch_bounds__(256) void k_mf_masks(
    const uint8_t *__restrict__ codes, long long cells, long long M,
    long long Mp, ulonglong2 *__restrict__ masks,
    unsigned long long *__restrict__ bad)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= Mp) return;
    const long long j0 = (long long)blockIdx.y * 64;
    unsigned long long ones = 0ull, zeros = 0ull;
    if (m < M) {
        const int n = (int)(cells - j0 < 64 ? cells - j0 : 64);
        for (int l = 0; l < n; l++) {
            const size_t at = (size_t)(j0 + l) * M + m;
            const unsigned c = codes[at];
            if (c == 1u)
                ones |= 1ull << l;
            else if (c == 0u)
                zeros |= 1ull << l;
            else if (c != 3u)
                atomicMin(bad, (unsigned long long)at);
        }
    }
    masks[(size_t)blockIdx.y * Mp + m] = make_ulonglong2(ones, zeros);
}

// one chunk of sc samples: P its [sc][W][M] trace, rank its [sc][N] rows by
// cell, perm the cells in sorted order, masks the [nb][Mp] lane masks of the
// sorted cells; sub the chunk's [6][sc][M] subtotals (ll, efn, efp, eg1 as
// float64, call1_obs1, call1_obs0 as int64)
__global__ __launch_bounds__(64) void k_mf_count(
    const float *__restrict__ P, int sc, int W, long long M, long long Mp,
    const int *__restrict__ distinct, const double *__restrict__ FN,
    const double *__restrict__ FP, const unsigned short *__restrict__ rank,
    const int *__restrict__ perm, long long N,
    const ulonglong2 *__restrict__ masks, long long nb,
    double *__restrict__ sub)
{
    __shared__ unsigned cnt[MF_ROWS][2][64];
    const int lane = threadIdx.x;
    const long long m = (long long)blockIdx.x * 64 + lane;
    const bool mv = m < M;
    const ulonglong2 *mk_col = masks + m;           // m < Mp always
    const size_t plane = (size_t)sc * M;
    for (int q = blockIdx.y; q < sc; q += gridDim.y) {
        const int D = distinct[q];
        const double fn = FN[q], fp = FP[q];
        const unsigned short *rk = rank + (size_t)q * N;
        const float *Pq = P + (size_t)q * W * M + (mv ? m : 0);
        double ll = 0.0, efn = 0.0, efp = 0.0, eg1 = 0.0;
        long long k1 = 0, k0 = 0;
        for (int r0 = 0; r0 < D; r0 += MF_ROWS) {
            const int rows = D - r0 < MF_ROWS ? D - r0 : MF_ROWS;
            for (int r = 0; r < rows; r++) {
                cnt[r][0][lane] = 0u;
                cnt[r][1][lane] = 0u;
            }
            for (long long b = 0; b < nb; b++) {
                // lane = cell of the block here
                const long long j = b * 64 + lane;
                const bool in = j < N;
                const int mine = in ? (int)rk[perm[j]] : -1;
                const ulonglong2 w = mk_col[(size_t)b * Mp];
                unsigned long long left = __ballot(in);
                while (left) {
                    const int first = __ffsll((unsigned long long)left) - 1;
                    const int r = __builtin_amdgcn_readlane(mine, first);
                    const unsigned long long members = __ballot(mine == r);
                    left &= ~members;
                    const int at = r - r0;
                    if (at >= 0 && at < rows) {     // the same in every lane
                        cnt[at][0][lane] += (unsigned)__popcll(w.x & members);
                        cnt[at][1][lane] += (unsigned)__popcll(w.y & members);
                    }
                }
            }
            // lane = mutation: the pass's rows in increasing r
            for (int r = 0; r < rows; r++) {
                const unsigned u1 = cnt[r][0][lane], u0 = cnt[r][1][lane];
                const float th = mv ? Pq[(size_t)(r0 + r) * M] : 0.5f;
                const double t = (double)th;
                const double o = (double)(1.0f - th);
                const double a1 = t * (1.0 - fn), b1 = o * fp;
                const double a0 = t * fn, b0 = o * (1.0 - fp);
                const double d1 = a1 + b1, d0 = a0 + b0;
                const double qfp = b1 / d1, qfn = a0 / d0;
                const double c1 = (double)u1, c0 = (double)u0;
                ll += c1 * log(d1) + c0 * log(d0);
                efn += c0 * qfn;
                efp += c1 * qfp;
                eg1 += c1 * (a1 / d1) + c0 * qfn;
                if (th > 0.5f) {
                    k1 += u1;
                    k0 += u0;
                }
            }
        }
        if (mv) {
            const size_t at = (size_t)q * M + m;
            sub[at] = ll;
            sub[plane + at] = efn;
            sub[2 * plane + at] = efp;
            sub[3 * plane + at] = eg1;
            ((long long *)sub)[4 * plane + at] = k1;
            ((long long *)sub)[5 * plane + at] = k0;
        }
    }
}

// mutation m: the chunk's sc subtotals in sample order into acc, [7][M]:
// sum_ll, sum_ll2, efn, efp, eg1 (float64), call1_obs1, call1_obs0 (int64)
__global__ __launch_bounds__(256) void k_mf_reduce(
    const double *__restrict__ sub, int sc, long long M,
    double *__restrict__ acc)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const size_t plane = (size_t)sc * M;
    const long long *isub = (const long long *)sub;
    long long *iacc = (long long *)acc;
    double s1 = acc[m], s2 = acc[M + m], fn = acc[2 * M + m];
    double fp = acc[3 * M + m], g1 = acc[4 * M + m];
    long long k1 = iacc[5 * M + m], k0 = iacc[6 * M + m];
    for (int q = 0; q < sc; q++) {
        const size_t at = (size_t)q * M + m;
        const double v = sub[at];
        s1 += v;
        s2 += v * v;
        fn += sub[plane + at];
        fp += sub[2 * plane + at];
        g1 += sub[3 * plane + at];
        k1 += isub[4 * plane + at];
        k0 += isub[5 * plane + at];
    }
    acc[m] = s1;
    acc[M + m] = s2;
    acc[2 * M + m] = fn;
    acc[3 * M + m] = fp;
    acc[4 * M + m] = g1;
    iacc[5 * M + m] = k1;
    iacc[6 * M + m] = k0;
}

// ms (NULL, or 5 floats): device-event milliseconds summed over the call -
// ms[0] the uploads (data, permutation, trace) and k_mf_masks, ms[1]
// k_cg_rank, ms[2] k_mf_count, ms[3] 0 (the subtotals are the tail of
// k_mf_count), ms[4] k_mf_reduce
static int mf_run(bnpc_post *p, const uint8_t *codes, const float *params,
                  int64_t W, int64_t M, const double *FN, const double *FP,
                  const int32_t *order_hint, int64_t chunk, double *const out[5],
                  int64_t *const iout[2], double *ll, float *ms)
{
    if (!p || !codes || !params || !FN || !FP || W < 1
        || W >= (int64_t)GT_MIXED || M < 1
        || (W * M + 255) / 256 > (int64_t)INT_MAX || chunk < 0) {
        bnpc_set_error("bad argument: the mutation fit needs the data's codes, "
                       "a 1 <= W < 65534 x M >= 1 trace, FN, FP and chunk >= 0");
        return 2;
    }
    if (!p->assign || !p->labels_in_range) {
        bnpc_set_error("mutation fit: the sample labels must lie in [0, N = "
                       "%lld)", (long long)p->N);
        return 2;
    }
    const int64_t S = p->S, N = p->N;
    for (int64_t s = 0; s < S; s++) {
        if (!(FN[s] > 0.0 && FN[s] < 1.0 && FP[s] > 0.0 && FP[s] < 1.0)) {
            bnpc_set_error("mutation fit: FN = %g, FP = %g of sample %lld are "
                           "not both inside (0, 1)", FN[s], FP[s],
                           (long long)s);
            return 2;
        }
    }
    PCK(hipSetDevice(p->device));
    GtBuffers buf;
    CgEvents evs;
    auto oom = [](hipError_t e) {
        (void)hipGetLastError();
        bnpc_set_error("mutation fit: out of device memory (%s)",
                       hipGetErrorString(e));
        return 5;
    };
#define MFA(expr)                                                            \
    do {                                                                     \
        hipError_t a_ = (expr);                                              \
        if (a_ == hipErrorOutOfMemory) return oom(a_);                       \
        PCK(a_);                                                             \
    } while (0)

    // every sample's cluster count against the trace's rows, before anything
    // is added up; the counting kernel reads the counts too
    GtArea area;
    int *d_distinct;
    MFA(buf.alloc(&d_distinct, S));
    if ((size_t)cg_rank_words(N) * 4 <= CG_LDS_MAX) {
        area.grid = (unsigned)std::min<int64_t>(S, 65535);
        area.lds = (size_t)cg_rank_words(N) * 4;
    } else {
        area.grid = (unsigned)std::min<int64_t>(S, GT_GLOBAL_WG);
        area.stride = cg_rank_words(N);
        MFA(buf.alloc(&area.scratch, (size_t)area.grid * area.stride));
    }
    std::vector<int> distinct(S);
    for (int64_t s0 = 0; s0 < S; s0 += INT_MAX) {
        const int64_t n = std::min<int64_t>(INT_MAX, S - s0);
        hipLaunchKernelGGL(k_cg_rank, dim3(area.grid), dim3(256), area.lds, 0,
                           p->assign, (long long)s0, (int)n, (long long)N, 0LL,
                           0LL, 0LL, area.scratch, area.stride,
                           (unsigned short *)nullptr, d_distinct + s0);
        PCK(hipGetLastError());
    }
    PCK(hipMemcpy(distinct.data(), d_distinct, S * sizeof(int),
                  hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < S; s++) {
        if (distinct[s] > W) {
            bnpc_set_error("mutation fit: sample %lld has %d clusters, the "
                           "trace %lld rows", (long long)s, distinct[s],
                           (long long)W);
            return 2;
        }
    }

    // the cells in the order of the hint's labels (stable): the labels of the
    // last sample where there is no hint
    std::vector<int32_t> hint(N);
    if (order_hint)
        memcpy(hint.data(), order_hint, (size_t)N * sizeof(int32_t));
    else
        PCK(hipMemcpy(hint.data(), p->assign + (size_t)(S - 1) * N,
                      (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int> perm(N);
    for (int64_t i = 0; i < N; i++) perm[i] = (int)i;
    std::stable_sort(perm.begin(), perm.end(),
                     [&](int a, int b) { return hint[a] < hint[b]; });

    // the working set: the lane masks, a slab of the data while they are
    // built, the chunk of the trace with its ranks and subtotals
    const int64_t nb = (N + 63) / 64;
    const int64_t Mp = (M + 63) / 64 * 64;
    const size_t sample_floats = (size_t)W * M;
    const size_t per_sample = sample_floats * 4 + (size_t)M * 48 + (size_t)N * 2;
    int64_t sc = chunk;
    if (sc == 0)
        sc = std::max<int64_t>(1, (int64_t)(((size_t)512 << 20) / per_sample));
    sc = std::min<int64_t>(std::min(sc, S), INT_MAX);
    // (64 cells at the least, about 64 MB of codes and what a launch's second
    // dimension takes at the most)
    const int64_t slab_blocks = std::min<int64_t>(std::min<int64_t>(nb, 65535),
        std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / ((size_t)M * 64))));
    const int64_t slab_cells = slab_blocks * 64;
    const size_t need = (size_t)nb * Mp * 16 + (size_t)slab_cells * M
        + (size_t)sc * per_sample + (size_t)M * 56 + (size_t)N * 4
        + (size_t)S * 16;
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    if (need + ((size_t)64 << 20) > free_b) {
        bnpc_set_error("mutation fit: %lld cells x %lld mutations with chunks "
                       "of %lld samples need %.1f GB, %.1f GB of device memory "
                       "are free", (long long)N, (long long)M, (long long)sc,
                       need / 1e9, free_b / 1e9);
        return 5;
    }
    ulonglong2 *d_masks;
    uint8_t *d_codes;
    unsigned long long *d_bad;
    int *d_perm;
    float *d_P;
    unsigned short *d_rank;
    double *d_sub, *d_acc, *d_FN, *d_FP;
    MFA(buf.alloc(&d_masks, (size_t)nb * Mp));
    MFA(buf.alloc(&d_codes, (size_t)slab_cells * M));
    MFA(buf.alloc(&d_bad, 1));
    MFA(buf.alloc(&d_perm, (size_t)N));
    MFA(buf.alloc(&d_P, (size_t)sc * sample_floats));
    MFA(buf.alloc(&d_rank, (size_t)sc * N));
    MFA(buf.alloc(&d_sub, (size_t)6 * sc * M));
    MFA(buf.alloc(&d_acc, (size_t)7 * M));
    MFA(buf.alloc(&d_FN, (size_t)S));
    MFA(buf.alloc(&d_FP, (size_t)S));
#undef MFA
    if (ms) {
        for (int k = 0; k < 5; k++) ms[k] = 0.0f;
        PCK(hipEventCreate(&evs.ev[0]));
        PCK(hipEventCreate(&evs.ev[1]));
    }
    // a lap of the device's clock: begin(), the work, end(its slot of ms)
    int lap_rc = 0;
    auto begin = [&]() {
        if (ms && hipEventRecord(evs.ev[0], 0) != hipSuccess) lap_rc = 1;
    };
    auto end = [&](int which) {
        if (!ms) return;
        float t = 0.0f;
        if (hipEventRecord(evs.ev[1], 0) != hipSuccess
            || hipEventSynchronize(evs.ev[1]) != hipSuccess
            || hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]) != hipSuccess)
            lap_rc = 1;
        ms[which] += t;
    };

    // the lane masks, a slab of sorted cells at a time
    PCK(hipMemset(d_bad, 0xff, sizeof(unsigned long long)));
    PCK(hipMemset(d_acc, 0, (size_t)7 * M * sizeof(double)));
    PCK(hipMemcpy(d_FN, FN, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_FP, FP, S * sizeof(double), hipMemcpyHostToDevice));
    std::vector<uint8_t> stage((size_t)std::min(slab_cells, N) * M);
    for (int64_t j0 = 0; j0 < N; j0 += slab_cells) {
        const int64_t cells = std::min(slab_cells, N - j0);
        for (int64_t j = 0; j < cells; j++)
            memcpy(stage.data() + (size_t)j * M,
                   codes + (size_t)perm[j0 + j] * M, (size_t)M);
        begin();
        PCK(hipMemcpy(d_codes, stage.data(), (size_t)cells * M,
                      hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_mf_masks,
                           dim3((unsigned)((Mp + 255) / 256),
                                (unsigned)((cells + 63) / 64)),
                           dim3(256), 0, 0, d_codes, (long long)cells,
                           (long long)M, (long long)Mp,
                           d_masks + (size_t)(j0 / 64) * Mp, d_bad);
        PCK(hipGetLastError());
        end(0);
        unsigned long long bad = 0;
        PCK(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
        if (bad != ~0ull) {
            const int64_t j = j0 + (int64_t)(bad / (unsigned long long)M);
            const int64_t m = (int64_t)(bad % (unsigned long long)M);
            bnpc_set_error("mutation fit: code %d of cell %lld at mutation "
                           "%lld is not 0, 1 or 3",
                           (int)codes[(size_t)perm[j] * M + m],
                           (long long)perm[j], (long long)m);
            return 2;
        }
    }
    begin();
    PCK(hipMemcpy(d_perm, perm.data(), (size_t)N * sizeof(int),
                  hipMemcpyHostToDevice));
    end(0);

    const unsigned mtiles = (unsigned)(Mp / 64);
    for (int64_t s0 = 0; s0 < S; s0 += sc) {
        const int64_t n = std::min(sc, S - s0);
        begin();
        PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                      (size_t)n * sample_floats * sizeof(float),
                      hipMemcpyHostToDevice));
        end(0);
        begin();
        hipLaunchKernelGGL(k_cg_rank,
                           dim3((unsigned)std::min<int64_t>(n, area.grid)),
                           dim3(256), area.lds, 0, p->assign, (long long)s0,
                           (int)n, (long long)N, 0LL, (long long)N,
                           (long long)N, area.scratch, area.stride, d_rank,
                           (int *)nullptr);
        PCK(hipGetLastError());
        end(1);
        begin();
        hipLaunchKernelGGL(k_mf_count,
                           dim3(mtiles, (unsigned)std::min<int64_t>(n, 65535)),
                           dim3(64), 0, 0, d_P, (int)n, (int)W, (long long)M,
                           (long long)Mp, d_distinct + s0, d_FN + s0,
                           d_FP + s0, d_rank, d_perm, (long long)N, d_masks,
                           (long long)nb, d_sub);
        PCK(hipGetLastError());
        end(2);
        begin();
        hipLaunchKernelGGL(k_mf_reduce, dim3((unsigned)((M + 255) / 256)),
                           dim3(256), 0, 0, d_sub, (int)n, (long long)M,
                           d_acc);
        PCK(hipGetLastError());
        end(4);
        // (the chunk's ll: the first plane of its subtotals; a failure here
        // is a device failure, not an argument's)
        if (ll)
            PCK(hipMemcpy(ll + (size_t)s0 * M, d_sub,
                          (size_t)n * M * sizeof(double),
                          hipMemcpyDeviceToHost));
    }
    PCK(hipDeviceSynchronize());
    for (int k = 0; k < 5; k++)
        if (out[k])
            PCK(hipMemcpy(out[k], d_acc + (size_t)k * M, M * sizeof(double),
                          hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; k++)
        if (iout[k])
            PCK(hipMemcpy(iout[k], d_acc + (size_t)(5 + k) * M,
                          M * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (lap_rc) {
        bnpc_set_error("mutation fit: the device events failed");
        return 1;
    }
    return 0;
}

extern "C" int bnpc_post_mutation_fit(bnpc_post *p, const uint8_t *codes,
                                      const float *params, int64_t W,
                                      int64_t M, const double *FN,
                                      const double *FP,
                                      const int32_t *order_hint, int64_t chunk,
                                      double *sum_ll, double *sum_ll2,
                                      double *efn, double *efp, double *eg1,
                                      int64_t *call1_obs1, int64_t *call1_obs0,
                                      double *ll)
{
    double *const out[5] = {sum_ll, sum_ll2, efn, efp, eg1};
    int64_t *const iout[2] = {call1_obs1, call1_obs0};
    return mf_run(p, codes, params, W, M, FN, FP, order_hint, chunk, out, iout,
                  ll, nullptr);
}

// diagnostic (tools/posterior_bench.py): one bnpc_post_mutation_fit call
// without its results' way back, by device events (see mf_run)
extern "C" int bnpc_post_mutation_fit_times(bnpc_post *p, const uint8_t *codes,
                                            const float *params, int64_t W,
                                            int64_t M, const double *FN,
                                            const double *FP,
                                            const int32_t *order_hint,
                                            int64_t chunk, float *ms)
{
    if (!ms) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    double *const out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t *const iout[2] = {nullptr, nullptr};
    return mf_run(p, codes, params, W, M, FN, FP, order_hint, chunk, out, iout,
                  nullptr, ms);
}

// ---------------------------------------------------------------------------
// Doublet scores (-pd): the log-likelihood of every cell under every single
// posterior cluster and under every unordered pair of them.  Candidate c < K
// is the cluster c; then the pairs (a, b), a < b, in lexicographic order,
// P = K + K (K - 1) / 2 in all.  With theta the K x M cluster genotypes
// (float64) and one FN, FP:
//   single  t = theta[k][m], o = 1.0 - t
//   pair    o = (1.0 - theta[a][m]) * (1.0 - theta[b][m]), t = 1.0 - o
//   L1 = log(t * (1 - FN) + o * FP)      L0 = log(t * FN + o * (1 - FP))
// (every operation rounded on its own), score[i][c] the sum over the mutations,
// strictly in increasing m from 0.0, of L1[c][m] where cell i shows a 1 and
// L0[c][m] where it shows a 0, and per cell, over its candidates in index
// order, the reductions of postproc.host_doublets, the host loop this is
// pinned to.
//
// Once per call the data go up, the cells in their own order, and k_mf_masks
// turns them into the lane masks {ones, zeros}[block of 64 cells][mutation].
// Per slab of cells and chunk of candidates:
// k_db_tables  thread = (candidate of the chunk, mutation): L1 and L0 as
//              T[tile][m][2][DB_TILE], so that what a tile needs at one
//              mutation is 2 * DB_TILE contiguous doubles
// k_db_sums    wave = (block of 64 cells, tile of DB_TILE candidates), lane =
//              cell, DB_TILE accumulators in registers, the loop over the
//              mutations in increasing m.  The masks and the tile's table
//              values depend on the wave alone (the wave's number goes
//              through readfirstlane), so they arrive by scalar loads and
//              stay in scalar registers.  A lane's weight of L1 is the mask
//              select w1 = its bit of `ones` ? 1.0 : 0.0 (one v_cndmask on the
//              scalar mask, once per mutation for the whole tile), w0 likewise
//              from `zeros`, and per candidate acc = fma(w1, L1, acc),
//              acc = fma(w0, L0, acc) with the table value as the scalar
//              operand: fma(1.0, L, acc) is the rounded sum acc + L and
//              fma(0.0, L, acc) is acc itself (L is finite and acc is never
//              -0.0), so each score is bit for bit the sequential sum of the
//              device's own tables.  No atomics, no cross-lane step, no split
//              of the mutations.  The four waves of a workgroup take
//              different cell blocks of one tile and share its table lines in
//              cache.  Results go to SCO[candidate][cell of the slab], which
//              stays on the device over all chunks.
// and after the last chunk
// k_db_reduce  thread = cell: its P scores in candidate order.
// SCO resident (P x slab x 8 bytes) is what makes the reductions independent
// of the chunking: the largest weighted score of a group is needed before
// its exp-sum.
// ---------------------------------------------------------------------------
#define DB_TILE 8                   // candidates of a wave: 16 accumulator VGPRs
#define DB_UNROLL 2                 // mutations per trip of the sums loop

__global__ __launch_bounds__(256) void k_db_tables(
    const double *__restrict__ theta, long long M,
    const int2 *__restrict__ pair, int slots, double fn, double fp,
    double *__restrict__ T)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    for (int q = blockIdx.y; q < slots; q += gridDim.y) {
        // (a, -1): the single a; (-1, -1): a padding slot of the last tile
        const int2 ab = pair[q];
        double l1 = 0.0, l0 = 0.0;
        if (ab.x >= 0) {
            double t, o;
            if (ab.y < 0) {
                t = theta[(size_t)ab.x * M + m];
                o = 1.0 - t;
            } else {
                o = (1.0 - theta[(size_t)ab.x * M + m])
                    * (1.0 - theta[(size_t)ab.y * M + m]);
                t = 1.0 - o;
            }
            l1 = log(t * (1.0 - fn) + o * fp);
            l0 = log(t * fn + o * (1.0 - fp));
        }
        double *dst = T + ((size_t)(q / DB_TILE) * M + m) * (2 * DB_TILE)
            + q % DB_TILE;
        dst[0] = l1;
        dst[DB_TILE] = l0;
    }
}

// 1.0 in the lanes whose bit of the wave-uniform mask is set, else 0.0
__device__ __forceinline__ double db_weight(unsigned long long mask)
{
    return __builtin_amdgcn_inverse_ballot_w64(mask) ? 1.0 : 0.0;
}

#define DB_STEP(mm)                                                          \
    do {                                                                     \
        const ulonglong2 w_ = mk[mm];                                        \
        const double w1_ = db_weight(w_.x), w0_ = db_weight(w_.y);           \
        const double *row_ = tab + (size_t)(mm) * (2 * DB_TILE);             \
        _Pragma("unroll") for (int j = 0; j < DB_TILE; j++) {                \
            acc[j] = fma(w1_, row_[j], acc[j]);                              \
            acc[j] = fma(w0_, row_[DB_TILE + j], acc[j]);                    \
        }                                                                    \
    } while (0)

// one chunk of n candidates, the first of them candidate c0: T its tables,
// masks the [blocks][Mp] lane masks of all cells, b0 the slab's first block,
// nblk its blocks; SCO the slab's [P][pitch = 64 nblk] scores
__global__ __launch_bounds__(256) void k_db_sums(
    const double *__restrict__ T, int n, long long M, long long Mp,
    const ulonglong2 *__restrict__ masks, long long b0, long long nblk,
    long long pitch, long long c0, double *__restrict__ SCO)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int tile = (int)blockIdx.x;
    const double *tab = T + (size_t)tile * M * (2 * DB_TILE);
    for (long long b = (long long)blockIdx.y * 4 + wave; b < nblk;
         b += (long long)gridDim.y * 4) {
        const ulonglong2 *mk = masks + (size_t)(b0 + b) * Mp;
        double acc[DB_TILE];
#pragma unroll
        for (int j = 0; j < DB_TILE; j++) acc[j] = 0.0;
        long long m = 0;
        for (; m + DB_UNROLL <= M; m += DB_UNROLL) {
#pragma unroll
            for (int u = 0; u < DB_UNROLL; u++) DB_STEP(m + u);
        }
        for (; m < M; m++) DB_STEP(m);
#pragma unroll
        for (int j = 0; j < DB_TILE; j++)
            if (tile * DB_TILE + j < n)
                SCO[(size_t)(c0 + tile * DB_TILE + j) * pitch + b * 64 + lane]
                    = acc[j];
    }
}
#undef DB_STEP

// cell i of the slab: its column SCO[0 .. P)[off + i] in candidate order.
// prior[c] is the log-weight of candidate c; the pair of a candidate is
// carried along the walk
__global__ __launch_bounds__(256) void k_db_reduce(
    const double *__restrict__ SCO, long long pitch, long long off,
    long long nc, const int *__restrict__ labels, int K,
    const double *__restrict__ prior, double *__restrict__ own,
    double *__restrict__ ll_single, double *__restrict__ lse_single,
    double *__restrict__ ll_pair, double *__restrict__ lse_pair,
    int *__restrict__ best_single, int2 *__restrict__ best_pair)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const double *col = SCO + off + i;
    double best = col[0], mx = best + prior[0];
    int arg = 0;
    for (int k = 1; k < K; k++) {
        const double v = col[(size_t)k * pitch];
        const double y = v + prior[k];
        if (v > best) {
            best = v;
            arg = k;
        }
        mx = y > mx ? y : mx;
    }
    double es = 0.0;
    for (int k = 0; k < K; k++)
        es += exp((col[(size_t)k * pitch] + prior[k]) - mx);
    own[i] = col[(size_t)labels[i] * pitch];
    ll_single[i] = best;
    best_single[i] = arg;
    lse_single[i] = mx + log(es);
    if (K < 2) {
        ll_pair[i] = -INFINITY;
        lse_pair[i] = -INFINITY;
        best_pair[i] = make_int2(-1, -1);
        return;
    }
    const double *pcol = col + (size_t)K * pitch;
    const double *pprior = prior + K;
    best = pcol[0];
    mx = best + pprior[0];
    int2 at = make_int2(0, 1), ab = make_int2(0, 1);
    long long c = 0;
    for (;;) {
        const double v = pcol[(size_t)c * pitch];
        const double y = v + pprior[c];
        if (v > best) {
            best = v;
            at = ab;
        }
        mx = y > mx ? y : mx;
        c++;
        if (++ab.y == K) {
            if (++ab.x == K - 1) break;
            ab.y = ab.x + 1;
        }
    }
    es = 0.0;
    for (long long q = 0; q < c; q++)
        es += exp((pcol[(size_t)q * pitch] + pprior[q]) - mx);
    ll_pair[i] = best;
    lse_pair[i] = mx + log(es);
    best_pair[i] = at;
}

namespace {
struct DbOut {
    double *own, *ll_single, *lse_single, *ll_pair, *lse_pair;
    int32_t *best_single, *best_pair;
    double *scores, *L1, *L0;
};
}  // namespace

// ms (NULL, or 4 floats): device-event milliseconds summed over the call -
// ms[0] the uploads and k_mf_masks, ms[1] k_db_tables, ms[2] k_db_sums, ms[3]
// k_db_reduce
static int db_run(bnpc_post *p, const uint8_t *codes, int64_t M,
                  const int32_t *labels, int64_t K, const double *theta,
                  double FN, double FP, const double *logw, double lN,
                  double lT, int64_t chunk, int64_t slab, const DbOut &out,
                  float *ms)
{
    if (!p || !codes || !labels || !theta || !logw || M < 1 || K < 1
        || (M + 255) / 256 > (int64_t)INT_MAX || chunk < 0 || slab < 0) {
        bnpc_set_error("bad argument: the doublet scores need the data's "
                       "codes, M >= 1, N labels, K >= 1 x M cluster genotypes, "
                       "K log-weights, chunk >= 0 and slab >= 0");
        return 2;
    }
    const int64_t N = p->N;
    // (K (K + 1) / 2 < 2^31 is K < 65536)
    if (K >= 65536) {
        bnpc_set_error("doublets: %lld clusters give 2^31 candidates or more",
                       (long long)K);
        return 2;
    }
    const int64_t P = K + K * (K - 1) / 2;
    if (!(FN > 0.0 && FN < 1.0 && FP > 0.0 && FP < 1.0)) {
        bnpc_set_error("doublets: FN = %g, FP = %g are not both inside (0, 1)",
                       FN, FP);
        return 2;
    }
    if (!std::isfinite(lN) || (K > 1 && !std::isfinite(lT))) {
        bnpc_set_error("doublets: the log-weights' norms lN = %g, lT = %g are "
                       "not finite", lN, lT);
        return 2;
    }
    std::vector<int64_t> sizes(K, 0);
    for (int64_t i = 0; i < N; i++) {
        if (labels[i] < 0 || labels[i] >= K) {
            bnpc_set_error("doublets: label %d of cell %lld is not in [0, K = "
                           "%lld)", (int)labels[i], (long long)i, (long long)K);
            return 2;
        }
        sizes[labels[i]]++;
    }
    for (int64_t k = 0; k < K; k++) {
        if (!sizes[k]) {
            bnpc_set_error("doublets: cluster %lld is empty", (long long)k);
            return 2;
        }
        if (!std::isfinite(logw[k])) {
            bnpc_set_error("doublets: the log-weight %g of cluster %lld is not "
                           "finite", logw[k], (long long)k);
            return 2;
        }
    }
    for (int64_t at = 0; at < K * M; at++) {
        if (!(theta[at] >= 0.0 && theta[at] <= 1.0)) {
            bnpc_set_error("doublets: the genotype %g of cluster %lld at "
                           "mutation %lld is not in [0, 1]", theta[at],
                           (long long)(at / M), (long long)(at % M));
            return 2;
        }
    }
    // the candidates' log-weights, in the definition's arithmetic
    std::vector<double> prior((size_t)P);
    for (int64_t k = 0; k < K; k++) prior[k] = logw[k] - lN;
    {
        size_t c = (size_t)K;
        for (int64_t a = 0; a < K; a++)
            for (int64_t b = a + 1; b < K; b++)
                prior[c++] = (logw[a] + logw[b]) - lT;
    }

    PCK(hipSetDevice(p->device));
    GtBuffers buf;
    CgEvents evs;
    auto oom = [](hipError_t e) {
        (void)hipGetLastError();
        bnpc_set_error("doublets: out of device memory (%s)",
                       hipGetErrorString(e));
        return 5;
    };
#define DBA(expr)                                                            \
    do {                                                                     \
        hipError_t a_ = (expr);                                              \
        if (a_ == hipErrorOutOfMemory) return oom(a_);                       \
        PCK(a_);                                                             \
    } while (0)

    // the working set: the lane masks of all cells, a slab of the data while
    // they are built, the genotypes, a chunk's tables, and per resident cell
    // its P scores and seven results
    const int64_t nb = (N + 63) / 64;
    const int64_t Mp = (M + 63) / 64 * 64;
    const int64_t code_blocks = std::min<int64_t>(std::min<int64_t>(nb, 65535),
        std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / ((size_t)M * 64))));
    const int64_t code_cells = code_blocks * 64;
    // (a launch's first dimension times its 256 threads stays below 2^32)
    const int64_t chunk_max = std::min<int64_t>(P, (int64_t)1 << 24);
    int64_t sc = chunk ? std::min(chunk, chunk_max)
                       : std::min<int64_t>(chunk_max, std::max<int64_t>(DB_TILE,
                             (int64_t)(((size_t)512 << 20) / ((size_t)M * 16))));
    const size_t per_cell = (size_t)P * 8 + 56;
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    auto fixed = [&](int64_t cands) {
        const size_t tiles = (size_t)((cands + DB_TILE - 1) / DB_TILE);
        return (size_t)nb * Mp * 16 + (size_t)code_cells * M
            + (size_t)K * M * 8 + tiles * M * (16 * DB_TILE)
            + tiles * DB_TILE * 8 + (size_t)P * 8 + (size_t)N * 4
            + ((size_t)64 << 20);
    };
    // (an unaligned slab of nc cells touches (nc + 62) / 64 + 1 blocks)
    auto blocks_of = [](int64_t nc) { return (nc + 62) / 64 + 1; };
    auto room = [&](int64_t cands) {
        const size_t f = fixed(cands);
        return free_b > f ? (int64_t)((free_b - f) / per_cell) : (int64_t)0;
    };
    // (the pitch of nc cells is below nc + 128)
    if (!chunk && room(sc) < 192) sc = std::min<int64_t>(sc, DB_TILE);
    const int64_t fit = room(sc) - 128;
    int64_t nc;
    if (slab) {
        nc = std::min(slab, N);
        if (nc > fit) nc = 0;
    } else {
        nc = std::min(N, fit);
        if (nc < N) nc = nc / 64 * 64;          // whole blocks
    }
    if (nc < 1) {
        bnpc_set_error("doublets: %lld candidates x 64 cells beside a chunk of "
                       "%lld candidates x %lld mutations need %.1f GB, %.1f GB "
                       "of device memory are free", (long long)P,
                       (long long)sc, (long long)M,
                       (fixed(sc) + 128.0 * per_cell) / 1e9, free_b / 1e9);
        return 5;
    }
    const int64_t tiles_c = (sc + DB_TILE - 1) / DB_TILE;
    const int64_t slots = tiles_c * DB_TILE;
    const int64_t nblk_max = nc >= N ? nb : blocks_of(nc);
    const int64_t pitch = nblk_max * 64;
    ulonglong2 *d_masks;
    uint8_t *d_codes;
    unsigned long long *d_bad;
    int2 *d_pair, *d_bp;
    int *d_labels, *d_bs;
    double *d_theta, *d_T, *d_prior, *d_SC, *d_res;
    DBA(buf.alloc(&d_masks, (size_t)nb * Mp));
    DBA(buf.alloc(&d_codes, (size_t)code_cells * M));
    DBA(buf.alloc(&d_bad, 1));
    DBA(buf.alloc(&d_theta, (size_t)K * M));
    DBA(buf.alloc(&d_T, (size_t)tiles_c * M * (2 * DB_TILE)));
    DBA(buf.alloc(&d_pair, (size_t)slots));
    DBA(buf.alloc(&d_prior, (size_t)P));
    DBA(buf.alloc(&d_labels, (size_t)N));
    DBA(buf.alloc(&d_SC, (size_t)P * pitch));
    DBA(buf.alloc(&d_res, (size_t)5 * nc));
    DBA(buf.alloc(&d_bs, (size_t)nc));
    DBA(buf.alloc(&d_bp, (size_t)nc));
#undef DBA
    if (ms) {
        for (int k = 0; k < 4; k++) ms[k] = 0.0f;
        PCK(hipEventCreate(&evs.ev[0]));
        PCK(hipEventCreate(&evs.ev[1]));
    }
    // a lap of the device's clock: begin(), the work, end(its slot of ms)
    int lap_rc = 0;
    auto begin = [&]() {
        if (ms && hipEventRecord(evs.ev[0], 0) != hipSuccess) lap_rc = 1;
    };
    auto end = [&](int which) {
        if (!ms) return;
        float t = 0.0f;
        if (hipEventRecord(evs.ev[1], 0) != hipSuccess
            || hipEventSynchronize(evs.ev[1]) != hipSuccess
            || hipEventElapsedTime(&t, evs.ev[0], evs.ev[1]) != hipSuccess)
            lap_rc = 1;
        ms[which] += t;
    };

    // the lane masks of all cells, a slab of the data at a time: every code
    // is looked at before anything is written
    PCK(hipMemset(d_bad, 0xff, sizeof(unsigned long long)));
    for (int64_t j0 = 0; j0 < N; j0 += code_cells) {
        const int64_t cells = std::min(code_cells, N - j0);
        begin();
        PCK(hipMemcpy(d_codes, codes + (size_t)j0 * M, (size_t)cells * M,
                      hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_mf_masks,
                           dim3((unsigned)((Mp + 255) / 256),
                                (unsigned)((cells + 63) / 64)),
                           dim3(256), 0, 0, d_codes, (long long)cells,
                           (long long)M, (long long)Mp,
                           d_masks + (size_t)(j0 / 64) * Mp, d_bad);
        PCK(hipGetLastError());
        end(0);
        unsigned long long bad = 0;
        PCK(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
        if (bad != ~0ull) {
            const int64_t i = j0 + (int64_t)(bad / (unsigned long long)M);
            const int64_t m = (int64_t)(bad % (unsigned long long)M);
            bnpc_set_error("doublets: code %d of cell %lld at mutation %lld is "
                           "not 0, 1 or 3", (int)codes[(size_t)i * M + m],
                           (long long)i, (long long)m);
            return 2;
        }
    }
    begin();
    PCK(hipMemcpy(d_theta, theta, (size_t)K * M * sizeof(double),
                  hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_prior, prior.data(), (size_t)P * sizeof(double),
                  hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_labels, labels, (size_t)N * sizeof(int),
                  hipMemcpyHostToDevice));
    end(0);

    std::vector<int2> pairs((size_t)slots);
    std::vector<double> stage;
    const bool one_chunk = sc >= P;
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t cells = std::min(nc, N - i0);
        const int64_t b0 = i0 / 64, off = i0 - b0 * 64;
        const int64_t nblk = (i0 + cells - 1) / 64 - b0 + 1;
        // the walk over the candidates: (a, -1) the singles, then the pairs
        int64_t a = 0, b = -1;
        for (int64_t c0 = 0; c0 < P; c0 += sc) {
            const int64_t n = std::min(sc, P - c0);
            const int64_t tiles = (n + DB_TILE - 1) / DB_TILE;
            if (!one_chunk || i0 == 0) {
                for (int64_t q = 0; q < tiles * DB_TILE; q++) {
                    if (q >= n) {
                        pairs[q] = make_int2(-1, -1);
                        continue;
                    }
                    pairs[q] = make_int2((int)a, (int)b);
                    if (b < 0) {            // the next single, or pair (0, 1)
                        if (++a == K) {
                            a = 0;
                            b = 1;
                        }
                    } else if (++b == K) {
                        a++;
                        b = a + 1;
                    }
                }
                begin();
                PCK(hipMemcpy(d_pair, pairs.data(),
                              (size_t)tiles * DB_TILE * sizeof(int2),
                              hipMemcpyHostToDevice));
                end(0);
                begin();
                hipLaunchKernelGGL(k_db_tables,
                                   dim3((unsigned)((M + 255) / 256),
                                        (unsigned)std::min<int64_t>(
                                            tiles * DB_TILE, 65535)),
                                   dim3(256), 0, 0, d_theta, (long long)M,
                                   d_pair, (int)(tiles * DB_TILE), FN, FP, d_T);
                PCK(hipGetLastError());
                end(1);
                if (i0 == 0 && (out.L1 || out.L0)) {
                    stage.resize((size_t)tiles * M * (2 * DB_TILE));
                    PCK(hipMemcpy(stage.data(), d_T,
                                  stage.size() * sizeof(double),
                                  hipMemcpyDeviceToHost));
                    for (int64_t q = 0; q < n; q++) {
                        const double *src = stage.data()
                            + (size_t)(q / DB_TILE) * M * (2 * DB_TILE)
                            + q % DB_TILE;
                        for (int64_t m = 0; m < M; m++) {
                            if (out.L1)
                                out.L1[(size_t)(c0 + q) * M + m]
                                    = src[(size_t)m * (2 * DB_TILE)];
                            if (out.L0)
                                out.L0[(size_t)(c0 + q) * M + m]
                                    = src[(size_t)m * (2 * DB_TILE) + DB_TILE];
                        }
                    }
                }
            }
            begin();
            hipLaunchKernelGGL(k_db_sums,
                               dim3((unsigned)tiles,
                                    (unsigned)std::min<int64_t>((nblk + 3) / 4,
                                                                65535)),
                               dim3(256), 0, 0, d_T, (int)n, (long long)M,
                               (long long)Mp, d_masks, (long long)b0,
                               (long long)nblk, (long long)pitch,
                               (long long)c0, d_SC);
            PCK(hipGetLastError());
            end(2);
        }
        begin();
        hipLaunchKernelGGL(k_db_reduce, dim3((unsigned)((cells + 255) / 256)),
                           dim3(256), 0, 0, d_SC, (long long)pitch,
                           (long long)off, (long long)cells, d_labels + i0,
                           (int)K, d_prior, d_res, d_res + nc, d_res + 2 * nc,
                           d_res + 3 * nc, d_res + 4 * nc, d_bs, d_bp);
        PCK(hipGetLastError());
        end(3);
        double *host[5] = {out.own, out.ll_single, out.lse_single, out.ll_pair,
                           out.lse_pair};
        for (int k = 0; k < 5; k++)
            if (host[k])
                PCK(hipMemcpy(host[k] + i0, d_res + (size_t)k * nc,
                              cells * sizeof(double), hipMemcpyDeviceToHost));
        if (out.best_single)
            PCK(hipMemcpy(out.best_single + i0, d_bs, cells * sizeof(int),
                          hipMemcpyDeviceToHost));
        if (out.best_pair)
            PCK(hipMemcpy(out.best_pair + 2 * i0, d_bp, cells * sizeof(int2),
                          hipMemcpyDeviceToHost));
        if (out.scores) {
            // SCO is [candidate][cell]: through the host, turned
            stage.resize((size_t)P * cells);
            PCK(hipMemcpy2D(stage.data(), (size_t)cells * sizeof(double),
                            d_SC + off, (size_t)pitch * sizeof(double),
                            (size_t)cells * sizeof(double), (size_t)P,
                            hipMemcpyDeviceToHost));
            for (int64_t c = 0; c < P; c++)
                for (int64_t i = 0; i < cells; i++)
                    out.scores[(size_t)(i0 + i) * P + c]
                        = stage[(size_t)c * cells + i];
        }
    }
    PCK(hipDeviceSynchronize());
    if (lap_rc) {
        bnpc_set_error("doublets: the device events failed");
        return 1;
    }
    return 0;
}

extern "C" int bnpc_post_doublets(bnpc_post *p, const uint8_t *codes,
                                  int64_t M, const int32_t *labels, int64_t K,
                                  const double *theta, double FN, double FP,
                                  const double *logw, double lN, double lT,
                                  int64_t chunk, int64_t slab, double *own,
                                  double *ll_single, double *lse_single,
                                  double *ll_pair, double *lse_pair,
                                  int32_t *best_single, int32_t *best_pair,
                                  double *scores, double *L1, double *L0)
{
    const DbOut out = {own, ll_single, lse_single, ll_pair, lse_pair,
                       best_single, best_pair, scores, L1, L0};
    return db_run(p, codes, M, labels, K, theta, FN, FP, logw, lN, lT, chunk,
                  slab, out, nullptr);
}

// diagnostic (tools/posterior_bench.py): one bnpc_post_doublets call without
// its results' way back, by device events (see db_run)
extern "C" int bnpc_post_doublets_times(bnpc_post *p, const uint8_t *codes,
                                        int64_t M, const int32_t *labels,
                                        int64_t K, const double *theta,
                                        double FN, double FP,
                                        const double *logw, double lN,
                                        double lT, int64_t chunk, int64_t slab,
                                        float *ms)
{
    if (!ms) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    const DbOut out = {};
    return db_run(p, codes, M, labels, K, theta, FN, FP, logw, lN, lT, chunk,
                  slab, out, ms);
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
    GtBuffers buf;
    CgEvents evs;
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
    if (reps) {
        PCK(hipEventCreate(&evs.ev[0]));
        PCK(hipEventCreate(&evs.ev[1]));
    }
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
                hipLaunchKernelGGL(k_codist, dim3(nt, nt), dim3(256), 0, 0,
                                   p->assign, (long long)S, (long long)N,
                                   p->differ);
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
