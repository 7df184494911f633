// bnpc_post_passes.hip - the posterior passes that walk the parameter trace
// or the data behind a bnpc_post handle: the cluster genotypes, and per cell
// or per mutation the genotypes (-pg), the fit (-pf, -pm), the doublet
// scores (-pd), the placement of held-out cells and the ordering of every pair
// of mutations (-po).  The passes over the labels and the pair counts alone are in
// bnpc_codist.hip; the pieces every driver here is made of in bnpc_post.h.
//
// Every kernel here is launched from this file only (k_cg_rank and k_mf_masks
// by several passes).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "bnpc_hip.h"
#include "bnpc_internal.h"
#include "bnpc_post.h"

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
// (GT_MIXED and GT_GLOBAL_WG: bnpc_post.h)
#define GT_LDS_MAX 163840

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
    if (int rc = post_check_handle("genotypes", p)) return rc;
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
    PostBuffers buf;
    unsigned short *d_cl;
    unsigned char *d_flags;
    int *d_rank, *d_distinct;
    PCK(buf.alloc(&d_cl, N));
    PCK(buf.alloc(&d_flags, (size_t)K * S));
    PCK(buf.alloc(&d_rank, (size_t)K * S));
    PCK(buf.alloc(&d_distinct, S));
    PCK(hipMemcpy(d_cl, cl.data(), N * sizeof(unsigned short),
                  hipMemcpyHostToDevice));

    // pass 1 (its LDS limit, and pass 1b's, raised to GT_LDS_MAX)
    {
        PostArea area;
        PCK(post_rank_area((const void *)k_gt_flags, gt_flags_words(N, K),
                           GT_LDS_MAX, S, buf, area));
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
        PostArea area;
        PCK(post_rank_area((const void *)k_gt_hist, gt_hist_words(N),
                           GT_LDS_MAX, S, buf, area));
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

// Every sample's cluster count against the trace's W rows, before a pass adds
// anything up: where k_cg_rank's working set goes (area: LDS up to
// CG_LDS_MAX, no limit to raise), the counts (d_distinct, which stays on the
// device for the kernels that read it) and the check.  0, 1, 2 (a sample has
// more clusters than the trace rows) or 5.  A driver's first allocations:
// the counts, then the global slices if there are any.
static int post_check_distinct(const char *pass, const bnpc_post *p, int64_t W,
                               PostBuffers &buf, PostArea &area,
                               int **d_distinct)
{
    const int64_t S = p->S, N = p->N;
    POST_ALLOC(buf, pass, d_distinct, (size_t)S);
    if (int rc = post_alloc_rc(pass, post_rank_area(nullptr, cg_rank_words(N),
                                                    CG_LDS_MAX, S, buf, area)))
        return rc;
    std::vector<int> distinct(S);
    for (int64_t s0 = 0; s0 < S; s0 += INT_MAX) {
        const int64_t n = std::min<int64_t>(INT_MAX, S - s0);
        hipLaunchKernelGGL(k_cg_rank, dim3(area.grid), dim3(256), area.lds, 0,
                           p->assign, (long long)s0, (int)n, (long long)N, 0LL,
                           0LL, 0LL, area.scratch, area.stride,
                           (unsigned short *)nullptr, *d_distinct + s0);
        PCK(hipGetLastError());
    }
    PCK(hipMemcpy(distinct.data(), *d_distinct, S * sizeof(int),
                  hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < S; s++) {
        if (distinct[s] > W) {
            bnpc_set_error("%s: sample %lld has %d clusters, the trace %lld "
                           "rows", pass, (long long)s, distinct[s],
                           (long long)W);
            return 2;
        }
    }
    return 0;
}

// a chunk's ranks: samples [s0, s0 + n), cells [i0, i0 + cells) into
// d_rank[n][pitch]
static void post_launch_rank(const bnpc_post *p, const PostArea &area,
                             int64_t s0, int64_t n, int64_t i0, int64_t cells,
                             int64_t pitch, unsigned short *d_rank)
{
    hipLaunchKernelGGL(k_cg_rank,
                       dim3((unsigned)std::min<int64_t>(n, area.grid)),
                       dim3(256), area.lds, 0, p->assign, (long long)s0,
                       (int)n, (long long)p->N, (long long)i0,
                       (long long)cells, (long long)pitch, area.scratch,
                       area.stride, d_rank, (int *)nullptr);
}

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
    const char *const pass = "cell genotypes";
    if (int rc = post_check_handle(pass, p)) return rc;
    const int64_t S = p->S, N = p->N;
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    PostLaps laps;
    PostArea area;
    int *d_distinct;
    if (int rc = post_check_distinct(pass, p, W, buf, area, &d_distinct))
        return rc;

    // the chunk of the trace, then as many cells as fit beside it (what is
    // free is asked once the chunk is allocated)
    const size_t sample_floats = (size_t)W * M;
    const int64_t sc = post_default_chunk(chunk,
                                          sample_floats * sizeof(float), S);
    float *d_P;
    POST_ALLOC(buf, pass, &d_P, (size_t)sc * sample_floats);
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
    POST_ALLOC(buf, pass, &d_rank, (size_t)sc * pitch);
    POST_ALLOC(buf, pass, &d_sum1, (size_t)nc * M);
    POST_ALLOC(buf, pass, &d_sum2, (size_t)nc * M);
    POST_ALLOC(buf, pass, &d_ones, (size_t)nc * M);
    // (the padding cells of a row keep rank 0: a row every trace has)
    PCK(hipMemset(d_rank, 0, (size_t)sc * pitch * sizeof(unsigned short)));
    PCK(laps.start(ms, 3));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t cells = std::min(nc, N - i0);
        PCK(hipMemset(d_sum1, 0, (size_t)cells * M * sizeof(double)));
        PCK(hipMemset(d_sum2, 0, (size_t)cells * M * sizeof(double)));
        PCK(hipMemset(d_ones, 0, (size_t)cells * M * sizeof(unsigned)));
        for (int64_t s0 = 0; s0 < S; s0 += sc) {
            const int64_t n = std::min(sc, S - s0);
            laps.begin();
            PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                          (size_t)n * sample_floats * sizeof(float),
                          hipMemcpyHostToDevice));
            laps.end(0);
            laps.begin();
            post_launch_rank(p, area, s0, n, i0, cells, pitch, d_rank);
            PCK(hipGetLastError());
            laps.end(1);
            laps.begin();
            hipLaunchKernelGGL(k_cg_accum,
                               dim3((unsigned)((cells + CG_CELLS - 1) / CG_CELLS),
                                    (unsigned)((M + 255) / 256)),
                               dim3(256), 0, 0, d_P, (int)n, (int)W,
                               (long long)M, d_rank, (long long)pitch,
                               (long long)cells, d_sum1, d_sum2, d_ones);
            PCK(hipGetLastError());
            laps.end(2);
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
    return laps.result(pass);
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
    const char *const pass = "cell fit";
    if (int rc = post_check_handle(pass, p)) return rc;
    const int64_t S = p->S, N = p->N;
    if (int rc = post_check_rates(pass, FN, FP, S)) return rc;
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
    PostBuffers buf;
    PostLaps laps;
    // (the table kernel reads the samples' cluster counts too)
    PostArea area;
    int *d_distinct;
    if (int rc = post_check_distinct(pass, p, W, buf, area, &d_distinct))
        return rc;

    // the chunk of the trace and its two tables (20 bytes per parameter),
    // then as many cells as fit beside them (what is free is asked once
    // these five are allocated)
    const size_t sample_floats = (size_t)W * M;
    const int64_t sc = post_default_chunk(chunk, sample_floats * 20, S);
    float *d_P;
    double *d_L1, *d_L0, *d_FN, *d_FP;
    POST_ALLOC(buf, pass, &d_P, (size_t)sc * sample_floats);
    POST_ALLOC(buf, pass, &d_L1, (size_t)sc * sample_floats);
    POST_ALLOC(buf, pass, &d_L0, (size_t)sc * sample_floats);
    POST_ALLOC(buf, pass, &d_FN, (size_t)S);
    POST_ALLOC(buf, pass, &d_FP, (size_t)S);
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
    POST_ALLOC(buf, pass, &d_rank, (size_t)sc * pitch);
    POST_ALLOC(buf, pass, &d_planes, (size_t)pitch * nwm);
    POST_ALLOC(buf, pass, &d_LL, (size_t)S * pitch);
    POST_ALLOC(buf, pass, &d_out, (size_t)3 * nc);
    // (the padding cells of a row keep rank 0, a row every trace has, and
    // empty planes)
    PCK(hipMemset(d_rank, 0, (size_t)sc * pitch * sizeof(unsigned short)));
    PCK(hipMemset(d_planes, 0, (size_t)pitch * nwm * sizeof(uint2)));
    PCK(hipMemcpy(d_FN, FN, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_FP, FP, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(laps.start(ms, 5));
    const unsigned table_blocks = (unsigned)((W * M + 255) / 256);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t cells = std::min(nc, N - i0);
        const unsigned tiles = (unsigned)((cells + CG_CELLS - 1) / CG_CELLS);
        laps.begin();
        PCK(hipMemcpy(d_planes, planes.data() + (size_t)i0 * nwm,
                      (size_t)cells * nwm * sizeof(uint2),
                      hipMemcpyHostToDevice));
        // (a last, shorter slab: its tile's padding cells are empty too)
        if (cells < pitch)
            PCK(hipMemset(d_planes + (size_t)cells * nwm, 0,
                          (size_t)(pitch - cells) * nwm * sizeof(uint2)));
        laps.end(0);
        for (int64_t s0 = 0; s0 < S; s0 += sc) {
            const int64_t n = std::min(sc, S - s0);
            const unsigned rows = (unsigned)std::min<int64_t>(n, 65535);
            laps.begin();
            PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                          (size_t)n * sample_floats * sizeof(float),
                          hipMemcpyHostToDevice));
            laps.end(0);
            laps.begin();
            post_launch_rank(p, area, s0, n, i0, cells, pitch, d_rank);
            PCK(hipGetLastError());
            laps.end(1);
            laps.begin();
            hipLaunchKernelGGL(k_cf_tables, dim3(table_blocks, rows),
                               dim3(256), 0, 0, d_P, (int)n, (int)W,
                               (long long)M, d_distinct + s0, d_FN + s0,
                               d_FP + s0, d_L1, d_L0);
            PCK(hipGetLastError());
            laps.end(2);
            laps.begin();
            hipLaunchKernelGGL(k_cf_sums, dim3(tiles, rows), dim3(256), 0, 0,
                               d_L1, d_L0, (int)n, (int)W, (long long)M,
                               d_rank, (long long)pitch, (long long)cells,
                               d_planes, (long long)nwm, (long long)s0, d_LL);
            PCK(hipGetLastError());
            laps.end(3);
        }
        laps.begin();
        hipLaunchKernelGGL(k_cf_reduce, dim3((unsigned)((cells + 255) / 256)),
                           dim3(256), 0, 0, d_LL, (long long)S,
                           (long long)pitch, (long long)cells, d_out,
                           d_out + nc, d_out + 2 * nc);
        PCK(hipGetLastError());
        laps.end(4);
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
    return laps.result(pass);
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

// The lane masks of all N cells, in the order of perm (NULL: as they stand),
// a slab of post_mask_slab_cells codes at a time through d_codes: every code
// is looked at before anything is added up.  Each slab's upload and launch is
// a lap of `slot`.  0, 1, or 2 with the first code of a slab that is not 0, 1
// or 3.
static int post_build_masks(const char *pass, const uint8_t *codes,
                            const int *perm, int64_t N, int64_t M, int64_t Mp,
                            uint8_t *d_codes, ulonglong2 *d_masks,
                            unsigned long long *d_bad, PostLaps &laps, int slot)
{
    const int64_t slab_cells = post_mask_slab_cells(N, M);
    std::vector<uint8_t> stage(perm ? (size_t)std::min(slab_cells, N) * M : 0);
    PCK(hipMemset(d_bad, 0xff, sizeof(unsigned long long)));
    for (int64_t j0 = 0; j0 < N; j0 += slab_cells) {
        const int64_t cells = std::min(slab_cells, N - j0);
        for (int64_t j = 0; perm && j < cells; j++)
            memcpy(stage.data() + (size_t)j * M,
                   codes + (size_t)perm[j0 + j] * M, (size_t)M);
        laps.begin();
        PCK(hipMemcpy(d_codes, perm ? stage.data() : codes + (size_t)j0 * M,
                      (size_t)cells * M, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_mf_masks,
                           dim3((unsigned)((Mp + 255) / 256),
                                (unsigned)((cells + 63) / 64)),
                           dim3(256), 0, 0, d_codes, (long long)cells,
                           (long long)M, (long long)Mp,
                           d_masks + (size_t)(j0 / 64) * Mp, d_bad);
        PCK(hipGetLastError());
        laps.end(slot);
        unsigned long long bad = 0;
        PCK(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
        if (bad != ~0ull) {
            const int64_t j = j0 + (int64_t)(bad / (unsigned long long)M);
            const int64_t i = perm ? perm[j] : j;
            const int64_t m = (int64_t)(bad % (unsigned long long)M);
            bnpc_set_error("%s: code %d of cell %lld at mutation %lld is not "
                           "0, 1 or 3", pass, (int)codes[(size_t)i * M + m],
                           (long long)i, (long long)m);
            return 2;
        }
    }
    return 0;
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
    const char *const pass = "mutation fit";
    if (int rc = post_check_handle(pass, p)) return rc;
    const int64_t S = p->S, N = p->N;
    if (int rc = post_check_rates(pass, FN, FP, S)) return rc;
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    PostLaps laps;
    // (the counting kernel reads the samples' cluster counts too)
    PostArea area;
    int *d_distinct;
    if (int rc = post_check_distinct(pass, p, W, buf, area, &d_distinct))
        return rc;

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
    const int64_t sc = post_default_chunk(chunk, per_sample, S);
    const int64_t slab_cells = post_mask_slab_cells(N, M);
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
    POST_ALLOC(buf, pass, &d_masks, (size_t)nb * Mp);
    POST_ALLOC(buf, pass, &d_codes, (size_t)slab_cells * M);
    POST_ALLOC(buf, pass, &d_bad, 1);
    POST_ALLOC(buf, pass, &d_perm, (size_t)N);
    POST_ALLOC(buf, pass, &d_P, (size_t)sc * sample_floats);
    POST_ALLOC(buf, pass, &d_rank, (size_t)sc * N);
    POST_ALLOC(buf, pass, &d_sub, (size_t)6 * sc * M);
    POST_ALLOC(buf, pass, &d_acc, (size_t)7 * M);
    POST_ALLOC(buf, pass, &d_FN, (size_t)S);
    POST_ALLOC(buf, pass, &d_FP, (size_t)S);
    PCK(laps.start(ms, 5));

    PCK(hipMemset(d_acc, 0, (size_t)7 * M * sizeof(double)));
    PCK(hipMemcpy(d_FN, FN, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_FP, FP, S * sizeof(double), hipMemcpyHostToDevice));
    // the lane masks, a slab of sorted cells at a time
    if (int rc = post_build_masks(pass, codes, perm.data(), N, M, Mp, d_codes,
                                  d_masks, d_bad, laps, 0))
        return rc;
    laps.begin();
    PCK(hipMemcpy(d_perm, perm.data(), (size_t)N * sizeof(int),
                  hipMemcpyHostToDevice));
    laps.end(0);

    const unsigned mtiles = (unsigned)(Mp / 64);
    for (int64_t s0 = 0; s0 < S; s0 += sc) {
        const int64_t n = std::min(sc, S - s0);
        laps.begin();
        PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                      (size_t)n * sample_floats * sizeof(float),
                      hipMemcpyHostToDevice));
        laps.end(0);
        laps.begin();
        post_launch_rank(p, area, s0, n, 0, N, N, d_rank);
        PCK(hipGetLastError());
        laps.end(1);
        laps.begin();
        hipLaunchKernelGGL(k_mf_count,
                           dim3(mtiles, (unsigned)std::min<int64_t>(n, 65535)),
                           dim3(64), 0, 0, d_P, (int)n, (int)W, (long long)M,
                           (long long)Mp, d_distinct + s0, d_FN + s0,
                           d_FP + s0, d_rank, d_perm, (long long)N, d_masks,
                           (long long)nb, d_sub);
        PCK(hipGetLastError());
        laps.end(2);
        laps.begin();
        hipLaunchKernelGGL(k_mf_reduce, dim3((unsigned)((M + 255) / 256)),
                           dim3(256), 0, 0, d_sub, (int)n, (long long)M,
                           d_acc);
        PCK(hipGetLastError());
        laps.end(4);
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
    return laps.result(pass);
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

    const char *const pass = "doublets";
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    PostLaps laps;

    // the working set: the lane masks of all cells, a slab of the data while
    // they are built, the genotypes, a chunk's tables, and per resident cell
    // its P scores and seven results
    const int64_t nb = (N + 63) / 64;
    const int64_t Mp = (M + 63) / 64 * 64;
    const int64_t code_cells = post_mask_slab_cells(N, M);
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
    POST_ALLOC(buf, pass, &d_masks, (size_t)nb * Mp);
    POST_ALLOC(buf, pass, &d_codes, (size_t)code_cells * M);
    POST_ALLOC(buf, pass, &d_bad, 1);
    POST_ALLOC(buf, pass, &d_theta, (size_t)K * M);
    POST_ALLOC(buf, pass, &d_T, (size_t)tiles_c * M * (2 * DB_TILE));
    POST_ALLOC(buf, pass, &d_pair, (size_t)slots);
    POST_ALLOC(buf, pass, &d_prior, (size_t)P);
    POST_ALLOC(buf, pass, &d_labels, (size_t)N);
    POST_ALLOC(buf, pass, &d_SC, (size_t)P * pitch);
    POST_ALLOC(buf, pass, &d_res, (size_t)5 * nc);
    POST_ALLOC(buf, pass, &d_bs, (size_t)nc);
    POST_ALLOC(buf, pass, &d_bp, (size_t)nc);
    PCK(laps.start(ms, 4));

    // the lane masks of all cells: every code is looked at before anything
    // is written
    if (int rc = post_build_masks(pass, codes, nullptr, N, M, Mp, d_codes,
                                  d_masks, d_bad, laps, 0))
        return rc;
    laps.begin();
    PCK(hipMemcpy(d_theta, theta, (size_t)K * M * sizeof(double),
                  hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_prior, prior.data(), (size_t)P * sizeof(double),
                  hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_labels, labels, (size_t)N * sizeof(int),
                  hipMemcpyHostToDevice));
    laps.end(0);

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
                laps.begin();
                PCK(hipMemcpy(d_pair, pairs.data(),
                              (size_t)tiles * DB_TILE * sizeof(int2),
                              hipMemcpyHostToDevice));
                laps.end(0);
                laps.begin();
                hipLaunchKernelGGL(k_db_tables,
                                   dim3((unsigned)((M + 255) / 256),
                                        (unsigned)std::min<int64_t>(
                                            tiles * DB_TILE, 65535)),
                                   dim3(256), 0, 0, d_theta, (long long)M,
                                   d_pair, (int)(tiles * DB_TILE), FN, FP, d_T);
                PCK(hipGetLastError());
                laps.end(1);
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
            laps.begin();
            hipLaunchKernelGGL(k_db_sums,
                               dim3((unsigned)tiles,
                                    (unsigned)std::min<int64_t>((nblk + 3) / 4,
                                                                65535)),
                               dim3(256), 0, 0, d_T, (int)n, (long long)M,
                               (long long)Mp, d_masks, (long long)b0,
                               (long long)nblk, (long long)pitch,
                               (long long)c0, d_SC);
            PCK(hipGetLastError());
            laps.end(2);
        }
        laps.begin();
        hipLaunchKernelGGL(k_db_reduce, dim3((unsigned)((cells + 255) / 256)),
                           dim3(256), 0, 0, d_SC, (long long)pitch,
                           (long long)off, (long long)cells, d_labels + i0,
                           (int)K, d_prior, d_res, d_res + nc, d_res + 2 * nc,
                           d_res + 3 * nc, d_res + 4 * nc, d_bs, d_bp);
        PCK(hipGetLastError());
        laps.end(3);
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
    return laps.result(pass);
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
// Placement of held-out cells: the Gibbs conditional of one cell that
// was not part of the run (libs/CRP.py:223-234 with the weights of :84-85 and
// the mixing constants of :42-44), evaluated in every posterior sample and
// averaged.  Per sample s, with D_s its clusters, the candidates of a new cell
// are the sample's rows r < D_s in rank order and then a new cluster.  A row's
// tables are those of k_cf_tables from the float32 trace and the sample's own
// FN[s], FP[s]; the new cluster's are the constants
//   L1 = log(mix1 * (1 - FN[s]) + mix0 * FP[s])
//   L0 = log(mix1 * FN[s] + mix0 * (1 - FP[s]))
// score[s][j][c] is the sum over the mutations, strictly in increasing m from
// 0.0, of L1 where new cell j shows a 1 and L0 where it shows a 0;
// y_c = score_c + log(n_c) for a row of n_c training cells and
// score + log(alpha[s]) for the new cluster; mx = max y_c, e_c = exp(y_c - mx),
// es their sum in candidate order, pr_c = e_c / es.  Per cell, one sample at a
// time in increasing s from 0.0:
//   prob_sum[j][k] += sum over r, in increasing r from 0.0, of
//                     pr_r * (cnt[r][k] / n_r)
//   new_sum[j] += pr_new     ent_sum[j] += log(es) - (sum of e_c (y_c - mx)) / es
//   lp[s][j] = (mx + log(es)) - log(N + alpha[s])
// with cnt[r][k] the training cells of row r that the clustering `labels` puts
// into k, and lpd[j] = mxs + log(sum of exp(lp[s][j] - mxs)) - log(S) over the
// column.  postproc.host_place is the host loop this is pinned to.
//
// Once per call the new cells go up and k_mf_masks turns them into lane masks,
// as for -pd.  Per slab of new cells and chunk of samples:
// k_cg_rank    all N training cells' ranks in the chunk's samples
// k_pn_tables  thread = (candidate of the chunk, mutation): the candidates of
//              all the chunk's samples are one flat list - each sample's D_s
//              rows, then its new cluster - cut into tiles of DB_TILE whatever
//              sample they belong to, in the layout k_db_sums reads
// k_pn_counts  workgroup = sample: cnt[r][k] by integer atomics (any order, the
//              same integers), then per row n_r, log(n_r) and the shares
//              cnt[r][k] / n_r, each divided once; log(alpha[s]) for the new
//              cluster and log(N + alpha[s])
// k_db_sums    as it stands: SCO[candidate of the chunk][cell of the slab],
//              each score bit for bit the sequential sum of the tables
// k_pn_soft    thread = (new cell, sample): the sample's candidates in order
//              - mx, e_c, es, pr_c (the scores' slots are reused for e_c and
//              pr_c), the sample's entropy term and lp, which stays resident
//              (S x slab)
// k_pn_accum   thread = (new cell, accumulator): prob_sum[k], new_sum or
//              ent_sum of the cell, the chunk's samples in increasing s; the
//              accumulators stay on the device between chunks.  (One thread
//              per new cell for all of it left a 5000-cell slab on 79 waves
//              and took five times the sums kernel's time.)
// and after the last chunk
// k_pn_lpd     thread = new cell: its column of lp, the maximum first.
// ---------------------------------------------------------------------------
// cand[c] = (sample of the chunk, row), (sample, -1) its new cluster, (-1, -1)
// a padding slot of the last tile; P the chunk's [.][W][M] trace, FN / FP the
// chunk's rates
__global__ __launch_bounds__(256) void k_pn_tables(
    const float *__restrict__ P, int W, long long M,
    const int2 *__restrict__ cand, int slots, const double *__restrict__ FN,
    const double *__restrict__ FP, double mix1, double mix0,
    double *__restrict__ T)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    for (int c = blockIdx.y; c < slots; c += gridDim.y) {
        const int2 qr = cand[c];
        double l1 = 0.0, l0 = 0.0;
        if (qr.x >= 0) {
            const double fn = FN[qr.x], fp = FP[qr.x];
            double t = mix1, o = mix0;
            if (qr.y >= 0) {
                const float th = P[((size_t)qr.x * W + qr.y) * M + m];
                t = (double)th;
                o = (double)(1.0f - th);
            }
            l1 = log(t * (1.0 - fn) + o * fp);
            l0 = log(t * fn + o * (1.0 - fp));
        }
        double *dst = T + ((size_t)(c / DB_TILE) * M + m) * (2 * DB_TILE)
            + c % DB_TILE;
        dst[0] = l1;
        dst[DB_TILE] = l0;
    }
}

// one chunk of sc samples: rank its [sc][N] rows, labels the N labels in
// [0, K), first[q] the chunk's first candidate of sample q, distinct / alpha
// the chunk's; cnt [candidates][K] zero on entry.  lw[c] the log-weight of
// candidate c, share the [candidates][K] shares of the rows (a new cluster's
// row is not written), lna[q] = log(N + alpha[q])
__global__ __launch_bounds__(256) void k_pn_counts(
    const unsigned short *__restrict__ rank, long long N, int sc,
    const int *__restrict__ labels, int K, const int *__restrict__ first,
    const int *__restrict__ distinct, const double *__restrict__ alpha,
    int *cnt, double *__restrict__ share, double *__restrict__ lw,
    double *__restrict__ lna)
{
    const int tid = threadIdx.x;
    for (int q = blockIdx.x; q < sc; q += gridDim.x) {
        const int base = first[q], D = distinct[q];
        const unsigned short *rk = rank + (size_t)q * N;
        for (long long i = tid; i < N; i += 256)
            atomicAdd(&cnt[(size_t)(base + rk[i]) * K + labels[i]], 1);
        __threadfence();
        __syncthreads();
        for (int r = tid; r < D; r += 256) {
            int *row = cnt + (size_t)(base + r) * K;
            long long n = 0;
            for (int k = 0; k < K; k++)
                n += __hip_atomic_load(row + k, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            const double dn = (double)n;
            lw[base + r] = log(dn);
            double *out = share + (size_t)(base + r) * K;
            for (int k = 0; k < K; k++)
                out[k] = (double)__hip_atomic_load(row + k, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT)
                    / dn;
        }
        if (tid == 0) {
            lw[base + D] = log(alpha[q]);
            lna[q] = log((double)N + alpha[q]);
        }
    }
}

// thread = (new cell i of the slab, sample q of the chunk): the sample's
// candidates in order down the cell's column SCO[.][off + i].  The scores'
// slots are reused: e_c, then pr_c, which k_pn_accum reads.  ET [sc][pp] takes
// the sample's entropy term, LP [S][pp] its log predictive density
__global__ __launch_bounds__(256) void k_pn_soft(
    double *__restrict__ SCO, long long pitch, long long off, long long nc,
    int sc, long long s0, const int *__restrict__ first,
    const int *__restrict__ distinct, const double *__restrict__ lw,
    const double *__restrict__ lna, long long pp, double *__restrict__ ET,
    double *__restrict__ LP)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    for (int q = blockIdx.y; q < sc; q += gridDim.y) {
        const int base = first[q], D = distinct[q];
        double *col = SCO + (size_t)base * pitch + off + i;
        const double *w = lw + base;
        double mx = col[0] + w[0];
        for (int c = 1; c <= D; c++) {
            const double y = col[(size_t)c * pitch] + w[c];
            mx = y > mx ? y : mx;
        }
        double es = 0.0, h = 0.0;
        for (int c = 0; c <= D; c++) {
            const double d = (col[(size_t)c * pitch] + w[c]) - mx;
            const double e = exp(d);
            es += e;
            h += e * d;
            col[(size_t)c * pitch] = e;
        }
        for (int c = 0; c <= D; c++)
            col[(size_t)c * pitch] = col[(size_t)c * pitch] / es;
        const double les = log(es);
        ET[(size_t)q * pp + i] = les - h / es;
        LP[(size_t)(s0 + q) * pp + i] = (mx + les) - lna[q];
    }
}

// thread = (new cell i of the slab, accumulator j): j < K the cell's
// prob_sum[j], j = K its new_sum, j = K + 1 its ent_sum, each one sample at a
// time in increasing q from where the last chunk left it.  SCO holds pr_c
// (k_pn_soft); acc is [K + 2][pp]
__global__ __launch_bounds__(256) void k_pn_accum(
    const double *__restrict__ SCO, long long pitch, long long off,
    long long nc, int sc, const int *__restrict__ first,
    const int *__restrict__ distinct, const double *__restrict__ share, int K,
    const double *__restrict__ ET, long long pp, double *__restrict__ acc)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const int j = (int)blockIdx.y;
    double sum = acc[(size_t)j * pp + i];
    if (j == K + 1) {
        for (int q = 0; q < sc; q++) sum += ET[(size_t)q * pp + i];
    } else if (j == K) {
        for (int q = 0; q < sc; q++)
            sum += SCO[(size_t)(first[q] + distinct[q]) * pitch + off + i];
    } else {
        for (int q = 0; q < sc; q++) {
            const int base = first[q], D = distinct[q];
            const double *col = SCO + (size_t)base * pitch + off + i;
            const double *sh = share + (size_t)base * K + j;
            // (a share of zero adds nothing: the same bits with or without
            // it; the share is the same in every lane)
            double t = 0.0;
            for (int r = 0; r < D; r++) {
                const double f = sh[(size_t)r * K];
                if (f != 0.0) t += col[(size_t)r * pitch] * f;
            }
            sum += t;
        }
    }
    acc[(size_t)j * pp + i] = sum;
}

// new cell i of the slab: its column LP[0 .. S)[i] in increasing s
__global__ __launch_bounds__(256) void k_pn_lpd(
    const double *__restrict__ LP, long long S, long long pp, long long nc,
    double *__restrict__ lpd)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const double *col = LP + i;
    double mx = col[0];
    for (long long s = 1; s < S; s++) {
        const double v = col[(size_t)s * pp];
        mx = v > mx ? v : mx;
    }
    double es = 0.0;
    for (long long s = 0; s < S; s++) es += exp(col[(size_t)s * pp] - mx);
    lpd[i] = (mx + log(es)) - log((double)S);
}

namespace {
struct PnOut {
    double *prob_sum, *new_sum, *ent_sum, *lpd, *lp, *scores;
};
}  // namespace

// ms (NULL, or 6 floats): device-event milliseconds summed over the call -
// ms[0] the uploads and k_mf_masks, ms[1] k_cg_rank, ms[2] k_pn_tables, ms[3]
// k_pn_counts (with its table's zeroing), ms[4] k_db_sums, ms[5] k_pn_soft,
// k_pn_accum and k_pn_lpd
static int pn_run(bnpc_post *p, const uint8_t *codes, int64_t Q, int64_t M,
                  const int32_t *labels, int64_t K, const float *params,
                  int64_t W, const double *FN, const double *FP,
                  const double *alpha, double mix1, double mix0, int64_t chunk,
                  int64_t slab, const PnOut &out, float *ms)
{
    if (!p || !codes || !labels || !params || !FN || !FP || !alpha || Q < 1
        || M < 1 || (M + 255) / 256 > (int64_t)INT_MAX || K < 1
        || K >= (int64_t)GT_MIXED || W < 1 || W >= (int64_t)GT_MIXED || chunk < 0
        || slab < 0 || !(mix1 > 0.0 && mix1 < 1.0 && mix0 > 0.0 && mix0 < 1.0)) {
        bnpc_set_error("bad argument: the placement needs the new cells' "
                       "codes, Q >= 1, M >= 1, N labels, 1 <= K < 65534, a 1 <= W < "
                       "65534 x M trace, FN, FP, alpha, mix1 and mix0 inside "
                       "(0, 1), chunk >= 0 and slab >= 0");
        return 2;
    }
    const char *const pass = "placement";
    if (int rc = post_check_handle(pass, p)) return rc;
    const int64_t S = p->S, N = p->N;
    for (int64_t i = 0; i < N; i++) {
        if (labels[i] < 0 || labels[i] >= K) {
            bnpc_set_error("placement: label %d of cell %lld is not in [0, K = "
                           "%lld)", (int)labels[i], (long long)i, (long long)K);
            return 2;
        }
    }
    if (int rc = post_check_rates(pass, FN, FP, S)) return rc;
    for (int64_t s = 0; s < S; s++) {
        if (!(std::isfinite(alpha[s]) && alpha[s] > 0.0)) {
            bnpc_set_error("placement: alpha = %g of sample %lld is not a "
                           "finite value above 0", alpha[s], (long long)s);
            return 2;
        }
    }
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    PostLaps laps;
    PostArea area;
    int *d_distinct;
    if (int rc = post_check_distinct(pass, p, W, buf, area, &d_distinct))
        return rc;
    std::vector<int> distinct((size_t)S);
    PCK(hipMemcpy(distinct.data(), d_distinct, S * sizeof(int),
                  hipMemcpyDeviceToHost));

    // the new cells' lane masks: every code is looked at before anything is
    // added up
    const int64_t nb = (Q + 63) / 64;
    const int64_t Mp = (M + 63) / 64 * 64;
    ulonglong2 *d_masks;
    uint8_t *d_codes;
    unsigned long long *d_bad;
    POST_ALLOC(buf, pass, &d_masks, (size_t)nb * Mp);
    POST_ALLOC(buf, pass, &d_codes, (size_t)post_mask_slab_cells(Q, M) * M);
    POST_ALLOC(buf, pass, &d_bad, 1);
    PCK(laps.start(ms, 6));
    if (int rc = post_build_masks(pass, codes, nullptr, Q, M, Mp, d_codes,
                                  d_masks, d_bad, laps, 0))
        return rc;

    // the chunk of samples: its trace and, at W + 1 candidates a sample, its
    // tables (a launch's first dimension times its 256 threads stays below
    // 2^32: at most 2^24 candidates), then its true candidates, the most of
    // any chunk
    const size_t sample_floats = (size_t)W * M;
    int64_t sc = post_default_chunk(chunk, sample_floats * sizeof(float)
                                    + (size_t)(W + 1) * M * 16, S);
    sc = std::min<int64_t>(sc, std::max<int64_t>(1, ((int64_t)1 << 24)
                                                  / (W + 1)));
    int64_t cand_max = 0;
    for (int64_t s0 = 0; s0 < S; s0 += sc) {
        int64_t c = 0;
        for (int64_t s = s0; s < std::min(S, s0 + sc); s++)
            c += distinct[s] + 1;
        cand_max = std::max(cand_max, c);
    }
    const int64_t tiles_max = (cand_max + DB_TILE - 1) / DB_TILE;
    const int64_t slots_max = tiles_max * DB_TILE;
    float *d_P;
    double *d_T, *d_FN, *d_FP, *d_alpha, *d_share, *d_lw, *d_lna;
    int2 *d_cand;
    int *d_first, *d_labels, *d_cnt;
    unsigned short *d_rank;
    POST_ALLOC(buf, pass, &d_P, (size_t)sc * sample_floats);
    POST_ALLOC(buf, pass, &d_T, (size_t)tiles_max * M * (2 * DB_TILE));
    POST_ALLOC(buf, pass, &d_FN, (size_t)S);
    POST_ALLOC(buf, pass, &d_FP, (size_t)S);
    POST_ALLOC(buf, pass, &d_alpha, (size_t)S);
    POST_ALLOC(buf, pass, &d_cand, (size_t)slots_max);
    POST_ALLOC(buf, pass, &d_first, (size_t)sc);
    POST_ALLOC(buf, pass, &d_labels, (size_t)N);
    POST_ALLOC(buf, pass, &d_rank, (size_t)sc * N);
    POST_ALLOC(buf, pass, &d_cnt, (size_t)cand_max * K);
    POST_ALLOC(buf, pass, &d_share, (size_t)cand_max * K);
    POST_ALLOC(buf, pass, &d_lw, (size_t)cand_max);
    POST_ALLOC(buf, pass, &d_lna, (size_t)sc);
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    // per resident new cell: its scores of a chunk, its column of lp, a
    // chunk's entropy terms, its K + 2 sums and its lpd (the pitch of nc
    // cells is below nc + 128)
    const size_t per_cell = (size_t)cand_max * 8 + (size_t)S * 8
        + (size_t)sc * 8 + (size_t)K * 8 + 24;
    const size_t margin = (size_t)64 << 20;
    const int64_t fit = (free_b > margin
        ? (int64_t)std::min<size_t>((free_b - margin) / per_cell,
                                    (size_t)1 << 40) : 0) - 128;
    int64_t nc;
    if (slab) {
        nc = std::min(slab, Q);
        if (nc > fit) nc = 0;
    } else {
        nc = std::min(Q, fit);
        if (nc < Q) nc = nc / 64 * 64;          // whole blocks
    }
    if (nc < 1) {
        bnpc_set_error("placement: %lld candidates and %lld samples x 64 new "
                       "cells need %.1f GB, %.1f GB of device memory are free",
                       (long long)cand_max, (long long)S,
                       (margin + 192.0 * per_cell) / 1e9, free_b / 1e9);
        return 5;
    }
    // (an unaligned slab of nc cells touches (nc + 62) / 64 + 1 blocks)
    const int64_t nblk_max = nc >= Q ? nb : (nc + 62) / 64 + 1;
    const int64_t pitch = nblk_max * 64;
    // d_acc: [K + 2][nc] - prob_sum by cluster, new_sum, ent_sum - then lpd
    double *d_SC, *d_acc, *d_ET, *d_LP;
    POST_ALLOC(buf, pass, &d_SC, (size_t)cand_max * pitch);
    POST_ALLOC(buf, pass, &d_acc, (size_t)(K + 3) * nc);
    POST_ALLOC(buf, pass, &d_ET, (size_t)sc * nc);
    POST_ALLOC(buf, pass, &d_LP, (size_t)S * nc);
    double *const d_lpd = d_acc + (size_t)(K + 2) * nc;
    laps.begin();
    PCK(hipMemcpy(d_FN, FN, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_FP, FP, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_alpha, alpha, S * sizeof(double), hipMemcpyHostToDevice));
    PCK(hipMemcpy(d_labels, labels, (size_t)N * sizeof(int),
                  hipMemcpyHostToDevice));
    laps.end(0);
    if (out.scores) {
        const size_t count = (size_t)S * Q * (W + 1);
        for (size_t at = 0; at < count; at++) out.scores[at] = NAN;
    }

    std::vector<int2> cand((size_t)slots_max);
    std::vector<int> first((size_t)sc);
    std::vector<double> stage;
    const bool one_chunk = sc >= S;
    for (int64_t i0 = 0; i0 < Q; i0 += nc) {
        const int64_t cells = std::min(nc, Q - i0);
        const int64_t b0 = i0 / 64, off = i0 - b0 * 64;
        const int64_t nblk = (i0 + cells - 1) / 64 - b0 + 1;
        PCK(hipMemset(d_acc, 0, (size_t)(K + 2) * nc * sizeof(double)));
        for (int64_t s0 = 0; s0 < S; s0 += sc) {
            const int64_t n = std::min(sc, S - s0);
            // the chunk's flat list of candidates
            int64_t cn = 0;
            for (int64_t q = 0; q < n; q++) {
                first[q] = (int)cn;
                for (int r = 0; r < distinct[s0 + q]; r++)
                    cand[cn++] = make_int2((int)q, r);
                cand[cn++] = make_int2((int)q, -1);
            }
            const int64_t tiles = (cn + DB_TILE - 1) / DB_TILE;
            for (int64_t c = cn; c < tiles * DB_TILE; c++)
                cand[c] = make_int2(-1, -1);
            if (!one_chunk || i0 == 0) {
                laps.begin();
                PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                              (size_t)n * sample_floats * sizeof(float),
                              hipMemcpyHostToDevice));
                PCK(hipMemcpy(d_cand, cand.data(),
                              (size_t)tiles * DB_TILE * sizeof(int2),
                              hipMemcpyHostToDevice));
                PCK(hipMemcpy(d_first, first.data(), (size_t)n * sizeof(int),
                              hipMemcpyHostToDevice));
                laps.end(0);
                laps.begin();
                post_launch_rank(p, area, s0, n, 0, N, N, d_rank);
                PCK(hipGetLastError());
                laps.end(1);
                laps.begin();
                hipLaunchKernelGGL(k_pn_tables,
                                   dim3((unsigned)((M + 255) / 256),
                                        (unsigned)std::min<int64_t>(
                                            tiles * DB_TILE, 65535)),
                                   dim3(256), 0, 0, d_P, (int)W, (long long)M,
                                   d_cand, (int)(tiles * DB_TILE), d_FN + s0,
                                   d_FP + s0, mix1, mix0, d_T);
                PCK(hipGetLastError());
                laps.end(2);
                laps.begin();
                PCK(hipMemset(d_cnt, 0, (size_t)cn * K * sizeof(int)));
                hipLaunchKernelGGL(k_pn_counts,
                                   dim3((unsigned)std::min<int64_t>(n, 65535)),
                                   dim3(256), 0, 0, d_rank, (long long)N,
                                   (int)n, d_labels, (int)K, d_first,
                                   d_distinct + s0, d_alpha + s0, d_cnt,
                                   d_share, d_lw, d_lna);
                PCK(hipGetLastError());
                laps.end(3);
            }
            laps.begin();
            hipLaunchKernelGGL(k_db_sums,
                               dim3((unsigned)tiles,
                                    (unsigned)std::min<int64_t>((nblk + 3) / 4,
                                                                65535)),
                               dim3(256), 0, 0, d_T, (int)cn, (long long)M,
                               (long long)Mp, d_masks, (long long)b0,
                               (long long)nblk, (long long)pitch, 0LL, d_SC);
            PCK(hipGetLastError());
            laps.end(4);
            if (out.scores) {
                // SCO is [candidate][cell]: through the host, turned
                stage.resize((size_t)cn * cells);
                PCK(hipMemcpy2D(stage.data(), (size_t)cells * sizeof(double),
                                d_SC + off, (size_t)pitch * sizeof(double),
                                (size_t)cells * sizeof(double), (size_t)cn,
                                hipMemcpyDeviceToHost));
                for (int64_t q = 0; q < n; q++) {
                    const int D = distinct[s0 + q];
                    for (int r = 0; r <= D; r++) {
                        const double *src = stage.data()
                            + (size_t)(first[q] + r) * cells;
                        const int64_t slot = r < D ? r : W;
                        for (int64_t i = 0; i < cells; i++)
                            out.scores[((size_t)(s0 + q) * Q + i0 + i)
                                       * (W + 1) + slot] = src[i];
                    }
                }
            }
            laps.begin();
            hipLaunchKernelGGL(k_pn_soft,
                               dim3((unsigned)((cells + 255) / 256),
                                    (unsigned)std::min<int64_t>(n, 65535)),
                               dim3(256), 0, 0, d_SC, (long long)pitch,
                               (long long)off, (long long)cells, (int)n,
                               (long long)s0, d_first, d_distinct + s0, d_lw,
                               d_lna, (long long)nc, d_ET, d_LP);
            PCK(hipGetLastError());
            hipLaunchKernelGGL(k_pn_accum,
                               dim3((unsigned)((cells + 255) / 256),
                                    (unsigned)(K + 2)),
                               dim3(256), 0, 0, d_SC, (long long)pitch,
                               (long long)off, (long long)cells, (int)n,
                               d_first, d_distinct + s0, d_share, (int)K, d_ET,
                               (long long)nc, d_acc);
            PCK(hipGetLastError());
            laps.end(5);
        }
        laps.begin();
        hipLaunchKernelGGL(k_pn_lpd, dim3((unsigned)((cells + 255) / 256)),
                           dim3(256), 0, 0, d_LP, (long long)S, (long long)nc,
                           (long long)cells, d_lpd);
        PCK(hipGetLastError());
        laps.end(5);
        double *host[3] = {out.new_sum, out.ent_sum, out.lpd};
        for (int k = 0; k < 3; k++)
            if (host[k])
                PCK(hipMemcpy(host[k] + i0, d_acc + (size_t)(K + k) * nc,
                              cells * sizeof(double), hipMemcpyDeviceToHost));
        if (out.lp)
            PCK(hipMemcpy2D(out.lp + i0, (size_t)Q * sizeof(double), d_LP,
                            (size_t)nc * sizeof(double),
                            (size_t)cells * sizeof(double), (size_t)S,
                            hipMemcpyDeviceToHost));
        if (out.prob_sum) {
            // prob is [cluster][cell]: through the host, turned
            stage.resize((size_t)K * cells);
            PCK(hipMemcpy2D(stage.data(), (size_t)cells * sizeof(double),
                            d_acc, (size_t)nc * sizeof(double),
                            (size_t)cells * sizeof(double), (size_t)K,
                            hipMemcpyDeviceToHost));
            for (int64_t k = 0; k < K; k++)
                for (int64_t i = 0; i < cells; i++)
                    out.prob_sum[(size_t)(i0 + i) * K + k]
                        = stage[(size_t)k * cells + i];
        }
    }
    PCK(hipDeviceSynchronize());
    return laps.result(pass);
}

extern "C" int bnpc_post_place(bnpc_post *p, const uint8_t *codes, int64_t Q,
                               int64_t M, const int32_t *labels, int64_t K,
                               const float *params, int64_t W,
                               const double *FN, const double *FP,
                               const double *alpha, double mix1, double mix0,
                               int64_t chunk, int64_t slab, double *prob_sum,
                               double *new_sum, double *ent_sum, double *lpd,
                               double *lp, double *scores)
{
    const PnOut out = {prob_sum, new_sum, ent_sum, lpd, lp, scores};
    return pn_run(p, codes, Q, M, labels, K, params, W, FN, FP, alpha, mix1,
                  mix0, chunk, slab, out, nullptr);
}

// diagnostic (tools/posterior_bench.py): one bnpc_post_place call without its
// results' way back, by device events (see pn_run)
extern "C" int bnpc_post_place_times(bnpc_post *p, const uint8_t *codes,
                                     int64_t Q, int64_t M,
                                     const int32_t *labels, int64_t K,
                                     const float *params, int64_t W,
                                     const double *FN, const double *FP,
                                     const double *alpha, double mix1,
                                     double mix0, int64_t chunk, int64_t slab,
                                     float *ms)
{
    if (!ms) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    const PnOut out = {};
    return pn_run(p, codes, Q, M, labels, K, params, W, FN, FP, alpha, mix1,
                  mix0, chunk, slab, out, ms);
}

// ---------------------------------------------------------------------------
// Posterior ordering of every pair of mutations (-po): in every sample each
// live cluster (a row r < D_s whose label has min_cells cells or more) has a
// called genotype, P[s][r][m] > 0.5f, so mutation m is a set A_m of live rows
// and two mutations stand in one relation under the three-gamete rule - from
//   x11 = A_a and A_b meet, x10 = A_a \ A_b not empty, x01 = A_b \ A_a not empty
// same (x11 only), a ancestral to b (x11, x10), b ancestral to a (x11, x01),
// exclusive (x10, x01), conflict (all three), else absent.  anc, same, excl,
// conf count the samples per ordered pair, uint32 M x M;
// postproc.host_mutation_order is the host loop this is pinned to.
//
// Per slab of table rows a and chunk of samples:
// k_cg_rank    all N cells' ranks in the chunk's samples
// k_po_live    workgroup = sample: the sizes of its rows by integer atomics
//              (LDS up to PO_LDS_ROWS rows, past that a global slice per
//              workgroup), then the live rows as ceil(W / 64) 64-bit words
// k_po_masks   thread = mutation, a launch row per (sample, word): the bits of
//              the word's live rows r < D_s with P > 0.5f.  masks[sample]
//              [word][M]: the lanes run along the mutations for the trace's
//              loads, the mask's store and the pair kernel's loads alike
// k_po_pairs   workgroup = tile of PO_TILE x PO_TILE pairs, thread = PO_BLOCK
//              a x PO_BLOCK b of them with their counters in registers over
//              the whole chunk.  PO_STAGE mask rows of the tile's a and b side
//              go through LDS at a time (16 KiB); a thread reads its a masks
//              as 16-byte pieces (the same address in 16 lanes) and its b
//              masks at stride 16, so that the lanes of an 8-byte read lie
//              side by side.  The three any-bits come from and / and-not of
//              the words; the five counters take sums of their products - no
//              branch.  With one word a sample (W <= 64) a mask row is a
//              sample; with more the any-bits of the words met so far are
//              kept packed per pair until the sample's last word.  Where the
//              slab holds all M rows only the tiles on and above the diagonal
//              run, and a tile writes anc[b][a] (its fifth counter) and the
//              mirrored same, excl, conf as well.  The tables are read at the
//              kernel's start and written at its end: no atomics.
// ---------------------------------------------------------------------------
#define PO_TILE 64                  // mutations along a side of a tile
#define PO_BLOCK 4                  // a thread's pairs: PO_BLOCK a x PO_BLOCK b
#define PO_STAGE 16                 // mask rows of a tile side in LDS at a time
#define PO_LDS_ROWS 8192            // rows whose sizes k_po_live keeps in LDS
#define PO_WG 1024                  // workgroups of k_po_live, launch rows of k_po_masks

// one chunk of sc samples: rank its [sc][N] rows; live [sc][ww]
template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_po_live(
    const unsigned short *__restrict__ rank, long long N, int sc, int W,
    int ww, long long min_cells, int *gsizes,
    unsigned long long *__restrict__ live)
{
    extern __shared__ int po_sizes[];
    int *sizes = GLOBAL ? gsizes + (size_t)blockIdx.x * W : po_sizes;
    const int tid = threadIdx.x;
    for (int q = blockIdx.x; q < sc; q += gridDim.x) {
        for (int r = tid; r < W; r += 256) {
            if (GLOBAL)
                __hip_atomic_store(sizes + r, 0, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            else
                sizes[r] = 0;
        }
        if (GLOBAL) __threadfence();
        __syncthreads();
        const unsigned short *rk = rank + (size_t)q * N;
        for (long long i = tid; i < N; i += 256) atomicAdd(&sizes[rk[i]], 1);
        if (GLOBAL) __threadfence();
        __syncthreads();
        for (int w = tid; w < ww; w += 256) {
            const int r0 = w * 64, r1 = min(W, r0 + 64);
            unsigned long long bits = 0;
            for (int r = r0; r < r1; r++) {
                const int n = GLOBAL
                    ? __hip_atomic_load(sizes + r, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT)
                    : sizes[r];
                bits |= (unsigned long long)((long long)n >= min_cells)
                    << (r - r0);
            }
            live[(size_t)q * ww + w] = bits;
        }
        __syncthreads();                    // the sizes are reused
    }
}

// one chunk of sc samples: P its [sc][W][M] trace, distinct / live the
// chunk's; masks [sc * ww][M]
__global__ __launch_bounds__(256) void k_po_masks(
    const float *__restrict__ P, int sc, int W, int ww, long long M,
    const int *__restrict__ distinct,
    const unsigned long long *__restrict__ live,
    unsigned long long *__restrict__ masks)
{
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const long long units = (long long)sc * ww;
    for (long long u = blockIdx.y; u < units; u += gridDim.y) {
        const int q = (int)(u / ww), w = (int)(u - (long long)q * ww);
        const int r0 = w * 64, r1 = min(distinct[q], r0 + 64);
        const unsigned long long lv = live[u];
        const float *col = P + ((size_t)q * W + r0) * M + m;
        unsigned long long bits = 0;
        // (the word's live bits are the same in every lane)
        for (int r = r0; r < r1; r++, col += M)
            if ((lv >> (r - r0)) & 1)
                bits |= (unsigned long long)(*col > 0.5f) << (r - r0);
        masks[(size_t)u * M + m] = bits;
    }
}

// masks: `units` rows of M, ww of them a sample (ONE: ww == 1).  The tables
// are the slab's [na][M], its rows the mutations a0 .. a0 + na; SYM: a0 == 0,
// na == M, and the tiles below the diagonal leave at once
template <bool ONE, bool SYM>
__global__ __launch_bounds__(256) void k_po_pairs(
    const unsigned long long *__restrict__ masks, long long units, int ww,
    long long M, long long a0, long long na, unsigned *anc, unsigned *same,
    unsigned *excl, unsigned *conf)
{
    __shared__ __attribute__((aligned(16)))
        unsigned long long sa[PO_STAGE][PO_TILE];
    __shared__ __attribute__((aligned(16)))
        unsigned long long sb[PO_STAGE][PO_TILE];
    if (SYM && blockIdx.x < blockIdx.y) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long at = a0 + (long long)blockIdx.y * PO_TILE;
    const long long bt = (long long)blockIdx.x * PO_TILE;
    const long long a_end = a0 + na;
    unsigned c_anc[PO_BLOCK][PO_BLOCK], c_desc[PO_BLOCK][PO_BLOCK],
        c_same[PO_BLOCK][PO_BLOCK], c_excl[PO_BLOCK][PO_BLOCK],
        c_conf[PO_BLOCK][PO_BLOCK], any[PO_BLOCK][PO_BLOCK];
#pragma unroll
    for (int i = 0; i < PO_BLOCK; i++) {
#pragma unroll
        for (int j = 0; j < PO_BLOCK; j++) {
            const long long a = at + ty * PO_BLOCK + i, b = bt + tx + 16 * j;
            const bool in = a < a_end && b < M;
            const size_t idx = in ? (size_t)(a - a0) * M + b : 0;
            c_anc[i][j] = in ? anc[idx] : 0u;
            c_same[i][j] = in ? same[idx] : 0u;
            c_excl[i][j] = in ? excl[idx] : 0u;
            c_conf[i][j] = in ? conf[idx] : 0u;
            c_desc[i][j] = SYM && in ? anc[(size_t)b * M + a] : 0u;
            any[i][j] = 0u;
        }
    }
    int w = 0;
    for (long long u0 = 0; u0 < units; u0 += PO_STAGE) {
        const int nu = (int)min((long long)PO_STAGE, units - u0);
        __syncthreads();                    // the last rows have been read
        for (int e = tid; e < nu * PO_TILE; e += 256) {
            const int k = e >> 6, c = e & 63;
            const unsigned long long *row = masks + (size_t)(u0 + k) * M;
            sa[k][c] = at + c < M ? row[at + c] : 0ull;
            sb[k][c] = bt + c < M ? row[bt + c] : 0ull;
        }
        __syncthreads();
        for (int k = 0; k < nu; k++) {
            unsigned long long va[PO_BLOCK], vb[PO_BLOCK];
            const ulonglong2 *pa = (const ulonglong2 *)&sa[k][ty * PO_BLOCK];
#pragma unroll
            for (int i = 0; i < PO_BLOCK; i += 2) {
                const ulonglong2 t = pa[i >> 1];
                va[i] = t.x;
                va[i + 1] = t.y;
            }
#pragma unroll
            for (int j = 0; j < PO_BLOCK; j++) vb[j] = sb[k][tx + 16 * j];
            const bool last = ONE || w == ww - 1;   // (the same in every lane)
#pragma unroll
            for (int i = 0; i < PO_BLOCK; i++) {
#pragma unroll
                for (int j = 0; j < PO_BLOCK; j++) {
                    unsigned x11 = (va[i] & vb[j]) != 0ull;
                    unsigned x10 = (va[i] & ~vb[j]) != 0ull;
                    unsigned x01 = (vb[j] & ~va[i]) != 0ull;
                    if (!ONE) {
                        any[i][j] |= x11 | (x10 << 1) | (x01 << 2);
                        if (!last) continue;
                        x11 = any[i][j] & 1u;
                        x10 = (any[i][j] >> 1) & 1u;
                        x01 = any[i][j] >> 2;
                        any[i][j] = 0u;
                    }
                    const unsigned both = x11 & x10, only = x11 & (x10 ^ 1u);
                    const unsigned n01 = x01 ^ 1u;
                    c_conf[i][j] += both & x01;
                    c_anc[i][j] += both & n01;
                    c_desc[i][j] += only & x01;
                    c_same[i][j] += only & n01;
                    c_excl[i][j] += (x11 ^ 1u) & x10 & x01;
                }
            }
            if (!ONE) w = w + 1 == ww ? 0 : w + 1;
        }
    }
    const bool mirror = SYM && blockIdx.x != blockIdx.y;
#pragma unroll
    for (int i = 0; i < PO_BLOCK; i++) {
#pragma unroll
        for (int j = 0; j < PO_BLOCK; j++) {
            const long long a = at + ty * PO_BLOCK + i, b = bt + tx + 16 * j;
            if (a >= a_end || b >= M) continue;
            const size_t idx = (size_t)(a - a0) * M + b;
            anc[idx] = c_anc[i][j];
            same[idx] = c_same[i][j];
            excl[idx] = c_excl[i][j];
            conf[idx] = c_conf[i][j];
            if (mirror) {
                const size_t back = (size_t)b * M + a;
                anc[back] = c_desc[i][j];
                same[back] = c_same[i][j];
                excl[back] = c_excl[i][j];
                conf[back] = c_conf[i][j];
            }
        }
    }
}

// ms (NULL, or 4 floats): device-event milliseconds summed over the call -
// ms[0] the trace uploads, ms[1] k_cg_rank and k_po_live, ms[2] k_po_masks,
// ms[3] k_po_pairs (with its tables' zeroing)
static int po_run(bnpc_post *p, const float *params, int64_t W, int64_t M,
                  int64_t min_cells, int64_t chunk, int64_t slab,
                  uint32_t *anc, uint32_t *same, uint32_t *excl,
                  uint32_t *conf, float *ms)
{
    if (!p || !params || min_cells < 1 || W < 1 || W >= (int64_t)GT_MIXED
        || M < 1 || M > (int64_t)65535 * PO_TILE || chunk < 0 || slab < 0) {
        bnpc_set_error("bad argument: the mutation order needs min_cells >= 1, "
                       "a 1 <= W < 65534 x 1 <= M <= 65535 * 64 trace, chunk "
                       ">= 0 and slab >= 0");
        return 2;
    }
    const char *const pass = "mutation order";
    if (int rc = post_check_handle(pass, p)) return rc;
    const int64_t S = p->S, N = p->N;
    PCK(hipSetDevice(p->device));
    PostBuffers buf;
    PostLaps laps;
    PostArea area;
    int *d_distinct;
    if (int rc = post_check_distinct(pass, p, W, buf, area, &d_distinct))
        return rc;

    // the chunk of samples: its trace, its masks, its ranks and live rows (a
    // launch counts its mask rows as an int), then as many table rows as fit
    // beside it
    const int64_t ww = (W + 63) / 64;
    const size_t sample_floats = (size_t)W * M;
    int64_t sc = post_default_chunk(chunk, sample_floats * sizeof(float)
                                    + (size_t)ww * M * 8 + (size_t)N * 2
                                    + (size_t)ww * 8, S);
    sc = std::min<int64_t>(sc, std::max<int64_t>(1, ((int64_t)1 << 30) / ww));
    const bool in_lds = W <= PO_LDS_ROWS;
    const unsigned live_grid = (unsigned)std::min<int64_t>(sc, PO_WG);
    float *d_P;
    unsigned short *d_rank;
    unsigned long long *d_live, *d_masks;
    int *d_sizes = nullptr;
    POST_ALLOC(buf, pass, &d_P, (size_t)sc * sample_floats);
    POST_ALLOC(buf, pass, &d_rank, (size_t)sc * N);
    POST_ALLOC(buf, pass, &d_live, (size_t)sc * ww);
    POST_ALLOC(buf, pass, &d_masks, (size_t)sc * ww * M);
    if (!in_lds) POST_ALLOC(buf, pass, &d_sizes, (size_t)live_grid * W);
    size_t free_b = 0, total_b = 0;
    PCK(hipMemGetInfo(&free_b, &total_b));
    const size_t per_row = (size_t)M * 16;
    const size_t margin = (size_t)64 << 20;
    const size_t room = free_b > margin ? (free_b - margin) / per_row : 0;
    const int64_t na = slab ? std::min(slab, M)
                            : (int64_t)std::min<size_t>((size_t)M, room);
    if (na < 1 || (size_t)na > room) {
        bnpc_set_error("mutation order: a slab of %lld x %lld pairs needs "
                       "%.1f GB, %.1f GB of device memory are free",
                       (long long)std::max<int64_t>(na, 1), (long long)M,
                       (double)std::max<int64_t>(na, 1) * per_row / 1e9,
                       free_b / 1e9);
        return 5;
    }
    unsigned *d_tab[4];
    uint32_t *const host[4] = {anc, same, excl, conf};
    for (int t = 0; t < 4; t++)
        POST_ALLOC(buf, pass, &d_tab[t], (size_t)na * M);
    PCK(laps.start(ms, 4));
    const bool sym = na >= M, one = ww == 1, one_chunk = sc >= S;
    const unsigned tiles_b = (unsigned)((M + PO_TILE - 1) / PO_TILE);
    for (int64_t a0 = 0; a0 < M; a0 += na) {
        const int64_t rows = std::min(na, M - a0);
        laps.begin();
        for (int t = 0; t < 4; t++)
            PCK(hipMemset(d_tab[t], 0, (size_t)rows * M * sizeof(unsigned)));
        laps.end(3);
        for (int64_t s0 = 0; s0 < S; s0 += sc) {
            const int64_t n = std::min(sc, S - s0);
            const int64_t units = n * ww;
            if (!one_chunk || a0 == 0) {
                laps.begin();
                PCK(hipMemcpy(d_P, params + (size_t)s0 * sample_floats,
                              (size_t)n * sample_floats * sizeof(float),
                              hipMemcpyHostToDevice));
                laps.end(0);
                laps.begin();
                post_launch_rank(p, area, s0, n, 0, N, N, d_rank);
                PCK(hipGetLastError());
                const dim3 lg((unsigned)std::min<int64_t>(n, live_grid));
                if (in_lds)
                    hipLaunchKernelGGL(k_po_live<false>, lg, dim3(256),
                                       (size_t)W * sizeof(int), 0, d_rank,
                                       (long long)N, (int)n, (int)W, (int)ww,
                                       (long long)min_cells, (int *)nullptr,
                                       d_live);
                else
                    hipLaunchKernelGGL(k_po_live<true>, lg, dim3(256), 0, 0,
                                       d_rank, (long long)N, (int)n, (int)W,
                                       (int)ww, (long long)min_cells, d_sizes,
                                       d_live);
                PCK(hipGetLastError());
                laps.end(1);
                laps.begin();
                hipLaunchKernelGGL(k_po_masks,
                                   dim3((unsigned)((M + 255) / 256),
                                        (unsigned)std::min<int64_t>(units,
                                                                    PO_WG)),
                                   dim3(256), 0, 0, d_P, (int)n, (int)W,
                                   (int)ww, (long long)M, d_distinct + s0,
                                   d_live, d_masks);
                PCK(hipGetLastError());
                laps.end(2);
            }
            laps.begin();
            const dim3 grid(tiles_b,
                            (unsigned)((rows + PO_TILE - 1) / PO_TILE));
#define PO_LAUNCH(ONE_, SYM_)                                                \
            hipLaunchKernelGGL((k_po_pairs<ONE_, SYM_>), grid, dim3(256), 0,  \
                               0, d_masks, (long long)units, (int)ww,        \
                               (long long)M, (long long)a0, (long long)rows, \
                               d_tab[0], d_tab[1], d_tab[2], d_tab[3])
            if (one && sym) PO_LAUNCH(true, true);
            else if (one) PO_LAUNCH(true, false);
            else if (sym) PO_LAUNCH(false, true);
            else PO_LAUNCH(false, false);
#undef PO_LAUNCH
            PCK(hipGetLastError());
            laps.end(3);
        }
        for (int t = 0; t < 4; t++)
            if (host[t])
                PCK(hipMemcpy(host[t] + (size_t)a0 * M, d_tab[t],
                              (size_t)rows * M * sizeof(unsigned),
                              hipMemcpyDeviceToHost));
    }
    PCK(hipDeviceSynchronize());
    return laps.result(pass);
}

extern "C" int bnpc_post_mutation_order(bnpc_post *p, const float *params,
                                        int64_t W, int64_t M,
                                        int64_t min_cells, int64_t chunk,
                                        int64_t slab, uint32_t *anc,
                                        uint32_t *same, uint32_t *excl,
                                        uint32_t *conf)
{
    return po_run(p, params, W, M, min_cells, chunk, slab, anc, same, excl,
                  conf, nullptr);
}

// diagnostic (tools/posterior_bench.py): one bnpc_post_mutation_order call
// without its tables' way back, by device events (see po_run)
extern "C" int bnpc_post_mutation_order_times(bnpc_post *p,
                                              const float *params, int64_t W,
                                              int64_t M, int64_t min_cells,
                                              int64_t chunk, int64_t slab,
                                              float *ms)
{
    if (!ms) {
        bnpc_set_error("bad argument: NULL");
        return 2;
    }
    return po_run(p, params, W, M, min_cells, chunk, slab, nullptr, nullptr,
                  nullptr, nullptr, ms);
}
