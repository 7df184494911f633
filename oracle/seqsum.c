/*
 * TEST INFRASTRUCTURE - part of the CPU oracle, never of the product path.
 *
 * Strictly sequential, NaN-skipping float64 sums: the arithmetic of
 * bottleneck.nansum (Bottleneck==1.3.5, requirements.txt:1 of the reference),
 * which the reference uses for every likelihood reduction:
 *   libs/CRP.py:202,204,234 (per-cell / flat log-likelihood sums)
 *   libs/CRP.py:363,366     (per-mutation sums over a cell subset)
 *   libs/CRP_learning_errors.py:63
 * bottleneck is a third-party dependency absent from /root/reference and from
 * the GPU box; its published algorithm for nansum is "asum = 0; for each
 * element in index order: if (ai == ai) asum += ai".  Verified bit-for-bit
 * against bottleneck 1.3.2 through the golden vectors in tests/golden/.
 *
 * Built by oracle/Makefile into oracle/_build/liboracle_seqsum.so.
 */
#include <stddef.h>

double bnpc_oracle_nansum(const double *v, long n)
{
    double s = 0.0;
    for (long i = 0; i < n; i++) {
        double a = v[i];
        if (a == a) s += a;
    }
    return s;
}

/* v is (r, c) C-contiguous; out[i] = sum_j v[i, j] */
void bnpc_oracle_nansum_axis1(const double *v, long r, long c, double *out)
{
    for (long i = 0; i < r; i++) {
        const double *row = v + (size_t)i * c;
        double s = 0.0;
        for (long j = 0; j < c; j++) {
            double a = row[j];
            if (a == a) s += a;
        }
        out[i] = s;
    }
}

/* v is (r, c) C-contiguous; out[j] = sum_i v[i, j], rows added in order */
void bnpc_oracle_nansum_axis0(const double *v, long r, long c, double *out)
{
    for (long j = 0; j < c; j++) out[j] = 0.0;
    for (long i = 0; i < r; i++) {
        const double *row = v + (size_t)i * c;
        for (long j = 0; j < c; j++) {
            double a = row[j];
            if (a == a) out[j] += a;
        }
    }
}

/*
 * Strict-order sums over per-cluster tables (the arithmetic of the NumPy
 * table_sums of tests/test_gpu_parity.py: bottleneck.nansum of each row's
 * elements, in mutation order):
 *   out[i][k] = sum over m, in order, of T1[m][k] where x[i][m] == 1 and
 *               T0[m][k] where x[i][m] == 0; other x (missing) are skipped,
 *               and so are NaN table entries.
 * x is (n, M) C-contiguous; T1 / T0 are the tables TRANSPOSED to (M, K);
 * out is (n, K).  Every out[i][k] has its own accumulator that sees the
 * mutations in order, so the loop over k (innermost, independent entries)
 * may be vectorised without changing a bit.  Adding +0.0 for a NaN entry is
 * the same as skipping it: an accumulator that starts at +0.0 never holds
 * -0.0 (x + (-0.0) == x, and +0.0 + (-0.0) == +0.0).
 */
#define TS_ROWS 8

static void table_row_add(double *restrict o, const double *restrict t, long K)
{
    for (long k = 0; k < K; k++) {
        const double a = t[k];
        o[k] += (a == a) ? a : 0.0;
    }
}

void bnpc_oracle_table_sums(const double *x, long n, long M,
                            const double *T1, const double *T0, long K,
                            double *out)
{
    for (long i = 0; i < n * K; i++) out[i] = 0.0;
    /* blocks of cells: the table rows of one mutation serve TS_ROWS cells */
    for (long i0 = 0; i0 < n; i0 += TS_ROWS) {
        const long i1 = i0 + TS_ROWS < n ? i0 + TS_ROWS : n;
        for (long m = 0; m < M; m++) {
            const double *t1 = T1 + (size_t)m * K, *t0 = T0 + (size_t)m * K;
            for (long i = i0; i < i1; i++) {
                const double v = x[(size_t)i * M + m];
                if (v == 1.0)
                    table_row_add(out + (size_t)i * K, t1, K);
                else if (v == 0.0)
                    table_row_add(out + (size_t)i * K, t0, K);
            }
        }
    }
}
