"""TEST INFRASTRUCTURE - the dense likelihood arithmetic of the CPU oracle.

This is the array op the HIP kernels replace (SURVEY.md section 8(a) rows
a1-a4, a8): cells x clusters x mutations float64 temporaries, `(1 - theta)`
in theta's own dtype, a log per element and a strictly sequential
NaN-skipping sum over mutations.  Nothing here is optimised - the point of
the oracle is to do what the reference does, the way it does it.
"""
import numpy as np

from .constants import log_EPSILON
from .seqsum import first_nanargmax, seqsum


def crp_log_weight(n_i, n, alpha, dtype=np.float64):
    """log(n_i / (n - 1 + alpha)), libs/CRP.py:83-85."""
    return np.log(n_i, dtype=dtype) - np.log(n - 1 + alpha, dtype=dtype)


def weights_to_probs(log_w):
    """Log-weights -> probabilities with a 1e-15 floor (libs/CRP.py:88-100):
    shift by the first maximum, normalise with log1p over the others."""
    top = first_nanargmax(log_w)
    rest = np.arange(log_w.size) != top
    gap = log_w[rest] - log_w[top]
    try:
        tail = np.exp(gap)
    except FloatingPointError:
        tail = np.exp(np.clip(gap, log_EPSILON, 0))
    log_p = log_w - log_w[top] - np.log1p(seqsum(tail))
    return np.exp(np.clip(log_p, log_EPSILON, 0))


def weights_to_log_probs(log_w):
    """Log-weights -> normalised log-probabilities (libs/CRP.py:103-116); a
    trapped underflow collapses a PAIR to (0, log 1e-15)."""
    top = first_nanargmax(log_w)
    rest = np.arange(log_w.size) != top
    try:
        return log_w - log_w[top] \
            - np.log1p(seqsum(np.exp(log_w[rest] - log_w[top])))
    except FloatingPointError:
        if log_w[0] > log_w[1]:
            return np.array([0, log_EPSILON])
        return np.array([log_EPSILON, 0])


# ---------------------------------------------------------------------------
# The flat total from per-cluster counts, in extended precision.
#   total = sum_{k,m} n1[k,m] * log(t (1 - FN) + o FP)
#                   + n0[k,m] * log(t FN + o (1 - FP))
# with t = float64(theta) and o = float64(float32(1) - theta): the float32
# `1 - theta` is an INPUT here, as it is for the device kernel (k_ll_total).
# Everything after that - the arguments of the logs, the logs, the products
# and the sum - is evaluated with a 64-bit significand or more: NumPy's
# longdouble where it has one (x87), else mpmath at 80 bits, else not at all
# (TOTAL_REFERENCE is None and total_ll_reference raises; tests skip).
# ---------------------------------------------------------------------------
TOTAL_REFERENCE = None
if np.finfo(np.longdouble).nmant >= 63:
    TOTAL_REFERENCE = 'longdouble'
else:                                               # pragma: no cover
    try:
        import mpmath as _mp
        TOTAL_REFERENCE = 'mpmath'
    except ImportError:
        _mp = None

TOTAL_BLOCKS = 256          # k_ll_total: the grid's cap, 256 threads a block
TOTAL_SPAN = TOTAL_BLOCKS * 256
U53 = 2.0 ** -53
# |got - reference| <= U53 * (TOTAL_A * sum(n1 + n0)
#                             + (TOTAL_B + chain) * sum|term|)
# for a float64 evaluation whose log is within 1 ulp: see total_ll_bound
TOTAL_A = 4
TOTAL_B = 5


def _total_inputs(theta, n1, n0):
    theta = np.asarray(theta)
    assert theta.dtype == np.float32
    n1 = np.asarray(n1)
    n0 = np.asarray(n0)
    assert n1.dtype == np.int32 and n0.dtype == np.int32
    assert theta.shape == n1.shape == n0.shape
    t = theta.astype(np.float64).ravel()
    o = (np.float32(1) - theta).astype(np.float64).ravel()
    return t, o, n1.ravel(), n0.ravel()


def total_ll_reference(theta, n1, n0, FP, FN):
    """(total, sum |term|, sum (n1 + n0)) of the flat total for one error
    pair; the total in extended precision (a longdouble or an mpf), the two
    magnitudes as floats (they scale the error bound)."""
    if TOTAL_REFERENCE is None:
        raise RuntimeError('no arithmetic with a 64-bit significand here')
    t, o, c1, c0 = _total_inputs(theta, n1, n0)
    live = np.flatnonzero((c1 | c0) != 0)
    mass = float(c1.sum(dtype=np.int64) + c0.sum(dtype=np.int64))
    if TOTAL_REFERENCE == 'longdouble':
        ld = np.longdouble
        t, o = t[live].astype(ld), o[live].astype(ld)
        fp, fn = ld(float(FP)), ld(float(FN))
        term = c1[live].astype(ld) * np.log(t * (1 - fn) + o * fp) \
            + c0[live].astype(ld) * np.log(t * fn + o * (1 - fp))
        return term.sum(), float(np.abs(term).sum()), mass
    with _mp.workprec(80):                          # pragma: no cover
        fp, fn = _mp.mpf(float(FP)), _mp.mpf(float(FN))
        total, mag = _mp.mpf(0), _mp.mpf(0)
        for i in live:
            ti, oi = _mp.mpf(float(t[i])), _mp.mpf(float(o[i]))
            term = int(c1[i]) * _mp.log(ti * (1 - fn) + oi * fp) \
                + int(c0[i]) * _mp.log(ti * fn + oi * (1 - fp))
            total += term
            mag += abs(term)
        return total, float(mag), mass


def total_ll_distance(got, total):
    """|got - total| as a float, the difference taken in `total`'s precision"""
    if TOTAL_REFERENCE == 'longdouble':
        return float(abs(np.longdouble(got) - total))
    with _mp.workprec(80):                          # pragma: no cover
        return float(abs(_mp.mpf(float(got)) - total))


def total_ll_chain(KM):
    """The longest chain of float64 additions an element's term goes through
    in k_ll_total + bnpc_ll_total_wait: one per trip of its thread's strided
    loop, 8 levels of the block's tree, one per block partial on the host."""
    blocks = max(1, min((KM + 255) // 256, TOTAL_BLOCKS))
    trips = max(1, -(-KM // TOTAL_SPAN))
    return trips + 8 + blocks


def total_ll_bound(KM, mag, mass):
    """What separates a float64 evaluation in the kernel's order from the
    exact total, to first order in u = 2^-53:

      * a log's argument, t * (1 - FN) + o * FP, is a sum of two positive
        products and takes three roundings on its longer side (1 - FN, the
        product, the add): relative error <= 3 u, that is <= 3 u absolute in
        its log;
      * the device log is within 1 ulp, <= 2 u relative to the log;
      * count * log is one rounding, the add of the two products (both
        negative, nothing cancels) another: <= 2 u relative to the term;
      * every term is negative, so the additions it then goes through
        (total_ll_chain of them) cost <= u relative each.

    Per element |error| <= 3 u (n1 + n0) + (2 + 2 + chain) u |term|.  TOTAL_A
    = 3 + 1 and TOTAL_B = 4 + 1: the spare unit on each covers the terms of
    second order and the reference's own rounding (2^-63 per operation, a
    pairwise sum of < 2^20 terms: under 0.02 of a unit)."""
    return U53 * (TOTAL_A * mass + (TOTAL_B + total_ll_chain(KM)) * mag)


def total_ll_kernel_order(theta, n1, n0, FP, FN):
    """The same total in NumPy float64 in k_ll_total's grouping: thread j of
    block b adds elements b * 256 + j, + 65536, ... in order; the block's 256
    sums fold in halves (128, 64, .. 1); the host adds the block partials in
    index order.  Differs from the device only in the log's last bit."""
    t, o, c1, c0 = _total_inputs(theta, n1, n0)
    KM = t.size
    blocks = max(1, min((KM + 255) // 256, TOTAL_BLOCKS))
    span = blocks * 256
    trips = -(-KM // span)
    pad = trips * span - KM
    with np.errstate(all='ignore'):
        term = c1.astype(np.float64) * np.log(t * (1.0 - FN) + o * FP) \
            + c0.astype(np.float64) * np.log(t * FN + o * (1.0 - FP))
    term = np.where((c1 | c0) != 0, term, 0.0)
    term = np.concatenate([term, np.zeros(pad)]).reshape(trips, span)
    acc = np.zeros(span)
    for trip in term:
        acc = acc + trip
    red = acc.reshape(blocks, 256)
    s = 128
    while s:
        red = red[:, :s] + red[:, s:2 * s]
        s >>= 1
    total = 0.0
    for part in red[:, 0]:
        total += part
    return total


class Likelihood:
    """Needs: data, parameters, assignment, cells_per_cluster, CRP_prior,
    FP, FN, _beta_mix_const, DP_a, DP_a_prior, param_prior,
    beta_prior_uniform."""

    log_CRP_prior = staticmethod(crp_log_weight)
    _normalize_log_probs = staticmethod(weights_to_probs)
    _normalize_log = staticmethod(weights_to_log_probs)

    # emission of an observation given the true genotype, libs/CRP.py:207-212
    def _Bernoulli_FN(self, x):
        """genotype 1: observed 1 w.p. 1-FN, observed 0 w.p. FN"""
        return (1 - self.FN) ** x * self.FN ** (1 - x)

    def _Bernoulli_FP(self, x):
        """genotype 0: observed 1 w.p. FP, observed 0 w.p. 1-FP"""
        return (1 - self.FP) ** (1 - x) * self.FP ** x

    def _calc_ll(self, x, theta, flat=False):
        """libs/CRP.py:197-204.  x (r, M) against theta (K, M) or (M,);
        NaN observations drop out of the sum."""
        per_element = np.log(theta * self._Bernoulli_FN(x)
            + (1 - theta) * self._Bernoulli_FP(x))
        return seqsum(per_element) if flat else seqsum(per_element, axis=1)

    def _cluster_sizes(self):
        return np.fromiter(self.cells_per_cluster.values(), dtype=int)

    def _cluster_ids(self):
        return np.fromiter(self.cells_per_cluster.keys(), dtype=int)

    def get_lpost_single(self, cell_id, cl_ids):
        """One cell against the given clusters, + their CRP weights
        (libs/CRP.py:223-227; sizes in dict order)."""
        row = self.data[[cell_id]]
        return self._calc_ll(row, self.parameters[cl_ids]) \
            + self.CRP_prior[self._cluster_sizes()]

    def get_lpost_single_new_cluster(self):
        """Every cell against a not-yet-existing cluster whose profile is
        integrated out under the Beta prior (libs/CRP.py:230-234)."""
        mix0, mix1 = self._beta_mix_const
        wt = mix0 * self._Bernoulli_FP(self.data)
        mut = mix1 * self._Bernoulli_FN(self.data)
        return seqsum(np.log(mut + wt), axis=1) + self.CRP_prior[-1]

    def get_ll_full(self):
        """libs/CRP.py:237-238"""
        return self._calc_ll(self.data, self.parameters[self.assignment],
            flat=True)

    def get_lprior_full(self):
        """libs/CRP.py:241-251"""
        total = self.DP_a_prior.logpdf(self.DP_a) \
            + seqsum(self.CRP_prior[self._cluster_sizes()])
        if not self.beta_prior_uniform:
            live = self.parameters[self._cluster_ids()]
            total += seqsum(self.param_prior.logpdf(live))
        return total
