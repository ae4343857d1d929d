"""Plain Python restatement of the tie expectation -- shared by tests/test_tie_expected_cpu.py and
tests/test_tie_expected_gpu.py; not a test itself.

For one query, bucket d (ascending Hamming distance) holds n_d gallery rows of which r_d are relevant.  A tie order ascends in distance;
every bucket is independently and uniformly permuted.  `expected_one` gives E[AP@R], E[hits@k] and E[R@k] in closed form, in one of two
number systems:

* `EXACT`: `fractions.Fraction` throughout, hypergeometric weights from binomials -- what `brute_force` (every tie order of a tiny
  problem, equal weight per distinct relevance pattern) must equal AS FRACTIONS;
* `FIXED`: Python integers in fixed point, 256 fractional bits, for problems whose counts make Fractions slow or binomials
  impossible (2^31 rows in a bucket): L is a sum of floor(2^256 / (B + i)), a quotient by an integer is a floor division (each loses
  < 2^-256), and the weights are the ratio recurrence from the mode in integers, w <- w * num // den with the mode's weight 2^256, over
  the whole feasible range or until a weight reaches 0 (then it is < 2^-256 of the mode's, the pmf is log-concave, and everything
  beyond it is smaller still).  Far more than 100 bits; nothing takes `comb` of a large argument.

`expected_float64` is the same closed form in Python floats, written the way csrc/hamming_tie_expected.hip computes it (positive-term
sums for L and M, weights from the mode with the proven early stop); the CPU tests hold it to `error_bound`, like the kernel.

The error bound (`error_bound`, `hits_bound`)
---------------------------------------------
u = 2^-53, gamma(k) = k u / (1 - k u): a result that went through at most k roundings, each a factor (1 + delta), |delta| <= u, is
off by a relative gamma(k) at most; a sum of POSITIVE terms inherits the largest relative error of its terms plus one rounding per
addition.  The kernel compiles without contraction, so its roundings are the operations of its source:

* L(B, m) = sum 1 / (B + i): B + i < 2^53 is exact, a term is one division, lane j adds its c = ceil(m / 64) terms (c - 1 additions), the
  butterfly adds 6 times: relative gamma(c + 6).  M(B, m) = sum (i - 1) / (B + i) is summed as written, term = (i - 1) * (1 / (B + i)),
  two roundings: gamma(c + 7).  M replaces m - (B + 1) L, whose absolute error would be (B + 1) times that of L: no cancellation is left.
* T = (h / m) ((K + 1) L + ((h - 1) / (m - 1)) M): five more roundings on positive parts: gamma(c + 12).
* S = sum of T over D buckets: gamma(C + 12 + D), C the largest c.  A limit that cuts no bucket: AP = S / K <= 1, absolute
  gamma(C + D + 13).
* The cut bucket: v_h = (S + T_h) / (K + h) <= 1, gamma(C + D + 14).  A weight at distance j from the mode is a product of j ratios
  (two integer products and a division each: 3 roundings) joined by at most j + j / 64 + 1 multiplications: gamma(5 j + 2), j <= J =
  tmax - tmin, the feasible range -- the kept terms are never more.  Numerator sum w_h v_h: one product each, at most J / 64 + 2
  additions per lane and 6 in the butterfly; the denominator likewise; one division.  Positive sums again, so
  |E^ - E| <= gamma(10 J + 2 ceil(J / 64) + C + D + 40).
* The early stop of a direction: past the mode the ratio rho < 1 falls, so the mass beyond a weight w is <= w rho / (1 - rho); the
  kernel stops when that is < 2^-70 of the mode's weight (<= the sum of weights).  Two directions, numerator and denominator, and the
  test itself evaluated in floating point: an absolute 2^-67 covers it.
* remove_first mixes two such values with weights (n0 - r0) / n0 and r0 / n0: three more roundings.
* hits@k = sum take_d r_d / n_d <= k: a product, a division and D additions: k gamma(D + 2) (+ 3 with remove_first); R@k = hits / total
  <= 1: gamma(D + 6).

C and D are taken over the buckets that lie inside the limit whole plus the stretch the limit cuts off the next one (C skips a bucket
without a relevant row: its T is 0 and the kernel sums nothing for it; for hits, D runs over every bucket), so the bound is a function of the bucket counts, the limit and remove_first alone.  Four more roundings are granted for the reference's own conversion
to float64.
"""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

from tie_bracket_ref import counts_from_codes  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -53


class Exact:
    """numbers are Fractions"""
    name = "exact"

    def num(self, x):
        return Fraction(x)

    def div(self, x, n):
        return x / n

    def L(self, B, m):
        return sum((Fraction(1, B + i) for i in range(1, m + 1)), Fraction(0))

    def weights(self, n, r, take, tmin, tmax):
        return {h: math.comb(r, h) * math.comb(n - r, take - h) for h in range(tmin, tmax + 1)}

    def to_float(self, x):
        return float(x)


class Fixed:
    """numbers are integers scaled by 2^P"""
    name = "fixed"

    def __init__(self, P=256):
        self.P = P
        self._L = {}

    def num(self, x):
        return int(x) << self.P

    def div(self, x, n):
        return x // n

    def L(self, B, m):
        key = (B, m)
        if key not in self._L:
            one = 1 << self.P
            self._L[key] = sum(one // (B + i) for i in range(1, m + 1))
        return self._L[key]

    def weights(self, n, r, take, tmin, tmax):
        mode = min(max(((take + 1) * (r + 1)) // (n + 2), tmin), tmax)
        irr = n - r
        out = {mode: 1 << self.P}
        w = out[mode]
        for h in range(mode, tmax):                      # P(h + 1) / P(h)
            w = w * ((r - h) * (take - h)) // ((h + 1) * (irr - take + h + 1))
            if w == 0:
                break
            out[h + 1] = w
        w = out[mode]
        for h in range(mode, tmin, -1):                  # P(h - 1) / P(h)
            w = w * (h * (irr - take + h)) // ((r - h + 1) * (take - h + 1))
            if w == 0:
                break
            out[h - 1] = w
        return out

    def to_float(self, x):
        return float(Fraction(x, 1 << self.P))


EXACT = Exact()


def placed_sum(ctx, B, K, m, h):
    """T(B, K, m, h): the expected sum of precision terms of h relevant rows uniform on the ranks B + 1 .. B + m"""
    if h == 0:
        return ctx.num(0)
    L = ctx.L(B, m)
    t = (K + 1) * L
    if m > 1:
        M = ctx.num(m) - (B + 1) * L
        t = t + ctx.div((h - 1) * M, m - 1)
    return ctx.div(h * t, m)


def _drop_first(buckets):
    """-> [(weight numerator, buckets)] of remove_first, and the weight denominator n0; a query without a row: itself, weight 1 / 1"""
    d0 = next((d for d, (n, _) in enumerate(buckets) if n > 0), None)
    if d0 is None:
        return [(1, buckets)], 1
    n0, r0 = buckets[d0]
    out = []
    if n0 > r0:
        out.append((n0 - r0, buckets[:d0] + [(n0 - 1, r0)] + buckets[d0 + 1:]))
    if r0 > 0:
        out.append((r0, buckets[:d0] + [(n0 - 1, r0 - 1)] + buckets[d0 + 1:]))
    return out, n0


def _ap_walk(ctx, buckets, R):
    B = K = 0
    S = ctx.num(0)
    for n, r in buckets:
        if n == 0:
            continue
        if 0 < R < B + n and R > B:                      # the bucket the limit cuts
            take = R - B
            tmin, tmax = max(0, take - (n - r)), min(r, take)
            w = ctx.weights(n, r, take, tmin, tmax)
            acc = ctx.num(0)
            for h, wh in w.items():
                if K + h:
                    acc = acc + wh * ctx.div(S + placed_sum(ctx, B, K, take, h), K + h)
            return ctx.div(acc, sum(w.values()))
        if 0 < R <= B:                                   # on the boundary in front of this bucket
            break
        S = S + placed_sum(ctx, B, K, n, r)
        B += n
        K += r
    return ctx.div(S, K) if K else ctx.num(0)


def _hits_walk(ctx, buckets, k):
    B = 0
    h = ctx.num(0)
    for n, r in buckets:
        take = min(max(k - B, 0), n)
        if n and take:
            h = h + ctx.div(ctx.num(take * r), n)
        B += n
    tot = sum(r for _, r in buckets)
    return h, (ctx.div(h, tot) if tot else ctx.num(0))


def expected_one(buckets, R, ks=(), remove_first=False, ctx=EXACT):
    """-> (E[AP@R], [E[hits@k]], [E[R@k]]) as numbers of `ctx` (EXACT: Fractions).  R <= 0: no limit; R None: no AP (0)."""
    buckets = [(int(n), int(r)) for n, r in buckets]
    branches, den = _drop_first(buckets) if remove_first else ([(1, buckets)], 1)
    ap = ctx.num(0)
    hits = [ctx.num(0) for _ in ks]
    rec = [ctx.num(0) for _ in ks]
    for wgt, b in branches:
        if R is not None:
            ap = ap + wgt * _ap_walk(ctx, b, int(R))
        for t, k in enumerate(ks):
            h, rc = _hits_walk(ctx, b, int(k))
            hits[t] = hits[t] + wgt * h
            rec[t] = rec[t] + wgt * rc
    return ctx.div(ap, den), [ctx.div(h, den) for h in hits], [ctx.div(r, den) for r in rec]


def expected_from_counts(counts, limits, ks, remove_first=False, ctx=None):
    """counts [Qn, nb, 2] -> float64 lists ap [nlimits][Qn], hits [nk][Qn], recall [nk][Qn] (what ch_hamming_tie_expected returns), from
    the FIXED reference unless a ctx is given"""
    ctx = ctx or Fixed()
    Qn = len(counts)
    ap = [[0.0] * Qn for _ in limits]
    hits = [[0.0] * Qn for _ in ks]
    rec = [[0.0] * Qn for _ in ks]
    for qi in range(Qn):
        b = [(int(n), int(r)) for n, r in counts[qi]]
        if isinstance(ctx, Fixed):
            ctx._L.clear()
        for li, R in enumerate(limits):
            ap[li][qi] = ctx.to_float(expected_one(b, int(R), (), remove_first, ctx)[0])
        _, h, rc = expected_one(b, None, ks, remove_first, ctx)
        for t in range(len(ks)):
            hits[t][qi], rec[t][qi] = ctx.to_float(h[t]), ctx.to_float(rc[t])
    return ap, hits, rec


# ---- brute force -------------------------------------------------------------------------------------------------------------------
def brute_force_size(buckets):
    return math.prod(math.comb(int(n), int(r)) for n, r in buckets)


def brute_force(buckets, Rs, ks=(), remove_first=False):
    """Every tie order of a tiny problem, one per distinct relevance pattern (each bucket's C(n, r) patterns are equally likely):
    -> ({R: E[AP@R]}, {k: E[hits@k]}, {k: E[R@k]}) as Fractions."""
    per_bucket = []
    for n, r in buckets:
        n, r = int(n), int(r)
        per_bucket.append([tuple(1 if i in c else 0 for i in range(n)) for c in itertools.combinations(range(n), r)])
    ap = {R: Fraction(0) for R in Rs}
    hits = {k: Fraction(0) for k in ks}
    rec = {k: Fraction(0) for k in ks}
    count = 0
    for combo in itertools.product(*per_bucket):
        order = [f for part in combo for f in part]
        if remove_first:
            order = order[1:]
        count += 1
        s, kk, at = Fraction(0), 0, {0: Fraction(0)}     # AP of the first `rank` rows, for every rank
        for rank, f in enumerate(order, 1):
            if f:
                kk += 1
                s += Fraction(kk, rank)
            at[rank] = s / kk if kk else Fraction(0)
        for R in Rs:
            ap[R] += at[len(order) if R <= 0 else min(R, len(order))]
        tot = sum(order)
        for k in ks:
            h = sum(order[:k])
            hits[k] += h
            rec[k] += Fraction(h, tot) if tot else 0
    return ({R: v / count for R, v in ap.items()}, {k: v / count for k, v in hits.items()}, {k: v / count for k, v in rec.items()})


# ---- the kernel's arithmetic in Python floats ----------------------------------------------------------------------------------------
def _sums_f(B, m):
    L = M = 0.0
    for i in range(m):
        inv = 1.0 / float(B + i + 1)
        L += inv
        M += float(i) * inv
    return L, M


def _cut_f(B, K, S, n, r, take):
    irr = n - r
    tmin, tmax = max(0, take - irr), min(r, take)
    L, M = _sums_f(B, take)
    A = float(K + 1) * L
    C = M / float(take - 1) if take > 1 else 0.0

    def value(h):
        if K + h == 0:
            return 0.0
        T = (float(h) / float(take)) * (A + float(h - 1) * C) if h else 0.0
        return (S + T) / float(K + h)

    md = math.floor((float(take) + 1.0) * (float(r) + 1.0) / (float(n) + 2.0))
    mode = tmax if md >= tmax else (tmin if md <= tmin else int(md))
    cut = 2.0 ** -70
    num, den, kept = value(mode), 1.0, 1
    w = 1.0
    for h in range(mode, tmax):                          # the step h -> h + 1; the kernel tests the stop once per 64 steps
        rho = (float(r - h) * float(take - h)) / (float(h + 1) * float(irr + h + 1 - take))
        if (h - mode) % 64 == 63 and rho < 1.0 and w * rho < cut * (1.0 - rho):
            break
        w *= rho
        num += w * value(h + 1)
        den += w
        kept += 1
    w = 1.0
    for h in range(mode, tmin, -1):                      # the step h -> h - 1
        rho = (float(h) * float(irr + h - take)) / (float(r - h + 1) * float(take - h + 1))
        if (mode - h) % 64 == 0 and h != mode and rho < 1.0 and w * rho < cut * (1.0 - rho):
            break
        w *= rho
        num += w * value(h - 1)
        den += w
        kept += 1
    return num / den, kept


def _walk_f(buckets, limits, ks):
    """limits: ascending, <= 0 = none, last -> ([E AP], [hits], [recall], most kept terms of a cut)"""
    lim = [R if R > 0 else float("inf") for R in limits]
    B = K = 0
    S = 0.0
    hits = [0.0] * len(ks)
    ap = []
    kept = 0
    for n, r in buckets:
        if n == 0:
            continue
        for t, k in enumerate(ks):
            tk = min(max(k - B, 0), n)
            hits[t] += float(r) if tk == n else float(tk) * float(r) / float(n)
        while len(ap) < len(lim) and lim[len(ap)] < B + n:
            take = int(lim[len(ap)]) - B
            if take == 0:
                ap.append(S / float(K) if K else 0.0)
            else:
                e, kp = _cut_f(B, K, S, n, r, take)
                kept = max(kept, kp)
                ap.append(e)
        if len(ap) < len(lim) and r > 0:
            L, M = _sums_f(B, n)
            second = (float(r - 1) / float(n - 1)) * M if n > 1 else 0.0
            S += (float(r) / float(n)) * (float(K + 1) * L + second)
        B += n
        K += r
    while len(ap) < len(lim):
        ap.append(S / float(K) if K else 0.0)
    tot = sum(r for _, r in buckets)
    return ap, hits, [h / float(tot) if tot else 0.0 for h in hits], kept


def expected_float64(buckets, limits, ks=(), remove_first=False):
    """-> ([E AP per limit], [E hits per k], [E recall per k], most kept terms of a cut bucket) in Python floats"""
    buckets = [(int(n), int(r)) for n, r in buckets]
    branches, den = _drop_first(buckets) if remove_first else ([(1, buckets)], 1)
    ap, hits, rec, kept = [0.0] * len(limits), [0.0] * len(ks), [0.0] * len(ks), 0
    for wgt, b in branches:
        scale = float(wgt) / float(den)
        a, h, rc, kp = _walk_f(b, limits, ks)
        kept = max(kept, kp)
        ap = [x + scale * y for x, y in zip(ap, a)]
        hits = [x + scale * y for x, y in zip(hits, h)]
        rec = [x + scale * y for x, y in zip(rec, rc)]
    return ap, hits, rec, kept


# ---- the derived bound ---------------------------------------------------------------------------------------------------------------
def gamma(k):
    return k * U / (1.0 - k * U)


def _bound_walk(buckets, R):
    C = D = B = 0                                        # over the buckets the limit holds whole, and the stretch it cuts off the next
    for n, r in buckets:
        if not n:
            continue
        if 0 < R <= B:
            break
        D += 1
        if 0 < R < B + n:
            take = R - B
            J = min(r, take) - max(0, take - (n - r))
            C = max(C, -(-take // 64))
            return gamma(10 * J + 2 * -(-J // 64) + C + D + 40) + 2.0 ** -67
        if r:                                            # a bucket without a relevant row adds T = 0 exactly: nothing is summed for it
            C = max(C, -(-n // 64))
        B += n
    return gamma(C + D + 13 + 4)


def error_bound(buckets, R, remove_first=False):
    """the largest |kernel - exact| of E[AP@R] for this query that the derivation above allows (module docstring)"""
    buckets = [(int(n), int(r)) for n, r in buckets]
    if not remove_first:
        return _bound_walk(buckets, int(R))
    return max(_bound_walk(b, int(R)) for _, b in _drop_first(buckets)[0]) + gamma(3)


def hits_bound(buckets, k, remove_first=False):
    """-> (bound of E[hits@k], bound of E[R@k])"""
    D = sum(1 for n, _ in buckets if int(n))
    extra = 3 if remove_first else 0
    return int(k) * gamma(D + 2 + extra + 4), gamma(D + 6 + extra + 4)
