// strk_mi.h — Mendelian inheritance and the de novo test of a child / mother / father trio, per locus.
// Reference: strkit/mi/result.py:275-501 (MILocusData.respects_mi, de_novo_test) and strkit/utils.py:49-57 (cis_overlap); the
// statistics are scipy.stats.chi2_contingency(correction=False) and scipy.stats.mannwhitneyu(use_continuity=False,
// method="auto") as scipy 1.15 computes them.  tests/mi_restatement.py is the readable statement.
//
// Everything that is arithmetic is written once, for host and device (STRK_MI_HD), over a locus's TABLE: its distinct copy
// numbers in ascending order and, per distinct value, how many reads of each of the six groups (child 0, child 1, mother 0,
// mother 1, father 0, father 1) carry it.  Rank sums, tie terms, bins and the sums behind the means are integer sums over the
// table in ascending order, so every path that builds the same table gives the same bits.  Only building the table differs:
//   host_locus   std::sort of (value, group) keys;
//   k_mi_small   one wave per locus, counting in LDS (every read counts the first occurrences below it);
//   k_mi_large   one workgroup per locus, a bitonic sort of the keys in the global workspace, then a chunked scan.
// The special functions (exp, erfc, the chi-square tail, the exact Mann-Whitney tail) use + - * / and sqrt alone, so that host
// and device agree bit for bit (the library is built with -ffp-contract=off).  Without HIP the header compiles with the host
// compiler alone (tools/mi_asan.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define STRK_MI_HD __host__ __device__ inline
#else
#define STRK_MI_HD inline
#endif

namespace strk_mi {

constexpr int kGroups = 6;             // child 0, child 1, mother 0, mother 1, father 0, father 1
constexpr int kMaxGroup = 65535;       // reads of one group (the cap of strk_call_alleles)
constexpr int kSmallReads = 256;       // k_mi_small takes the loci whose six groups hold at most this many reads together
constexpr int kSmallWaves = 4;         // loci (waves) per workgroup of k_mi_small
constexpr int kExactShort = 8;         // scipy's _mwu_choose_method: exact when a side has at most 8 values and nothing is tied
constexpr int kKinds = 7;              // strict, pm1, ci_95, ci_99, seq, sl, sl_pm1

constexpr int kTestNone = 0, kTestX2 = 1, kTestWmw = 2, kTestWmwGt = 3;
constexpr int kTested = 0, kOverlap = 1, kEmptyParent = 2, kEmptyChild = 3;          // out_status
constexpr int kFromNone = 0, kFromUnknown = 1, kFromMat = 2, kFromPat = 3, kFromBoth = 4;   // out_mutation_from

constexpr uint32_t kChildMask = 3u;
STRK_MI_HD uint32_t mother_bit(int a) { return 1u << (2 + a); }
STRK_MI_HD uint32_t father_bit(int b) { return 1u << (4 + b); }

// ---- special functions -----------------------------------------------------------------------------------------------------
STRK_MI_HD double from_bits(uint64_t b) {
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
STRK_MI_HD double nan_d() { return from_bits(0x7ff8000000000000ull); }
STRK_MI_HD double pow2i(int k) { return from_bits((uint64_t)(k + 1023) << 52); }   // 2^k, -1022 <= k <= 1023
STRK_MI_HD double sqrt_d(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return __builtin_sqrt(x);
#endif
}

// e^x: x = k ln 2 + r, |r| <= ln 2 / 2, a Taylor polynomial of degree 14 in r (its remainder is below 2^-62).
STRK_MI_HD double exp_d(double x) {
    if (x != x) return x;
    if (x > 709.0) return from_bits(0x7ff0000000000000ull);
    if (x < -745.2) return 0.0;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.44269504088896338700e+00;
    const int k = (int)(x * inv_ln2 + (x < 0.0 ? -0.5 : 0.5));
    const double r = (x - k * ln2_hi) - k * ln2_lo;
    double s = 1.0;
    for (int i = 14; i >= 1; --i) s = 1.0 + (r / i) * s;
    return k >= -1000 ? s * pow2i(k) : s * pow2i(k + 1000) * pow2i(-1000);
}

// erfc(x).  Below 1.5: 1 - erf(x), erf by the series of positive terms 2/sqrt(pi) e^(-x^2) sum 2^n x^(2n+1) / (2n+1)!!.
// From 1.5 on: the continued fraction e^(-x^2) / sqrt(pi) / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...)))), 150 levels (at 1.5
// what is cut off is below 1e-20 of the value; 1 - erf loses at most two digits below 1.5, where erfc is above 0.03).
// flush: give 0 where scipy's erfc does (cephes: once x^2 is above MAXLOG = 709.78), so that a normal tail that is 0 there is 0 here;
// the chi-square tail, which scipy takes from igamc, asks for the value itself
STRK_MI_HD double erfc_d(double x, bool flush = true) {
    if (x != x) return x;
    if (x < 0.0) return 2.0 - erfc_d(-x, flush);
    if (x < 1.5) {
        double term = x, sum = x;
        const double xx2 = 2.0 * x * x;
        for (int n = 0; n < 300; ++n) {
            term = term * xx2 / (double)(2 * n + 3);
            sum += term;
            if (term < sum * 1e-18) break;
        }
        return 1.0 - 1.1283791670955126 * exp_d(-x * x) * sum;
    }
    if (flush && x * x > 709.78271289338397) return 0.0;
    double f = x;
    for (int k = 150; k >= 1; --k) f = x + (0.5 * k) / f;
    return exp_d(-x * x) * 0.5641895835477563 / f;
}

STRK_MI_HD double norm_sf(double z) { return 0.5 * erfc_d(z * 0.70710678118654752440); }

// The chi-square survival function = the regularised upper incomplete gamma Q(dof / 2, x / 2).  dof is a whole number, so the
// finite forms hold: Q(m, h) = e^-h sum_{j<m} h^j / j!, and Q(k + 1/2, h) = erfc(sqrt h) + e^-h sum_{j=1..k} h^(j-1/2) / Gamma(j+1/2).
// All terms are positive.  The sum is kept below 2^600 by rescaling, its power of two goes into the exponent, and the exponent
// is applied in two halves: p stays good to about h * 1e-16 relative down to 1e-300 whatever dof and x are.
STRK_MI_HD double chi2_sf(int64_t dof, double x) {
    if (x != x) return x;
    if (dof <= 0 || !(x > 0.0)) return 1.0;
    const double h = 0.5 * x;
    const bool odd = (dof & 1) != 0;
    const int64_t n_terms = dof / 2;                // the terms of the sum
    double term = odd ? sqrt_d(h) * 1.1283791670955126 : 1.0, sum = 0.0;
    int scale = 0;                                   // the sum stands for sum * 2^(600 scale)
    bool whole = true;                               // the sum ran to its last term
    for (int64_t j = 0; j < n_terms; ++j) {
        if (j > 0) term = term * h / (odd ? (double)j + 0.5 : (double)j);
        sum += term;
        if (term > 4.149515568880993e+180) { term *= 2.409919865102884e-181; sum *= 2.409919865102884e-181; ++scale; }   // 2^600, 2^-600
        if (term < sum * 1e-19 && (double)j > h) { whole = false; break; }
    }
    // sum * e^(-h + 600 scale ln 2): e^-h alone is denormal from h = 708 on and 0 from 745 while the product may still be far
    // above 1e-300 (the sum is large then), so the exponent goes in as two halves and no factor underflows before the product
    const double half = 0.5 * (-h + scale * 415.88830833596718565);   // 600 ln 2
    // Where scipy gives 0: its igamc (cephes) multiplies by the factor h^a e^-h / Gamma(a), a = dof / 2, and returns 0 once that
    // factor is below e^-709.78 (MAXLOG) while |a - h| > 0.4 a, which is a tail of about 1e-311.  The factor is the sum's last
    // term times h e^-h (half the first term for one degree); it is compared 2^200 higher up, out of the denormal range.
    // Without this a locus whose four p-values are 0 in scipy would get a denormal winner here instead of configuration 0.
    const double a = 0.5 * (double)dof;
    if (whole && (a > h ? a - h : h - a) > 0.4 * a) {
        const double last = n_terms > 0 ? term * h : 0.5 * term, up = half + 69.31471805599453;   // 100 ln 2
        if ((last * exp_d(up)) * exp_d(up) < 8.938889586303633e-249) return 0.0;                  // e^-MAXLOG 2^200
    }
    double q = n_terms > 0 ? (sum * exp_d(half)) * exp_d(half) : 0.0;
    if (odd) q += erfc_d(sqrt_d(h), false);
    return q > 1.0 ? 1.0 : q;
}

// ---- 128-bit counts of the exact Mann-Whitney distribution -------------------------------------------------------------------
struct U128 {
    uint64_t lo, hi;
};
STRK_MI_HD void add128(U128* a, const U128& b) {
    const uint64_t lo = a->lo + b.lo;
    a->hi += b.hi + (lo < a->lo ? 1u : 0u);
    a->lo = lo;
}
STRK_MI_HD void sub128(U128* a, const U128& b) {
    const uint64_t lo = a->lo - b.lo;
    a->hi -= b.hi + (a->lo < b.lo ? 1u : 0u);
    a->lo = lo;
}
STRK_MI_HD double to_double(const U128& a) { return (double)a.hi * 18446744073709551616.0 + (double)a.lo; }

// Entries of the workspace that mwu_exact_sf needs for sides of n1 and n2 values: floor(n1 n2 / 2) + 1.
STRK_MI_HD int64_t exact_entries_for(int64_t n1, int64_t n2) { return n1 * n2 / 2 + 1; }

// P(U >= u) under the null for sides of n1 and n2 untied values.  The numbers of arrangements with U = j are the coefficients of
// the Gaussian binomial [n1 + n2 choose a]_q = prod_{i=1..a} (1 - q^(b+i)) / (1 - q^i), a the short side and b the long one;
// only those up to k = min(n1 n2 - u, u - 1) <= n1 n2 / 2 are built (the distribution is symmetric), exactly, in 128 bits.
// ws: room for `cap` entries.  NaN when the workspace is too small (the callers size it with exact_entries_for).
STRK_MI_HD double mwu_exact_sf(int64_t n1, int64_t n2, int64_t u, U128* ws, int64_t cap) {
    const int64_t mn = n1 * n2;
    if (u <= 0) return 1.0;
    if (u > mn) return 0.0;
    const int64_t a = n1 < n2 ? n1 : n2, b = n1 < n2 ? n2 : n1;
    const bool upper = mn - u <= u - 1;            // the tail itself is the shorter sum
    const int64_t k = upper ? mn - u : u - 1;
    if (!ws || k + 1 > cap) return nan_d();
    ws[0] = U128{1, 0};
    for (int64_t j = 1; j <= k; ++j) ws[j] = U128{0, 0};
    for (int64_t i = 1; i <= a; ++i) {
        for (int64_t j = i; j <= k; ++j) add128(&ws[j], ws[j - i]);             // / (1 - q^i)
        for (int64_t j = k; j >= b + i; --j) sub128(&ws[j], ws[j - (b + i)]);   // * (1 - q^(b+i))
    }
    U128 part{0, 0};
    for (int64_t j = 0; j <= k; ++j) add128(&part, ws[j]);
    double total = 1.0;                             // C(a + b, a)
    for (int64_t i = 1; i <= a; ++i) total = total * (double)(b + i) / (double)i;
    return upper ? to_double(part) / total : (total - to_double(part)) / total;
}

// ---- the table of a locus ------------------------------------------------------------------------------------------------------
struct Table {
    const int32_t* val;   // [n_distinct], ascending
    const int32_t* cnt;   // [n_distinct][kGroups]
    int32_t n_distinct;
};

STRK_MI_HD int64_t masked(const int32_t* c, uint32_t mask) {
    int64_t n = 0;
    for (int g = 0; g < kGroups; ++g)
        if ((mask >> g) & 1u) n += c[g];
    return n;
}

// scipy.stats.mannwhitneyu(x, y, use_continuity=False, alternative = greater ? "greater" : "two-sided", method="auto").pvalue for
// x = the reads of the groups in xmask, y = those in ymask (both non-empty).
STRK_MI_HD double mwu_p(const Table& t, uint32_t xmask, uint32_t ymask, bool greater, U128* ws, int64_t ws_cap) {
    int64_t n1 = 0, n2 = 0, u2 = 0, tie = 0;       // u2 = 2 U1 = sum over x of 2 #(y < x) + #(y == x)
    for (int32_t d = 0; d < t.n_distinct; ++d) {
        const int64_t xd = masked(t.cnt + (size_t)d * kGroups, xmask), yd = masked(t.cnt + (size_t)d * kGroups, ymask);
        u2 += xd * (2 * n2 + yd);
        n1 += xd; n2 += yd;
        const int64_t s = xd + yd;
        tie += s * s * s - s;
    }
    const double u1 = (double)u2 / 2.0, mn = (double)(n1 * n2), u2nd = mn - u1;
    const double u = greater ? u1 : (u1 > u2nd ? u1 : u2nd), f = greater ? 1.0 : 2.0;
    double p;
    if ((n1 > kExactShort && n2 > kExactShort) || tie > 0) {
        const double n = (double)(n1 + n2), mu = mn / 2.0;
        const double s = sqrt_d(mn / 12.0 * ((n + 1.0) - (double)tie / (n * (n - 1.0))));
        p = norm_sf((u - mu) / s);
    } else {
        p = mwu_exact_sf(n1, n2, (int64_t)u, ws, ws_cap);
    }
    p *= f;
    if (p != p) return p;
    return p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
}

// The terms (observed - expected)^2 / expected of the 2 x bins table [[y bins], [x bins]] in row-major order, one after the
// other: the jointly empty bins of the two masks are passed over.
struct X2Terms {
    const Table& t;
    uint32_t xmask, ymask;
    int64_t n1, n2;
    double total;
    int32_t d;
    int row;      // 0: the y row, 1: the x row
    STRK_MI_HD double next() {
        for (;; ++d) {
            if (d == t.n_distinct) { d = 0; row = 1; }
            const int64_t xd = masked(t.cnt + (size_t)d * kGroups, xmask), yd = masked(t.cnt + (size_t)d * kGroups, ymask);
            if (xd + yd == 0) continue;
            ++d;
            const double e = (double)((row ? n1 : n2) * (xd + yd)) / total, o = (double)(row ? xd : yd);
            return (o - e) * (o - e) / e;
        }
    }
};

// The sum of the next n terms in the order of numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, pairwise_sum:
// below 8 terms one after the other; up to 128 eight running sums combined as a tree, the rest one after the other; beyond that
// the halves, the first a multiple of 8), so that the statistic has the bits chi2_contingency gives it and two configurations
// whose p-values are equal there are equal here.
STRK_MI_HD double pairwise_block(X2Terms& c, int64_t n) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += c.next();
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = c.next();
    int64_t i = 8;
    for (; i < n - n % 8; i += 8)
        for (int j = 0; j < 8; ++j) r[j] += c.next();
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += c.next();
    return res;
}
STRK_MI_HD double pairwise_sum(X2Terms& c, int64_t n) {
    struct Frame { int64_t n; double left; int stage; } st[48];   // (the halves of 2^63 terms would not need more)
    int sp = 0;
    double ret = 0.0;
    st[0] = Frame{n, 0.0, 0};
    while (sp >= 0) {
        const int64_t fn = st[sp].n;
        int64_t n2 = fn / 2;
        n2 -= n2 % 8;
        if (fn <= 128) { ret = pairwise_block(c, fn); --sp; }
        else if (st[sp].stage == 0) { st[sp].stage = 1; st[sp + 1] = Frame{n2, 0.0, 0}; ++sp; }
        else if (st[sp].stage == 1) { st[sp].left = ret; st[sp].stage = 2; st[sp + 1] = Frame{fn - n2, 0.0, 0}; ++sp; }
        else { ret = st[sp].left + ret; --sp; }
    }
    return ret;
}

// scipy.stats.chi2_contingency([[y bins], [x bins]], correction=False).pvalue over the bins min .. max without the jointly empty.
STRK_MI_HD double x2_p(const Table& t, uint32_t xmask, uint32_t ymask) {
    int64_t n1 = 0, n2 = 0, bins = 0;
    for (int32_t d = 0; d < t.n_distinct; ++d) {
        const int64_t xd = masked(t.cnt + (size_t)d * kGroups, xmask), yd = masked(t.cnt + (size_t)d * kGroups, ymask);
        n1 += xd; n2 += yd;
        bins += xd + yd > 0 ? 1 : 0;
    }
    if (bins <= 1) return 1.0;
    X2Terms terms{t, xmask, ymask, n1, n2, (double)(n1 + n2), 0, 0};
    return chi2_sf(bins - 1, pairwise_sum(terms, 2 * bins));
}

// What one pass over the table gives: sizes and sums of the groups, and whether the child's reads are all one value.
struct Summary {
    int64_t n[kGroups], sum[kGroups];
    int32_t child_distinct;
    bool all_child_value[kGroups];   // every read of the group carries the child's single value (true for an empty group)
};

STRK_MI_HD void summarise(const Table& t, Summary* s) {
    for (int g = 0; g < kGroups; ++g) { s->n[g] = 0; s->sum[g] = 0; s->all_child_value[g] = true; }
    s->child_distinct = 0;
    int32_t at = -1;
    for (int32_t d = 0; d < t.n_distinct; ++d) {
        const int32_t* c = t.cnt + (size_t)d * kGroups;
        if (c[0] + c[1] > 0) { ++s->child_distinct; at = d; }
        for (int g = 0; g < kGroups; ++g) { s->n[g] += c[g]; s->sum[g] += (int64_t)c[g] * t.val[d]; }
    }
    for (int g = 0; g < kGroups; ++g) s->all_child_value[g] = s->child_distinct == 1 && t.cnt[(size_t)at * kGroups + g] == s->n[g];
}

// The early returns of de_novo_test (result.py:416-428), in the order of its loop over the four parent configurations.  A child
// without reads is this project's own status: the reference fails on it (chi2_contingency of an empty row raises).
STRK_MI_HD int early_status(const Summary& s, int test) {
    if (s.n[0] + s.n[1] == 0) return kEmptyChild;
    for (int c = 0; c < 4; ++c) {
        const int m = 2 + (c >> 1), f = 4 + (c & 1);
        if (test != kTestX2 && s.child_distinct == 1 && s.n[m] + s.n[f] > 0 && s.all_child_value[m] && s.all_child_value[f]) return kOverlap;
        if (s.n[m] == 0 || s.n[f] == 0) return kEmptyParent;
    }
    return kTested;
}

// Entries of the exact workspace a locus may need: the largest exact_entries_for over the tests it can run with a side of at
// most kExactShort (four configurations against the whole child, the two parent groups against either child group); 0: none.
STRK_MI_HD int64_t exact_entries(const int64_t* n) {
    int64_t best = 0;
    for (int c = 0; c < 4; ++c) {
        const int64_t n1 = n[2 + (c >> 1)] + n[4 + (c & 1)], n2 = n[0] + n[1];
        if ((n1 <= kExactShort || n2 <= kExactShort) && exact_entries_for(n1, n2) > best) best = exact_entries_for(n1, n2);
    }
    for (int g = 2; g < kGroups; ++g)
        for (int k = 0; k < 2; ++k)
            if ((n[g] <= kExactShort || n[k] <= kExactShort) && exact_entries_for(n[g], n[k]) > best) best = exact_entries_for(n[g], n[k]);
    return best;
}

// p of one parent configuration (mother's allele c >> 1, father's c & 1) against all of the child's reads.
STRK_MI_HD double config_p(const Table& t, int test, int c, U128* ws, int64_t ws_cap) {
    const uint32_t parents = mother_bit(c >> 1) | father_bit(c & 1);
    return test == kTestX2 ? x2_p(t, parents, kChildMask) : mwu_p(t, parents, kChildMask, test == kTestWmwGt, ws, ws_cap);
}

STRK_MI_HD int from_p_values(double mat_p, double pat_p, double sig) {
    if (mat_p < sig && pat_p < sig) return kFromBoth;
    if (mat_p < sig) return kFromMat;
    if (pat_p < sig) return kFromPat;
    return kFromUnknown;
}

STRK_MI_HD double abs_d(double x) { return x < 0.0 ? -x : x; }

// The rest of de_novo_test behind the four p-values: the first largest one (a NaN and a 0 never win), and below the level the
// two sums of distances between means and the two second tests.
STRK_MI_HD void choose_config(const Table& t, const Summary& s, const double* p4, double sig, U128* ws, int64_t ws_cap, double* out_p,
                              int32_t* out_config, int32_t* out_from) {
    double best = 0.0;
    int cfg = 0;
    for (int c = 0; c < 4; ++c)
        if (p4[c] > best) { best = p4[c]; cfg = c; }
    *out_p = best;
    *out_config = cfg;
    *out_from = kFromNone;
    if (!(best < sig)) return;
    const int m = 2 + (cfg >> 1), f = 4 + (cfg & 1);
    const double c0 = (double)s.sum[0] / (double)s.n[0], c1 = (double)s.sum[1] / (double)s.n[1];
    const double mm = (double)s.sum[m] / (double)s.n[m], fm = (double)s.sum[f] / (double)s.n[f];
    const double dist1 = abs_d(c0 - mm) + abs_d(c1 - fm), dist2 = abs_d(c1 - mm) + abs_d(c0 - fm);
    if (dist2 > dist1)
        *out_from = from_p_values(mwu_p(t, 1u << m, 1u, false, ws, ws_cap), mwu_p(t, 1u << f, 2u, false, ws, ws_cap), sig);
    else if (dist1 > dist2)
        *out_from = from_p_values(mwu_p(t, 1u << m, 2u, false, ws, ws_cap), mwu_p(t, 1u << f, 1u, false, ws, ws_cap), sig);
    else
        *out_from = kFromUnknown;
}

// ---- respects MI (result.py:275-389, decimal=False) ----------------------------------------------------------------------------
STRK_MI_HD bool cis_overlap(double a_lo, double a_hi, double b_lo, double b_hi) {   // strkit/utils.py:49-57
    const double epsilon = -0.0001;
    return (b_hi - a_lo) > epsilon && (a_hi - b_lo) > epsilon;
}
STRK_MI_HD bool respects_strict(const int32_t* g) {   // g: child 0, child 1, mother 0, mother 1, father 0, father 1
    const bool c0m = g[0] == g[2] || g[0] == g[3], c1m = g[1] == g[2] || g[1] == g[3];
    const bool c0f = g[0] == g[4] || g[0] == g[5], c1f = g[1] == g[4] || g[1] == g[5];
    return (c0m && c1f) || (c0f && c1m);
}
// ci: six intervals (lo, hi) in the order of the groups; the parents' are widened
STRK_MI_HD bool respects_ci(const double* ci, double widen) {
    double w[8];
    for (int i = 0; i < 4; ++i) {
        w[2 * i] = ci[4 + 2 * i] - ci[4 + 2 * i] * widen;
        w[2 * i + 1] = ci[5 + 2 * i] + ci[5 + 2 * i] * widen;
    }
    bool ov[2][4];   // child allele x parent allele (mother 0, mother 1, father 0, father 1)
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 4; ++i) ov[c][i] = cis_overlap(ci[2 * c], ci[2 * c + 1], w[2 * i], w[2 * i + 1]);
    return ((ov[0][0] || ov[0][1]) && (ov[1][2] || ov[1][3])) || ((ov[1][0] || ov[1][1]) && (ov[0][2] || ov[0][3]));
}
STRK_MI_HD bool respects_pm1(const int32_t* g) {
    double ci[12];
    for (int c = 0; c < 2; ++c) { ci[2 * c] = (double)g[c] - 1.0; ci[2 * c + 1] = (double)g[c] + 1.0; }
    for (int i = 2; i < 6; ++i) ci[2 * i] = ci[2 * i + 1] = (double)g[i];
    return respects_ci(ci, 0.0);
}
// out7: 1, 0 or -1 (None) per kind.  ci99, seq_id, seq_len: the locus's own six / twelve entries, or NULL.
STRK_MI_HD void respects_mi(const int32_t* gt, const int32_t* ci95, const int32_t* ci99, const int32_t* seq_id, const int32_t* seq_len,
                            double widen, int8_t* out7) {
    double ci[12];
    out7[0] = respects_strict(gt) ? 1 : 0;
    out7[1] = respects_pm1(gt) ? 1 : 0;
    for (int i = 0; i < 12; ++i) ci[i] = (double)ci95[i];
    out7[2] = respects_ci(ci, widen) ? 1 : 0;
    out7[3] = -1;
    if (ci99) {
        for (int i = 0; i < 12; ++i) ci[i] = (double)ci99[i];
        out7[3] = respects_ci(ci, widen) ? 1 : 0;
    }
    bool seqs = seq_id != nullptr;
    for (int i = 0; seqs && i < 6; ++i) seqs = seq_id[i] >= 0;
    out7[4] = seqs ? (respects_strict(seq_id) ? 1 : 0) : -1;
    out7[5] = seqs ? (respects_strict(seq_len) ? 1 : 0) : -1;
    out7[6] = seqs ? (respects_pm1(seq_len) ? 1 : 0) : -1;
}

// ---- one call ------------------------------------------------------------------------------------------------------------------
// The arrays of a call (or of a piece of one: then grp_off counts from the piece's first read and every array begins at the
// piece's first locus).  Host pointers for host_locus, device pointers for the kernels.
struct Args {
    const int64_t* grp_off;    // [6 n + 1]; NULL with test == kTestNone
    const int32_t* cn;
    const int32_t *gt, *ci95, *ci99, *seq_id, *seq_len;
    const int64_t* ws_off;     // [n] byte offsets into ws (device only)
    char* ws;
    int32_t test;
    double sig_level, widen;
    int8_t* respects;          // [7 n]
    double* p;
    int32_t *config, *from, *status;
};

STRK_MI_HD void write_respects(const Args& a, int64_t l) {
    respects_mi(a.gt + 6 * l, a.ci95 + 12 * l, a.ci99 ? a.ci99 + 12 * l : nullptr, a.seq_id ? a.seq_id + 6 * l : nullptr,
                a.seq_len ? a.seq_len + 6 * l : nullptr, a.widen, a.respects + kKinds * l);
}
STRK_MI_HD void write_untested(const Args& a, int64_t l, int status) {
    a.p[l] = nan_d(); a.config[l] = -1; a.from[l] = kFromNone; a.status[l] = status;
}

// Host twin: locus l of a checked call, one thread.  keys / tval / tcnt / ws are the thread's scratch.
inline void host_locus(const Args& a, int64_t l, std::vector<uint64_t>& keys, std::vector<int32_t>& tval, std::vector<int32_t>& tcnt,
                       std::vector<U128>& ws) {
    write_respects(a, l);
    if (a.test == kTestNone) return;
    const int64_t* off = a.grp_off + 6 * l;
    keys.clear();
    int64_t n[kGroups];
    for (int g = 0; g < kGroups; ++g) {
        n[g] = off[g + 1] - off[g];
        for (int64_t r = off[g]; r < off[g + 1]; ++r) keys.push_back((uint64_t)(uint32_t)a.cn[r] << 3 | (uint64_t)g);
    }
    std::sort(keys.begin(), keys.end());
    tval.clear(); tcnt.clear();
    for (const uint64_t k : keys) {
        const int32_t v = (int32_t)(k >> 3);
        if (tval.empty() || tval.back() != v) { tval.push_back(v); tcnt.insert(tcnt.end(), kGroups, 0); }
        ++tcnt[tcnt.size() - kGroups + (k & 7u)];
    }
    const Table t{tval.data(), tcnt.data(), (int32_t)tval.size()};
    Summary s;
    summarise(t, &s);
    const int st = early_status(s, a.test);
    if (st != kTested) return write_untested(a, l, st);
    const int64_t cap = exact_entries(n);
    ws.resize((size_t)cap);
    double p4[4];
    for (int c = 0; c < 4; ++c) p4[c] = config_p(t, a.test, c, ws.data(), cap);
    choose_config(t, s, p4, a.sig_level, ws.data(), cap, &a.p[l], &a.config[l], &a.from[l]);
    a.status[l] = kTested;
}

// Bytes of a locus's workspace: what k_mi_large sorts and tabulates (large = true), then four exact workspaces (one per
// configuration, evaluated side by side).
STRK_MI_HD int64_t pow2_at_least(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
STRK_MI_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
STRK_MI_HD int64_t round256(int64_t n) { return (n + 255) & ~(int64_t)255; }
STRK_MI_HD int64_t large_part_bytes(int64_t n_reads) { return round256(pow2_at_least(n_reads) * 8) + round256(n_reads * 4) + round256(n_reads * 4 * kGroups); }
STRK_MI_HD int64_t locus_ws_bytes(const int64_t* n, bool large) {
    int64_t total = 0;
    for (int g = 0; g < kGroups; ++g) total += n[g];
    return (large ? large_part_bytes(total) : 0) + round256(4 * exact_entries(n) * (int64_t)sizeof(U128));
}

}  // namespace strk_mi

#if defined(__HIPCC__)
namespace strk_mi {

// What both kernels do once the table stands: lanes 0 .. 3 of a wave take one parent configuration each, lane 0 the rest.
// Called by all 64 lanes of one wave; `exact` = the locus's four exact workspaces of `cap` entries each.
__device__ inline void device_finish(const Args& a, int64_t l, const Table& t, U128* exact, int64_t cap, int lane) {
    double my_p = 0.0;
    int st = kTested;
    Summary s;
    if (lane < 4) {
        summarise(t, &s);
        st = early_status(s, a.test);
        if (st == kTested) my_p = config_p(t, a.test, lane, cap > 0 ? exact + (size_t)lane * cap : nullptr, cap);
    }
    double p4[4];
    for (int c = 0; c < 4; ++c) p4[c] = __shfl(my_p, c, 64);
    if (lane == 0) {
        if (st != kTested) {
            write_untested(a, l, st);
        } else {
            choose_config(t, s, p4, a.sig_level, cap > 0 ? exact : nullptr, cap, &a.p[l], &a.config[l], &a.from[l]);
            a.status[l] = kTested;
        }
    }
}

// One wave per locus, kSmallWaves loci per workgroup; list[i] = the locus of wave i (NULL: locus i).  A locus of at most
// kSmallReads reads.  The wave's slice of LDS: the reads, whether each is the first occurrence of its value, the table.
// Every read counts the first occurrences below it, which is its value's place in the table; integer atomics in LDS count the
// groups, so the table does not depend on the order of the lanes.  The slice belongs to one wave: its LDS operations are issued
// in order and the loops around them are wave-uniform in what they store and load, so a fence orders them and no barrier stands.
__global__ void __launch_bounds__(64 * kSmallWaves) k_mi_small(Args a, const int32_t* list, int32_t n_list) {
    __shared__ int32_t s_val[kSmallWaves][kSmallReads], s_first[kSmallWaves][kSmallReads], s_tval[kSmallWaves][kSmallReads],
        s_tcnt[kSmallWaves][kSmallReads * kGroups];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kSmallWaves + w);
    if (i >= n_list) return;
    const int64_t l = list ? list[i] : i;
    if (lane == 0) write_respects(a, l);
    if (a.test == kTestNone) return;
    const int64_t* off = a.grp_off + 6 * l;
    const int64_t base = off[0];
    int32_t rel[kGroups + 1];
    for (int g = 0; g <= kGroups; ++g) rel[g] = (int32_t)(off[g] - base);
    const int32_t n = rel[kGroups];
    if (n > kSmallReads) return;   // (the host sends such a locus to k_mi_large)
    int32_t* const val = s_val[w];
    int32_t* const first = s_first[w];
    int32_t* const tval = s_tval[w];
    int32_t* const tcnt = s_tcnt[w];
    for (int32_t e = lane; e < n; e += 64) val[e] = a.cn[base + e];
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    for (int32_t e = lane; e < n; e += 64) {
        const int32_t v = val[e];
        int32_t seen = 0;
        for (int32_t f = 0; f < e; ++f) seen |= val[f] == v ? 1 : 0;
        first[e] = seen ? 0 : 1;
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    int32_t n_first = 0;
    for (int32_t e = lane; e < n; e += 64) n_first += first[e];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n_first += __shfl_xor(n_first, d, 64);
    for (int32_t k = lane; k < n_first * kGroups; k += 64) tcnt[k] = 0;
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    for (int32_t e = lane; e < n; e += 64) {
        const int32_t v = val[e];
        int32_t d = 0;
        for (int32_t f = 0; f < n; ++f) d += (first[f] && val[f] < v) ? 1 : 0;
        int g = 0;
        for (int k = 1; k < kGroups; ++k) g += e >= rel[k] ? 1 : 0;
        if (first[e]) tval[d] = v;
        atomicAdd(&tcnt[d * kGroups + g], 1);
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    int64_t ng[kGroups];
    for (int g = 0; g < kGroups; ++g) ng[g] = rel[g + 1] - rel[g];
    const int64_t cap = exact_entries(ng);
    device_finish(a, l, Table{tval, tcnt, n_first}, reinterpret_cast<U128*>(a.ws + a.ws_off[l]), cap, lane);
}

// One workgroup per locus, list[blockIdx.x] = the locus.  The workspace of the locus: keys (value << 3 | group, padded with
// all-ones to a power of two), the table's values, the table's counts, the exact workspaces (large_part_bytes, locus_ws_bytes).
// A bitonic sort of the keys in place, the first occurrences counted per chunk of consecutive keys (one chunk per thread) and
// scanned by thread 0, then every thread writes its chunk's part of the table.  Wave 0 does the statistics.
__global__ void __launch_bounds__(256) k_mi_large(Args a, const int32_t* list) {
    __shared__ int32_t s_heads[256], s_total;
    const int tid = threadIdx.x;
    const int64_t l = list[blockIdx.x];
    if (tid == 0) write_respects(a, l);
    if (a.test == kTestNone) return;
    const int64_t* off = a.grp_off + 6 * l;
    const int64_t base = off[0], n = off[kGroups] - base, P = pow2_at_least(n);
    char* const ws = a.ws + a.ws_off[l];
    uint64_t* const keys = reinterpret_cast<uint64_t*>(ws);
    int32_t* const tval = reinterpret_cast<int32_t*>(ws + round256(P * 8));
    int32_t* const tcnt = reinterpret_cast<int32_t*>(ws + round256(P * 8) + round256(n * 4));
    U128* const exact = reinterpret_cast<U128*>(ws + large_part_bytes(n));
    for (int64_t e = tid; e < P; e += 256) {
        uint64_t key = ~0ull;
        if (e < n) {
            int g = 0;
            for (int k = 1; k < kGroups; ++k) g += e >= off[k] - base ? 1 : 0;
            key = (uint64_t)(uint32_t)a.cn[base + e] << 3 | (uint64_t)g;
        }
        keys[e] = key;
    }
    for (int64_t e = tid; e < n * kGroups; e += 256) tcnt[e] = 0;
    __syncthreads();
    for (int64_t k = 2; k <= P; k <<= 1)
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t e = tid; e < P; e += 256) {
                const int64_t o = e ^ j;
                if (o > e) {
                    const uint64_t x = keys[e], y = keys[o];
                    if (((e & k) == 0) == (x > y)) { keys[e] = y; keys[o] = x; }
                }
            }
            __syncthreads();
        }
    const int64_t chunk = (P + 255) / 256, e0 = min64(n, tid * chunk), e1 = min64(n, e0 + chunk);
    int32_t heads = 0;
    for (int64_t e = e0; e < e1; ++e) heads += (e == 0 || (keys[e] >> 3) != (keys[e - 1] >> 3)) ? 1 : 0;
    s_heads[tid] = heads;
    __syncthreads();
    if (tid == 0) {
        int32_t run = 0;
        for (int k = 0; k < 256; ++k) { const int32_t h = s_heads[k]; s_heads[k] = run; run += h; }
        s_total = run;
    }
    __syncthreads();
    int32_t d = s_heads[tid];   // first occurrences in front of the chunk
    for (int64_t e = e0; e < e1; ++e) {
        const uint64_t key = keys[e];
        if (e == 0 || (key >> 3) != (keys[e - 1] >> 3)) tval[d++] = (int32_t)(key >> 3);
        atomicAdd(&tcnt[(size_t)(d - 1) * kGroups + (key & 7u)], 1);
    }
    __syncthreads();
    if (tid >= 64) return;
    int64_t ng[kGroups];
    for (int g = 0; g < kGroups; ++g) ng[g] = off[g + 1] - off[g];
    device_finish(a, l, Table{tval, tcnt, s_total}, exact, exact_entries(ng), tid);
}

}  // namespace strk_mi
#endif
