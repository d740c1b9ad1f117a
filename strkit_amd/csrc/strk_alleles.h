// strk_alleles.h — allele calling on gfx950: bootstrapped GMM genotypes per locus, one to six alleles.
//
// Replaces STRkit's call_alleles (strkit/call/allele.py:176-336, gmm.py) and the distance-based peak assignment of
// call_locus.py:1536-1600, restated with one specified random stream (the CPU restatement that the tests
// compare against is tests/alleles_restatement.py; for more than two alleles DESIGN.md §15 and tests/alleles_n_restatement.py).
//
// k_alleles_w<W>: one workgroup per locus, rows of W allele slots per locus.  k_alleles = k_alleles_w<2> (strk_call_alleles, and
// the groups of strk_call_alleles_phased as single-allele loci), k_alleles_n = k_alleles_w<kMaxAlleles> (strk_call_alleles_n).
//   1. the locus's sorted distinct copy numbers v[0..d) and each read's index into them (O(n^2) over the block);
//   2. thread 0 forms the weight CDF (sequential sum, as numpy's cumsum);
//   3. lane b owns bootstrap b (b = tid, tid + blockDim, ...): its n draws as a count row over v (uint16, column-major
//      [k][b] so that the lanes of a wave touch consecutive words), then its whole fit, which loops over the d distinct
//      values, not the n reads — lanes leave EM at their own iteration counts.  The fit is a GMM of c = n_alleles
//      components whose useless components are removed round by round (strkit/call/allele.py:78-123), then filled up to
//      n_alleles again by a weighted draw (:276-288).  k-means++ and EM are templates on the component count, fully
//      unrolled, so that a lane's component state (mean, var, weight and the E-step sums of up to six components) stays in
//      registers under compile-time indices; the reduction loop dispatches on c with a switch.  What is indexed by a
//      run-time value lies in the workspace (rows bm/bw/bs[a][b]) or in LDS (thread 0's per-allele results);
//   4. per allele row: a stable rank sort over the B bootstrap means, the percentiles and the median (thread 0);
//   5. thread 0 assigns the reads to the peaks in read order (the rule is order-dependent).
// Everything is float64; the library builds with -ffp-contract=off, so no step is fused.
// The per-locus workspace (CDF, distinct values, count rows, per-bootstrap results) lies in global memory at
// ws + ws_off[locus]; its layout is AlleleWs, sized on the host by allele_ws_bytes().
// For n_alleles <= 2 the two instantiations run the same operations in the same order: the results are the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace strk {

constexpr int kAlleleMaxBootstrap = 1024;
constexpr int kAlleleMaxInit = 15;
constexpr int kAlleleMaxReads = 65535;   // count rows are uint16
constexpr int kMaxAlleles = 6;
// The per-locus rows of k_alleles_w<W>.  Ints: status, modal_n, call[W], ci95[W][2], ci99[W][2], peak_n_reads[2]; doubles:
// means[W], weights[W], stdevs[W].
template <int W>
struct AlleleRow {
    static constexpr int kCall = 2, kCi95 = 2 + W, kCi99 = 2 + 3 * W, kPeak = 2 + 5 * W, kOutI = 2 + 5 * W + 2, kOutD = 3 * W;
};
constexpr int kAlleleOutI = AlleleRow<2>::kOutI, kAlleleOutD = AlleleRow<2>::kOutD;   // 14 and 6: the rows of k_alleles
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr double kEps64 = 2.220446049250313e-16;
constexpr double kEps32 = 1.1920928955078125e-07;
constexpr double kLog2Pi = 1.8378770664093453;
constexpr double kSmallAlleleMin = 8.0;   // allele.py:46

struct AlleleArgs {
    const int32_t* read_off;     // [n_loci + 1], relative to cn / w / read_peak
    const int32_t* cn;
    const double* w;
    const int32_t* n_alleles;
    const uint64_t* seed;
    const int64_t* ws_off;       // bytes into ws per locus
    char* ws;
    int32_t* out_i;              // [n_loci][AlleleRow<W>::kOutI]
    double* out_d;               // [n_loci][AlleleRow<W>::kOutD]
    int32_t* read_peak;          // [n_reads]
    int32_t n_loci;
    int32_t min_reads, min_allele_reads, B, n_init, max_iter, filter_factor, force_gm_filter;
    double tol, reg_covar, expansion_ratio;
};

__host__ __device__ inline size_t allele_align(size_t x) { return (x + 15) & ~(size_t)15; }

// workspace of one locus of n reads with B bootstraps and `rows` allele rows (k_alleles: 2; k_alleles_n: the locus's n_alleles)
struct AlleleWs {
    double *cdf, *v, *bm, *bw, *bs, *srt;   // cdf[n], v[n], bm/bw/bs[rows][B], srt[B]
    int32_t *didx, *flag, *kb, *perm;       // didx[n], flag[n], kb[B], perm[B]
    uint16_t* cnt;                          // cnt[k * B + b], k < d <= n
};

__host__ __device__ inline size_t allele_ws_layout(char* base, int n, int B, int rows, AlleleWs* ws) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base + o; o += allele_align(bytes); return p; };
    char* cdf = take(8 * (size_t)n);
    char* v = take(8 * (size_t)n);
    char* bm = take(8 * (size_t)rows * (size_t)B);
    char* bw = take(8 * (size_t)rows * (size_t)B);
    char* bs = take(8 * (size_t)rows * (size_t)B);
    char* srt = take(8 * (size_t)B);
    char* didx = take(4 * (size_t)n);
    char* flag = take(4 * (size_t)n);
    char* kb = take(4 * (size_t)B);
    char* perm = take(4 * (size_t)B);
    char* cnt = take(2 * (size_t)B * (size_t)n);
    if (ws) {
        ws->cdf = reinterpret_cast<double*>(cdf);
        ws->v = reinterpret_cast<double*>(v);
        ws->bm = reinterpret_cast<double*>(bm);
        ws->bw = reinterpret_cast<double*>(bw);
        ws->bs = reinterpret_cast<double*>(bs);
        ws->srt = reinterpret_cast<double*>(srt);
        ws->didx = reinterpret_cast<int32_t*>(didx);
        ws->flag = reinterpret_cast<int32_t*>(flag);
        ws->kb = reinterpret_cast<int32_t*>(kb);
        ws->perm = reinterpret_cast<int32_t*>(perm);
        ws->cnt = reinterpret_cast<uint16_t*>(cnt);
    }
    return (o + 255) & ~(size_t)255;
}

inline size_t allele_ws_bytes(int n, int B, int rows) { return allele_ws_layout(nullptr, n, B, rows, nullptr); }

__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// U(s, b, i, j) of the specified stream (key = mix64(seed))
__device__ inline double allele_unif(uint64_t key, uint64_t s, uint64_t b, uint64_t i, uint64_t j) {
    const uint64_t ctr = (s << 60) | (b << 40) | (i << 36) | j;
    return (double)(mix64(key + kGolden * (1 + ctr)) >> 11) * 0x1.0p-53;
}

// sklearn's spherical _estimate_log_gaussian_prob (expanded form) + log weight, for one component
__device__ inline double allele_wlp(double x, double x2, double mean, double pc, double lw) {
    const double prec = pc * pc;
    const double lp = mean * mean * prec - 2.0 * (x * (mean * prec)) + x2 * prec;
    return -0.5 * (kLog2Pi + lp) + log(pc) + lw;
}

template <int C>
struct FitC {
    double mean[C], var[C], w[C], lb;
};

// k-means++ seeds of init `init` in reduction round r (sklearn's _kmeans_plusplus, C clusters, 2 + floor(ln C) local
// trials), as values.  minD^2 of a value is formed anew from the centres chosen so far: the minimum of the same squares
// that sklearn's running np.minimum keeps.
template <int C>
__device__ inline void allele_kmeanspp_c(const uint16_t* cnt, int B, const double* v, int d, int m, uint64_t key, int b,
                                         int init, int r, double (&ctr)[C]) {
    constexpr int T = C == 2 ? 2 : 3;
    double f = floor(allele_unif(key, 1, b, init, 64 * r) * (double)m);
    if (f > (double)(m - 1)) f = (double)(m - 1);
    const int s0 = (int)f;
    int k0 = d - 1;
    for (int k = 0, cum = 0; k < d; ++k) {
        cum += cnt[(size_t)k * B];
        if (cum > s0) { k0 = k; break; }
    }
    ctr[0] = v[k0];
#pragma unroll
    for (int q = 1; q < C; ++q) {
        auto min_d2 = [&](double x) {
            const double d0 = x - ctr[0];
            double md = d0 * d0;
#pragma unroll
            for (int e = 1; e < q; ++e) {
                const double de = x - ctr[e];
                md = fmin(md, de * de);
            }
            return md;
        };
        double pot = 0.0;
        for (int k = 0; k < d; ++k) pot = pot + (double)cnt[(size_t)k * B] * min_d2(v[k]);
        double best_v = 0.0, best_pot = 0.0;
        for (int t = 0; t < T; ++t) {
            const double target = allele_unif(key, 1, b, init, 64 * r + 8 * (q - 1) + 1 + t) * pot;
            int kc = d - 1;
            double s = 0.0;
            for (int k = 0; k < d; ++k) {
                const int c = cnt[(size_t)k * B];
                s = s + (double)c * min_d2(v[k]);
                if (c > 0 && s >= target) { kc = k; break; }
            }
            const double vc = v[kc];
            double cp = 0.0;
            for (int k = 0; k < d; ++k) {
                const double dc = v[k] - vc;
                cp = cp + (double)cnt[(size_t)k * B] * fmin(min_d2(v[k]), dc * dc);
            }
            if (t == 0 || cp < best_pot) { best_v = vc; best_pot = cp; }
        }
        ctr[q] = best_v;
    }
}

// EM of a C-component spherical GMM from seed values s (sklearn 1.7 GaussianMixture.fit with one init); sums over the
// components run in index order
template <int C>
__device__ inline FitC<C> allele_em_c(const uint16_t* cnt, int B, const double* v, int d, int m, const double (&s)[C],
                                      const AlleleArgs& a) {
    FitC<C> f;
    const double nk_init = 1.0 + 10.0 * kEps64;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        f.mean[j] = s[j] / nk_init;
        f.var[j] = (s[j] * s[j]) / nk_init - f.mean[j] * f.mean[j] + a.reg_covar;
        f.w[j] = nk_init / (double)m;
    }
    f.lb = -INFINITY;
    for (int it = 1; it <= a.max_iter; ++it) {
        double pc[C], lw[C], nk[C], sx[C], sxx[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            pc[j] = 1.0 / sqrt(f.var[j]);
            lw[j] = log(f.w[j]);
            nk[j] = sx[j] = sxx[j] = 0.0;
        }
        double lbs = 0.0;
        for (int k = 0; k < d; ++k) {
            const int c = cnt[(size_t)k * B];
            if (c == 0) continue;
            const double cf = (double)c, x = v[k], x2 = x * x;
            double wl[C];
#pragma unroll
            for (int j = 0; j < C; ++j) wl[j] = allele_wlp(x, x2, f.mean[j], pc[j], lw[j]);
            double mx = wl[0];
#pragma unroll
            for (int j = 1; j < C; ++j) mx = fmax(mx, wl[j]);
            double se = exp(wl[0] - mx);
#pragma unroll
            for (int j = 1; j < C; ++j) se = se + exp(wl[j] - mx);
            const double lse = mx + log(se);
            lbs = lbs + cf * lse;
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const double cr = cf * exp(wl[j] - lse);
                nk[j] = nk[j] + cr;
                sx[j] = sx[j] + cr * x;
                sxx[j] = sxx[j] + cr * x2;
            }
        }
        const double new_lb = lbs / (double)m;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            nk[j] = nk[j] + 10.0 * kEps64;
            f.mean[j] = sx[j] / nk[j];
            f.var[j] = sxx[j] / nk[j] - f.mean[j] * f.mean[j] + a.reg_covar;
        }
        double tot = nk[0];
#pragma unroll
        for (int j = 1; j < C; ++j) tot = tot + nk[j];
#pragma unroll
        for (int j = 0; j < C; ++j) f.w[j] = nk[j] / tot;
        const double change = new_lb - f.lb;
        f.lb = new_lb;
        if (fabs(change) < a.tol) break;
    }
    return f;
}

__device__ inline void allele_single(const uint16_t* cnt, int B, const double* v, int d, int m, double* mean, double* var) {
    double s = 0.0;
    for (int k = 0; k < d; ++k) s = s + (double)cnt[(size_t)k * B] * v[k];
    const double mu = s / (double)m;
    double q = 0.0;
    for (int k = 0; k < d; ++k) {
        const double dv = v[k] - mu;
        q = q + (double)cnt[(size_t)k * B] * (dv * dv);
    }
    *mean = mu;
    *var = q / (double)m;
}

// One round of fit_gmm's loop (allele.py:85-121) with C components: the best fit over n_init inits of reduction round r
// into `out` (through a local, copied once: see the register counts at allele_fit_bootstrap); returns the number of useless
// components.
template <int C>
__device__ inline int allele_fit_c(const uint16_t* cnt, int B, const double* v, int d, int m, uint64_t key, int b, int r,
                                   const AlleleArgs& a, FitC<C>& out) {
    FitC<C> best;
    best.lb = -INFINITY;
    for (int i = 0; i < a.n_init; ++i) {
        double ctr[C];
        allele_kmeanspp_c<C>(cnt, B, v, d, m, key, b, i, r, ctr);
        const FitC<C> f = allele_em_c<C>(cnt, B, v, d, m, ctr, a);
        if (i == 0 || f.lb > best.lb || best.lb == -INFINITY) best = f;
    }
    const double allele_filter = ((double)a.min_allele_reads - 0.1) / (double)B;
    bool strict = true;
    if (C == 2) {
        const bool sw = best.mean[1] < best.mean[0];
        const double lo = sw ? best.mean[1] : best.mean[0], hi = sw ? best.mean[0] : best.mean[1];
        strict = a.force_gm_filter != 0 || hi < a.expansion_ratio * fmax(lo, kSmallAlleleMin);
    }
    const double thr = strict ? 1.0 / (double)(a.filter_factor * C) : kEps32;
    int ok = 0;
#pragma unroll
    for (int j = 0; j < C; ++j) ok += (best.w[j] > allele_filter && best.w[j] > thr) ? 1 : 0;
    out = best;
    return C - ok;
}

// allele_fit_c into rows 0 .. C-1 of bm (means), bs (variances) and bw (weights) of bootstrap b
template <int C>
__device__ inline int allele_fit_rows(const AlleleWs& ws, int B, int d, int m, uint64_t key, int b, int r, const AlleleArgs& a) {
    FitC<C> best;
    const int nu = allele_fit_c<C>(ws.cnt + b, B, ws.v, d, m, key, b, r, a, best);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        ws.bm[(size_t)j * B + b] = best.mean[j];
        ws.bs[(size_t)j * B + b] = best.var[j];
        ws.bw[(size_t)j * B + b] = best.w[j];
    }
    return nu;
}

// stable sort of the first `count` components of bootstrap b by mean (insertion: an element moves only past a strictly
// larger mean)
__device__ inline void allele_sort_by_mean(const AlleleWs& ws, int B, int b, int count) {
    for (int i = 1; i < count; ++i) {
        const double xm = ws.bm[(size_t)i * B + b], xw = ws.bw[(size_t)i * B + b], xs = ws.bs[(size_t)i * B + b];
        int j = i;
        while (j > 0 && xm < ws.bm[(size_t)(j - 1) * B + b]) {
            ws.bm[(size_t)j * B + b] = ws.bm[(size_t)(j - 1) * B + b];
            ws.bw[(size_t)j * B + b] = ws.bw[(size_t)(j - 1) * B + b];
            ws.bs[(size_t)j * B + b] = ws.bs[(size_t)(j - 1) * B + b];
            --j;
        }
        ws.bm[(size_t)j * B + b] = xm;
        ws.bw[(size_t)j * B + b] = xw;
        ws.bs[(size_t)j * B + b] = xs;
    }
}

// one bootstrap sample (fit_gmm, allele.py:57-123, the fill-up of :276-288 and the sort by mean); writes
// bm/bw/bs[a * B + b] for a < A and kb[b].  Components above W are compiled out.
template <int W>
__device__ inline void allele_fit_bootstrap(const AlleleWs& ws, int B, int d, int m, int A, uint64_t key, int b,
                                            const AlleleArgs& a) {
    const uint16_t* cnt = ws.cnt + b;
    int nz = 0;
    for (int k = 0; k < d && nz < 2; ++k) nz += cnt[(size_t)k * B] > 0;
    int kk = 1;
    [[maybe_unused]] FitC<2> two;   // W == 2: the one fit there is, kept in registers
    if (A > 1 && nz > 1) {
        // a round removes at least one component, so W - 1 rounds reach c == 1 (and with two slots the loop is one trip)
        for (int c = A, r = 0; r < W - 1 && c > 1; ++r) {
            int nu;
            if constexpr (W == 2) {
                nu = allele_fit_c<2>(cnt, B, ws.v, d, m, key, b, r, a, two);
            } else {
                switch (c) {
                    case 2: nu = allele_fit_rows<2>(ws, B, d, m, key, b, r, a); break;
                    case 3: nu = allele_fit_rows<3>(ws, B, d, m, key, b, r, a); break;
                    case 4: nu = allele_fit_rows<4>(ws, B, d, m, key, b, r, a); break;
                    case 5: nu = allele_fit_rows<5>(ws, B, d, m, key, b, r, a); break;
                    default: nu = allele_fit_rows<6>(ws, B, d, m, key, b, r, a); break;
                }
            }
            if (nu == 0 || c - nu <= 0) { kk = c; break; }   // none useless: keep; all useless: the loop ends with this fit
            c -= nu;
        }
    }
    if constexpr (W == 2) {
        // The finish for two slots: both components in registers, stored once in the order of their means.  The same values
        // as the general finish below gives (a single component fills slot 1 with itself: the draw can only pick it).
        // Through the general finish k_alleles_w<2> takes 148 VGPRs and runs 3 waves per SIMD; with this one 128 and 4
        // (hipcc -O3 -Rpass-analysis=kernel-resource-usage; allele_fit_c's local `best` is part of that: fitting into the
        // caller's struct directly costs the same 20 registers).
        double mean[2], var[2], w[2] = {1.0, 1.0};
        if (kk == 2) {
            for (int j = 0; j < 2; ++j) { mean[j] = two.mean[j]; var[j] = two.var[j]; w[j] = two.w[j]; }
        } else {
            allele_single(cnt, B, ws.v, d, m, &mean[0], &var[0]);
            mean[1] = mean[0];
            var[1] = var[0];
        }
        const double sd[2] = {sqrt(var[0]), sqrt(var[1])};
        const int o0 = mean[1] < mean[0] ? 1 : 0, o1 = 1 - o0;
        ws.bm[b] = mean[o0];
        ws.bm[B + b] = mean[o1];
        ws.bw[b] = w[o0];
        ws.bw[B + b] = w[o1];
        ws.bs[b] = sd[o0];
        ws.bs[B + b] = sd[o1];
    } else {
        if (kk == 1) {
            double mean, var;
            allele_single(cnt, B, ws.v, d, m, &mean, &var);
            ws.bm[b] = mean;
            ws.bs[b] = var;
            ws.bw[b] = 1.0;
        }
        for (int j = 0; j < kk; ++j) ws.bs[(size_t)j * B + b] = sqrt(ws.bs[(size_t)j * B + b]);
        if (kk < A) {
            // the kept components in the order of their means first: the draw must not rest on how an init labelled them
            allele_sort_by_mean(ws, B, b, kk);
            // rng.choice(k, size = A - k, p = w / sum |w|): a uniform against the CDF, divided by its last entry
            double tot = 0.0;
            for (int j = 0; j < kk; ++j) tot = tot + fabs(ws.bw[(size_t)j * B + b]);
            double last = 0.0;
            for (int j = 0; j < kk; ++j) last = last + ws.bw[(size_t)j * B + b] / tot;
            for (int t = 0; t < A - kk; ++t) {
                const double u = allele_unif(key, 2, b, 0, t);
                int pick = 0;
                double cum = 0.0;
                for (int j = 0; j < kk; ++j) {
                    cum = cum + ws.bw[(size_t)j * B + b] / tot;
                    pick += (cum / last <= u) ? 1 : 0;
                }
                if (pick > kk - 1) pick = kk - 1;
                ws.bm[(size_t)(kk + t) * B + b] = ws.bm[(size_t)pick * B + b];
                ws.bw[(size_t)(kk + t) * B + b] = ws.bw[(size_t)pick * B + b];
                ws.bs[(size_t)(kk + t) * B + b] = ws.bs[(size_t)pick * B + b];
            }
        }
        allele_sort_by_mean(ws, B, b, A);
    }
    ws.kb[b] = kk;
}

// the order of numpy's stable argsort: NaN after every number, NaNs equal among themselves.  A total order, so the
// ranks of a row are a permutation even if a mean is NaN.
__device__ inline bool allele_before(double y, double x) { return y < x || (isnan(x) && !isnan(y)); }
__device__ inline bool allele_same(double y, double x) { return y == x || (isnan(x) && isnan(y)); }

// np.percentile(sorted, pct, method="interpolated_inverted_cdf")
__device__ inline double allele_pct(const double* s, int n, double pct) {
    const double q = pct / 100.0;
    const double vi = (double)n * q - 1.0;
    if (vi >= (double)(n - 1)) return s[n - 1];
    if (vi < 0.0) return s[0];
    const double prev = floor(vi);
    const double g = vi - prev;
    const int i = (int)prev;
    const double lo = s[i], hi = s[i + 1], diff = hi - lo;
    return g >= 0.5 ? hi - diff * (1.0 - g) : lo + diff * g;
}

template <int W>
__global__ void __launch_bounds__(256) k_alleles_w(AlleleArgs a) {
    static_assert(W >= 2 && W <= kMaxAlleles, "the reduction loop dispatches on 2 .. 6 components");
    using R = AlleleRow<W>;
    const int l = blockIdx.x;
    if (l >= a.n_loci) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int r0 = a.read_off[l], n = a.read_off[l + 1] - r0;
    const int32_t* cn = a.cn + r0;
    int32_t* oi = a.out_i + (size_t)l * R::kOutI;
    double* od = a.out_d + (size_t)l * R::kOutD;
    int32_t* rp = a.read_peak + r0;
    const int A = a.n_alleles[l];
    const int B = a.B;
    __shared__ int s_d;
    __shared__ double s_total;
    // the per-allele results (in LDS: they are indexed by the allele, a run-time value)
    __shared__ double mean_out[W], w_out[W], sd_out[W];
    __shared__ int s_kc[W + 1];

    if (n < a.min_reads) {
        for (int j = tid; j < n; j += nt) rp[j] = -1;
        if (tid < R::kOutI) oi[tid] = tid == 0 ? 1 : (tid == 1 || tid >= R::kPeak) ? 0 : -1;
        if (tid < R::kOutD) od[tid] = NAN;
        return;
    }
    AlleleWs ws;
    allele_ws_layout(a.ws + a.ws_off[l], n, B, W == 2 ? 2 : A, &ws);

    // 1. distinct values: flag the first occurrence of each value, then rank the flagged ones
    if (tid == 0) s_d = 0;
    if (tid < W) mean_out[tid] = w_out[tid] = sd_out[tid] = NAN;
    if (tid >= 2 && tid < R::kPeak) oi[tid] = -1;
    __syncthreads();
    for (int j = tid; j < n; j += nt) {
        const int x = cn[j];
        int first = 1;
        for (int q = 0; q < j; ++q)
            if (cn[q] == x) { first = 0; break; }
        ws.flag[j] = first;
        if (first) atomicAdd(&s_d, 1);
    }
    __syncthreads();
    const int d = s_d;
    if (d > 1 && n < A) {   // sklearn refuses n_samples < n_components
        for (int j = tid; j < n; j += nt) rp[j] = -1;
        if (tid < 2 || (tid >= R::kPeak && tid < R::kOutI)) oi[tid] = tid == 0 ? 1 : 0;
        if (tid < R::kOutD) od[tid] = NAN;
        return;
    }
    for (int j = tid; j < n; j += nt) {
        const int x = cn[j];
        int di = 0;
        for (int q = 0; q < n; ++q) di += (ws.flag[q] && cn[q] < x) ? 1 : 0;
        ws.didx[j] = di;
        if (ws.flag[j]) ws.v[di] = (double)x;
    }
    // 2. CDF of the weights
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) {
            s = s + a.w[r0 + j];
            ws.cdf[j] = s;
        }
        s_total = s;
    }
    __syncthreads();
    int modal_n = 1;

    if (d == 1) {   // one value
        if (tid < A) {
            oi[R::kCall + tid] = cn[0];
            for (int e = 0; e < 2; ++e) {
                oi[R::kCi95 + 2 * tid + e] = cn[0];
                oi[R::kCi99 + 2 * tid + e] = cn[0];
            }
            mean_out[tid] = (double)cn[0];
            w_out[tid] = 1.0 / (double)A;
            sd_out[tid] = 0.0;
        }
        __syncthreads();
    } else {
        const double total = s_total;
        for (int j = tid; j < n; j += nt) ws.cdf[j] = ws.cdf[j] / total;
        __syncthreads();
        const uint64_t key = mix64(a.seed[l]);
        // 3. resampling + one fit per lane
        for (int b = tid; b < B; b += nt) {
            uint16_t* row = ws.cnt + b;
            for (int k = 0; k < d; ++k) row[(size_t)k * B] = 0;
            for (int j = 0; j < n; ++j) {
                const double u = allele_unif(key, 0, b, 0, j);
                int lo = 0, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ws.cdf[mid] <= u) lo = mid + 1; else hi = mid;
                }
                if (lo > n - 1) lo = n - 1;
                row[(size_t)ws.didx[lo] * B] += 1;
            }
            allele_fit_bootstrap<W>(ws, B, d, n, A, key, b, a);
        }
        __syncthreads();
        // 4. per allele row: stable rank sort, percentiles, median
        for (int al = 0; al < A; ++al) {
            const double* row = ws.bm + (size_t)al * B;
            for (int b = tid; b < B; b += nt) {
                const double x = row[b];
                int r = 0;
                for (int q = 0; q < B; ++q) {
                    const double y = row[q];
                    r += (allele_before(y, x) || (allele_same(y, x) && q < b)) ? 1 : 0;
                }
                ws.srt[r] = x;
                ws.perm[r] = b;
            }
            __syncthreads();
            if (tid == 0) {
                const int mid = B / 2;
                oi[R::kCall + al] = (int32_t)rint(ws.srt[mid]);
                oi[R::kCi95 + 2 * al] = (int32_t)rint(allele_pct(ws.srt, B, 2.5));
                oi[R::kCi95 + 2 * al + 1] = (int32_t)rint(allele_pct(ws.srt, B, 97.5));
                oi[R::kCi99 + 2 * al] = (int32_t)rint(allele_pct(ws.srt, B, 0.5));
                oi[R::kCi99 + 2 * al + 1] = (int32_t)rint(allele_pct(ws.srt, B, 99.5));
                mean_out[al] = ws.srt[mid];
                w_out[al] = ws.bw[(size_t)al * B + ws.perm[mid]];
                sd_out[al] = ws.bs[(size_t)al * B + ws.perm[mid]];
            }
            __syncthreads();
        }
        if (tid == 0) {
            // the most frequent number of peaks, the smaller one on ties
            for (int k = 0; k <= W; ++k) s_kc[k] = 0;
            for (int b = 0; b < B; ++b) s_kc[ws.kb[b]] += 1;
            for (int k = 2; k <= W; ++k)
                if (s_kc[k] > s_kc[modal_n]) modal_n = k;
            double tot = w_out[0];
            for (int al = 1; al < A; ++al) tot = tot + w_out[al];
            for (int al = 0; al < A; ++al) w_out[al] = w_out[al] / tot;
        }
    }
    if (tid != 0) return;
    for (int al = 0; al < W; ++al) {
        od[al] = mean_out[al];
        od[W + al] = w_out[al];
        od[2 * W + al] = sd_out[al];
    }
    oi[1] = modal_n;
    if (W > 2 && modal_n > 2) {   // call_locus.py: "We cannot call read-level cluster labels with >2 peaks"
        for (int j = 0; j < n; ++j) rp[j] = -1;
        oi[0] = 0;
        oi[R::kPeak] = oi[R::kPeak + 1] = 0;
        return;
    }
    // 5. peak assignment in read order (call_locus.py:1536-1600) on the first modal_n rows
    double sd[2] = {sd_out[0], modal_n == 2 ? sd_out[1] : 1.0};
    if (sd[0] == 0.0 || (modal_n == 2 && sd[1] == 0.0)) {
        sd[0] = sd[0] + 0.00001;
        sd[1] = sd[1] + 0.00001;
    }
    const double pc[2] = {1.0 / sd[0], 1.0 / sd[1]};
    const double lw[2] = {log(w_out[0]), modal_n == 2 ? log(w_out[1]) : 0.0};
    const double m0 = mean_out[0], m1 = mean_out[1];
    int cnt[2] = {0, 0};
    for (int j = 0; j < n; ++j) {
        const double x = (double)cn[j];
        int pk = 0;
        if (modal_n == 2) {
            if (fabs((m0 - x) / sd[0]) < 1.0 && fabs((m1 - x) / sd[1]) < 1.0) {
                pk = cnt[0] > cnt[1] ? 1 : 0;
            } else {
                const double x2 = x * x;
                const double l0 = allele_wlp(x, x2, m0, pc[0], lw[0]);
                const double l1 = allele_wlp(x, x2, m1, pc[1], lw[1]);
                pk = l1 > l0 ? 1 : 0;
            }
        }
        rp[j] = pk;
        cnt[pk] += 1;
    }
    oi[0] = (cnt[0] == 0 || (modal_n == 2 && cnt[1] == 0)) ? 2 : 0;
    oi[R::kPeak] = cnt[0];
    oi[R::kPeak + 1] = cnt[1];
}

constexpr auto k_alleles = k_alleles_w<2>;
constexpr auto k_alleles_n = k_alleles_w<kMaxAlleles>;

}  // namespace strk
