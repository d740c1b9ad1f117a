// strk_alleles.h — allele calling on gfx950: bootstrapped two-component GMM genotypes per locus.
//
// Replaces STRkit's call_alleles (strkit/call/allele.py:176-336, gmm.py) and the distance-based peak assignment of
// call_locus.py:1536-1600, restated with one specified random stream (the CPU restatement that the tests
// compare against is tests/alleles_restatement.py).
//
// k_alleles: one workgroup per locus.
//   1. the locus's sorted distinct copy numbers v[0..d) and each read's index into them (O(n^2) over the block);
//   2. thread 0 forms the weight CDF (sequential sum, as numpy's cumsum);
//   3. lane b owns bootstrap b (b = tid, tid + blockDim, ...): its n draws as a count row over v (uint16, column-major
//      [k][b] so that the lanes of a wave touch consecutive words), then its whole fit, which loops over the d distinct
//      values, not the n reads — lanes leave EM at their own iteration counts;
//   4. per allele row: a stable rank sort over the B bootstrap means, the percentiles and the median (thread 0);
//   5. thread 0 assigns the reads to the peaks in read order (the rule is order-dependent).
// Everything is float64; the library builds with -ffp-contract=off, so no step is fused.
// The per-locus workspace (CDF, distinct values, count rows, per-bootstrap results) lies in global memory at
// ws + ws_off[locus]; its layout is AlleleWs, sized on the host by allele_ws_bytes().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace strk {

constexpr int kAlleleMaxBootstrap = 1024;
constexpr int kAlleleMaxInit = 15;
constexpr int kAlleleMaxReads = 65535;   // count rows are uint16
constexpr int kAlleleOutI = 14;          // per locus: status, modal_n, call[2], ci95[4], ci99[4], peak_n_reads[2]
constexpr int kAlleleOutD = 6;           // per locus: means[2], weights[2], stdevs[2]
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
    int32_t* out_i;              // [n_loci][kAlleleOutI]
    double* out_d;               // [n_loci][kAlleleOutD]
    int32_t* read_peak;          // [n_reads]
    int32_t n_loci;
    int32_t min_reads, min_allele_reads, B, n_init, max_iter, filter_factor, force_gm_filter;
    double tol, reg_covar, expansion_ratio;
};

__host__ __device__ inline size_t allele_align(size_t x) { return (x + 15) & ~(size_t)15; }

// workspace of one locus of n reads with B bootstraps
struct AlleleWs {
    double *cdf, *v, *bm, *bw, *bs, *srt;   // cdf[n], v[n], bm/bw/bs[2][B], srt[B]
    int32_t *didx, *flag, *kb, *perm;       // didx[n], flag[n], kb[B], perm[B]
    uint16_t* cnt;                          // cnt[k * B + b], k < d <= n
};

__host__ __device__ inline size_t allele_ws_layout(char* base, int n, int B, AlleleWs* ws) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base + o; o += allele_align(bytes); return p; };
    char* cdf = take(8 * (size_t)n);
    char* v = take(8 * (size_t)n);
    char* bm = take(16 * (size_t)B);
    char* bw = take(16 * (size_t)B);
    char* bs = take(16 * (size_t)B);
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

inline size_t allele_ws_bytes(int n, int B) { return allele_ws_layout(nullptr, n, B, nullptr); }

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

struct Fit2 {
    double mean[2], var[2], w[2], lb;
};

// EM of a two-component spherical GMM from seed values s0, s1 (sklearn 1.7 GaussianMixture.fit with one init)
__device__ inline Fit2 allele_em(const uint16_t* cnt, int B, const double* v, int d, int m, double s0, double s1,
                                 const AlleleArgs& a) {
    Fit2 f;
    const double nk_init = 1.0 + 10.0 * kEps64;
    f.mean[0] = s0 / nk_init;
    f.mean[1] = s1 / nk_init;
    f.var[0] = (s0 * s0) / nk_init - f.mean[0] * f.mean[0] + a.reg_covar;
    f.var[1] = (s1 * s1) / nk_init - f.mean[1] * f.mean[1] + a.reg_covar;
    f.w[0] = f.w[1] = nk_init / (double)m;
    f.lb = -INFINITY;
    for (int it = 1; it <= a.max_iter; ++it) {
        double pc[2], lw[2];
        for (int j = 0; j < 2; ++j) {
            pc[j] = 1.0 / sqrt(f.var[j]);
            lw[j] = log(f.w[j]);
        }
        double lbs = 0.0, nk[2] = {0.0, 0.0}, sx[2] = {0.0, 0.0}, sxx[2] = {0.0, 0.0};
        for (int k = 0; k < d; ++k) {
            const int c = cnt[(size_t)k * B];
            if (c == 0) continue;
            const double cf = (double)c, x = v[k], x2 = x * x;
            const double w0 = allele_wlp(x, x2, f.mean[0], pc[0], lw[0]);
            const double w1 = allele_wlp(x, x2, f.mean[1], pc[1], lw[1]);
            const double mx = fmax(w0, w1);
            const double lse = mx + log(exp(w0 - mx) + exp(w1 - mx));
            const double cr0 = cf * exp(w0 - lse), cr1 = cf * exp(w1 - lse);
            lbs = lbs + cf * lse;
            nk[0] = nk[0] + cr0;
            nk[1] = nk[1] + cr1;
            sx[0] = sx[0] + cr0 * x;
            sx[1] = sx[1] + cr1 * x;
            sxx[0] = sxx[0] + cr0 * x2;
            sxx[1] = sxx[1] + cr1 * x2;
        }
        const double new_lb = lbs / (double)m;
        for (int j = 0; j < 2; ++j) {
            nk[j] = nk[j] + 10.0 * kEps64;
            f.mean[j] = sx[j] / nk[j];
            f.var[j] = sxx[j] / nk[j] - f.mean[j] * f.mean[j] + a.reg_covar;
        }
        const double tot = nk[0] + nk[1];
        f.w[0] = nk[0] / tot;
        f.w[1] = nk[1] / tot;
        const double change = new_lb - f.lb;
        f.lb = new_lb;
        if (fabs(change) < a.tol) break;
    }
    return f;
}

// k-means++ seeds of init i (sklearn's _kmeans_plusplus, 2 clusters, 2 local trials), as distinct-value indices
__device__ inline void allele_kmeanspp(const uint16_t* cnt, int B, const double* v, int d, int m, uint64_t key, int b,
                                       int init, int* k0_out, int* k1_out) {
    double f = floor(allele_unif(key, 1, b, init, 0) * (double)m);
    if (f > (double)(m - 1)) f = (double)(m - 1);
    const int s0 = (int)f;
    int k0 = d - 1;
    for (int k = 0, cum = 0; k < d; ++k) {
        cum += cnt[(size_t)k * B];
        if (cum > s0) { k0 = k; break; }
    }
    const double c0 = v[k0];
    double pot = 0.0;
    for (int k = 0; k < d; ++k) {
        const double dd = v[k] - c0;
        pot = pot + (double)cnt[(size_t)k * B] * (dd * dd);
    }
    int best_k = 0;
    double best_pot = 0.0;
    for (int t = 0; t < 2; ++t) {
        const double target = allele_unif(key, 1, b, init, 1 + t) * pot;
        int kc = d - 1;
        double s = 0.0;
        for (int k = 0; k < d; ++k) {
            const int c = cnt[(size_t)k * B];
            const double dd = v[k] - c0;
            s = s + (double)c * (dd * dd);
            if (c > 0 && s >= target) { kc = k; break; }
        }
        const double vc = v[kc];
        double cp = 0.0;
        for (int k = 0; k < d; ++k) {
            const double dd = v[k] - c0, dc = v[k] - vc;
            cp = cp + (double)cnt[(size_t)k * B] * fmin(dd * dd, dc * dc);
        }
        if (t == 0 || cp < best_pot) { best_k = kc; best_pot = cp; }
    }
    *k0_out = k0;
    *k1_out = best_k;
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

// one bootstrap sample (fit_gmm, allele.py:57-123, then step 7); writes bm/bw/bs[a * B + b] and kb[b]
__device__ inline void allele_fit_bootstrap(const AlleleWs& ws, int B, int d, int m, int n_alleles, uint64_t key, int b,
                                            const AlleleArgs& a) {
    const uint16_t* cnt = ws.cnt + b;
    int nz = 0;
    for (int k = 0; k < d && nz < 2; ++k) nz += cnt[(size_t)k * B] > 0;
    double mean[2], w[2] = {1.0, 1.0}, var[2];
    int kk = 1;
    if (n_alleles == 2 && nz > 1) {
        Fit2 best;
        best.lb = -INFINITY;
        for (int i = 0; i < a.n_init; ++i) {
            int k0, k1;
            allele_kmeanspp(cnt, B, ws.v, d, m, key, b, i, &k0, &k1);
            const Fit2 f = allele_em(cnt, B, ws.v, d, m, ws.v[k0], ws.v[k1], a);
            if (i == 0 || f.lb > best.lb || best.lb == -INFINITY) best = f;
        }
        const double allele_filter = ((double)a.min_allele_reads - 0.1) / (double)B;
        const bool sw = best.mean[1] < best.mean[0];
        const double lo = sw ? best.mean[1] : best.mean[0], hi = sw ? best.mean[0] : best.mean[1];
        const bool strict = a.force_gm_filter != 0 || hi < a.expansion_ratio * fmax(lo, kSmallAlleleMin);
        const double thr = strict ? 1.0 / (double)(a.filter_factor * 2) : kEps32;
        int ok = 0;
        for (int j = 0; j < 2; ++j) ok += (best.w[j] > allele_filter && best.w[j] > thr) ? 1 : 0;
        if (ok != 1) {   // 0 useless: keep; 2 useless: the loop ends with the two-component fit
            kk = 2;
            for (int j = 0; j < 2; ++j) { mean[j] = best.mean[j]; var[j] = best.var[j]; w[j] = best.w[j]; }
        }
    }
    if (kk == 1) {
        allele_single(cnt, B, ws.v, d, m, &mean[0], &var[0]);
        mean[1] = mean[0];
        var[1] = var[0];
    }
    double sd[2] = {sqrt(var[0]), sqrt(var[1])};
    int o0 = 0, o1 = 1;
    if (mean[1] < mean[0]) { o0 = 1; o1 = 0; }
    ws.bm[b] = mean[o0];
    ws.bm[B + b] = mean[o1];
    ws.bw[b] = w[o0];
    ws.bw[B + b] = w[o1];
    ws.bs[b] = sd[o0];
    ws.bs[B + b] = sd[o1];
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

__global__ void __launch_bounds__(256) k_alleles(AlleleArgs a) {
    const int l = blockIdx.x;
    if (l >= a.n_loci) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int r0 = a.read_off[l], n = a.read_off[l + 1] - r0;
    const int32_t* cn = a.cn + r0;
    int32_t* oi = a.out_i + (size_t)l * kAlleleOutI;
    double* od = a.out_d + (size_t)l * kAlleleOutD;
    int32_t* rp = a.read_peak + r0;
    const int n_alleles = a.n_alleles[l];
    const int B = a.B;
    __shared__ int s_d;
    __shared__ double s_total;
    // thread 0's per-allele results (in LDS rather than in a dynamically indexed private array, which would go to scratch)
    __shared__ double mean_out[2], w_out[2], sd_out[2];

    if (n < a.min_reads) {
        for (int j = tid; j < n; j += nt) rp[j] = -1;
        if (tid < kAlleleOutI) oi[tid] = tid == 0 ? 1 : (tid == 1 || tid >= 12) ? 0 : -1;
        if (tid < kAlleleOutD) od[tid] = NAN;
        return;
    }
    AlleleWs ws;
    allele_ws_layout(a.ws + a.ws_off[l], n, B, &ws);

    // 1. distinct values: flag the first occurrence of each value, then rank the flagged ones
    if (tid == 0) s_d = 0;
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
    const int d = s_d;
    int modal_n = 1;

    if (d == 1) {   // step 2: one value
        const double x = (double)cn[0];
        modal_n = 1;
        if (tid == 0) {
            for (int al = 0; al < 2; ++al) {
                const bool used = al < n_alleles;
                oi[2 + al] = used ? cn[0] : -1;
                for (int e = 0; e < 2; ++e) {
                    oi[4 + 2 * al + e] = used ? cn[0] : -1;
                    oi[8 + 2 * al + e] = used ? cn[0] : -1;
                }
                mean_out[al] = used ? x : NAN;
                w_out[al] = used ? 1.0 / (double)n_alleles : NAN;
                sd_out[al] = used ? 0.0 : NAN;
            }
        }
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
            allele_fit_bootstrap(ws, B, d, n, n_alleles, key, b, a);
        }
        __syncthreads();
        // 4. per allele row: stable rank sort, percentiles, median
        for (int al = 0; al < n_alleles; ++al) {
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
                oi[2 + al] = (int32_t)rint(ws.srt[mid]);
                oi[4 + 2 * al] = (int32_t)rint(allele_pct(ws.srt, B, 2.5));
                oi[4 + 2 * al + 1] = (int32_t)rint(allele_pct(ws.srt, B, 97.5));
                oi[8 + 2 * al] = (int32_t)rint(allele_pct(ws.srt, B, 0.5));
                oi[8 + 2 * al + 1] = (int32_t)rint(allele_pct(ws.srt, B, 99.5));
                mean_out[al] = ws.srt[mid];
                w_out[al] = ws.bw[(size_t)al * B + ws.perm[mid]];
                sd_out[al] = ws.bs[(size_t)al * B + ws.perm[mid]];
            }
            __syncthreads();
        }
        if (tid == 0) {
            int n1 = 0;
            for (int b = 0; b < B; ++b) n1 += ws.kb[b] == 1;
            modal_n = n1 >= B - n1 ? 1 : 2;
            const double tot = n_alleles == 2 ? w_out[0] + w_out[1] : w_out[0];
            for (int al = 0; al < n_alleles; ++al) w_out[al] = w_out[al] / tot;
            if (n_alleles == 1) {
                oi[3] = -1;
                oi[6] = oi[7] = oi[10] = oi[11] = -1;
                mean_out[1] = w_out[1] = sd_out[1] = NAN;
            }
        }
    }
    if (tid != 0) return;
    // 5. peak assignment in read order (call_locus.py:1536-1600)
    double sd[2] = {sd_out[0], modal_n == 2 ? sd_out[1] : 1.0};
    if (sd[0] == 0.0 || (modal_n == 2 && sd[1] == 0.0)) {
        sd[0] = sd[0] + 0.00001;
        sd[1] = sd[1] + 0.00001;
    }
    const double pc[2] = {1.0 / sd[0], 1.0 / sd[1]};
    const double lw[2] = {log(w_out[0]), modal_n == 2 ? log(w_out[1]) : 0.0};
    int cnt[2] = {0, 0};
    for (int j = 0; j < n; ++j) {
        const double x = (double)cn[j];
        int pk = 0;
        if (modal_n == 2) {
            if (fabs((mean_out[0] - x) / sd[0]) < 1.0 && fabs((mean_out[1] - x) / sd[1]) < 1.0) {
                pk = cnt[0] > cnt[1] ? 1 : 0;
            } else {
                const double x2 = x * x;
                const double l0 = allele_wlp(x, x2, mean_out[0], pc[0], lw[0]);
                const double l1 = allele_wlp(x, x2, mean_out[1], pc[1], lw[1]);
                pk = l1 > l0 ? 1 : 0;
            }
        }
        rp[j] = pk;
        cnt[pk] += 1;
    }
    oi[0] = (cnt[0] == 0 || (modal_n == 2 && cnt[1] == 0)) ? 2 : 0;
    oi[1] = modal_n;
    oi[12] = cnt[0];
    oi[13] = cnt[1];
    for (int al = 0; al < 2; ++al) {
        od[al] = mean_out[al];
        od[2 + al] = w_out[al];
        od[4 + al] = sd_out[al];
    }
}

}  // namespace strk
