// band_host.cpp — strk_search.h compiled for the host as a small shared library (tests/band_cases.py builds and loads it): the band
// geometry, the bound and the certificate search exactly as k_plan, the band kernels and k_replay compile them for the device.
#include <cstdint>

#include "../strkit_amd/csrc/strk_search.h"

using namespace strk;

extern "C" {

// {kNumBandClasses, kBandMaxFlank, kBandFlyMaxMotif, kBandFlyMaxFlank, kBandRowSlack, kBandNarrowSlack, kBandSpanWhole, 0}, then
// per class {G, D, wd, layout, max_db, max_col, fly, lmax}
void band_host_constants(int32_t* out) {
    const int32_t head[8] = {kNumBandClasses, kBandMaxFlank, kBandFlyMaxMotif, kBandFlyMaxFlank, kBandRowSlack, kBandNarrowSlack, kBandSpanWhole, 0};
    for (int k = 0; k < 8; ++k) out[k] = head[k];
    for (int c = 0; c < kNumBandClasses; ++c) {
        int32_t* o = out + 8 + 8 * c;
        o[0] = band_class_G(c); o[1] = band_class_D(c); o[2] = band_class_wd(c); o[3] = band_class_layout(c);
        o[4] = band_max_db(c); o[5] = band_max_col(c); o[6] = band_class_fly(c); o[7] = band_class_lmax(c);
    }
}

// out: {ok, cls, G, wd, dlo, bwd, bdlo, cmin, ncol}; `of_class` >= 0: band_geometry_of_class (what the band kernels recompute)
void band_host_geometry(int32_t nfl, int32_t ntr, int32_t nfr, int32_t m, int32_t lo, int32_t n, const int32_t* tune, int32_t of_class, int32_t* out) {
    const BandTune t = {tune[0], tune[1], tune[2]};
    const BandGeo g = of_class >= 0 ? band_geometry_of_class(of_class, nfl, ntr, m, lo, n, t) : band_geometry(nfl, ntr, nfr, m, lo, n, t);
    const int32_t v[9] = {g.ok, g.cls, g.G, g.wd, g.dlo, g.bwd, g.bdlo, g.cmin, g.ncol};
    for (int k = 0; k < 9; ++k) out[k] = v[k];
}

static BandGeo geo_of(const int32_t* v) {
    BandGeo g;
    g.ok = v[0]; g.cls = v[1]; g.G = v[2]; g.wd = v[3]; g.dlo = v[4]; g.bwd = v[5]; g.bdlo = v[6]; g.cmin = v[7]; g.ncol = v[8];
    return g;
}

// band_ub of the candidates lo .. lo + n - 1
void band_host_ub(const int32_t* geo, int32_t nfl, int32_t ntr, int32_t nfr, int32_t m, int32_t lo, int32_t n, int32_t end_flags, int32_t* out) {
    const BandGeo g = geo_of(geo);
    for (int32_t k = 0; k < n; ++k) out[k] = band_ub(g, nfl, ntr, nfr, m, lo + k, end_flags);
}

// search_replay_cert from `start` on (scores, ub): out = {cn, score, n_explored, miss, empty, uncertain}
void band_host_cert(int32_t start, int32_t step, int32_t lsr, int32_t max_iters, int32_t tie_last, const int32_t* scores, const int32_t* ub,
                    int32_t lo, int32_t n, int32_t narrow, int32_t* out) {
    SeenMask64 seen;
    auto u = [&](int k) { return ub[k]; };
    const CertResult cr = search_replay_cert(start, step, lsr, max_iters, tie_last, scores, lo, n < 64 ? n : 64, seen, u, narrow);
    out[0] = cr.res.cn; out[1] = cr.res.score; out[2] = cr.res.n_explored; out[3] = cr.res.miss; out[4] = cr.res.empty; out[5] = cr.uncertain;
}

}  // extern "C"
