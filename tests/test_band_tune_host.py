"""Host build of strk_search.h: BandTune::max_m restricts the inner span to short motifs, consistently in band_geometry (k_plan,
k_replay, the window-miss path) and band_geometry_of_class (the band kernels)."""
import os
import shutil
import subprocess

import pytest


def test_inner_span_applies_up_to_max_m_and_the_two_geometries_agree(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "tune_check.cpp"
    src.write_text(r"""
#include <cstdio>
#include <random>
#include <algorithm>
#include "%s/strkit_amd/csrc/strk_search.h"
static bool same(const strk::BandGeo& a, const strk::BandGeo& b) {
    return a.ok == b.ok && a.cls == b.cls && a.G == b.G && a.wd == b.wd && a.dlo == b.dlo && a.bwd == b.bwd && a.bdlo == b.bdlo &&
           a.cmin == b.cmin && a.ncol == b.ncol;
}
int main() {
    std::mt19937 rng(15);
    long n_ok = 0, bad = 0, narrowed = 0;
    for (long it = 0; it < 1000000; ++it) {
        int nfl = 1 + rng() %% 260, nfr = 1 + rng() %% 127, m = 1 + rng() %% 14;
        int est = rng() %% ((rng() %% 4 == 0) ? 900 : 60);
        int W = 3 + rng() %% 13;
        int lo = std::max(0, est - W), n = std::min(32, est + W - lo + 1);
        int ntr = std::max(0, est * m + (int)(rng() %% 41) - 20);
        const int span = 3 + rng() %% 5, max_m = 1 + rng() %% 12;
        const strk::BandTune lim = {span, 0, max_m}, all = {span, 0, 0}, two = {span, 0};
        const strk::BandGeo a = strk::band_geometry(nfl, ntr, nfr, m, lo, n, lim);
        // up to max_m bases: the span applies, as with max_m = 0 (and as in the two-initialiser form); beyond: the whole table
        const strk::BandGeo want = m <= max_m ? strk::band_geometry(nfl, ntr, nfr, m, lo, n, all) : strk::band_geometry(nfl, ntr, nfr, m, lo, n);
        if (!same(a, want) || !same(strk::band_geometry(nfl, ntr, nfr, m, lo, n, two), strk::band_geometry(nfl, ntr, nfr, m, lo, n, all))) ++bad;
        if (!a.ok) continue;
        ++n_ok;
        if (!same(a, strk::band_geometry(nfl, ntr, nfr, m, lo, n))) ++narrowed;
        if (!same(a, strk::band_geometry_of_class(a.cls, nfl, ntr, m, lo, n, lim))) ++bad;
    }
    printf("%%ld %%ld %%ld\n", n_ok, bad, narrowed);
    return 0;
}
""" % root)
    exe = tmp_path / "tune_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    n_ok, bad, narrowed = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert n_ok > 300_000 and bad == 0
    assert narrowed > 10_000     # the knob does move bands
