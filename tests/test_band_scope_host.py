"""Host builds of what round 19 changed in the plan of a call (no GPU): layout class 0 of the band kernels holds windows of up to
512 bases (strk_search.h: band_max_db), and k_plan orders the band items of a block of reads by a counting sort
(strk_plan_order.h), restated for the host as plan_order_host and driven by tools/plan_order_asan.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gxx():
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")


GEOMETRY_SRC = r"""
#include <cstdio>
#include "%s/strkit_amd/csrc/strk_search.h"
using namespace strk;
static bool same(const BandGeo& a, const BandGeo& b) {
    return a.ok == b.ok && a.cls == b.cls && a.G == b.G && a.wd == b.wd && a.dlo == b.dlo && a.bwd == b.bwd && a.bdlo == b.bdlo &&
           a.cmin == b.cmin && a.ncol == b.ncol;
}
// what the issue states, in its own numbers: an 8-lane class (96 or 128 diagonals) takes a window of at most 512 bases whose
// candidates' span plus slack fits the band, whose fork columns fit 320 and whose prefix rows fit 512 + 96
static bool fits8(int wd, int narrow, int nfl, int ntr, int nfr, int m, int lo, int n) {
    const long ndb = (long)nfl + ntr + nfr;
    const long e_lo = (long)ntr - (long)(lo + n - 1) * m, e_hi = (long)ntr - (long)lo * m;
    const long span = (e_hi > 0 ? e_hi : 0) - (e_lo < 0 ? e_lo : 0) + 1;
    long slack = ndb >> 5;
    if (slack < 12) slack = 12;
    if (narrow && slack < 22) slack = 22;
    return span + 2 * slack <= wd && ndb <= 512 && (long)(n - 1) * m + wd <= 320 && (long)nfl + (long)(lo + n - 1) * m <= 512 + 96;
}
int main() {
    long cases = 0, ok8 = 0, over448 = 0, bad_pair = 0, bad_cls = 0;
    const int flanks[4][2] = {{70, 70}, {1, 127}, {127, 1}, {33, 90}};
    for (int W = 400; W <= 560; ++W)
        for (int m = 1; m <= 16; ++m)
            for (int f = 0; f < 4; ++f)
                for (int half = 4; half <= 8; half += 2)
                    for (int d = -3; d <= 3; ++d) {
                        const int nfl = flanks[f][0], nfr = flanks[f][1], ntr = W - nfl - nfr;
                        const int est = (ntr + m / 2) / m + d;
                        if (est < 0) continue;
                        const int lo = est - half > 0 ? est - half : 0, n = est + half - lo + 1;
                        if (n > 32) continue;
                        ++cases;
                        const BandGeo g = band_geometry(nfl, ntr, nfr, m, lo, n);
                        if (g.ok && !same(g, band_geometry_of_class(g.cls, nfl, ntr, m, lo, n))) ++bad_pair;
                        // the search takes the narrowest class that fits: 8 x 12 (class 4), then 8 x 16 (class 0)
                        const int want = fits8(96, 1, nfl, ntr, nfr, m, lo, n) ? 4 : (fits8(128, 0, nfl, ntr, nfr, m, lo, n) ? 0 : -1);
                        const int got = (g.ok && (g.cls & 3) == 0) ? g.cls : -1;
                        if (want != got) ++bad_cls;
                        if (got >= 0) { ++ok8; over448 += W > 448; }
                        if (W > 512 && got >= 0) ++bad_cls;
                    }
    printf("%%ld %%ld %%ld %%ld %%ld\n", cases, ok8, over448, bad_pair, bad_cls);
    return 0;
}
"""


def test_the_two_geometries_agree_and_class_0_takes_exactly_the_windows_up_to_512_that_fit(tmp_path):
    """Windows of 400-560 bases, motifs of 1-16 bases, four flank splits, tables of +-4, 6, 8 sizes around estimates up to three
    sizes off: band_geometry (k_plan) and band_geometry_of_class (the band kernels) give the same numbers, and an item lands
    in an 8-lane class exactly when its window has at most 512 bases and fits that class's band, columns and rows."""
    _need_gxx()
    src = tmp_path / "geo.cpp"
    src.write_text(GEOMETRY_SRC % ROOT)
    exe = tmp_path / "geo"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    cases, ok8, over448, bad_pair, bad_cls = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert cases > 50_000 and ok8 > 5_000
    assert over448 > 1_000          # windows of 449-512 bases do reach the 8-lane classes
    assert bad_pair == 0 and bad_cls == 0


def test_the_counting_sort_gives_every_item_a_slot_of_its_own_in_key_order(tmp_path):
    """plan_order_host on 20 000 random key sets (empty to full blocks, one class to all eight, one bin to all, rows beyond the
    class limits): slots are a permutation of 0 .. count - 1 and follow (class, bin, read index).  The same program runs a
    million sets under AddressSanitizer + UBSan from tools/plan_order_asan.sh."""
    _need_gxx()
    exe = tmp_path / "plan_order"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "plan_order_asan.cpp")], check=True)
    out = subprocess.run([str(exe), "20000", "7"], capture_output=True, text=True)
    sets, items, errors = (int(x) for x in out.stdout.split())
    assert out.returncode == 0 and sets == 20000 and errors == 0
    assert items > 3_000_000


def test_the_model_mirrors_the_class_limits_and_the_sort_scope(tmp_path):
    """tools/band_order_model.py restates band_max_db, the row bins and the sort scope: they must be the header's."""
    _need_gxx()
    src = tmp_path / "consts.cpp"
    src.write_text('#include <cstdio>\n#include "%s/strkit_amd/csrc/strk_plan_order.h"\nint main() { using namespace strk;\n'
                   'printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d\\n", band_max_db(0), band_max_db(1), band_max_db(2), band_max_db(3), plan_bin_shift(0), '
                   'plan_bin_shift(1), plan_bin_shift(2), plan_bin_shift(3), kPlanScope); return 0; }\n' % ROOT)
    exe = tmp_path / "consts"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(src)], check=True)
    v = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    import importlib.util
    spec = importlib.util.spec_from_file_location("band_order_model", os.path.join(ROOT, "tools", "band_order_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert tuple(v[:4]) == tuple(mod.MAX_DB) and tuple(v[4:8]) == tuple(mod.BIN_SHIFT) and v[8] == mod.SCOPE
