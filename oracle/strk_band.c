/*
 * strk_band.c — the banded first pass restated (TEST INFRASTRUCTURE ONLY; DESIGN.md, "Band path: seam corpus").
 *
 * What k_dp_band / k_dp_band_wide are meant to compute, in H-space, row by row: no skew, no G-space, no pads.  The band
 * geometry (dlo, wd, bdlo, bwd, cmin, ncol) is an ARGUMENT: the tests take it from band_geometry itself, compiled for the host.
 *
 * The candidate of size i is fl + motif * i + fr with fl = db[0, nfl) and fr = db[ndb - nfr, ndb); rows are candidate
 * bases, columns are db bases (the oracle's s1 is the db side).
 *   Forward   F(r, j), r = 0 .. nfl + (lo + n - 1) m, j = 0 .. |db|: the cell exists when dlo <= j - r < dlo + wd.
 *             F(0, j) = 0 (STRK_DB_BEG_FREE) or -g j;  F(r, 0) = 0 (STRK_CAND_BEG_FREE) or -g r;  where in the band, and in the ONE
 *             boundary cell on each side whose neighbour (1, j) resp. (r, 1) is the band's edge cell: (0, dlo + wd) and (1 - dlo, 0).
 *             The kernels hand those two values in (band_pass: keepU, keepL): an alignment that starts there has every cell it
 *             scores inside the band.  They take part as a start only, never in the sum of a fork row.
 *             F(r, j) = max(F(r-1, j-1) + W, F(r-1, j) - g, F(r, j-1) - g) over the neighbours that exist.
 *   Backward  B(k, j') over the reversed right flank (rows) and the reversed window (columns), band [bdlo, bdlo + bwd);
 *             top row free under STRK_DB_END_FREE, left column under STRK_CAND_END_FREE.
 *   Score     S_band[i] = max over j in [cmin, cmin + ncol) and [0, |db|] of F(R, j) + B(nfr, |db| - j), R = nfl + i m, where
 *             both cells exist; with `lmax` and STRK_CAND_END_FREE also max over r = 1 .. R of F(r, c(r)) - g (|db| - c(r)),
 *             c(r) = min(|db|, r + dlo + wd - 1) the band's rightmost column of row r (gap the rest of the window and end in
 *             the last column above the fork row: a real alignment).
 *   An entry without any such cell is STRK_O_BAND_NONE.  out_top (optional): per entry the largest G-space value
 *   of the fork row's band, completed by gaps, see below.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

const int8_t* strk_o_matrix(void);
int strk_o_encode(int c);

#define STRK_O_BAND_NONE INT32_MIN
#define BAND_NEG (INT32_MIN / 4)
#define BAND_G 5

static int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }
static int exists(int32_t v) { return v > BAND_NEG / 2; }

/* A row array holds the row before last when a row is written into it.  The band moves one column to the right per row and a row
 * writes every cell of its range, so what is left over of the older row lies in the few columns left of the new range (the
 * arrays start out empty, and nothing was ever written right of a range that the next ranges do not cover). */
static void clear_left(int32_t* row, int64_t first, int32_t ndb) {
    for (int64_t j = first - 4; j < first; j++)
        if (j >= 0 && j <= ndb) row[j] = BAND_NEG;
}

/* the encoded window and motif: row r >= 1 of the forward pass is a left-flank base, then the motif cyclically */
typedef struct {
    const uint8_t *db, *motif;
    int32_t ndb, nfl, m;
} band_seq;

static int fwd_row_sym(const band_seq* s, int32_t r) { return r <= s->nfl ? s->db[r - 1] : s->motif[(r - s->nfl - 1) % s->m]; }

int strk_o_band_scores(const uint8_t* db, int32_t ndb, int32_t nfl, int32_t nfr, const uint8_t* motif, int32_t m, int32_t lo,
                       int32_t n, int32_t dlo, int32_t wd, int32_t bdlo, int32_t bwd, int32_t cmin, int32_t ncol, int32_t lmax,
                       int32_t flags, int32_t* out, int32_t* out_top) {
    if (ndb < 1 || nfl < 0 || nfr < 0 || nfl + nfr > ndb || m < 1 || lo < 0 || n < 1 || wd < 1 || bwd < 1) return -1;
    const int8_t* mat = strk_o_matrix();
    const int db_beg = flags & 1, db_end = flags & 2, c_beg = flags & 4, c_end = flags & 8, g = BAND_G;
    uint8_t* edb = (uint8_t*)malloc((size_t)ndb);
    uint8_t* emo = (uint8_t*)malloc((size_t)m);
    for (int32_t k = 0; k < ndb; k++) edb[k] = (uint8_t)strk_o_encode(db[k]);
    for (int32_t k = 0; k < m; k++) emo[k] = (uint8_t)strk_o_encode(motif[k]);
    const band_seq sq = {edb, emo, ndb, nfl, m};
    const size_t w = (size_t)ndb + 1;
    int32_t* a = (int32_t*)malloc(sizeof(int32_t) * w);
    int32_t* b = (int32_t*)malloc(sizeof(int32_t) * w);
    int32_t* bl = (int32_t*)malloc(sizeof(int32_t) * w);   /* B(nfr, j') */
    /* ---- backward: rows k = 0 .. nfr (row k is db[ndb - k]), columns j' = 0 .. ndb (column j' is db[ndb - j']) ---- */
    for (size_t j = 0; j < w; j++) a[j] = b[j] = BAND_NEG;
    int32_t *prev = a, *cur = b;
    for (int32_t k = 0; k <= nfr; k++) {
        const int64_t j0 = (int64_t)k + bdlo - (k > 0 && (int64_t)k + bdlo == 1), j1 = (int64_t)k + bdlo + bwd - 1 + (k == 0);
        clear_left(cur, j0, ndb);
        for (int64_t j = j0 < 0 ? 0 : j0; j <= j1 && j <= ndb; j++) {
            int32_t v;
            if (k == 0) v = db_end ? 0 : -g * (int32_t)j;
            else if (j == 0) v = c_end ? 0 : -g * k;
            else {
                v = BAND_NEG;
                if (exists(prev[j - 1])) v = max2(v, prev[j - 1] + mat[edb[ndb - j] * 17 + edb[ndb - k]]);
                if (exists(prev[j])) v = max2(v, prev[j] - g);
                if (exists(cur[j - 1])) v = max2(v, cur[j - 1] - g);
            }
            cur[j] = v;
        }
        int32_t* t = prev; prev = cur; cur = t;
    }
    memcpy(bl, prev, sizeof(int32_t) * w);
    for (int64_t j = 0; j <= ndb; j++)   /* (the fork rows meet cells of the band only, not a boundary cell beside it) */
        if (j < (int64_t)nfr + bdlo || j > (int64_t)nfr + bdlo + bwd - 1) bl[j] = BAND_NEG;
    /* ---- forward, with the fork rows and the running last-column term ---- */
    const int32_t rows = nfl + (lo + n - 1) * m;
    int32_t lastcol = BAND_NEG, gtop = BAND_NEG;
    for (int32_t i = 0; i < n; i++) out[i] = STRK_O_BAND_NONE;
    prev = a; cur = b;
    for (size_t j = 0; j < w; j++) a[j] = b[j] = BAND_NEG;
    for (int32_t r = 0; r <= rows; r++) {
        const int64_t j0 = (int64_t)r + dlo, j1 = (int64_t)r + dlo + wd - 1;
        const int64_t x0 = j0 - (r > 0 && j0 == 1), x1 = j1 + (r == 0);   /* with the boundary cell beside the band */
        clear_left(cur, x0, ndb);
        const int rs = r >= 1 ? fwd_row_sym(&sq, r) : 0;
        for (int64_t j = x0 < 0 ? 0 : x0; j <= x1 && j <= ndb; j++) {
            int32_t v;
            if (r == 0) v = db_beg ? 0 : -g * (int32_t)j;
            else if (j == 0) v = c_beg ? 0 : -g * r;
            else {
                v = BAND_NEG;
                if (exists(prev[j - 1])) v = max2(v, prev[j - 1] + mat[edb[j - 1] * 17 + rs]);
                if (exists(prev[j])) v = max2(v, prev[j] - g);
                if (exists(cur[j - 1])) v = max2(v, cur[j - 1] - g);
            }
            cur[j] = v;
        }
        if (ndb >= j0 && ndb <= x1 && exists(cur[ndb])) gtop = max2(gtop, cur[ndb] + g * (r + ndb));
        if (r >= 1) {
            const int64_t c = j1 < ndb ? j1 : ndb;
            if (c >= 0 && c >= j0 && exists(cur[c])) lastcol = max2(lastcol, cur[c] - g * (int32_t)(ndb - c));
        }
        if (r >= nfl + lo * m && (r - nfl - lo * m) % m == 0) {
            const int32_t i = (r - nfl - lo * m) / m;
            int32_t best = BAND_NEG;
            for (int64_t j = cmin < 0 ? 0 : cmin; j < (int64_t)cmin + ncol && j <= ndb; j++)
                if (j >= j0 && j <= j1 && exists(cur[j]) && exists(bl[ndb - j])) best = max2(best, cur[j] + bl[ndb - j]);
            if (lmax && c_end) best = max2(best, lastcol);
            if (i < n && exists(best)) out[i] = best;
            /* the largest G = F + g (r + j) of the fork row's band, less g (R + |db| + nfr): what a kernel that sums in G-space with
             * a constant for a missing backward cell leaves, plus that constant, in an entry without a cell.  G does not fall
             * along a row, so that is the cell on the band's last diagonal; where that diagonal has left the window the columns
             * behind it carry the last column's largest G so far (gtop) */
            if (i < n && out_top) {
                if (j1 <= ndb) out_top[i] = (j1 >= 0 && exists(cur[j1])) ? cur[j1] - g * (int32_t)(ndb - j1) - g * nfr : STRK_O_BAND_NONE;
                else out_top[i] = exists(gtop) ? gtop - g * (r + ndb + nfr) : STRK_O_BAND_NONE;
            }
        }
        int32_t* t = prev; prev = cur; cur = t;
    }
    free(edb); free(emo); free(a); free(b); free(bl);
    return 0;
}
