/* The cell arithmetic of k_realign_dp and the walk of k_realign_trace (strkit_amd/csrc/strk_realign.h) with nothing of the
 * device around them: no lanes, no pad columns, no tiles, no strips; one cell after the other in 32-bit two's complement.
 * tests/realign_cases.py builds it (scalar()); where a device result differs from the oracle's, this tells "arithmetic" from
 * "lanes / tiles / trace layout".  enc: 256 bytes -> symbol; mat: 17 x 17 scores [s1 symbol][s2 symbol]. */
#include <stdint.h>
#include <stdlib.h>

#define NEG (-(1 << 28))
static int32_t add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }   /* wraps as the device does */
static int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }

int32_t realign_scalar(const uint8_t* s1, int32_t n1, const uint8_t* s2, int32_t n2, int32_t open, int32_t ext, int32_t gap_pref,
                       const uint8_t* enc, const int8_t* mat, int32_t* out_score, int32_t* out_end2, uint32_t* cigar, int32_t cap) {
    const int32_t o16 = open * 16, e16 = ext * 16, tagGi = gap_pref ? 0 : 4, tagGd = gap_pref ? 4 : 0;
    int32_t* H = malloc(sizeof(int32_t) * (size_t)n1);
    int32_t* Gd = malloc(sizeof(int32_t) * (size_t)n1);
    uint8_t* T = malloc((size_t)n1 * (size_t)n2);
    for (int32_t i = 0; i < n1; i++) {
        H[i] = (int32_t)(0u - 16u * ((uint32_t)open + (uint32_t)i * (uint32_t)ext));   /* row -1: -16 * (open + i * ext) */
        Gd[i] = NEG + tagGd;
    }
    int32_t best = INT32_MIN, bestj = 0;
    for (int32_t j = 0; j < n2; j++) {
        int32_t diag = 0, upH = 0, upE = NEG + tagGi;   /* left of column 0: H = 0 on every row, no gap yet */
        for (int32_t i = 0; i < n1; i++) {
            const int32_t Dp = add(diag, 16 * mat[17 * enc[s1[i]] + enc[s2[j]]] + 8);
            const int32_t Ei = max2(add(upE, -e16) | 1, add(upH, tagGi - o16));
            const int32_t Fj = max2(add(Gd[i], -e16) | 2, add(H[i], tagGd - o16));
            const int32_t Hp = max2(max2(Dp, Ei), Fj);
            T[(size_t)j * n1 + i] = (uint8_t)((Hp & 12) | (Ei & 1) | (Fj & 3));
            diag = H[i];
            H[i] = upH = Hp & ~15;
            Gd[i] = Fj;
            upE = Ei;
        }
        if (upH > best) { best = upH; bestj = j; }
    }
    *out_score = best >> 4;
    *out_end2 = bestj;
    int32_t n = 0, i = n1 - 1, j = bestj, where = 2;   /* 2: H, 1: 'I', 0: 'D'; runs end to start, then turned round */
    uint32_t* rev = malloc(sizeof(uint32_t) * (size_t)(2 * n1 + 4));
#define PUSH(op, len) do { if (n && (rev[n - 1] & 15u) == (op)) rev[n - 1] += (uint32_t)(len) << 4; else rev[n++] = ((uint32_t)(len) << 4) | (op); } while (0)
    while (i >= 0 && j >= 0) {
        const int nib = T[(size_t)j * n1 + i];
        if (where == 2) {
            if ((nib & 12) == 8) { PUSH(enc[s1[i]] == enc[s2[j]] ? 7u : 8u, 1); --i; --j; }
            else where = (nib & 12) == tagGi ? 1 : 0;
        } else if (where == 1) { PUSH(1u, 1); if (!(nib & 1)) where = 2; --i; }
        else { PUSH(2u, 1); if (!(nib & 2)) where = 2; --j; }
    }
    if (i >= 0) PUSH(1u, i + 1);
    if (j >= 0) PUSH(2u, j + 1);
#undef PUSH
    for (int32_t k = 0; k < n && k < cap; k++) cigar[k] = rev[n - 1 - k];
    free(rev); free(T); free(Gd); free(H);
    return n <= cap ? n : -1;
}
