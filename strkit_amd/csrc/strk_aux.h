// strk_aux.h — the walk over the auxiliary fields of a BAM record, for host and device: per wanted tag the place, size and
// integer value of its first occurrence of the wanted class of types.  strk_phase_inputs.h (HP / PS) and strk_methyl.h (MM / ML /
// MN) both call it.  Without HIP the header compiles with the host compiler alone.
#pragma once
#include <stdint.h>

#include "strk_bamrec.h"

namespace strk_fe {

// What a caller wants of a tag: its two letters and the class of types that count.  An occurrence of another class is passed over.
constexpr int kAuxInt = 1;     // c C s S i I
constexpr int kAuxInt32 = 2;   // the same, and the value fits an int32
constexpr int kAuxZ = 3;
constexpr int kAuxB = 4;
struct AuxWant { char a, b; int cls; };

// Walks the auxiliary fields aux[0 .. n_aux) of one record to their end.  Per wanted tag, at its first occurrence that counts:
// off = the offset of its value (behind the type letter), size = the bytes of the value (a Z with its NUL, a B with its five
// leading bytes), val = the value of an integer.  off = -1: absent.  false: the chain runs past the end of the record, a Z has
// no NUL, a B does not fit, or a type the format does not know — nothing outside aux[0 .. n_aux) is read in either case.
STRK_FE_HD bool aux_find(const uint8_t* aux, int64_t n_aux, const AuxWant* want, int n_want, int64_t* off, int64_t* size, int64_t* val) {
    for (int k = 0; k < n_want; ++k) { off[k] = -1; size[k] = 0; val[k] = 0; }
    int64_t t = 0;
    while (t < n_aux) {
        if (t + 3 > n_aux) return false;
        const char ty = (char)aux[t + 2];
        const int64_t v = t + 3, left = n_aux - v;
        int64_t sz = -1, x = 0;
        int cls = 0;
        if (ty == 'c' || ty == 'C' || ty == 'A') {
            sz = 1;
            if (left >= 1) x = ty == 'c' ? (int64_t)(int8_t)aux[v] : (int64_t)aux[v];
            cls = ty != 'A' ? kAuxInt : 0;
        } else if (ty == 's' || ty == 'S') {
            sz = 2;
            if (left >= 2) x = ty == 's' ? (int64_t)(int16_t)rd_u16(aux + v) : (int64_t)rd_u16(aux + v);
            cls = kAuxInt;
        } else if (ty == 'i' || ty == 'I' || ty == 'f') {
            sz = 4;
            if (left >= 4) x = ty == 'i' ? (int64_t)rd_i32(aux + v) : (int64_t)rd_u32(aux + v);
            cls = ty != 'f' ? kAuxInt : 0;
        } else if (ty == 'Z' || ty == 'H') {
            int64_t z = v;
            while (z < n_aux && aux[z]) ++z;
            if (z >= n_aux) return false;
            sz = z - v + 1;
            cls = ty == 'Z' ? kAuxZ : 0;
        } else if (ty == 'B') {
            if (left < 5) return false;
            const char sub = (char)aux[v];
            int64_t es;
            if (sub == 'c' || sub == 'C') es = 1;
            else if (sub == 's' || sub == 'S') es = 2;
            else if (sub == 'i' || sub == 'I' || sub == 'f') es = 4;
            else return false;
            sz = 5 + (int64_t)rd_u32(aux + v + 1) * es;   // at most 5 + 4 * (2^32 - 1): no overflow in 64 bits
            cls = kAuxB;
        }
        if (sz < 0 || sz > left) return false;
        for (int k = 0; k < n_want; ++k) {
            if (off[k] >= 0 || aux[t] != (uint8_t)want[k].a || aux[t + 1] != (uint8_t)want[k].b) continue;
            const bool counts = want[k].cls == kAuxInt32 ? (cls == kAuxInt && x <= (int64_t)INT32_MAX) : cls == want[k].cls;
            if (counts) { off[k] = v; size[k] = sz; val[k] = x; }
        }
        t = v + sz;
    }
    return true;
}

}  // namespace strk_fe
