// VP8 coefficient tokens (RFC 6386 section 13) for the host writer (vp8_bitstream.cpp) and the GPU
// coder (vp8_tokens.hip): one walk of a block's levels through the token tree, and the boolean coder
// in the form the GPU runs -- the arithmetic of BoolEncoder::put, with the bytes that a carry may
// still change held back instead of corrected in place.
#pragma once
#include <stdint.h>

#include "vp8_core.h"

namespace mx {
namespace vp8 {

#define MXV8T __host__ __device__ inline

MXV8T int coef_index(int type, int band, int ctx) { return ((type * 8 + band) * 3 + ctx) * 11; }

// Token coding over a probability table: Enc::tok(table index, bit) codes (or counts) a
// context-coded token branch, Enc::fix(prob, bit) a fixed-probability bit (extra bits, sign).
template <class Enc>
MXV8T void put_extra(Enc& e, int v, const uint8_t* p, int n) {
    for (int k = n - 1; k >= 0; --k) e.fix(p[n - 1 - k], (v >> k) & 1);
}

// One block's tokens (13.2 / 13.3).
template <class Enc>
MXV8T void put_block(Enc& e, const int16_t* lv, int first, int type, int ctx) {
    int last = 15;
    while (last >= first && lv[last] == 0) --last;
    if (last < first) {
        e.tok(coef_index(type, kBand[first], ctx) + 0, 0);  // EOB
        return;
    }
    bool prev_zero = false;
    for (int i = first; i <= last; ++i) {
        const int P = coef_index(type, kBand[i], ctx);
        if (!prev_zero) e.tok(P + 0, 1);  // not EOB
        const int v = lv[i], a = v < 0 ? -v : v;
        if (a == 0) {
            e.tok(P + 1, 0);
            ctx = 0;
            prev_zero = true;
            continue;
        }
        e.tok(P + 1, 1);
        if (a == 1) {
            e.tok(P + 2, 0);
        } else {
            e.tok(P + 2, 1);
            if (a <= 4) {
                e.tok(P + 3, 0);
                if (a == 2) {
                    e.tok(P + 4, 0);
                } else {
                    e.tok(P + 4, 1);
                    e.tok(P + 5, a == 4);
                }
            } else {
                e.tok(P + 3, 1);
                if (a <= 10) {
                    e.tok(P + 6, 0);
                    if (a <= 6) {
                        e.tok(P + 7, 0);
                        put_extra(e, a - 5, kPcat1, 1);
                    } else {
                        e.tok(P + 7, 1);
                        put_extra(e, a - 7, kPcat2, 2);
                    }
                } else {
                    e.tok(P + 6, 1);
                    if (a <= 34) {
                        e.tok(P + 8, 0);
                        if (a <= 18) {
                            e.tok(P + 9, 0);
                            put_extra(e, a - 11, kPcat3, 3);
                        } else {
                            e.tok(P + 9, 1);
                            put_extra(e, a - 19, kPcat4, 4);
                        }
                    } else {
                        e.tok(P + 8, 1);
                        if (a <= 66) {
                            e.tok(P + 10, 0);
                            put_extra(e, a - 35, kPcat5, 5);
                        } else {
                            e.tok(P + 10, 1);
                            put_extra(e, a - 67, kPcat6, 11);
                        }
                    }
                }
            }
        }
        e.fix(128, v < 0);
        ctx = a == 1 ? 1 : 2;
        prev_zero = false;
    }
    if (last < 15) e.tok(coef_index(type, kBand[last + 1], ctx) + 0, 0);  // EOB
}

// Bins a block can take at most: 16 coefficients of not-EOB, two tree branches to DCT_CAT6's five,
// 11 extra bits and the sign.
constexpr int kMaxBinsPerCoef = 19;

// BoolEncoder with final bytes only: the same split / masked select / clz renormalisation over a
// 64-bit low end, but a byte leaves for `Out::byte` only once no carry can reach it.  The last byte
// that is not 0xFF and the count of 0xFF bytes after it wait; the next byte that is not 0xFF, or a
// carry, settles them (low + range never exceeds the interval, so one carry at most passes any byte).
// finish() is BoolEncoder::flush() and then lets the waiting bytes go.
template <class Out>
struct HeldBoolCoder {
    Out& out;
    uint32_t range = 255;
    uint64_t low = 0;
    int pend = 8;
    int held = -1;      // the waiting byte (-1: none yet)
    uint32_t run = 0;   // 0xFF bytes after it
    MXV8T explicit HeldBoolCoder(Out& o) : out(o) {}
    MXV8T void put(uint32_t prob, uint32_t bit) {
        const uint32_t split = 1 + (((range - 1) * prob) >> 8);
        const uint32_t m = 0u - (uint32_t)(bit != 0);
        low += split & m;
        range = ((range - split) & m) | (split & ~m);
        const int s = __builtin_clz(range) - 24;
        range <<= s;
        low <<= s;
        pend += s;
        while (pend >= 32) {
            const uint32_t carry = (uint32_t)(low >> pend) & 1u;
            low &= (uint64_t(1) << pend) - 1;
            pend -= 8;
            const uint32_t b = (uint32_t)(low >> pend);
            low &= (uint64_t(1) << pend) - 1;
            if (carry || b != 0xff) {
                settle(carry);
                held = (int)b;
            } else {
                ++run;
            }
        }
    }
    MXV8T void finish() {
        for (int i = 0; i < 32; ++i) put(128, 0);
        settle(0);
        held = -1;
    }

   private:
    MXV8T void settle(uint32_t carry) {
        if (held >= 0) out.byte(((uint32_t)held + carry) & 0xffu);
        for (; run; --run) out.byte((0xffu + carry) & 0xffu);
    }
};

// ---- device layout of the GPU token coder's output (mapped host memory, one block per frame slot)
constexpr int kMaxTokenParts = 8;
constexpr int kNumCoefProbs = 1056;
struct Vp8TokenHeader {
    uint32_t len[kMaxTokenParts];       // bytes of each partition (as far as they were stored)
    uint32_t overflow[kMaxTokenParts];  // nonzero: the partition did not fit its region
    uint8_t probs[kNumCoefProbs];       // in: the frame's coefficient probabilities (written by prepare())
};
static_assert(sizeof(Vp8TokenHeader) % 16 == 0, "the counts and regions after it stay aligned");
// then uint32 counts[kMaxTokenParts][1056][2], then the partitions' byte regions (region_bytes each)

#undef MXV8T

}  // namespace vp8
}  // namespace mx
