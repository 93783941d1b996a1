// k_vp8_tokens: the VP8 token partitions (RFC 6386 section 13) boolean-coded on the GPU
// (EncoderConfig::vp8_tokens 1), byte for byte what code_tokens + BoolEncoder write on the host
// (vp8_bitstream.cpp).  It runs after the analysis kernels, which leave the records (b.mb) and the
// levels (b.lv, 400 per macroblock); the frame's probabilities are known beforehand (planned from the
// branch statistics of the frame kStatsLag back), so no counting pass comes first.
//
// One workgroup of four waves per token partition (macroblock rows p, p + n, ... in raster order).
// A boolean coder is a serial chain, so the workgroup is a producer / consumer pair around it:
//
//   waves 1-3  binarise.  A batch is the next (up to) 7 coded macroblocks of the partition, found by
//              a ballot over a window of 64 records (skipped macroblocks produce nothing, and their
//              context resets are their zero nz bits in the records).  One lane per block, 25 per
//              macroblock in coding order (Y2, Y0-15, U, V): its first coefficient, type and context
//              from the nz bits of this, the left and the above record, then put_block's walk (the
//              host's own, vp8_tokens.h) twice -- once counting bins, and after a wave scan of the
//              counts once writing 16-bit tokens (prob << 1 | bit), the probability resolved from the
//              frame's table in LDS, into an LDS token buffer.  The three waves share no state: each
//              stages the batch's levels in LDS of its own and counts all 175 blocks (so each knows
//              every offset and where the batch ends: at the last macroblock that still fits the
//              buffer), and writes the 64-block stripe that is its own.  Tree branches also count
//              into the LDS histogram n[1056][2] the next frames' probabilities are planned from.
//   wave 0     lane 0 runs the coder (HeldBoolCoder) over the tokens in order, eight per LDS read.
//              Bytes leave final, in dwords, for the partition's region in mapped host memory, each
//              store checked against the region's end (on overflow the flag is raised, nothing more
//              is stored and the host codes the frame again).
//
// Two token buffers: the producers fill one while the coder drains the other, handed over by the
// workgroup barrier alone -- no polling, nothing between workgroups.
#include <hip/hip_runtime.h>

#include "../common/hip_check.h"
#include "../common/wave.h"
#include "vp8_encoder.h"
#include "vp8_tokens.h"

namespace mx {
namespace vp8 {

namespace {

constexpr int kTokBuf = kBlocks * 16 * kMaxBinsPerCoef;  // tokens per buffer: one worst-case macroblock
constexpr int kBatchMbs = 7;                             // 175 blocks: the producers' 192 lanes
constexpr int kMbVec = kCoefPerMb / 8;                   // uint4 per macroblock's levels
static_assert(kTokBuf % 8 == 0, "the coder reads eight tokens at a time");
static_assert(kBatchMbs * kBlocks <= 192, "one lane per block");

struct CountSink {
    int n = 0;
    __device__ void tok(int, int) { ++n; }
    __device__ void fix(int, int) { ++n; }
};
struct TokenSink {
    uint16_t* dst;
    const uint8_t* probs;
    uint32_t* hist;
    __device__ void tok(int idx, int bit) {
        *dst++ = (uint16_t)(((uint32_t)probs[idx] << 1) | (uint32_t)bit);
        atomicAdd(&hist[2 * idx + bit], 1u);
    }
    __device__ void fix(int prob, int bit) { *dst++ = (uint16_t)(((uint32_t)prob << 1) | (uint32_t)bit); }
};
// Final bytes into a region of `cap` bytes (a multiple of 4), a dword at a time.
struct DwordOut {
    uint32_t* dst;
    uint32_t cap;
    uint32_t pos = 0, acc = 0, overflow = 0;
    __device__ void byte(uint32_t b) {
        acc |= b << (8 * (pos & 3));
        ++pos;
        if ((pos & 3) == 0) {
            if (pos <= cap && !overflow)
                dst[(pos >> 2) - 1] = acc;
            else
                overflow = 1;
            acc = 0;
        }
    }
    __device__ void finish() {
        if (pos & 3) {
            if (((pos + 3) & ~3u) <= cap && !overflow)
                dst[pos >> 2] = acc;
            else
                overflow = 1;
        }
    }
};

// A batch macroblock as its blocks' lanes need it.
struct MbTok {
    uint32_t nz, left, up;  // nz bits of the record, of the record to the left and above (0 outside)
    int32_t mbi;
    int32_t y2;             // has a Y2 block (not B_PRED)
    int32_t y2ctx;          // the Y2 block's context
};

__global__ __launch_bounds__(256) void k_vp8_tokens(h264::Geometry g, const Vp8Mb* __restrict__ mbs, const int16_t* __restrict__ lv,
                                                     uint8_t* __restrict__ out, uint32_t region, int nparts) {
    __shared__ __attribute__((aligned(16))) uint16_t tokbuf[2][kTokBuf];
    __shared__ uint4 stage[3][kBatchMbs * kMbVec];
    __shared__ uint32_t hist[2 * kNumCoefProbs];
    __shared__ uint8_t probs[kNumCoefProbs];
    __shared__ MbTok mbt[3][kBatchMbs];
    __shared__ int sel[3][kBatchMbs + 1];  // window lanes of the first coded macroblocks
    __shared__ int s_ntok[2], s_fin[2];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mb_w = g.mb_w, mb_h = g.mb_h;
    const int Q = ((mb_h - p + nparts - 1) / nparts) * mb_w;  // macroblocks of this partition

    for (int k = tid; k < 2 * kNumCoefProbs; k += 256) hist[k] = 0;
    for (int k = tid; k < kNumCoefProbs; k += 256) probs[k] = reinterpret_cast<const Vp8TokenHeader*>(out)->probs[k];
    __syncthreads();

    // ---- producers: fill tokbuf[buf] with the next batch; s_ntok / s_fin[buf] say what it holds
    int q = 0;  // next macroblock of the partition's sequence (rows p, p + n, ... in raster order)
    auto produce = [&](int buf) {
        const int pw = wave - 1;
        int ncoded = 0, K = 0;
        unsigned long long coded = 0;
        for (;;) {  // the next window of 64 records with a coded macroblock in it
            const int qi = q + lane;
            const bool valid = qi < Q;
            const int row = valid ? qi / mb_w : 0, mbx = valid ? qi - row * mb_w : 0;
            const int mby = p + row * nparts, i = mby * mb_w + mbx;
            const uint32_t nz = valid ? (mbs[i].nz & 0x1FFFFFFu) : 0u;
            coded = __ballot(nz != 0);
            ncoded = __popcll(coded);
            if (ncoded == 0) {
                q = min(q + 64, Q);
                if (q >= Q) break;
                continue;
            }
            const int rank = __popcll(coded & ((1ull << lane) - 1ull));
            if (nz != 0 && rank <= kBatchMbs) sel[pw][rank] = lane;
            if (nz != 0 && rank < kBatchMbs) {
                MbTok t;
                t.nz = nz;
                t.left = mbx > 0 ? (mbs[i - 1].nz & 0x1FFFFFFu) : 0u;
                t.up = mby > 0 ? (mbs[i - mb_w].nz & 0x1FFFFFFu) : 0u;
                t.mbi = i;
                t.y2 = mbs[i].ymode != kBPred;
                t.y2ctx = 0;
                if (t.y2) {  // the nearest macroblocks above and to the left that have a Y2 block
                    for (int y = mby - 1; y >= 0; --y) {
                        const Vp8Mb& u = mbs[y * mb_w + mbx];
                        if (u.ymode != kBPred) {
                            t.y2ctx += (int)((u.nz >> kY2) & 1u);
                            break;
                        }
                    }
                    for (int x = mbx - 1; x >= 0; --x) {
                        const Vp8Mb& u = mbs[mby * mb_w + x];
                        if (u.ymode != kBPred) {
                            t.y2ctx += (int)((u.nz >> kY2) & 1u);
                            break;
                        }
                    }
                }
                mbt[pw][rank] = t;
            }
            K = min(ncoded, kBatchMbs);
            break;
        }
        wave_lds_sync();
        // the batch's levels into this wave's LDS
        for (int t = lane; t < K * kMbVec; t += 64) {
            const int r = t / kMbVec, o = t - r * kMbVec;
            stage[pw][t] = reinterpret_cast<const uint4*>(lv + (size_t)mbt[pw][r].mbi * kCoefPerMb)[o];
        }
        wave_lds_sync();
        // bins per block, offsets by a scan over the batch's blocks in coding order
        int base = 0, nfit = 0, ntok = 0;
        int my_off = 0, my_first = 0, my_type = 0, my_ctx = 0, my_r = 0, my_b = 0;
        bool my_on = false;
#pragma unroll
        for (int round = 0; round < 3; ++round) {
            const int blk = round * 64 + lane;
            const bool act = blk < K * kBlocks;
            const int r = act ? blk / kBlocks : 0, o = blk - r * kBlocks;
            const int b = o == 0 ? kY2 : o - 1;  // coding order: Y2, Y0..15, U0..3, V0..3
            int first = 0, type = 0, ctx = 0, c = 0;
            bool on = false;
            if (act) {
                const MbTok m = mbt[pw][r];
                auto bit = [](uint32_t w, int k) { return (int)((w >> k) & 1u); };
                if (b == kY2) {
                    on = m.y2 != 0;
                    type = 1;
                    ctx = m.y2ctx;
                } else if (b < 16) {
                    const int bx = b & 3, by = b >> 2;
                    on = true;
                    first = m.y2 ? 1 : 0;
                    type = m.y2 ? 0 : 3;
                    ctx = (by > 0 ? bit(m.nz, b - 4) : bit(m.up, 12 + bx)) + (bx > 0 ? bit(m.nz, b - 1) : bit(m.left, b + 3));
                } else {
                    const int bb = (b - 16) & 3, bx = bb & 1, by = bb >> 1;
                    on = true;
                    type = 2;
                    ctx = (by > 0 ? bit(m.nz, b - 2) : bit(m.up, b + 2)) + (bx > 0 ? bit(m.nz, b - 1) : bit(m.left, b + 1));
                }
                if (on) {
                    CountSink cs;
                    put_block(cs, reinterpret_cast<const int16_t*>(stage[pw]) + r * kCoefPerMb + b * 16, first, type, ctx);
                    c = cs.n;
                }
            }
            const int incl = (int)wave_incl_scan((uint32_t)c);
            const int off = base + incl - c, end = off + c;
            base += __shfl(incl, 63, 64);
            // a macroblock ends with its last block in coding order; the ends grow, so those within
            // the buffer are the macroblocks that fit
            const bool last_fit = act && o == kBlocks - 1 && end <= kTokBuf;
            nfit += __popcll(__ballot(last_fit));
            ntok = max(ntok, wave_max(last_fit ? end : 0));
            if (round == pw) {
                my_on = on;
                my_off = off;
                my_first = first;
                my_type = type;
                my_ctx = ctx;
                my_r = r;
                my_b = b;
            }
        }
        if (my_on && my_r < nfit) {
            TokenSink ts{tokbuf[buf] + my_off, probs, hist};
            put_block(ts, reinterpret_cast<const int16_t*>(stage[pw]) + my_r * kCoefPerMb + my_b * 16, my_first, my_type,
                      my_ctx);
        }
        if (K > 0) q = nfit < ncoded ? q + sel[pw][nfit] : min(q + 64, Q);
        if (pw == 0 && lane == 0) {
            s_ntok[buf] = ntok;
            s_fin[buf] = q >= Q;
        }
        wave_lds_sync();  // sel / mbt / stage are written again by the next batch
    };

    // ---- the coder's state (lane 0 of wave 0)
    Vp8TokenHeader* hdr = reinterpret_cast<Vp8TokenHeader*>(out);
    uint32_t* counts = reinterpret_cast<uint32_t*>(out + sizeof(Vp8TokenHeader)) + (size_t)p * 2 * kNumCoefProbs;
    uint8_t* bytes = out + sizeof(Vp8TokenHeader) + sizeof(uint32_t) * 2 * kNumCoefProbs * kMaxTokenParts + (size_t)p * region;
    DwordOut dw{reinterpret_cast<uint32_t*>(bytes), region};
    HeldBoolCoder<DwordOut> coder(dw);

    if (wave > 0) produce(0);
    __syncthreads();
    for (int cur = 0;; cur ^= 1) {
        const int fin = s_fin[cur], n = s_ntok[cur];
        if (wave == 0) {
            if (tid == 0) {
                const uint4* t4 = reinterpret_cast<const uint4*>(tokbuf[cur]);
                for (int k = 0; k < n; k += 8) {
                    const uint4 v = t4[k >> 3];
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t t = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                        if (k + j < n) coder.put(t >> 1, t & 1u);
                    }
                }
            }
        } else if (!fin) {
            produce(cur ^ 1);
        }
        __syncthreads();
        if (fin) break;
    }
    if (tid == 0) {
        coder.finish();
        dw.finish();
        hdr->len[p] = dw.pos;
        hdr->overflow[p] = dw.overflow;
    }
    for (int k = tid; k < 2 * kNumCoefProbs; k += 256) counts[k] = hist[k];
}

}  // namespace

void launch_vp8_tokens(const h264::Geometry& g, const Vp8DeviceBuffers& b, int log2_parts, hipStream_t stream) {
    const int nparts = 1 << log2_parts;
    hipLaunchKernelGGL(k_vp8_tokens, dim3(nparts), dim3(256), 0, stream, g, b.mb, b.lv, b.tok_out, b.tok_region,
                       nparts);
}

}  // namespace vp8
}  // namespace mx
